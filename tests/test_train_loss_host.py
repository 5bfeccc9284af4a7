"""CPU: the trainer's loss (lib/train/trainers/if_nerf_clight.py:43-106) and the gradient of LPIPS (VGG16) that it
back-propagates through -- transhuman_amd/train_loss.py, th_lpips_train / th_lpips_bwd (K21).

``lpips_grad_oracle`` is torch autograd over the float64 formula of tests/test_lpips_host.py's ``lpips_oracle``; it is held to
tests/golden/g23_lpips_grad.npz, the vendored module's ``.double()`` gradients (tools/gen_golden_lpips_grad.py), and is what
tests/test_gpu_lpips_grad.py holds the kernels to.  ``lpips_margins`` measures how far an input's float64 forward stays from
a ReLU or max-pool decision boundary: a decision that flips between fp32 and float64 moves the gradient by a whole term,
whoever computes it, so every end-to-end pair is asserted to keep 2^-16 of its layer's rms (torch's own fp32 pre-activations
deviate by at most 3.3e-6 of it).  Also: unpack_patches against the looped restatement, NetworkWrapper's loss arithmetic
against the golden case, the pool backward's tie rule against torch, and the C-ABI surface of the new entries."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_lpips_host import LEVEL_LAYERS, vgg_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g23_lpips_grad.npz")
MARGIN = 2.0 ** -16

NEW_ENTRIES = ("th_lpips_bwd_pack_bytes", "th_lpips_pack_bwd", "th_lpips_train_state_bytes", "th_lpips_train",
               "th_lpips_bwd_workspace_bytes", "th_lpips_bwd", "th_lpips_dgrad", "th_lpips_pool_bwd", "th_lpips_head_bwd")


# ---------------------------------------------------------------------------
# float64 restatements
# ---------------------------------------------------------------------------
def _t(a, dtype):
    return torch.as_tensor(np.asarray(a)).to(dtype)


def _scaling(dtype):
    shift = torch.tensor([-.030, -.088, -.188], dtype=torch.float32).to(dtype)[None, :, None, None]
    scale = torch.tensor([.458, .448, .450], dtype=torch.float32).to(dtype)[None, :, None, None]
    return shift, scale


def lpips_chain(x0, x1, vgg_w, lin_w, dtype=torch.float64):
    """the formula of lpips_oracle on torch tensors, differentiable: x0, x1 [N, 3, H, W] -> the totals [N]"""
    ws, bs = vgg_w
    shift, scale = _scaling(dtype)
    n = x0.shape[0]
    h = (torch.cat([x0.to(dtype), x1.to(dtype)]) - shift) / scale
    total = 0
    for k, layers in enumerate(LEVEL_LAYERS):
        if k:
            h = F.max_pool2d(h, 2, 2)
        for l in layers:
            h = F.relu(F.conv2d(h, _t(ws[l], dtype), _t(bs[l], dtype), padding=1))
        f = h / (torch.sqrt((h * h).sum(1, keepdim=True) + 1e-10) + 1e-10)
        d = (f[:n] - f[n:]) ** 2
        total = total + (d * _t(lin_w[k], dtype).reshape(1, -1, 1, 1)).sum(1).mean((1, 2))
    return total


def lpips_grad_oracle(in0, in1, vgg_w, lin_w, dtype=torch.float64, g_out=None):
    """-> (totals [N], d sum_n g_out[n] total[n] / d in0 [N, 3, H, W]) as float64 numpy; dtype=torch.float32: torch's own fp32
    CPU autograd on the same input (the `parent` of the error bar)"""
    x0 = _t(in0, dtype).clone().requires_grad_(True)
    tot = lpips_chain(x0, _t(in1, dtype), vgg_w, lin_w, dtype)
    g = torch.ones_like(tot) if g_out is None else _t(g_out, dtype)
    tot.backward(g)
    return tot.detach().double().numpy(), x0.grad.double().numpy()


def lpips_margins(in0, vgg_w):
    """the float64 forward of the in0 branch -> (the smallest |pre-activation| / rms of its layer, the smallest lead of a
    positive pool-window maximum over its runner-up / rms of the pooled layer's pre-activations)"""
    ws, bs = vgg_w
    dt = torch.float64
    shift, scale = _scaling(dt)
    h = (_t(in0, dt) - shift) / scale
    act, pool = np.inf, np.inf
    rms = None
    with torch.no_grad():
        for k, layers in enumerate(LEVEL_LAYERS):
            if k:
                N, C, H, W = h.shape
                win = h[:, :, :H // 2 * 2, :W // 2 * 2].reshape(N, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5)
                top = torch.sort(win.reshape(N, C, H // 2, W // 2, 4), -1, descending=True).values
                lead = (top[..., 0] - top[..., 1])[top[..., 0] > 0]
                if lead.numel():
                    pool = min(pool, float(lead.min() / rms))
                h = F.max_pool2d(h, 2, 2)
            for l in layers:
                z = F.conv2d(h, _t(ws[l], dt), _t(bs[l], dt), padding=1)
                rms = torch.sqrt((z * z).mean())
                act = min(act, float(z.abs().min() / rms))
                h = F.relu(z)
    return act, pool


def assert_margin(in0, vgg_w, label=""):
    act, pool = lpips_margins(in0, vgg_w)
    assert act >= MARGIN and pool >= MARGIN, (f"{label}: the float64 forward comes within {act:.2e} (ReLU) / {pool:.2e} (pool) "
                                              f"of a decision boundary, margin {MARGIN:.2e}: a badly chosen seed")


def pool_bwd_restatement(g, y):
    """backward of max_pool2d(y, 2, 2): g [N, C, H // 2, W // 2], y [N, C, H, W] -> [N, C, H, W].  The gradient goes to the first
    element of the window, in row-major window order, that equals the pooled value; cropped rows / columns get 0."""
    g, y = np.asarray(g), np.asarray(y)
    N, C, H, W = y.shape
    out = np.zeros_like(y)
    for yo in range(H // 2):
        for xo in range(W // 2):
            win = y[:, :, 2 * yo:2 * yo + 2, 2 * xo:2 * xo + 2].reshape(N, C, 4)
            first = np.argmax(win == win.max(-1, keepdims=True), -1)          # argmax of a bool array: its first True
            for k in range(4):
                out[:, :, 2 * yo + k // 2, 2 * xo + k % 2] = np.where(first == k, g[:, :, yo, xo], 0)
    return out


def unpack_looped(rgbs, patch_masks, bgcolor, targets, div_indices):
    """the reference's loop (:94-106), restated"""
    imgs = bgcolor.expand(targets.shape).clone()
    for i in range(len(div_indices) - 1):
        imgs[i, patch_masks[i]] = rgbs[int(div_indices[i]):int(div_indices[i + 1])]
    return imgs


# ---------------------------------------------------------------------------
# the fixture
# ---------------------------------------------------------------------------
def golden():
    return np.load(GOLDEN, allow_pickle=False)


def golden_lin(g):
    return [g[f"lin{k}"] for k in range(5)]


def golden_pairs(g):
    return [(g[f"in0_{i}"], g[f"in1_{i}"], g[f"val64_{i}"], g[f"grad64_{i}"]) for i in range(int(g["n_pairs"]))]


def pair_of_seed(seed, n, h, w, noise):
    """the images of a margin-checked seed: in0 = RandomState(seed).uniform(-1, 1); in1 near it (noise > 0) or unrelated (None)"""
    rs = np.random.RandomState(seed)
    a = rs.uniform(-1, 1, size=(n, 3, h, w))
    b = rs.uniform(-1, 1, size=a.shape) if noise is None else np.clip(a + rs.normal(0, noise, size=a.shape), -1, 1)
    return a.astype(np.float32), b.astype(np.float32)


def test_golden_holds_plain_small_arrays():
    assert os.path.getsize(GOLDEN) < 400 * 1024
    g = golden()
    assert 3 <= int(g["n_pairs"]) <= 4
    for k in g.files:
        assert g[k].dtype.kind in "fiub", k


def test_oracle_matches_vendored_gradient():
    """torch autograd over the restated formula against the vendored module's .double() gradient of sum(LPIPS) wrt in0"""
    g = golden()
    w = vgg_weights(int(g["seed"]))
    for i, (in0, in1, val64, grad64) in enumerate(golden_pairs(g)):
        assert_margin(in0, w, f"golden pair {i}")
        val, grad = lpips_grad_oracle(in0, in1, w, golden_lin(g))
        np.testing.assert_allclose(val, val64, rtol=1e-10, atol=0)
        assert np.abs(grad - grad64).max() <= 1e-10 * np.abs(grad64).max(), i
        assert np.abs(grad64).max() > 0


def test_golden_pairs_are_the_recorded_seeds():
    g = golden()
    for i, (in0, in1, _, _) in enumerate(golden_pairs(g)):
        n, _, h, w = in0.shape
        noise = float(g[f"noise_{i}"])
        a, b = pair_of_seed(int(g[f"seed_{i}"]), n, h, w, None if noise < 0 else noise)
        assert np.array_equal(a, in0) and np.array_equal(b, in1)


# ---------------------------------------------------------------------------
# unpack_patches and the loss
# ---------------------------------------------------------------------------
def _patch_case(seed, n_patch=3, P=7, empty=(1,)):
    rs = np.random.RandomState(seed)
    masks = rs.uniform(size=(n_patch, P, P)) < 0.6
    for i in empty:
        masks[i] = False
    counts = masks.reshape(n_patch, -1).sum(1)
    div = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    rgb = rs.uniform(size=(int(div[-1]), 3))
    targets = rs.uniform(size=(n_patch, P, P, 3))
    return torch.from_numpy(rgb), torch.from_numpy(masks), torch.from_numpy(div), torch.from_numpy(targets)


@pytest.mark.parametrize("empty", [(), (0,), (1,), (0, 1, 2)])
def test_unpack_patches_equals_the_loop(empty):
    from transhuman_amd.train_loss import unpack_patches
    rgb, masks, div, targets = _patch_case(3 + len(empty), empty=empty)
    bg = torch.tensor([0.25, 0.5, 0.75], dtype=rgb.dtype)
    got = unpack_patches(rgb, masks, div, targets, bg)
    want = unpack_looped(rgb, masks, bg, targets, div)
    assert got.shape == want.shape and torch.equal(got, want)
    for i in empty:
        assert torch.equal(got[i], bg.expand(got[i].shape))                   # an empty patch leaves the background


def test_unpack_patches_gradient_scatters_back():
    from transhuman_amd.train_loss import unpack_patches
    rgb, masks, div, targets = _patch_case(11)
    bg = torch.zeros(3, dtype=rgb.dtype)
    leaf = rgb.clone().requires_grad_(True)
    g = torch.from_numpy(np.random.RandomState(5).normal(size=tuple(targets.shape)))
    unpack_patches(leaf, masks, div, targets, bg).backward(g)
    want = torch.cat([g[i][masks[i]] for i in range(masks.shape[0])])         # each ray's gradient is its pixel's
    assert torch.equal(leaf.grad, want)
    # and the same through the loop under autograd
    leaf2 = rgb.clone().requires_grad_(True)
    unpack_looped(leaf2, masks, bg, targets, div).backward(g)
    assert torch.equal(leaf.grad, leaf2.grad)


class _StubRenderer:
    def __init__(self, ret):
        self.ret = ret

    def render(self, batch):
        return self.ret


def _golden_loss_batch(g, dtype):
    rgb = torch.from_numpy(g["loss_rgb"]).to(dtype).requires_grad_(True)
    batch = {"patch_masks": torch.from_numpy(g["loss_masks"])[None], "target_patches": torch.from_numpy(g["loss_targets"]).to(dtype)[None],
             "patch_div_indices": torch.from_numpy(g["loss_div"])[None]}
    return rgb, batch


def test_loss_arithmetic_against_golden(monkeypatch):
    """NetworkWrapper with a float64 stand-in for the LPIPS term: the reference's mse_loss / lpips_loss / loss (made with its own
    _unpack_imgs and scale_for_lpips) and the gradient with respect to the ray colours"""
    from transhuman_amd.config import get_cfg
    from transhuman_amd.train_loss import NetworkWrapper
    g = golden()
    w, lin = vgg_weights(int(g["seed"])), golden_lin(g)
    cfg = get_cfg()
    monkeypatch.setattr(cfg, "l2rec_weight", float(g["l2rec_weight"]), raising=False)
    monkeypatch.setattr(cfg, "lpips_weight", float(g["lpips_weight"]), raising=False)
    masks = g["loss_masks"]
    assert masks.shape == (2, 16, 16) and not masks[0].any() and 0 < masks[1].sum() < 256
    rgb, batch = _golden_loss_batch(g, torch.float64)
    # the patch that carries the gradient keeps the margin (the empty one is constant background and carries none)
    from transhuman_amd.train_loss import unpack_patches
    fake = unpack_patches(rgb.detach(), batch["patch_masks"][0], batch["patch_div_indices"][0], batch["target_patches"][0],
                          torch.zeros(3, dtype=torch.float64))
    assert_margin((2 * fake[1:2] - 1).permute(0, 3, 1, 2).float().numpy(), w, "golden loss case")
    stand_in = lambda a, b: lpips_chain(a, b, w, lin).reshape(-1, 1, 1, 1)
    ret = {"rgb_map": rgb[None]}
    m = NetworkWrapper(net=None, renderer=_StubRenderer(ret), lpips=stand_in)
    ret2, loss, stats, image_stats = m(batch)
    assert ret2 is ret and image_stats == {} and set(stats) == {"mse_loss", "lpips_loss", "loss"}
    for key in ("mse_loss", "lpips_loss", "loss"):
        np.testing.assert_allclose(float(stats[key].detach()), float(g[f"loss_{key}"]), rtol=1e-10, atol=0)
    loss.backward()
    want = g["loss_grad_rgb"]
    assert np.abs(rgb.grad.numpy() - want).max() <= 1e-10 * np.abs(want).max()


def test_non_patch_branch_and_rgb0(monkeypatch):
    from transhuman_amd.config import get_cfg
    from transhuman_amd.train_loss import NetworkWrapper
    cfg = get_cfg()
    monkeypatch.setattr(cfg.patch, "use_patch_sampling", False)
    monkeypatch.setattr(cfg, "lpips_weight", 0.0, raising=False)
    rs = np.random.RandomState(0)
    pred, gt, rgb0 = (torch.from_numpy(rs.uniform(size=(1, 9, 3))) for _ in range(3))
    mask = torch.from_numpy(rs.uniform(size=(1, 9)) < 0.5)
    m = NetworkWrapper(net=None, renderer=_StubRenderer({"rgb_map": pred, "rgb0": rgb0}))
    _, loss, stats, _ = m({"mask_at_box": mask, "rgb": gt})
    assert set(stats) == {"img_loss", "img_loss0", "loss"}
    want = ((pred[mask] - gt[mask]) ** 2).mean() + ((rgb0 - gt) ** 2).mean()
    assert float(loss) == float(want) == float(stats["loss"])


def test_missing_weights_raise_at_construction(monkeypatch, tmp_path):
    from transhuman_amd.config import get_cfg
    from transhuman_amd.train_loss import NetworkWrapper
    cfg = get_cfg()
    assert float(cfg.l2rec_weight) == 1.0 and float(cfg.lpips_weight) == 0.1          # the defaults
    monkeypatch.setattr(cfg, "lpips_vgg16_path", None, raising=False)
    monkeypatch.setattr(cfg, "lpips_lin_path", None, raising=False)
    with pytest.raises(ValueError, match="vgg16-397923af.pth") as e:
        NetworkWrapper(net=None, renderer=_StubRenderer({}))
    assert "vgg.pth" in str(e.value)
    monkeypatch.setattr(cfg, "lpips_vgg16_path", str(tmp_path / "absent.pth"), raising=False)
    monkeypatch.setattr(cfg, "lpips_lin_path", str(tmp_path / "absent2.pth"), raising=False)
    with pytest.raises(FileNotFoundError):
        NetworkWrapper(net=None, renderer=_StubRenderer({}))
    monkeypatch.setattr(cfg, "lpips_weight", 0.0, raising=False)
    m = NetworkWrapper(net=None, renderer=_StubRenderer({}))                            # lpips_weight = 0 needs no weights
    assert m.lpips is None and m.lpips_weight == 0.0


def test_cpu_batch_with_lpips_weight_raises(monkeypatch, tmp_path):
    """no silent CPU fallback of the LPIPS term"""
    from test_lpips_host import write_weight_files
    from transhuman_amd import hip
    from transhuman_amd.config import get_cfg
    from transhuman_amd.train_loss import NetworkWrapper
    g = golden()
    pv, pl = write_weight_files(str(tmp_path), 0, golden_lin(g))
    cfg = get_cfg()
    monkeypatch.setattr(cfg, "lpips_vgg16_path", pv, raising=False)
    monkeypatch.setattr(cfg, "lpips_lin_path", pl, raising=False)
    rgb, batch = _golden_loss_batch(g, torch.float32)
    m = NetworkWrapper(net=None, renderer=_StubRenderer({"rgb_map": rgb[None]}))
    with pytest.raises(hip.HipError):
        m(batch)


# ---------------------------------------------------------------------------
# the pool backward's tie rule
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(2, 2), (5, 5), (4, 7), (6, 6)])
def test_pool_tie_rule_is_torchs(H, W):
    rs = np.random.RandomState(H * 10 + W)
    y = rs.randint(0, 3, size=(2, 4, H, W)).astype(np.float64)               # integers 0..2: ties in most windows
    g = rs.randint(-4, 5, size=(2, 4, H // 2, W // 2)).astype(np.float64)
    leaf = torch.from_numpy(y).requires_grad_(True)
    F.max_pool2d(leaf, 2, 2).backward(torch.from_numpy(g))
    assert np.array_equal(pool_bwd_restatement(g, y), leaf.grad.numpy())


# ---------------------------------------------------------------------------
# the C-ABI surface
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from transhuman_amd import build, hip
    build.build(force=False, verbose=False)
    return hip.load_library()


def test_new_entries_declared_exported_bound(lib):
    from transhuman_amd import hip
    header = open(os.path.join(ROOT, "include", "transhuman_hip.h")).read()
    raw = ctypes.CDLL(os.path.join(ROOT, "transhuman_amd", "libtranshuman_hip.so"))
    for name in NEW_ENTRIES:
        assert f"{name}(" in header
        assert hasattr(raw, name)
        assert name in hip.SYMBOLS
    assert lib.th_abi_version() == 12
    for name in ("lpips_pack_bwd", "lpips_train", "lpips_bwd"):
        assert callable(getattr(hip, name))


def test_size_queries_need_no_device(lib):
    from test_lpips_host import VGG_SHAPES
    # the input-gradient image: every layer's weights with the output side padded to 64 channels
    n_weights = sum(((ci + 63) // 64 * 64) * co * 9 for co, ci in VGG_SHAPES)
    assert lib.th_lpips_bwd_pack_bytes() == 4 * n_weights
    # the state keeps at least the 13 outputs of the in0 images and the five taps of the in1 images
    for n, h, w in ((1, 16, 16), (6, 20, 20), (2, 17, 23)):
        hl, wl, need = h, w, 0
        for k, layers in enumerate(LEVEL_LAYERS):
            if k:
                hl, wl = hl // 2, wl // 2
            need += sum(VGG_SHAPES[l][0] for l in layers) * hl * wl + VGG_SHAPES[layers[-1]][0] * hl * wl
        assert lib.th_lpips_train_state_bytes(n, h, w) >= 4 * n * need
        # ... and beyond them only scratch for the layers of in1 that pass through (one 64-channel full-size map at most), the
        # pooled maps and the partials -- not the 13 layers of both images
        both = 2 * sum(VGG_SHAPES[l][0] * (h >> k) * (w >> k) for k, layers in enumerate(LEVEL_LAYERS) for l in layers)
        assert lib.th_lpips_train_state_bytes(n, h, w) < 4 * n * both
        assert lib.th_lpips_bwd_workspace_bytes(n, h, w) >= 2 * 4 * n * 64 * h * w
    for fn in (lib.th_lpips_train_state_bytes, lib.th_lpips_bwd_workspace_bytes):
        assert fn(1, 15, 40) == 0 and fn(1, 40, 15) == 0 and fn(0, 40, 40) == 0


def test_small_images_rejected_before_any_device_work(lib):
    from transhuman_amd import hip
    assert lib.th_lpips_train(None, None, None, 1, 15, 40, None, None, None, 0, None) != 0
    assert "16 x 16" in hip._lib.th_last_error().decode()
    assert lib.th_lpips_bwd(None, None, None, 1, 40, 15, None, None, None, 0, None, None, 0, None) != 0
    assert "16 x 16" in hip._lib.th_last_error().decode()
    with pytest.raises(ValueError):
        hip.lpips_train(torch.zeros(1, 3, 15, 40), torch.zeros(1, 3, 15, 40), None)


def test_lpips_fn_refuses_a_target_gradient_and_a_cpu_input():
    from transhuman_amd import hip
    from transhuman_amd.networks.train_ops import LpipsFn
    a = torch.zeros(1, 3, 16, 16, requires_grad=True)
    with pytest.raises(NotImplementedError):
        LpipsFn.apply(a, torch.zeros(1, 3, 16, 16, requires_grad=True), None, None)
    with pytest.raises(hip.HipError):
        LpipsFn.apply(a, torch.zeros(1, 3, 16, 16), None, None)
