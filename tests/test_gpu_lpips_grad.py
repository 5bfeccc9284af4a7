"""GPU: LPIPS (VGG16) as the training loss (K21) -- th_lpips_train / th_lpips_bwd and their stages (csrc/k_lpips.hip),
train_ops.LpipsFn, LPIPS.forward under autograd and train_loss.NetworkWrapper, against float64.

The bar is tests/test_gpu_train_vit_dense.py's: with g64 torch's float64 evaluation and parent the error of torch's own fp32
CPU autograd on the same input against g64, per tensor

    max|got - g64| <= 4 max(parent, 2^-22 max|g64|)

Every check prints err / bar.  Routing and gating stages (pool backward, ReLU gates) have no bar: they are exact.  The unsplit
chain is run on pairs whose float64 forward keeps 2^-16 of the layer's rms from every ReLU and pool decision
(tests/test_train_loss_host.py: lpips_margins; asserted here, never skipped), because a decision that flips between fp32 and
float64 moves the gradient by a whole term whoever computes it.  Figures measured on an MI355X are in DESIGN.md section 4."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_lpips_host import VGG_SHAPES, vgg_weights, write_weight_files
from test_train_loss_host import (assert_margin, golden, golden_lin, golden_pairs, lpips_chain, lpips_grad_oracle,
                                  pair_of_seed, pool_bwd_restatement, unpack_looped)

pytestmark = pytest.mark.gpu

SEED = 20
FLOOR = 2.0 ** -22
SCALE = np.array([.458, .448, .450], np.float32)
# (n, h, w, seed): RandomState(seed).uniform(-1, 1) images that keep the margin with vgg_weights(20)
CLEAN = [(1, 16, 16, 1008), (1, 17, 23, 1000), (1, 16, 33, 1017), (2, 20, 20, 1002)]
PATCH20_SEEDS = (2003, 2010, 2017, 2018, 2020, 2022)


@pytest.fixture(scope="module")
def hip(gpu):
    from transhuman_amd import hip as H
    H.load_library()
    return H


@pytest.fixture(scope="module")
def net(hip, gpu):
    """(packed, packed_bwd, vgg weights, lin weights) of the seeded VGG16 and the golden lin weights"""
    w = vgg_weights(SEED)
    lin = golden_lin(golden())
    dw = [torch.from_numpy(x).to(gpu) for x in w[0]]
    packed = hip.lpips_pack(dw, [torch.from_numpy(x).to(gpu) for x in w[1]], [torch.from_numpy(x).to(gpu) for x in lin], gpu)
    return packed, hip.lpips_pack_bwd(dw, gpu), w, lin


def _bar(got, g64, g32, label):
    got, g64, g32 = (np.asarray(x, np.float64) for x in (got, g64, g32))
    err, parent, scale = np.abs(got - g64).max(), np.abs(g32 - g64).max(), np.abs(g64).max()
    bar = 4 * max(parent, FLOOR * scale)
    print(f"{label}: err {err:.3e}  parent {parent:.3e}  scale {scale:.3e}  err/bar {err / bar:.3f}")
    assert np.isfinite(got).all(), label
    assert err <= bar, (label, err, bar)
    return err / bar


def _dev(a, gpu, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(gpu)


# ---------------------------------------------------------------------------
# the input-gradient convolution on its own
# ---------------------------------------------------------------------------
def _dgrad_ref(g_nhwc, w, layer, dtype):
    g = torch.from_numpy(g_nhwc).to(dtype).permute(0, 3, 1, 2)
    r = F.conv_transpose2d(g, torch.from_numpy(w).to(dtype), padding=1)
    if layer == 0:
        return (r / torch.from_numpy(SCALE).to(dtype)[None, :, None, None]).double().numpy()          # NCHW
    return r.permute(0, 2, 3, 1).double().numpy()


@pytest.mark.parametrize("layer", [0, 1, 2, 7, 12])
def test_dgrad_convolution_vs_float64(hip, gpu, net, layer):
    """layers 64->3, 64->64, 128->64, 512->256, 512->512 at sizes below, at and across the 8 x 16 tile, Z in {1, 3}; then a
    gradient confined to one corner pixel (halo and edge handling)"""
    _, pkb, (ws, _), _ = net
    co, ci = VGG_SHAPES[layer]
    worst = 0.0
    for H, W in ((1, 1), (2, 3), (8, 16), (9, 17), (5, 40)):
        for Z in (1, 3):
            rs = np.random.RandomState(layer * 1000 + H * 50 + W + Z)
            kinds = [("gauss", rs.normal(size=(Z, H, W, co)).astype(np.float32))]
            if Z == 1:
                for cy, cx in ((0, 0), (H - 1, W - 1)):
                    g = np.zeros((Z, H, W, co), np.float32)
                    g[:, cy, cx] = rs.normal(size=co)
                    kinds.append((f"corner {cy},{cx}", g))
            for kind, g in kinds:
                got = hip.lpips_dgrad(layer, _dev(g, gpu), pkb).cpu().numpy()
                r = _bar(got, _dgrad_ref(g, ws[layer], layer, torch.float64), _dgrad_ref(g, ws[layer], layer, torch.float32),
                         f"dgrad layer {layer} {H}x{W} Z{Z} {kind}")
                worst = max(worst, r)
    print(f"dgrad layer {layer}: worst err/bar {worst:.3f}")


def test_dgrad_gate_is_exact(hip, gpu, net):
    """the epilogue's gate [y > 0] of the layer below: the ungated result with zeros exactly where y <= 0 (y has zeros and negatives)"""
    _, pkb, _, _ = net
    rs = np.random.RandomState(3)
    for layer, (H, W) in ((2, (9, 17)), (12, (3, 5))):
        co, ci = VGG_SHAPES[layer]
        g = _dev(rs.normal(size=(2, H, W, co)), gpu)
        y = _dev(rs.randint(-1, 2, size=(2, H, W, ci)), gpu)
        plain = hip.lpips_dgrad(layer, g, pkb)
        gated = hip.lpips_dgrad(layer, g, pkb, gate=y)
        assert torch.equal(gated, torch.where(y > 0, plain, torch.zeros_like(plain)))
        assert bool((gated != 0).any())


# ---------------------------------------------------------------------------
# pool backward and the tap's gate: exact
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(5, 5), (2, 2), (4, 6), (7, 9), (16, 33)])
def test_pool_backward_is_exact(hip, gpu, H, W):
    rs = np.random.RandomState(H * 100 + W)
    for C in (64, 128):
        y = rs.randint(0, 3, size=(2, C, H, W)).astype(np.float32)           # integers 0..2: ties and zeros in most windows
        g = rs.randint(-4, 5, size=(2, C, H // 2, W // 2)).astype(np.float32)
        got = hip.lpips_pool_bwd(_dev(g.transpose(0, 2, 3, 1), gpu), _dev(y.transpose(0, 2, 3, 1), gpu))
        assert np.array_equal(got.cpu().numpy().transpose(0, 3, 1, 2), pool_bwd_restatement(g, y))


def test_tap_gate_is_exact(hip, gpu):
    """f0 == f1 makes the head's own gradient exactly 0: what is left is the incoming gradient under the gate [f0 > 0]"""
    rs = np.random.RandomState(8)
    f = _dev(rs.randint(0, 3, size=(2, 33, 64)), gpu)
    g = _dev(rs.randint(-4, 5, size=(2, 33, 64)), gpu)
    lin = _dev(rs.uniform(size=64), gpu)
    go = torch.tensor([1.0, -2.0], dtype=torch.float64, device=gpu)
    keep = g.clone()
    out = hip.lpips_head_bwd(f, f, lin, go, g=g, gate=True)
    assert out.data_ptr() == g.data_ptr() and torch.equal(out, torch.where(f > 0, keep, torch.zeros_like(keep)))
    assert torch.equal(hip.lpips_head_bwd(f, f, lin, go, g=keep.clone(), gate=False), keep)


# ---------------------------------------------------------------------------
# the head backward
# ---------------------------------------------------------------------------
def _head_ref(f0, f1, lin, go, dtype):
    a = torch.from_numpy(f0).to(dtype).requires_grad_(True)
    b, w = torch.from_numpy(f1).to(dtype), torch.from_numpy(lin).to(dtype)
    n0 = torch.sqrt((a * a).sum(-1, keepdim=True) + 1e-10) + 1e-10
    n1 = torch.sqrt((b * b).sum(-1, keepdim=True) + 1e-10) + 1e-10
    d = (((a / n0 - b / n1) ** 2) * w).sum(-1).mean(-1)                      # [N]
    d.backward(torch.from_numpy(go).to(dtype))
    return a.grad.double().numpy()


@pytest.mark.parametrize("C", [64, 512])
@pytest.mark.parametrize("hw", [1, 31, 32, 33])
def test_head_backward_vs_float64(hip, gpu, C, hw):
    rs = np.random.RandomState(C + hw)
    lin = rs.uniform(0.0, 0.2, size=C).astype(np.float32)
    go = np.array([1.0, -0.37, 2.5])
    for kind in ("relu", "zero_pixel", "equal", "1e-4", "1e3"):
        f0 = np.maximum(rs.normal(size=(3, hw, C)), 0).astype(np.float32)
        f1 = np.maximum(rs.normal(size=(3, hw, C)), 0).astype(np.float32)
        if kind == "zero_pixel":
            f0[:, hw // 2] = 0
        elif kind == "equal":
            f1 = f0.copy()
        elif kind in ("1e-4", "1e3"):
            f0, f1 = f0 * np.float32(kind), f1 * np.float32(kind)
        got = hip.lpips_head_bwd(_dev(f0, gpu), _dev(f1, gpu), _dev(lin, gpu), _dev(go, gpu, torch.float64)).cpu().numpy()
        assert np.isfinite(got).all(), kind
        if kind == "equal":
            assert np.all(got == 0)
            continue
        _bar(got, _head_ref(f0, f1, lin, go, torch.float64), _head_ref(f0, f1, lin, go, torch.float32), f"head C{C} hw{hw} {kind}")
    # added to an incoming gradient: the fp32 sum of the two
    g_in = rs.normal(size=f0.shape).astype(np.float32)
    alone = hip.lpips_head_bwd(_dev(f0, gpu), _dev(f1, gpu), _dev(lin, gpu), _dev(go, gpu, torch.float64))
    both = hip.lpips_head_bwd(_dev(f0, gpu), _dev(f1, gpu), _dev(lin, gpu), _dev(go, gpu, torch.float64), g=_dev(g_in, gpu))
    assert torch.equal(both, _dev(g_in, gpu) + alone)


# ---------------------------------------------------------------------------
# the whole chain
# ---------------------------------------------------------------------------
def _grad(hip, gpu, net, a, b, g_out=None):
    packed, pkb = net[0], net[1]
    ta, tb = _dev(a, gpu), _dev(b, gpu)
    out, state = hip.lpips_train(ta, tb, packed)
    go = torch.ones(a.shape[0], dtype=torch.float64, device=gpu) if g_out is None else _dev(g_out, gpu, torch.float64)
    return out, hip.lpips_bwd(go, ta, state, packed, pkb)


@pytest.mark.parametrize("n,h,w,seed", CLEAN)
@pytest.mark.parametrize("noise", [0.05, None])
def test_chain_on_margin_checked_pairs(hip, gpu, net, n, h, w, seed, noise):
    _, _, vw, lin = net
    a, b = pair_of_seed(seed, n, h, w, noise)
    assert_margin(a, vw, f"seed {seed}")
    out, got = _grad(hip, gpu, net, a, b)
    val64, g64 = lpips_grad_oracle(a, b, vw, lin)
    _, g32 = lpips_grad_oracle(a, b, vw, lin, torch.float32)
    assert np.all(np.abs(out[:, 5].cpu().numpy() - val64) <= 1e-5 * np.abs(val64) + 1e-9)
    _bar(got.cpu().numpy(), g64, g32, f"chain {n}x{h}x{w} seed {seed} noise {noise}")


def test_chain_on_the_golden_pairs(hip, gpu, net):
    """the vendored module's .double() gradients"""
    _, _, vw, lin = net
    worst = 0.0
    for i, (a, b, val64, g64) in enumerate(golden_pairs(golden())):
        assert_margin(a, vw, f"golden pair {i}")
        out, got = _grad(hip, gpu, net, a, b)
        _, g32 = lpips_grad_oracle(a, b, vw, lin, torch.float32)
        worst = max(worst, _bar(got.cpu().numpy(), g64, g32, f"golden pair {i} {a.shape}"))
    print(f"golden pairs: worst err/bar {worst:.3f}")


def test_chain_with_a_general_g_out(hip, gpu, net):
    _, _, vw, lin = net
    a, b = pair_of_seed(1002, 2, 20, 20, None)
    go = np.array([0.731, -1.9])
    _, got = _grad(hip, gpu, net, a, b, go)
    _, g64 = lpips_grad_oracle(a, b, vw, lin, g_out=go)
    _, g32 = lpips_grad_oracle(a, b, vw, lin, torch.float32, g_out=go)
    _bar(got.cpu().numpy(), g64, g32, "chain g_out (0.731, -1.9)")


def test_properties(hip, gpu, net):
    packed, pkb, vw, lin = net
    a, b = pair_of_seed(1006, 2, 20, 20, None)
    ta, tb = _dev(a, gpu), _dev(b, gpu)
    ones = torch.ones(2, dtype=torch.float64, device=gpu)
    out, state = hip.lpips_train(ta, tb, packed)
    assert torch.equal(out, hip.lpips(ta, tb, packed))                       # the value: th_lpips's bits
    g = hip.lpips_bwd(ones, ta, state, packed, pkb)
    assert g.shape == (2, 3, 20, 20) and g.dtype is torch.float32 and bool((g != 0).any())
    # lpips(a, a): gradient exactly 0
    out_aa, state_aa = hip.lpips_train(ta, ta, packed)
    assert torch.all(out_aa == 0) and torch.all(hip.lpips_bwd(ones, ta, state_aa, packed, pkb) == 0)
    # run to run, and independent of what the buffers held: NaN-filled state and workspace
    lib = hip.load_library()
    nan_bytes = lambda n: torch.full(((int(n) + 3) // 4,), float("nan"), dtype=torch.float32, device=gpu).view(torch.uint8)
    st2 = nan_bytes(lib.th_lpips_train_state_bytes(2, 20, 20))
    out2, st2 = hip.lpips_train(ta, tb, packed, state=st2)
    g2 = hip.lpips_bwd(ones, ta, st2, packed, pkb, workspace=nan_bytes(lib.th_lpips_bwd_workspace_bytes(2, 20, 20)))
    assert torch.equal(out2, out) and torch.equal(g2, g)
    assert torch.equal(hip.lpips_bwd(ones, ta, state, packed, pkb), g)
    # linear in g_out: powers of two scale every rounding exactly, and image 0's gradient does not see g_out[1]
    gs = hip.lpips_bwd(torch.tensor([4.0, -0.5], dtype=torch.float64, device=gpu), ta, state, packed, pkb)
    assert torch.equal(gs[0], 4 * g[0]) and torch.equal(gs[1], -0.5 * g[1])
    g0 = hip.lpips_bwd(torch.tensor([1.0, 0.0], dtype=torch.float64, device=gpu), ta, state, packed, pkb)
    assert torch.equal(g0[0], g[0]) and torch.all(g0[1] == 0)
    # batch of one == its slice of the batch
    o1, s1 = hip.lpips_train(ta[1:], tb[1:], packed)
    assert torch.equal(hip.lpips_bwd(ones[:1], ta[1:], s1, packed, pkb)[0], g[1])


def test_autograd_function_and_module(hip, gpu, net, tmp_path):
    """LpipsFn and LPIPS.forward: grad-enabled calls on an in0 that requires grad carry the gradient, in in0's dtype; every other
    call is th_lpips as before; an in1 that requires grad raises"""
    from transhuman_amd.lpips import LPIPS
    from transhuman_amd.networks.train_ops import LpipsFn
    packed, pkb, vw, lin = net
    a, b = pair_of_seed(1002, 2, 20, 20, 0.05)
    ta, tb = _dev(a, gpu), _dev(b, gpu)
    _, want = _grad(hip, gpu, net, a, b)
    leaf = ta.clone().requires_grad_(True)
    val = LpipsFn.apply(leaf, tb, packed, pkb)
    assert val.dtype is torch.float64 and val.shape == (2,) and torch.equal(val, hip.lpips(ta, tb, packed)[:, 5])
    val.sum().backward()
    assert torch.equal(leaf.grad, want)
    with pytest.raises(NotImplementedError):
        LpipsFn.apply(leaf, tb.clone().requires_grad_(True), packed, pkb)
    pv, pl = write_weight_files(str(tmp_path), SEED, lin)
    m = LPIPS(net="vgg", vgg16_path=pv, model_path=pl, device=gpu)
    plain = m(ta, tb)
    assert m.packed_bwd is None and not plain.requires_grad                  # the second image is packed on first use only
    with torch.no_grad():
        assert not m(ta.clone().requires_grad_(True), tb).requires_grad and m.packed_bwd is None
    leaf64 = ta.double().requires_grad_(True)
    v = m(leaf64, tb)
    assert v.shape == (2, 1, 1, 1) and v.dtype is torch.float64 and torch.equal(v.detach(), plain) and m.packed_bwd is not None
    v.sum().backward()
    assert leaf64.grad.dtype is torch.float64 and torch.equal(leaf64.grad, want.double())
    with pytest.raises(NotImplementedError):
        m(leaf64, tb.clone().requires_grad_(True))


# ---------------------------------------------------------------------------
# the loss
# ---------------------------------------------------------------------------
class _Stub:
    def __init__(self, ret):
        self.ret = ret

    def render(self, batch):
        return self.ret


def _fab_patch(seed, P):
    rs = np.random.RandomState(seed)
    mask = rs.uniform(size=(P, P)) < 0.7
    rgb = rs.uniform(size=(int(mask.sum()), 3)).astype(np.float32)
    return mask, rgb, rs.uniform(size=(P, P, 3)).astype(np.float32)


def _loss_ref(rgb, masks, div, targets, vw, lin, dtype, w_mse, w_lpips):
    """the loss restated without the code under test: the reference's loop for the patches, 2 x - 1, the restated chain"""
    leaf = torch.from_numpy(rgb).to(dtype).requires_grad_(True)
    t = torch.from_numpy(targets).to(dtype)
    fake = unpack_looped(leaf, torch.from_numpy(masks), torch.zeros(3, dtype=dtype), t, torch.from_numpy(div))
    mse = w_mse * torch.mean((fake - t) ** 2)
    lp = w_lpips * torch.mean(lpips_chain(fake.permute(0, 3, 1, 2) * 2. - 1., t.permute(0, 3, 1, 2) * 2. - 1., vw, lin, dtype))
    (mse + lp).backward()
    return float(mse.detach()), float(lp.detach()), leaf.grad.double().numpy(), fake.detach()


def _run_wrapper(gpu, lp_mod, rgb, masks, div, targets):
    from transhuman_amd.train_loss import NetworkWrapper
    leaf = _dev(rgb, gpu).requires_grad_(True)
    batch = {"patch_masks": torch.from_numpy(masks)[None].to(gpu), "target_patches": _dev(targets, gpu)[None],
             "patch_div_indices": torch.from_numpy(div)[None]}
    m = NetworkWrapper(net=None, renderer=_Stub({"rgb_map": leaf[None]}), lpips=lp_mod)
    _, loss, stats, _ = m(batch)
    loss.backward()
    return {k: float(v.detach()) for k, v in stats.items()}, leaf.grad.cpu().numpy()


@pytest.fixture(scope="module")
def lp_mod(hip, gpu, net, tmp_path_factory):
    from transhuman_amd.lpips import LPIPS
    pv, pl = write_weight_files(str(tmp_path_factory.mktemp("lpips_w")), SEED, net[3])
    return LPIPS(net="vgg", vgg16_path=pv, model_path=pl, device=gpu)


def _check_loss(stats, grad, mse64, lp64, g64, g32, label):
    print(f"{label}: mse {stats['mse_loss']:.8f} ({mse64:.8f})  lpips {stats['lpips_loss']:.8f} ({lp64:.8f})")
    assert abs(stats["mse_loss"] - mse64) <= 1e-6 * abs(mse64)               # a mean of fp32 squares
    assert abs(stats["lpips_loss"] - lp64) <= 1e-5 * abs(lp64) + 1e-9         # the forward's bar (tests/test_gpu_lpips.py)
    assert abs(stats["loss"] - (mse64 + lp64)) <= 1e-5 * abs(mse64 + lp64)
    _bar(grad, g64, g32, label + " d loss / d rgb_map")


def test_network_wrapper_on_the_golden_case(hip, gpu, net, lp_mod, monkeypatch):
    """2 patches of 16 x 16, one empty: the reference's loss values and ray-colour gradient"""
    from transhuman_amd.config import get_cfg
    _, _, vw, lin = net
    g = golden()
    monkeypatch.setattr(get_cfg(), "l2rec_weight", float(g["l2rec_weight"]), raising=False)
    monkeypatch.setattr(get_cfg(), "lpips_weight", float(g["lpips_weight"]), raising=False)
    args = (g["loss_rgb"], g["loss_masks"], g["loss_div"], g["loss_targets"])
    stats, grad = _run_wrapper(gpu, lp_mod, *args)
    _, _, g32, fake = _loss_ref(*args, vw, lin, torch.float32, float(g["l2rec_weight"]), float(g["lpips_weight"]))
    assert_margin((2 * fake[1:2] - 1).permute(0, 3, 1, 2).numpy(), vw, "golden loss case")
    _check_loss(stats, grad, float(g["loss_mse_loss"]), float(g["loss_lpips_loss"]), g["loss_grad_rgb"], g32, "golden loss case")


def test_network_wrapper_on_six_patches_of_20(hip, gpu, net, lp_mod, monkeypatch):
    """the training shape: 6 patches of 20 x 20, partly masked, against the float64 restatement of the whole loss"""
    from transhuman_amd.config import get_cfg
    _, _, vw, lin = net
    monkeypatch.setattr(get_cfg(), "l2rec_weight", 1.0, raising=False)
    monkeypatch.setattr(get_cfg(), "lpips_weight", 0.1, raising=False)
    parts = [_fab_patch(s, 20) for s in PATCH20_SEEDS]
    masks = np.stack([p[0] for p in parts])
    rgb = np.concatenate([p[1] for p in parts])
    targets = np.stack([p[2] for p in parts])
    div = np.concatenate([[0], np.cumsum([p[0].sum() for p in parts])]).astype(np.int64)
    mse64, lp64, g64, fake = _loss_ref(rgb, masks, div, targets, vw, lin, torch.float64, 1.0, 0.1)
    _, _, g32, fake32 = _loss_ref(rgb, masks, div, targets, vw, lin, torch.float32, 1.0, 0.1)
    assert_margin((2 * fake32 - 1).permute(0, 3, 1, 2).numpy(), vw, "six patches")
    stats, grad = _run_wrapper(gpu, lp_mod, rgb, masks, div, targets)
    _check_loss(stats, grad, mse64, lp64, g64, g32, "six patches of 20 x 20")


def test_training_step_through_the_loss(hip, gpu, net, lp_mod, monkeypatch):
    """Renderer.render under autograd at tests/test_gpu_train_ops.py's shapes, NetworkWrapper's loss, backward(): every
    parameter that gets a gradient from the stand-in loss (MSE + acc + depth terms) gets a finite one from the reference's"""
    from train_step_case import STEP_CFG, setup
    from transhuman_amd import config
    from transhuman_amd.train_loss import NetworkWrapper
    with config.override(**STEP_CFG) as cfg:
        model, r, b = setup(gpu)
        monkeypatch.setattr(cfg, "l2rec_weight", 1.0, raising=False)
        monkeypatch.setattr(cfg, "lpips_weight", 0.1, raising=False)
        n = int(b["ray_o"].shape[1])
        P = 20
        n_patch = -(-n // (P * P))
        masks = torch.zeros(n_patch * P * P, dtype=torch.bool)
        masks[:n] = True                                     # the rays fill the patches in order; the last one partly
        masks = masks.reshape(n_patch, P, P)
        div = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(masks.reshape(n_patch, -1).sum(1), 0)])
        gen = torch.Generator().manual_seed(0)
        b = dict(b, patch_masks=masks[None].to(gpu), patch_div_indices=div[None],
                 target_patches=torch.rand((1, n_patch, P, P, 3), generator=gen).to(gpu))
        ret = r.render(b)
        target = torch.rand((1, n, 3), generator=gen).to(gpu)
        (torch.mean((ret["rgb_map"] - target) ** 2) + 0.1 * ret["acc_map"].mean() + 0.01 * ret["depth_map"].mean()).backward()
        had = [k for k, p in model.named_parameters() if p.grad is not None]
        assert len(had) > 20
        model.zero_grad(set_to_none=True)
        ret, loss, stats, _ = NetworkWrapper(model, renderer=r, lpips=lp_mod)(b)
        assert set(stats) == {"mse_loss", "lpips_loss", "loss"} and float(stats["lpips_loss"].detach()) > 0
        loss.backward()
        params = dict(model.named_parameters())
        bad = [k for k in had if params[k].grad is None or not bool(torch.isfinite(params[k].grad).all())]
        assert not bad, bad
        assert any(float(params[k].grad.abs().max()) > 0 for k in had)
