"""CPU: LPIPS (VGG16) of the evaluator (lib/evaluators/if_nerf.py:110-117, third_parties/lpips/lpips.py:81-124 with net "vgg",
version 0.1, lpips=True, spatial=False, eval mode).  ``lpips_oracle`` restates the metric in float64 with plain torch ops;
it is checked here against tests/golden/g20_lpips.npz, the vendored module's outputs (tools/gen_golden_lpips.py) in
float64 (``.double()``) and in fp32.  ``vgg_weights`` regenerates the seeded He-normal VGG16 weights of that fixture, so
it never holds the 59 MB.  Also: the C-ABI surface of the new entry points, the weight loader, and the evaluator without
weights or without a device.  tests/test_gpu_lpips.py checks the kernels against the oracle."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g20_lpips.npz")

VGG_CONV_INDICES = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
VGG_SHAPES = [(64, 3), (64, 64), (128, 64), (128, 128), (256, 128), (256, 256), (256, 256), (512, 256), (512, 512),
              (512, 512), (512, 512), (512, 512), (512, 512)]
TAP_CHANNELS = (64, 128, 256, 512, 512)
LEVEL_LAYERS = ((0, 1), (2, 3), (4, 5, 6), (7, 8, 9), (10, 11, 12))    # conv layers of each slice; a pool before 2..5


def vgg_weights(seed):
    """seeded He-normal VGG16 conv weights (std sqrt(2 / (9 CIN))) and small uniform biases, float32 numpy arrays:
    -> (w [13], b [13]).  Deep taps carry weight with these (with torch's default init tap 5 is ~1e-9)."""
    rs = np.random.RandomState(seed)
    ws, bs = [], []
    for co, ci in VGG_SHAPES:
        ws.append(rs.normal(0.0, np.sqrt(2.0 / (9 * ci)), size=(co, ci, 3, 3)).astype(np.float32))
        bs.append(rs.uniform(-0.05, 0.05, size=co).astype(np.float32))
    return ws, bs


def lpips_oracle(in0, in1, vgg_w, lin_w, dtype=torch.float64):
    """float64 LPIPS (VGG16, v0.1): in0 / in1 [N, 3, H, W] in [-1, 1]; vgg_w = (w [13], b [13]); lin_w: 5 arrays of C
    (or [1, C, 1, 1]).  -> float64 numpy [N, 6]: the five tap values (spatial means of lin_k((f0 - f1)^2)) and their sum.
    dtype=torch.float32 evaluates the same formula in fp32 on the CPU (the error bar of an fp32 evaluation)."""
    x0 = torch.as_tensor(np.asarray(in0)).to(dtype)
    x1 = torch.as_tensor(np.asarray(in1)).to(dtype)
    if x0.shape[-2] < 16 or x0.shape[-1] < 16:
        raise ValueError("LPIPS (VGG16) needs at least 16 x 16 pixels")
    ws, bs = vgg_w
    # ScalingLayer (lpips.py:126-133): its buffers are fp32 values
    shift = torch.tensor([-.030, -.088, -.188], dtype=torch.float32).to(dtype)[None, :, None, None]
    scale = torch.tensor([.458, .448, .450], dtype=torch.float32).to(dtype)[None, :, None, None]
    n = x0.shape[0]
    h = (torch.cat([x0, x1]) - shift) / scale
    out = np.zeros((n, 6))
    with torch.no_grad():
        for k, layers in enumerate(LEVEL_LAYERS):
            if k:
                h = F.max_pool2d(h, 2, 2)
            for l in layers:
                h = F.relu(F.conv2d(h, torch.as_tensor(np.asarray(ws[l])).to(dtype),
                                    torch.as_tensor(np.asarray(bs[l])).to(dtype), padding=1))
            f = h / (torch.sqrt((h * h).sum(1, keepdim=True) + 1e-10) + 1e-10)      # normalize_tensor, eps twice
            d = (f[:n] - f[n:]) ** 2
            lw = torch.as_tensor(np.asarray(lin_w[k])).to(dtype).reshape(1, -1, 1, 1)
            out[:, k] = (d * lw).sum(1).mean((1, 2)).double().numpy()
    out[:, 5] = out[:, 0] + out[:, 1] + out[:, 2] + out[:, 3] + out[:, 4]
    return out


def golden():
    return np.load(GOLDEN, allow_pickle=False)


def golden_lin(g):
    return [g[f"lin{k}"] for k in range(5)]


def golden_pairs(g):
    return [(g[f"in0_{i}"], g[f"in1_{i}"], g[f"out64_{i}"], g[f"out32_{i}"]) for i in range(int(g["n_pairs"]))]


def test_golden_holds_plain_arrays():
    g = golden()
    assert [g[f"lin{k}"].shape for k in range(5)] == [(c,) for c in TAP_CHANNELS]
    assert sum(g[f"lin{k}"].size for k in range(5)) == 1472
    sizes = [g[f"in0_{i}"].shape[-2:] for i in range(int(g["n_pairs"]))]
    assert 3 <= len(sizes) <= 4 and (16, 16) in [tuple(s) for s in sizes]
    assert any(s[0] % 2 or s[1] % 2 for s in sizes)


def test_oracle_matches_vendored_module():
    """the restatement against the vendored module: its .double() outputs to 1e-12 relative, its fp32 outputs to 1e-5"""
    g = golden()
    w = vgg_weights(int(g["seed"]))
    for in0, in1, out64, out32 in golden_pairs(g):
        got = lpips_oracle(in0, in1, w, golden_lin(g))
        assert np.all(out64[:, 4] > 1e-4 * out64[:, 5]), out64      # the deep taps carry weight
        np.testing.assert_allclose(got, out64, rtol=1e-12, atol=0)
        np.testing.assert_allclose(got, out32, rtol=1e-5, atol=1e-7)


def test_oracle_identical_and_small():
    g = golden()
    w = vgg_weights(int(g["seed"]))
    a = g["in0_0"]
    assert np.all(lpips_oracle(a, a, w, golden_lin(g)) == 0.0)
    for shape in ((1, 3, 15, 40), (1, 3, 40, 15)):
        with pytest.raises(ValueError):
            lpips_oracle(np.zeros(shape), np.zeros(shape), w, golden_lin(g))


@pytest.fixture(scope="module")
def lib():
    from transhuman_amd import build, hip
    build.build(force=False, verbose=False)
    return hip.load_library()


def test_lpips_entry_points_declared_exported_bound(lib):
    from transhuman_amd import hip
    header = open(os.path.join(ROOT, "include", "transhuman_hip.h")).read()
    raw = ctypes.CDLL(os.path.join(ROOT, "transhuman_amd", "libtranshuman_hip.so"))
    for name in ("th_lpips_pack_bytes", "th_lpips_pack", "th_lpips_workspace_bytes", "th_lpips"):
        assert f"{name}(" in header
        assert hasattr(raw, name)
        assert name in hip.SYMBOLS


def test_lpips_size_queries_need_no_device(lib):
    n_weights = sum(co * ((ci + 7) // 8 * 8) * 9 for co, ci in VGG_SHAPES)
    assert lib.th_lpips_pack_bytes() >= 4 * (n_weights + sum(co for co, _ in VGG_SHAPES) + sum(TAP_CHANNELS))
    # two ping-pong activation buffers of 2N x 64 x H x W floats, at least
    assert lib.th_lpips_workspace_bytes(1, 512, 512) >= 2 * 2 * 64 * 512 * 512 * 4
    assert lib.th_lpips_workspace_bytes(3, 16, 16) >= 2 * 6 * 64 * 16 * 16 * 4
    assert lib.th_lpips_workspace_bytes(1, 15, 40) == 0 and lib.th_lpips_workspace_bytes(1, 40, 15) == 0
    assert lib.th_lpips_workspace_bytes(0, 40, 40) == 0


def test_lpips_rejects_small_images_before_any_device_work(lib):
    from transhuman_amd import hip
    for shape in ((1, 3, 15, 40), (1, 3, 40, 15)):
        with pytest.raises(ValueError):
            hip.lpips(torch.zeros(shape), torch.zeros(shape), None)
    assert lib.th_lpips(None, None, None, 1, 15, 40, None, None, None, 0, None) != 0
    assert "16 x 16" in hip._lib.th_last_error().decode()


def write_weight_files(d, seed, lin):
    """the seeded VGG16 weights in torchvision's key format (with a classifier.* key, which the loader ignores) and
    the lin weights in LPIPS's -> (vgg16 path, lin path)"""
    ws, bs = vgg_weights(seed)
    vgg = {}
    for i, w, b in zip(VGG_CONV_INDICES, ws, bs):
        vgg[f"features.{i}.weight"] = torch.from_numpy(w)
        vgg[f"features.{i}.bias"] = torch.from_numpy(b)
    vgg["classifier.6.bias"] = torch.zeros(1000)
    lp = {f"lin{k}.model.1.weight": torch.from_numpy(np.asarray(lin[k], np.float32).reshape(1, -1, 1, 1))
          for k in range(5)}
    pv, pl = os.path.join(d, "vgg16-397923af.pth"), os.path.join(d, "vgg.pth")
    torch.save(vgg, pv)
    torch.save(lp, pl)
    return pv, pl


def test_weight_loader_key_sets(tmp_path):
    from transhuman_amd.lpips import load_lpips_weights
    g = golden()
    pv, pl = write_weight_files(str(tmp_path), 3, golden_lin(g))
    conv_w, conv_b, lin_w = load_lpips_weights(pv, pl)
    ws, bs = vgg_weights(3)
    assert len(conv_w) == 13 and len(conv_b) == 13 and len(lin_w) == 5
    for l in (0, 7, 12):
        assert torch.equal(conv_w[l], torch.from_numpy(ws[l])) and torch.equal(conv_b[l], torch.from_numpy(bs[l]))
    assert torch.equal(lin_w[4].reshape(-1), torch.from_numpy(g["lin4"]))

    sd = torch.load(pv, weights_only=True)
    del sd["features.14.bias"]
    torch.save(sd, str(tmp_path / "missing.pth"))
    with pytest.raises(KeyError, match="features.14.bias"):
        load_lpips_weights(str(tmp_path / "missing.pth"), pl)
    sd = torch.load(pv, weights_only=True)
    sd["features.26.weight"] = sd["features.26.weight"][:, :256]
    torch.save(sd, str(tmp_path / "shape.pth"))
    with pytest.raises(ValueError, match="features.26.weight"):
        load_lpips_weights(str(tmp_path / "shape.pth"), pl)
    sd = torch.load(pl, weights_only=True)
    del sd["lin2.model.1.weight"]
    torch.save(sd, str(tmp_path / "lin.pth"))
    with pytest.raises(KeyError, match="lin2.model.1.weight"):
        load_lpips_weights(pv, str(tmp_path / "lin.pth"))


def test_module_rejects_what_is_not_built():
    from transhuman_amd.lpips import LPIPS
    for kw in ({"net": "alex"}, {"net": "squeeze"}, {"spatial": True}, {"version": "0.0"}):
        with pytest.raises(NotImplementedError):
            LPIPS(vgg16_path="unused", model_path="unused", **kw)


def _batch(H, W, seed):
    mask = np.zeros((H, W), bool)
    mask[2:20, 3:22] = True
    n = int(mask.sum())
    gt = np.random.RandomState(seed).uniform(size=(n, 3)).astype(np.float32)
    return {"rgb": torch.from_numpy(gt)[None], "mask_at_box": torch.from_numpy(mask.reshape(-1))[None]}, gt


def test_evaluator_without_weights_has_no_lpips(tmp_path, monkeypatch):
    """no weights configured: no "lpips" key and no lpips.npy, with or without a device"""
    from transhuman_amd.evaluator import Evaluator
    monkeypatch.setattr(torch.hub, "get_dir", lambda: str(tmp_path / "hub"))     # no default VGG16 file either
    ev = Evaluator(result_dir=str(tmp_path / "res"))
    assert not ev.lpips_on
    batch, gt = _batch(24, 24, 0)
    if torch.cuda.is_available():
        batch = {k: v.cuda() for k, v in batch.items()}
    r = ev.evaluate({"rgb_map": batch["rgb"] * 0.9}, batch, 24, 24, save=False)
    assert "lpips" not in r and ev.lpips == []
    s = ev.summarize()
    assert "lpips" not in s and not (tmp_path / "res" / "lpips.npy").exists()


def test_evaluator_weight_paths(tmp_path, monkeypatch):
    from transhuman_amd.config import get_cfg
    from transhuman_amd.evaluator import Evaluator
    g = golden()
    pv, pl = write_weight_files(str(tmp_path), 0, golden_lin(g))
    monkeypatch.setattr(torch.hub, "get_dir", lambda: str(tmp_path / "hub"))
    with pytest.raises(FileNotFoundError):
        Evaluator(result_dir="unused", lpips_vgg16=str(tmp_path / "absent.pth"), lpips_lin=pl)
    with pytest.raises(FileNotFoundError):
        Evaluator(result_dir="unused", lpips_vgg16=pv, lpips_lin=str(tmp_path / "absent.pth"))
    assert not Evaluator(result_dir="unused", lpips_lin=pl).lpips_on         # no VGG16 file at the hub default
    os.makedirs(tmp_path / "hub" / "checkpoints")
    os.link(pv, tmp_path / "hub" / "checkpoints" / "vgg16-397923af.pth")
    ev = Evaluator(result_dir="unused", lpips_lin=pl)
    assert ev.lpips_on and ev.lpips_vgg16 == str(tmp_path / "hub" / "checkpoints" / "vgg16-397923af.pth")
    cfg = get_cfg()
    monkeypatch.setattr(cfg, "lpips_vgg16_path", pv, raising=False)
    monkeypatch.setattr(cfg, "lpips_lin_path", pl, raising=False)
    ev = Evaluator(result_dir="unused")
    assert ev.lpips_on and (ev.lpips_vgg16, ev.lpips_lin) == (pv, pl)
    monkeypatch.setattr(cfg, "lpips_lin_path", str(tmp_path / "absent.pth"), raising=False)
    with pytest.raises(FileNotFoundError):
        Evaluator(result_dir="unused")


def test_evaluator_with_weights_without_device_skips_lpips(tmp_path, monkeypatch):
    """weights found but no HIP device: LPIPS is skipped like SSIM (empty list, empty lpips.npy, NaN mean)"""
    if torch.cuda.is_available():
        pytest.skip("a GPU is present (tests/test_gpu_lpips.py covers the evaluator there)")
    from transhuman_amd.evaluator import Evaluator
    g = golden()
    pv, pl = write_weight_files(str(tmp_path), 0, golden_lin(g))
    ev = Evaluator(result_dir=str(tmp_path / "res"), lpips_vgg16=pv, lpips_lin=pl)
    assert ev.lpips_on
    batch, gt = _batch(24, 24, 1)
    r = ev.evaluate({"rgb_map": torch.from_numpy(gt * 0.9)[None]}, batch, 24, 24, save=False)
    assert "lpips" not in r and ev.lpips == []
    s = ev.summarize()
    assert np.isnan(s["lpips"]) and np.load(tmp_path / "res" / "lpips.npy").shape == (0,)
