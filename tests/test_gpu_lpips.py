"""GPU: LPIPS (VGG16) of the evaluator on the device (th_lpips_pack / th_lpips, csrc/k_lpips.hip) against the float64
restatement in tests/test_lpips_host.py and the vendored module's float64 outputs in tests/golden/g20_lpips.npz; the
bitwise properties (identical images, symmetry, run to run, batch vs single); the evaluator end to end on device batches.

The bar: per tap and on the total, |hip - float64| <= 1e-5 |float64| + 1e-9.  The absolute floor is where the error of
the same formula evaluated in fp32 on the CPU (``lpips_oracle(..., dtype=torch.float32)``) sits on these inputs (up to a
few 1e-10): on near-identical pairs (values ~1e-7) both are rounding noise.  Each check prints the HIP error and that fp32
CPU error."""
import numpy as np
import pytest
import torch

from test_lpips_host import golden, golden_lin, golden_pairs, lpips_oracle, vgg_weights, write_weight_files

pytestmark = pytest.mark.gpu

SEED = 20
RTOL = 1e-5
ATOL = 1e-9


@pytest.fixture(scope="module")
def hip(gpu):
    from transhuman_amd import hip as H
    H.load_library()
    return H


@pytest.fixture(scope="module")
def net(hip, gpu):
    """(packed image, vgg weights, lin weights) of the seeded VGG16 and the golden lin weights"""
    w = vgg_weights(SEED)
    lin = golden_lin(golden())
    packed = hip.lpips_pack([torch.from_numpy(x).to(gpu) for x in w[0]], [torch.from_numpy(x).to(gpu) for x in w[1]],
                            [torch.from_numpy(x).to(gpu) for x in lin], gpu)
    return packed, w, lin


def _run(hip, gpu, packed, a, b):
    return hip.lpips(torch.from_numpy(a).to(gpu), torch.from_numpy(b).to(gpu), packed).cpu().numpy()


def _check(got, ref, ref32, label):
    err, err32 = np.abs(got - ref), np.abs(ref32 - ref)
    rel = err / np.maximum(np.abs(ref), 1e-300)
    rel32 = err32 / np.maximum(np.abs(ref), 1e-300)
    print(f"{label}: max rel err per tap + total  hip {np.array2string(rel.max(0), precision=2)}  "
          f"fp32-cpu {np.array2string(rel32.max(0), precision=2)}  max abs err hip {err.max():.2e} fp32-cpu "
          f"{err32.max():.2e}  (ref {np.array2string(ref[0], precision=4)})")
    assert np.all(err <= RTOL * np.abs(ref) + ATOL), (label, got, ref, ref32)
    assert np.all(ref > 0)


def _pair(rs, h, w, noise, n=1):
    a = rs.uniform(-1, 1, size=(n, 3, h, w))
    b = rs.uniform(-1, 1, size=a.shape) if noise is None else np.clip(a + rs.normal(0, noise, size=a.shape), -1, 1)
    return a.astype(np.float32), b.astype(np.float32)


def test_golden_float64(hip, gpu, net):
    """the vendored module's .double() outputs (per tap and total) on the fixture's pairs"""
    packed, w, lin = net
    for i, (in0, in1, out64, out32) in enumerate(golden_pairs(golden())):
        got = _run(hip, gpu, packed, in0, in1)
        _check(got, out64, out32, f"golden pair {i} {in0.shape[-2:]}")


@pytest.mark.parametrize("h,w", [(16, 16), (16, 301), (17, 23), (64, 64), (131, 97), (217, 300)])
@pytest.mark.parametrize("noise", [1e-3, 0.05, 0.3, None])
def test_random_pairs_against_oracle(hip, gpu, net, h, w, noise):
    packed, vw, lin = net
    rs = np.random.RandomState(h * 7919 + w + (0 if noise is None else int(noise * 1e4)))
    a, b = _pair(rs, h, w, noise)
    got = _run(hip, gpu, packed, a, b)
    _check(got, lpips_oracle(a, b, vw, lin), lpips_oracle(a, b, vw, lin, torch.float32), f"{h}x{w} noise {noise}")


@pytest.fixture(scope="module")
def full_frame(net):
    """a 512 x 512 pair and its float64 / fp32 CPU values (the float64 oracle is ~320 GFLOP: computed once)"""
    _, vw, lin = net
    a, b = _pair(np.random.RandomState(512), 512, 512, 0.05)
    return a, b, lpips_oracle(a, b, vw, lin), lpips_oracle(a, b, vw, lin, torch.float32)


def test_full_frame_against_oracle(hip, gpu, net, full_frame):
    a, b, ref, ref32 = full_frame
    got = _run(hip, gpu, net[0], a, b)
    _check(got, ref, ref32, "512x512 noise 0.05")


def test_large_first_layer_no_fp16_anywhere(hip, gpu, net):
    """the first conv's weights and bias x 1e4: activations pass 65504 (fp16's max) but stay finite in fp32"""
    _, vw, lin = net
    ws, bs = [x.copy() for x in vw[0]], [x.copy() for x in vw[1]]
    ws[0] *= np.float32(1e4)
    bs[0] *= np.float32(1e4)
    packed = hip.lpips_pack([torch.from_numpy(x).to(gpu) for x in ws], [torch.from_numpy(x).to(gpu) for x in bs],
                            [torch.from_numpy(x).to(gpu) for x in lin], gpu)
    a, b = _pair(np.random.RandomState(4), 64, 64, 0.05)
    import torch.nn.functional as F
    x = (torch.from_numpy(a).double() - torch.tensor([-.030, -.088, -.188]).float().double()[None, :, None, None]) / \
        torch.tensor([.458, .448, .450]).float().double()[None, :, None, None]
    act = F.relu(F.conv2d(x, torch.from_numpy(ws[0]).double(), torch.from_numpy(bs[0]).double(), padding=1))
    assert float(act.max()) > 65504.0
    got = _run(hip, gpu, packed, a, b)
    _check(got, lpips_oracle(a, b, (ws, bs), lin), lpips_oracle(a, b, (ws, bs), lin, torch.float32), "conv1 x 1e4")


def test_bitwise_properties(hip, gpu, net):
    packed = net[0]
    a, b = _pair(np.random.RandomState(9), 3 * 37 + 2, 61, 0.1, n=3)
    ta, tb = torch.from_numpy(a).to(gpu), torch.from_numpy(b).to(gpu)
    assert torch.all(hip.lpips(ta, ta, packed) == 0)
    ab = hip.lpips(ta, tb, packed)
    assert torch.equal(ab, hip.lpips(tb, ta, packed))
    assert torch.equal(ab, hip.lpips(ta, tb, packed))
    for i in range(3):
        assert torch.equal(ab[i], hip.lpips(ta[i:i + 1], tb[i:i + 1], packed)[0])
    assert torch.all(ab > 0)


def test_module_forward(hip, gpu, net, tmp_path):
    """LPIPS(net="vgg").forward: the reference's signature and return shapes, normalize=True maps [0, 1] to [-1, 1]"""
    from transhuman_amd.lpips import LPIPS
    _, vw, lin = net
    pv, pl = write_weight_files(str(tmp_path), SEED, lin)
    m = LPIPS(net="vgg", vgg16_path=pv, model_path=pl, device=gpu)
    a, b = _pair(np.random.RandomState(2), 40, 33, 0.2, n=2)
    ta, tb = torch.from_numpy(a).to(gpu), torch.from_numpy(b).to(gpu)
    val = m(ta, tb)
    val2, res = m.forward(ta, tb, retPerLayer=True)
    assert val.shape == (2, 1, 1, 1) and len(res) == 5 and all(r.shape == (2, 1, 1, 1) for r in res)
    assert torch.equal(val, val2) and torch.equal(val, hip.lpips(ta, tb, m.packed)[:, 5].reshape(2, 1, 1, 1))
    ref = lpips_oracle(a, b, vw, lin)
    assert np.allclose(torch.cat(res, 1).reshape(2, 5).cpu().numpy(), ref[:, :5], rtol=1e-4, atol=1e-9)
    assert torch.allclose(m(ta * 0.5 + 0.5, tb * 0.5 + 0.5, normalize=True), val, rtol=1e-4, atol=0)


def _evaluator_batch(gpu, H, W, seed, rows=(5, 30), cols=(8, 28)):
    rs = np.random.RandomState(seed)
    mask = np.zeros((H, W), bool)
    (r0, r1), (c0, c1) = rows, cols
    mask[r0:r1, c0:c1] = rs.uniform(size=(r1 - r0, c1 - c0)) < 0.8
    mask[r0, c0] = mask[r1 - 1, c1 - 1] = True
    n = int(mask.sum())
    gt = rs.uniform(size=(n, 3)).astype(np.float32)
    pred = np.clip(gt + rs.normal(0, 0.05, size=(n, 3)), 0, 1).astype(np.float32)
    batch = {"rgb": torch.from_numpy(gt)[None].to(gpu), "mask_at_box": torch.from_numpy(mask.reshape(-1))[None].to(gpu),
             "human_name": ["CoreView_313"], "frame_index": torch.tensor([7]), "cam_ind": torch.tensor([3])}
    return pred, gt, batch


@pytest.mark.parametrize("white", [False, True])
def test_evaluator_lpips_on_a_device_batch(hip, gpu, net, tmp_path, monkeypatch, white):
    """evaluate() reports the LPIPS of images()'s crops mapped to [-1, 1] (lib/evaluators/if_nerf.py:110-117),
    summarize() stores lpips.npy and returns its mean; MSE / PSNR / SSIM are those of a run without LPIPS weights"""
    from transhuman_amd.config import get_cfg
    from transhuman_amd.evaluator import Evaluator
    _, vw, lin = net
    pv, pl = write_weight_files(str(tmp_path), SEED, lin)
    monkeypatch.setattr(torch.hub, "get_dir", lambda: str(tmp_path / "hub"))
    cfg = get_cfg()
    monkeypatch.setattr(cfg, "white_bkgd", white)
    H = W = 40
    ev = Evaluator(result_dir=str(tmp_path / "res"), lpips_vgg16=pv, lpips_lin=pl)
    plain = Evaluator(result_dir=str(tmp_path / "plain"))
    assert ev.lpips_on and not plain.lpips_on
    vals = []
    for seed in (0, 1):
        pred, gt, batch = _evaluator_batch(gpu, H, W, seed)
        out = {"rgb_map": torch.from_numpy(pred)[None].to(gpu)}
        r = ev.evaluate(out, batch, H, W)
        r0 = plain.evaluate(out, batch, H, W)
        assert {k: r[k] for k in ("mse", "psnr", "ssim")} == r0 and "lpips" not in r0
        ip, ig = ev.images(pred, gt, batch, H, W)
        assert ip.shape == (25, 20, 3)
        x0, x1 = (np.ascontiguousarray((2.0 * t - 1.0).transpose(2, 0, 1)[None]).astype(np.float32) for t in (ip, ig))
        ref, ref32 = lpips_oracle(x0, x1, vw, lin), lpips_oracle(x0, x1, vw, lin, torch.float32)
        _check(np.array([[r["lpips"]]]), ref[:, 5:], ref32[:, 5:], f"evaluator white={white}")
        vals.append(r["lpips"])
    s = ev.summarize()
    s0 = plain.summarize()
    stored = np.load(tmp_path / "res" / "lpips.npy")
    assert stored.shape == (2,) and np.array_equal(stored, np.array(vals))
    assert s["lpips"] == float(np.mean(stored))
    assert {k: s[k] for k in ("mse", "psnr", "ssim")} == s0 and not (tmp_path / "plain" / "lpips.npy").exists()
    for name in ("mse.npy", "psnr.npy", "ssim.npy"):
        assert np.array_equal(np.load(tmp_path / "res" / name), np.load(tmp_path / "plain" / name))


def test_evaluator_rejects_a_crop_below_16(hip, gpu, net, tmp_path):
    from transhuman_amd.evaluator import Evaluator
    pv, pl = write_weight_files(str(tmp_path), SEED, net[2])
    pred, gt, batch = _evaluator_batch(gpu, 40, 40, 3, rows=(5, 20), cols=(8, 30))     # 15 rows: SSIM is fine
    ev = Evaluator(result_dir=str(tmp_path / "res"), lpips_vgg16=pv, lpips_lin=pl)
    with pytest.raises(ValueError):
        ev.evaluate({"rgb_map": torch.from_numpy(pred)[None].to(gpu)}, batch, 40, 40, save=False)
