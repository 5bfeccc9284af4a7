"""GPU: SSIM of the evaluator on the device (th_ssim, csrc/k_metrics.hip) against the float64 restatement of skimage 0.19's
structural_similarity(multichannel=True) in tests/test_ssim_host.py; the evaluator's SSIM end to end on a device batch; and
the SSIM of a rendered frame against itself and against the same frame on the fp32 per-layer MLP path."""

import numpy as np
import pytest
import torch

from test_ssim_host import ssim_oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip(gpu):
    from transhuman_amd import hip as H
    H.load_library()
    return H


def _pair(rs, h, w, noise):
    """float32 images: b = a + noise (clipped), noise None: unrelated images"""
    a = rs.uniform(size=(h, w, 3))
    b = rs.uniform(size=(h, w, 3)) if noise is None else np.clip(a + rs.normal(0, noise, size=a.shape), 0, 1)
    return a.astype(np.float32), b.astype(np.float32)


@pytest.mark.parametrize("h,w", [(7, 7), (7, 301), (13, 29), (64, 64), (217, 300), (512, 512)])
@pytest.mark.parametrize("noise", [0.0, 1e-3, 0.05, 0.3, None])
def test_kernel_matches_oracle(hip, gpu, h, w, noise):
    rs = np.random.RandomState(h * 7919 + w + (0 if noise is None else int(noise * 1e4)))
    a, b = _pair(rs, h, w, noise)
    got = hip.ssim(torch.from_numpy(a).to(gpu), torch.from_numpy(b).to(gpu))
    ref = ssim_oracle(a, b)
    assert abs(got - ref) < 1e-9, (got, ref)
    if noise == 0.0:
        assert abs(got - 1.0) < 1e-12


def test_strided_crop_of_a_larger_frame(hip, gpu):
    """a crop is a view into the full frame (row pitch = the frame's row): same value as the copied crop and the oracle"""
    rs = np.random.RandomState(5)
    fa, fb = _pair(rs, 300, 260, 0.08)
    ta, tb = torch.from_numpy(fa).to(gpu), torch.from_numpy(fb).to(gpu)
    y, x, h, w = 37, 51, 190, 123
    va, vb = ta[y:y + h, x:x + w], tb[y:y + h, x:x + w]
    assert not va.is_contiguous()
    got = hip.ssim(va, vb)
    assert got == hip.ssim(va.contiguous(), vb.contiguous())
    assert abs(got - ssim_oracle(fa[y:y + h, x:x + w], fb[y:y + h, x:x + w])) < 1e-9


def test_identical_deterministic_and_small(hip, gpu):
    rs = np.random.RandomState(11)
    a, b = _pair(rs, 333, 271, 0.1)
    ta, tb = torch.from_numpy(a).to(gpu), torch.from_numpy(b).to(gpu)
    assert abs(hip.ssim(ta, ta) - 1.0) < 1e-12
    s1, s2 = hip.ssim(ta, tb), hip.ssim(ta, tb)
    assert np.float64(s1).tobytes() == np.float64(s2).tobytes()
    for shape in ((6, 40, 3), (40, 6, 3)):
        z = torch.zeros(shape, device=gpu)
        with pytest.raises(ValueError):
            hip.ssim(z, z)


def _evaluator_batch(gpu, H, W, seed):
    rs = np.random.RandomState(seed)
    mask = np.zeros((H, W), bool)
    mask[5:17, 8:20] = rs.uniform(size=(12, 12)) < 0.8
    mask[5, 8] = mask[16, 19] = True
    n = int(mask.sum())
    gt = rs.uniform(size=(n, 3)).astype(np.float32)
    pred = np.clip(gt + rs.normal(0, 0.05, size=(n, 3)), 0, 1).astype(np.float32)
    batch = {"rgb": torch.from_numpy(gt)[None].to(gpu), "mask_at_box": torch.from_numpy(mask.reshape(-1))[None].to(gpu),
             "human_name": ["CoreView_313"], "frame_index": torch.tensor([7]), "cam_ind": torch.tensor([3])}
    return pred, gt, batch


@pytest.mark.parametrize("white", [False, True])
def test_evaluator_ssim_on_a_device_batch(hip, gpu, tmp_path, white):
    """evaluate() reports the SSIM of images()'s crops (lib/evaluators/if_nerf.py:108, :131-133), summarize() stores
    ssim.npy and returns its mean; MSE / PSNR stay what they were"""
    from transhuman_amd.config import get_cfg
    from transhuman_amd.evaluator import Evaluator
    from transhuman_amd.mesh import psnr_metric
    from oracle import th_oracle as O
    cfg = get_cfg()
    H = W = 24
    old = cfg.white_bkgd
    cfg.white_bkgd = white
    try:
        ev = Evaluator(result_dir=str(tmp_path / "res"))
        vals = []
        for seed in (0, 1):
            pred, gt, batch = _evaluator_batch(gpu, H, W, seed)
            r = ev.evaluate({"rgb_map": torch.from_numpy(pred)[None].to(gpu)}, batch, H, W)
            # the evaluator's MSE / PSNR expressions on the host arrays, as before; the oracle's PSNR (float32 mean) within 1e-6
            assert r["mse"] == float(np.mean((pred - gt) ** 2)) and r["psnr"] == psnr_metric(pred, gt)
            assert abs(r["psnr"] - O.psnr_metric(pred, gt)) < 1e-6
            ip, ig = ev.images(pred, gt, batch, H, W)
            assert ip.shape == (12, 12, 3)
            ref = ssim_oracle(ip, ig)
            assert abs(r["ssim"] - ref) < 1e-9, (r["ssim"], ref)
            assert 0.5 < r["ssim"] < 1.0
            vals.append(r["ssim"])
        assert (tmp_path / "res" / "CoreView_313" / "pred" / "frame7_view3.png").exists()
        s = ev.summarize()
        stored = np.load(tmp_path / "res" / "ssim.npy")
        assert stored.shape == (2,) and np.array_equal(stored, np.array(vals))
        assert s["ssim"] == float(np.mean(stored))
        assert np.load(tmp_path / "res" / "psnr.npy").shape == (2,)
    finally:
        cfg.white_bkgd = old


def test_evaluator_rejects_a_crop_below_the_window(hip, gpu):
    from transhuman_amd.evaluator import Evaluator
    H = W = 16
    mask = np.zeros((H, W), bool)
    mask[4:10, 2:14] = True                    # 6 rows: skimage raises ValueError
    n = int(mask.sum())
    rgb = torch.full((1, n, 3), 0.5, device=gpu)
    batch = {"rgb": rgb, "mask_at_box": torch.from_numpy(mask.reshape(-1))[None].to(gpu)}
    with pytest.raises(ValueError):
        Evaluator(result_dir="unused").evaluate({"rgb_map": rgb * 0.9}, batch, H, W, save=False)


def test_rendered_frame(hip, gpu):
    """a synthetic 96 x 96 frame: SSIM against itself is 1; against the same frame on the fp32 per-layer MLP path it is
    > 0.9999 and equals the oracle"""
    from transhuman_amd import synth
    from transhuman_amd.config import get_cfg
    from transhuman_amd.networks.renderer import if_clight_renderer
    from util import make_net, synth_assign, can64
    cfg = get_cfg()
    cfg.N_samples, cfg.num_class = 32, 300
    res = 96
    r = if_clight_renderer.Renderer(make_net(12).to(gpu), vertex_can=can64().numpy(), pc2voxel_ind=synth_assign(300))
    b = synth.batch_to(synth.make_batch(res, res, 3, seed=0, all_rays=True), gpu)
    img = r.render_fast(b, is_train=False)["rgb_map"][0].reshape(res, res, 3).clone()
    try:
        hip.set_mlp_mode(0)
        img32 = r.render_fast(b, is_train=False)["rgb_map"][0].reshape(res, res, 3).clone()
    finally:
        hip.set_mlp_mode(1)
    torch.cuda.synchronize()
    assert float(img.max()) > 0.05 and not torch.equal(img, torch.zeros_like(img))
    assert abs(hip.ssim(img, img) - 1.0) < 1e-12
    s = hip.ssim(img, img32)
    ref = ssim_oracle(img.cpu().numpy(), img32.cpu().numpy())
    print(f"SSIM(fused, fp32 per-layer) = {s:.12f}  oracle {ref:.12f}  max|diff| {float((img - img32).abs().max()):.2e}")
    assert s > 0.9999 and abs(s - ref) < 1e-9
