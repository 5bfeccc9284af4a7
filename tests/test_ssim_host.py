"""CPU: the SSIM of the evaluator (lib/evaluators/if_nerf.py:108, skimage's structural_similarity(img_pred, img_gt,
multichannel=True) on float64 crops).  skimage is absent, so the metric is pinned by its formula, skimage 0.19's for a
float64 image without data_range: 7 x 7 uniform window, sample covariance 49 / 48, data_range 2, mean over the pixels whose
window lies inside the image, then over the channels.  ``ssim_oracle`` restates it with plain windowed sums; it is checked
here against the way skimage 0.19 computes it (scipy.ndimage.uniform_filter + crop).  tests/test_gpu_ssim.py checks the
kernel against the oracle.  Also: the C-ABI surface of the new entry points, which needs no device."""
import ctypes
import os

import numpy as np
import pytest
from numpy.lib.stride_tricks import sliding_window_view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ssim_oracle(a, b):
    """float64 restatement of skimage 0.19 structural_similarity(a, b, multichannel=True), a / b: [H, W, C]"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape[0] < 7 or a.shape[1] < 7:
        raise ValueError("win_size exceeds image extent")
    C1, C2 = 4e-4, 3.6e-3                    # (0.01 * 2)^2, (0.03 * 2)^2: data_range 2 (float64 dtype range [-1, 1])
    cov_norm = 49.0 / 48.0

    def mean7(z):                            # window mean at every pixel whose 7 x 7 window lies inside the image
        return sliding_window_view(z, (7, 7)).sum(axis=(-2, -1)) / 49.0

    per_channel = []
    for c in range(a.shape[2]):
        x, y = a[..., c], b[..., c]
        ux, uy = mean7(x), mean7(y)
        vx = cov_norm * (mean7(x * x) - ux * ux)
        vy = cov_norm * (mean7(y * y) - uy * uy)
        vxy = cov_norm * (mean7(x * y) - ux * uy)
        S = (2 * ux * uy + C1) * (2 * vxy + C2) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
        per_channel.append(S.mean())
    return float(np.mean(per_channel))


def _skimage019_way(a, b):
    """skimage 0.19 _structural_similarity per channel: uniform_filter (mode reflect) over the whole image, crop(S, 3)"""
    from scipy.ndimage import uniform_filter
    vals = []
    for c in range(a.shape[2]):
        X, Y = a[..., c].astype(np.float64), b[..., c].astype(np.float64)
        ux, uy = uniform_filter(X, size=7), uniform_filter(Y, size=7)
        uxx, uyy, uxy = uniform_filter(X * X, size=7), uniform_filter(Y * Y, size=7), uniform_filter(X * Y, size=7)
        cov_norm = 49 / 48
        vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
        R = 2.0
        C1, C2 = (0.01 * R) ** 2, (0.03 * R) ** 2
        A1, A2, B1, B2 = 2 * ux * uy + C1, 2 * vxy + C2, ux ** 2 + uy ** 2 + C1, vx + vy + C2
        S = (A1 * A2) / (B1 * B2)
        vals.append(S[3:-3, 3:-3].mean(dtype=np.float64))
    return float(np.mean(vals))


def _pair(rs, h, w, noise, base=None):
    a = rs.uniform(size=(h, w, 3)) if base is None else np.full((h, w, 3), base) + rs.normal(0, 1e-6, size=(h, w, 3))
    b = np.clip(a + rs.normal(0, noise, size=a.shape), 0, 1) if noise is not None else rs.uniform(size=a.shape)
    return a.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64)


@pytest.mark.parametrize("h,w,noise", [(7, 7, 0.1), (7, 31, 0.05), (13, 29, None), (40, 33, 0.01), (64, 64, 0.2),
                                       (50, 90, 0.0)])
def test_oracle_matches_skimage019_computation_random(h, w, noise):
    rs = np.random.RandomState(h * 1000 + w)
    a, b = _pair(rs, h, w, noise)
    ref = _skimage019_way(a, b)
    assert abs(ssim_oracle(a, b) - ref) < 1e-12
    assert -1.0 <= ref <= 1.0


@pytest.mark.parametrize("base", [0.0, 0.5, 1.0])
def test_oracle_matches_skimage019_computation_near_constant(base):
    rs = np.random.RandomState(7)
    a, b = _pair(rs, 21, 17, 1e-5, base=base)
    a, b = np.clip(a, 0, 1), np.clip(b, 0, 1)
    assert abs(ssim_oracle(a, b) - _skimage019_way(a, b)) < 1e-12
    c = np.full((9, 9, 3), base)
    assert ssim_oracle(c, c) == 1.0


def test_oracle_identical_and_small():
    rs = np.random.RandomState(1)
    a = rs.uniform(size=(20, 20, 3))
    assert abs(ssim_oracle(a, a) - 1.0) < 1e-15
    for shape in ((6, 40, 3), (40, 6, 3)):
        with pytest.raises(ValueError):
            ssim_oracle(np.zeros(shape), np.zeros(shape))


@pytest.fixture(scope="module")
def lib():
    from transhuman_amd import build, hip
    build.build(force=False, verbose=False)
    return hip.load_library()


def test_ssim_entry_points_declared_exported_bound(lib):
    from transhuman_amd import hip
    header = open(os.path.join(ROOT, "include", "transhuman_hip.h")).read()
    raw = ctypes.CDLL(os.path.join(ROOT, "transhuman_amd", "libtranshuman_hip.so"))
    for name in ("th_ssim", "th_ssim_workspace_bytes"):
        assert f"{name}(" in header
        assert hasattr(raw, name)
        assert name in hip.SYMBOLS


def test_ssim_workspace_query_needs_no_device(lib):
    # one double per (16 x 32 output tile, channel): 512 x 512 -> 32 x 16 tiles of the 506 x 506 valid outputs
    assert lib.th_ssim_workspace_bytes(512, 512, 3) >= 32 * 16 * 3 * 8
    assert lib.th_ssim_workspace_bytes(7, 7, 3) >= 3 * 8
    assert lib.th_ssim_workspace_bytes(6, 40, 3) == 0 and lib.th_ssim_workspace_bytes(40, 6, 3) == 0


def test_ssim_rejects_small_images_before_any_device_work(lib):
    import torch
    from transhuman_amd import hip
    for shape in ((6, 40, 3), (40, 6, 3)):
        with pytest.raises(ValueError):
            hip.ssim(torch.zeros(shape), torch.zeros(shape))
    assert lib.th_ssim(None, None, None, 6, 40, 3, 120, None, None, 0, None) != 0


def test_evaluator_without_device_keeps_ssim_empty(tmp_path):
    """no HIP device: SSIM is skipped (no CPU path), summarize() still writes ssim.npy and reports NaN"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present (tests/test_gpu_ssim.py covers the evaluator there)")
    from transhuman_amd.evaluator import Evaluator
    H = W = 16
    mask = np.zeros((H, W), bool)
    mask[2:14, 3:12] = True
    n = int(mask.sum())
    rs = np.random.RandomState(0)
    gt = rs.uniform(size=(n, 3)).astype(np.float32)
    batch = {"rgb": torch.from_numpy(gt)[None], "mask_at_box": torch.from_numpy(mask.reshape(-1))[None]}
    ev = Evaluator(result_dir=str(tmp_path / "res"))
    r = ev.evaluate({"rgb_map": torch.from_numpy(gt * 0.9)[None]}, batch, H, W, save=False)
    assert "ssim" not in r and ev.ssim == []
    s = ev.summarize()
    assert np.isnan(s["ssim"]) and np.load(tmp_path / "res" / "ssim.npy").shape == (0,)
