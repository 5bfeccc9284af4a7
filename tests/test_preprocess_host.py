"""CPU: the numpy restatement of K16's definition (transhuman_amd/preprocess.py: undistort, area resize, background, raw-mask union
and border) against independent implementations -- scipy.ndimage.map_coordinates on the quantised coordinates, the reshape-mean,
scipy's minimum_filter / maximum_filter -- and its own exact properties.  No GPU, no OpenCV (parity with cv2 is unpinned)."""
import numpy as np
import pytest
from scipy import ndimage

from transhuman_amd import preprocess as P

SIZES = [(96, 80, 2), (64, 64, 1), (64, 96, 4)]                      # (H0, W0, n)
D_PLUS = np.array([0.35, 0.1, 0.01, -0.01, 0.05], np.float32)        # taps leave the image along the border
D_MINUS = np.array([-0.3, 0.1, 0.01, -0.01, 0.05], np.float32)       # no tap leaves the image
D_ZERO = np.zeros(5, np.float32)
# fp32 four-tap sum against scipy's float64 one: 1.2e-7 (two fp32 roundings of values <= 1) was measured; four times that
SCIPY_TOL = 5e-7


def camera(H0, W0):
    return np.array([[0.9 * W0, 0, W0 / 2 - 3.25], [0, 0.85 * W0, H0 / 2 + 1.5], [0, 0, 1]], np.float32)


def picture(H0, W0, seed=0, V=None):
    rng = np.random.default_rng(seed)
    shape = (H0, W0) if V is None else (V, H0, W0)
    return rng.integers(0, 256, shape + (3,), dtype=np.uint8), rng.choice(np.array([0, 1, 100], np.uint8), shape)


def blob_mask(H0, W0):
    """a disc around the top-left corner, a box in the bottom-right one and a ring in the middle: touches two image corners"""
    y, x = np.mgrid[:H0, :W0]
    m = (y * y + x * x < (H0 // 3) ** 2) | ((y > H0 - 9) & (x > W0 - 14))
    r2 = (y - H0 // 2) ** 2 + (x - W0 // 2) ** 2
    return (m | ((r2 < 15 ** 2) & (r2 > 6 ** 2))).astype(np.uint8)


@pytest.mark.parametrize("H0,W0,n", SIZES)
def test_no_distortion_is_the_identity(H0, W0, n):
    """D = 0 at n = 1: u8 / 255 exactly, the mask unchanged"""
    img, msk = picture(H0, W0, V=1)
    out, m, _ = P.prepare_views_oracle(img, msk, camera(H0, W0)[None], D_ZERO[None], ratio=1, mask_bkgd=False)
    want = img[0].astype(np.float32) / np.float32(255.0)
    assert out.dtype == np.float32 and out.shape == (1, 3, H0, W0)
    assert np.array_equal(out[0].transpose(1, 2, 0).view(np.int32), want.view(np.int32))
    assert np.array_equal(m[0], msk[0])
    iu, iv = P.undistort_map_oracle(camera(H0, W0), D_ZERO, H0, W0)
    assert np.array_equal(iu, np.broadcast_to(32 * np.arange(W0)[None], (H0, W0)))
    assert np.array_equal(iv, np.broadcast_to(32 * np.arange(H0)[:, None], (H0, W0)))


@pytest.mark.parametrize("H0,W0,n", SIZES)
@pytest.mark.parametrize("name,D", [("minus", D_MINUS), ("plus", D_PLUS)])
def test_against_scipy_map_coordinates(H0, W0, n, name, D):
    """bilinear sampling of u8 / 255 at (iv / 32, iu / 32) by scipy (float64, constant 0 outside) against the definition's fp32 sum.
    D-: every pixel.  D+: the pixels whose four taps lie inside the image -- along the border scipy interpolates towards its
    constant in its own way, the project's rule there (a tap outside is 0) is pinned by test_taps_outside."""
    K = camera(H0, W0)
    img, msk = picture(H0, W0, seed=1)
    o, _ = P.undistort_oracle(img, msk, K, D)
    iu, iv = P.undistort_map_oracle(K, D, H0, W0)
    src = img.astype(np.float64) / 255.0
    ref = np.stack([ndimage.map_coordinates(src[..., c], [iv / 32.0, iu / 32.0], order=1, mode="constant", cval=0.0)
                    for c in range(3)], -1)
    outside = P.taps_outside_oracle(K, D, H0, W0)
    where = np.ones((H0, W0), bool) if name == "minus" else outside == 0
    diff = np.abs(o.astype(np.float64) - ref)[where].max()
    print(f"{H0} x {W0} D{name}: {int(where.sum())} of {H0 * W0} pixels compared, max |o - scipy| = {diff:.3g}")
    assert where.sum() > H0 * W0 // 2
    assert diff <= SCIPY_TOL


@pytest.mark.parametrize("H0,W0,n", SIZES)
def test_taps_outside(H0, W0, n):
    """D+ has pixels with 2, 3 and 4 taps outside the image at every size, D- has none: the border rule is exercised, and a pixel
    without a tap inside is 0 / mask 0 whatever the picture"""
    K = camera(H0, W0)
    plus, minus = P.taps_outside_oracle(K, D_PLUS, H0, W0), P.taps_outside_oracle(K, D_MINUS, H0, W0)
    counts = [int((plus == k).sum()) for k in range(5)]
    print(f"{H0} x {W0}: pixels with 0..4 taps outside under D+: {counts}")
    assert counts[2] > 0 and counts[3] > 0 and counts[4] > 0
    if (H0, W0) == (96, 80):
        assert counts[2:] == [205, 2, 1832]
    assert not minus.any()
    img = np.full((H0, W0, 3), 255, np.uint8)
    o, m = P.undistort_oracle(img, np.full((H0, W0), 200, np.uint8), K, D_PLUS)
    assert (o[plus == 4] == 0).all() and (m[plus == 4] == 0).all()
    assert (o[plus == 0] == 1).all() and (m[plus == 0] == 200).all()
    part = (plus > 0) & (plus < 4)
    assert (o[part] <= 1).all() and (o[part] < 1).any()


@pytest.mark.parametrize("H0,W0,n", SIZES)
def test_area_resize_of_exact_values_is_the_reshape_mean(H0, W0, n):
    """multiples of 1/64 below 4: every partial sum of up to 16 of them is exact in fp32, so the order of the sum cannot show"""
    rng = np.random.default_rng(2)
    o = (rng.integers(0, 256, (H0, W0, 3)) / 64.0).astype(np.float32)
    want = o.astype(np.float64).reshape(H0 // n, n, W0 // n, n, 3).mean((1, 3))
    got = P.area_resize_oracle(o, n)
    assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want)


@pytest.mark.parametrize("H0,W0,n", SIZES)
def test_resize_mask_and_background(H0, W0, n):
    """prepare_views_oracle = undistort_oracle + block mean + mask at [n y, n x] + background, NCHW"""
    K = camera(H0, W0)
    img, msk = picture(H0, W0, seed=3, V=2)
    Ds = np.stack([D_PLUS, D_MINUS])
    Ks = np.stack([K, K])
    plain, m, _ = P.prepare_views_oracle(img, msk, Ks, Ds, ratio=1.0 / n, mask_bkgd=False)
    black, m_b, _ = P.prepare_views_oracle(img, msk, Ks, Ds, ratio=1.0 / n, mask_bkgd=True, white_bkgd=False)
    white, m_w, _ = P.prepare_views_oracle(img, msk, Ks, Ds[..., None], ratio=1.0 / n, mask_bkgd=True, white_bkgd=True)
    assert plain.shape == (2, 3, H0 // n, W0 // n) and m.shape == (2, H0 // n, W0 // n) and m.dtype == np.uint8
    assert np.array_equal(m, m_b) and np.array_equal(m, m_w)
    for v in range(2):
        o, full = P.undistort_oracle(img[v], msk[v], K, Ds[v])
        assert np.array_equal(m[v], full[::n, ::n])
        assert np.array_equal(plain[v], P.area_resize_oracle(o, n).transpose(2, 0, 1))
    hole = np.broadcast_to((m == 0)[:, None], plain.shape)
    assert hole.any() and not hole.all()
    assert (black[hole] == 0).all() and (white[hole] == 1).all()
    assert np.array_equal(black[~hole], plain[~hole]) and np.array_equal(white[~hole], plain[~hole])
    assert set(np.unique(m)) - {0, 1, 100}            # (the 8-bit mask is interpolated: values between the three occur)


@pytest.mark.parametrize("H0,W0,n", SIZES)
@pytest.mark.parametrize("border", [3, 5, 15])
def test_mask_border_against_scipy(H0, W0, n, border):
    m = blob_mask(H0, W0)
    assert m[0, 0] and m[-1, -1] and not m[0, -1]
    ero = ndimage.minimum_filter(m, size=border, mode="constant", cval=255)
    dil = ndimage.maximum_filter(m, size=border, mode="constant", cval=0)
    want = m.copy()
    want[(dil - ero) == 1] = 100
    got = P.combine_masks_oracle(m * 255, border=border)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert set(np.unique(got)) == {0, 1, 100}
    assert got[0, 0] == 1                               # (the window is clipped to the image: a filled corner is no border)


def test_mask_union():
    H0, W0 = 64, 96
    a, b = blob_mask(H0, W0) * 255, np.zeros((H0, W0), np.uint8)
    b[20:30, 60:90] = 3
    u = P.combine_masks_oracle(np.stack([a, a]), np.stack([b, 0 * b]))
    assert np.array_equal(u[0], ((a != 0) | (b != 0)).astype(np.uint8)) and np.array_equal(u[1], (a != 0).astype(np.uint8))
    assert np.array_equal(P.combine_masks_oracle(a), u[1])
    assert np.array_equal(P.combine_masks_oracle(a != 0, border=5), P.combine_masks_oracle(a, border=5))
    marked = P.combine_masks_oracle(np.stack([a, a]), np.stack([b, 0 * b]), border=5)
    assert np.array_equal(marked[0], P.combine_masks_oracle(u[0], border=5))


def test_K_out():
    K = camera(96, 80)
    K[0, 1] = 0.125
    for ratio in (1, 0.5, 0.25):
        *_, K_out = P.prepare_views_oracle(*picture(96, 80, V=1), K[None], D_MINUS[None], ratio=ratio)
        assert K_out.dtype == np.float32 and K_out.shape == (1, 3, 3)
        assert np.array_equal(K_out[0, :2], K[:2] * np.float32(ratio)) and np.array_equal(K_out[0, 2], K[2])
    assert K[0, 0] == np.float32(0.9 * 80)              # (the caller's K is not written)


def test_default_ratio_and_background_come_from_cfg():
    from transhuman_amd.config import get_cfg
    cfg = get_cfg()
    img, msk = picture(64, 64, V=1)
    K, D = camera(64, 64)[None], D_PLUS[None]
    old = cfg.ratio, cfg.white_bkgd
    try:
        cfg.ratio, cfg.white_bkgd = 0.25, True
        got = P.prepare_views_oracle(img, msk, K, D)
    finally:
        cfg.ratio, cfg.white_bkgd = old
    want = P.prepare_views_oracle(img, msk, K, D, ratio=0.25, white_bkgd=True)
    assert got[0].shape == (1, 3, 16, 16) and all(np.array_equal(g, w) for g, w in zip(got, want))


def test_value_errors():
    img, msk = picture(96, 80, V=1)
    K, D = camera(96, 80)[None], D_MINUS[None]
    for ratio in (0.3, 2, 0.125, 0, -0.5, 1 / 3):
        with pytest.raises(ValueError, match="ratio"):
            P.prepare_views_oracle(img, msk, K, D, ratio=ratio)
    with pytest.raises(ValueError, match="divisible"):
        P.prepare_views_oracle(img[:, :, :78], msk[:, :, :78], K, D, ratio=0.25)          # 78 = 2 x 39
    with pytest.raises(ValueError, match="divisible"):
        P.prepare_views_oracle(img[:, :95], msk[:, :95], K, D, ratio=0.5)
    with pytest.raises(ValueError):
        P.prepare_views_oracle(img, msk[:, :-1], K, D, ratio=0.5)
    with pytest.raises(ValueError):
        P.prepare_views_oracle(img[..., :2], msk, K, D, ratio=0.5)
    with pytest.raises(TypeError):
        P.prepare_views_oracle(img.astype(np.float32), msk, K, D, ratio=0.5)
    for border in (2, 4, 17, -1, 2.5):
        with pytest.raises(ValueError, match="border"):
            P.combine_masks_oracle(msk, border=border)
    with pytest.raises(ValueError):
        P.combine_masks_oracle(msk, msk[:, :-1])
