"""GPU: the input views made on the device from raw camera frames (csrc/k_prep.hip, transhuman_amd/preprocess.py, K16) against the
numpy restatement of their definition -- picture and mask equal at EVERY pixel, bit for bit (every step of the definition is one
correctly rounded IEEE operation in a fixed order: there is no tolerance and no cap on mismatches) -- determinism, input
conversion, the C surface's argument checks, and the renderer's cfg.input_prep == "device"."""
import numpy as np
import pytest
import torch

from test_preprocess_host import SIZES, D_PLUS, D_MINUS, camera, picture, blob_mask

pytestmark = pytest.mark.gpu

V = 2                                                                  # one view per coefficient set


@pytest.fixture(scope="module")
def pp(gpu):
    from transhuman_amd import hip, preprocess
    hip.load_library()
    return preprocess


def _case(H0, W0, seed=0):
    img, msk = picture(H0, W0, seed=seed, V=V)
    K = camera(H0, W0)
    return img, msk, np.stack([K, K]), np.stack([D_PLUS, D_MINUS])


def _dev(gpu, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in arrays]


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("H0,W0,n", SIZES)
@pytest.mark.parametrize("mask_bkgd,white_bkgd", [(True, False), (True, True), (False, False)])
def test_prepare_views_equals_the_oracle(pp, gpu, H0, W0, n, mask_bkgd, white_bkgd):
    img, msk, K, D = _case(H0, W0)
    ref_img, ref_msk, ref_K = pp.prepare_views_oracle(img, msk, K, D, ratio=1.0 / n, mask_bkgd=mask_bkgd, white_bkgd=white_bkgd)
    out, m, K_out = pp.prepare_views(*_dev(gpu, img, msk, K, D), ratio=1.0 / n, mask_bkgd=mask_bkgd, white_bkgd=white_bkgd)
    assert out.shape == (V, 3, H0 // n, W0 // n) and out.dtype == torch.float32 and out.is_cuda and out.is_contiguous()
    assert m.shape == (V, H0 // n, W0 // n) and m.dtype == torch.uint8
    assert K_out.shape == (V, 3, 3) and K_out.dtype == torch.float32
    out, m = out.cpu().numpy(), m.cpu().numpy()
    bad = int((out.view(np.int32) != ref_img.view(np.int32)).sum())
    bad_m = int((m != ref_msk).sum())
    print(f"{H0} x {W0} / {n}: picture mismatches {bad} (max |d| {np.abs(out - ref_img).max():.3g}), mask mismatches {bad_m}, "
          f"masked pixels {int((ref_msk == 0).sum())}")
    assert bad == 0 and bad_m == 0
    assert np.array_equal(K_out.cpu().numpy(), ref_K)
    assert (ref_msk == 0).any() and len(np.unique(ref_msk)) > 3


def test_prepare_views_takes_arrays_and_column_D(pp, gpu):
    """ndarrays are uploaded; D may be [V,5,1] (the annotation files' shape); ratio and white_bkgd default to cfg"""
    from transhuman_amd.config import get_cfg
    H0, W0, _ = SIZES[0]
    img, msk, K, D = _case(H0, W0, seed=4)
    assert get_cfg().ratio == 0.5 and not get_cfg().white_bkgd
    ref = pp.prepare_views_oracle(img, msk, K, D, ratio=0.5, white_bkgd=False)
    got = pp.prepare_views(img, msk, K, D[..., None])
    assert all(g.is_cuda for g in got)
    assert all(np.array_equal(g.cpu().numpy(), r) for g, r in zip(got, ref))


@pytest.mark.parametrize("H0,W0,n", SIZES)
@pytest.mark.parametrize("border", [0, 5])
def test_combine_masks_equals_the_oracle(pp, gpu, H0, W0, n, border):
    a = np.stack([blob_mask(H0, W0) * 255, blob_mask(H0, W0)[::-1, ::-1] * 7]).astype(np.uint8)
    b = np.zeros_like(a)
    b[0, H0 // 4:H0 // 2, W0 // 2:W0 - 3] = 2
    b[1, :5, :] = 1
    ta, tb = _dev(gpu, a, b)
    one, two = pp.combine_masks(ta, border=border), pp.combine_masks(ta, tb, border=border)
    assert one.dtype == torch.uint8 and one.shape == ta.shape and one.is_cuda
    assert np.array_equal(one.cpu().numpy(), pp.combine_masks_oracle(a, border=border))
    assert np.array_equal(two.cpu().numpy(), pp.combine_masks_oracle(a, b, border=border))
    assert not torch.equal(one, two)
    assert set(np.unique(two.cpu().numpy())) == ({0, 1, 100} if border else {0, 1})
    # one [H0,W0] mask; the inputs are not written
    assert np.array_equal(pp.combine_masks(ta[1], tb[1], border=border).cpu().numpy(), pp.combine_masks_oracle(a[1], b[1], border=border))
    assert np.array_equal(ta.cpu().numpy(), a) and np.array_equal(tb.cpu().numpy(), b)


def test_largest_border(pp, gpu):
    H0, W0, _ = SIZES[0]
    a = blob_mask(H0, W0)
    assert np.array_equal(pp.combine_masks(a, border=15).cpu().numpy(), pp.combine_masks_oracle(a, border=15))


def test_two_calls_give_identical_bits(pp, gpu):
    H0, W0, n = SIZES[0]
    img, msk, K, D = _dev(gpu, *_case(H0, W0, seed=5))
    first = pp.prepare_views(img, msk, K, D, ratio=0.5)
    again = pp.prepare_views(img, msk, K, D, ratio=0.5)
    assert torch.equal(_bits(first[0]), _bits(again[0])) and torch.equal(first[1], again[1]) and torch.equal(first[2], again[2])
    assert torch.equal(pp.combine_masks(msk, border=5), pp.combine_masks(msk, border=5))


def test_input_conversion(pp, gpu):
    """non-contiguous uint8 inputs and float64 K / D are converted; pictures and masks of another type are rejected (a float
    picture would have to be guessed to be 0..1 or 0..255); shapes that do not fit raise"""
    H0, W0, n = SIZES[0]
    img, msk, K, D = _case(H0, W0, seed=6)
    ref = pp.prepare_views_oracle(img, msk, K, D, ratio=0.5)
    t_img, t_msk = _dev(gpu, img, msk)
    chw = t_img.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)             # the same picture, channel-first in memory
    wide = torch.zeros((V, H0, 2 * W0), dtype=torch.uint8, device=gpu)
    wide[:, :, ::2] = t_msk
    assert not chw.is_contiguous() and not wide[:, :, ::2].is_contiguous()
    got = pp.prepare_views(chw, wide[:, :, ::2], torch.from_numpy(K).double().to(gpu), torch.from_numpy(D).double(), ratio=0.5)
    assert all(np.array_equal(g.cpu().numpy(), r) for g, r in zip(got, ref))
    assert np.array_equal(pp.combine_masks(wide[:, :, ::2], border=5).cpu().numpy(), pp.combine_masks_oracle(msk, border=5))
    assert np.array_equal(pp.combine_masks(t_msk != 0, border=5).cpu().numpy(), pp.combine_masks_oracle(msk, border=5))
    with pytest.raises(TypeError, match="uint8"):
        pp.prepare_views(t_img.float() / 255, t_msk, K, D, ratio=0.5)
    with pytest.raises(TypeError, match="uint8"):
        pp.prepare_views(t_img, t_msk.to(torch.int32), K, D, ratio=0.5)
    with pytest.raises(TypeError, match="uint8"):
        pp.combine_masks(t_msk.float())
    with pytest.raises(ValueError):
        pp.prepare_views(t_img, t_msk[:, :-2], K, D, ratio=0.5)
    with pytest.raises(ValueError):
        pp.prepare_views(t_img, t_msk, K[:1], D, ratio=0.5)
    with pytest.raises(ValueError, match="ratio"):
        pp.prepare_views(t_img, t_msk, K, D, ratio=0.3)
    with pytest.raises(ValueError, match="divisible"):
        pp.prepare_views(t_img[:, :, :78], t_msk[:, :, :78], K, D, ratio=0.25)
    with pytest.raises(ValueError, match="border"):
        pp.combine_masks(t_msk, border=4)
    with pytest.raises(ValueError):
        pp.combine_masks(t_msk, t_msk[:1])


def test_c_surface_rejects_bad_arguments(pp, gpu):
    from transhuman_amd import hip
    lib = hip.load_library()
    H0, W0, n = SIZES[0]
    img, msk, K, D = _dev(gpu, *_case(H0, W0))
    lut = torch.from_numpy(pp.unit_table()).to(gpu)
    out = torch.empty((V, 3, H0 // n, W0 // n), dtype=torch.float32, device=gpu)
    out_m = torch.empty((V, H0 // n, W0 // n), dtype=torch.uint8, device=gpu)
    full = torch.empty((V, H0, W0), dtype=torch.uint8, device=gpu)
    ctx, p, s = hip.ctx(gpu), hip._p, hip._stream()

    def views(im=img, mk=msk, k=K, d=D, table=lut, o=out, om=out_m, v=V, h0=H0, w0=W0, fac=n):
        return lib.th_prep_views(ctx, p(im), p(mk), v, h0, w0, p(k), p(d), fac, 1, 0, p(table), p(o), p(om), s)

    def mask(a=msk, b=None, o=full, v=V, h0=H0, w0=W0, border=5):
        return lib.th_prep_mask(ctx, p(a), p(b), v, h0, w0, border, p(o), s)
    assert views() == 0
    for kw in ({"im": None}, {"mk": None}, {"k": None}, {"d": None}, {"table": None}, {"o": None}, {"om": None}):
        assert views(**kw) < 0 and b"null" in lib.th_last_error()
    for fac in (0, 3, 8, -1):
        assert views(fac=fac) < 0 and b"ratio" in lib.th_last_error()
    assert views(fac=4, w0=78) < 0 and b"divisible" in lib.th_last_error()
    assert views(h0=95) < 0 and b"divisible" in lib.th_last_error()
    for kw in ({"v": 0}, {"h0": 0}, {"w0": -2}, {"w0": 16386}):
        assert views(**kw) < 0 and b"size" in lib.th_last_error()
    assert mask() == 0 and mask(b=msk) == 0 and mask(border=0) == 0
    for kw in ({"a": None}, {"o": None}):
        assert mask(**kw) < 0 and b"null" in lib.th_last_error()
    for border in (2, 4, 17, -1):
        assert mask(border=border) < 0 and b"border" in lib.th_last_error()
    assert mask(o=msk) < 0 and b"in place" in lib.th_last_error()
    assert mask(v=0) < 0 and mask(h0=0) < 0
    assert views() == 0 and mask() == 0                                # and the context still works
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), pp.prepare_views_oracle(*_case(H0, W0), ratio=0.5, white_bkgd=False)[0])


# ---- the renderer ---------------------------------------------------------------------------------------------------------
class _Cfg:
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        from transhuman_amd.config import get_cfg
        self.cfg = get_cfg()
        self.old = {k: getattr(self.cfg, k) for k in self.kw}
        for k, val in self.kw.items():
            setattr(self.cfg, k, val)

    def __exit__(self, *exc):
        for k, val in self.old.items():
            setattr(self.cfg, k, val)


def _renderer(gpu):
    from transhuman_amd.networks.renderer import if_clight_renderer
    from util import make_net, synth_assign, can64
    return if_clight_renderer.Renderer(make_net(12).to(gpu), vertex_can=can64().numpy(), pc2voxel_ind=synth_assign(300))


def _snapshot(batch):
    flat = {}
    for k, val in batch.items():
        for i, t in enumerate(val if isinstance(val, (list, tuple)) else [val]):
            if torch.is_tensor(t):
                flat[(k, i)] = (t, t.clone())
    return flat


def test_renderer_prepares_its_input_views(pp, gpu):
    """cfg.input_prep == "device": raw 128 x 128 views + D- in the batch render to the same bits as the same batch with input_imgs /
    input_K filled from prepare_views; the batch is not touched; the default "batch" ignores the raw keys"""
    from transhuman_amd import synth
    from transhuman_amd.config import cfg_get, get_cfg
    assert cfg_get("input_prep", None) == "batch" and get_cfg().ratio == 0.5
    get_cfg().N_samples, get_cfg().num_class = 32, 300
    b = synth.batch_to(synth.make_batch(64, 64, 3, seed=0), gpu)
    nv = b["input_imgs"][0].shape[1]
    assert tuple(b["input_imgs"][0].shape) == (1, nv, 3, 64, 64)
    rng = np.random.default_rng(7)
    y, x = np.mgrid[:128, :128]
    # a smooth picture (the stem sees an image, not noise) under a body-sized mask
    raw = np.stack([np.stack([127.5 + 120 * np.sin(0.05 * (x + 2 * c) + v) * np.cos(0.04 * y - c) for c in range(3)], -1)
                    for v in range(nv)]) + rng.uniform(-4, 4, (nv, 128, 128, 3))
    raw = np.clip(np.rint(raw), 0, 255).astype(np.uint8)
    raw_msk = (((y - 64) / 56.0) ** 2 + ((x - 64) / 30.0) ** 2 < 1).astype(np.uint8)[None].repeat(nv, 0)
    K_raw = b["input_K"][0].clone()
    K_raw[..., :2, :] *= 2                                             # the cameras of the 128 x 128 pictures
    D = torch.from_numpy(np.stack([D_MINUS] * nv)).to(gpu)
    t_raw, t_msk = _dev(gpu, raw, raw_msk)
    imgs, msk, K_out = pp.prepare_views(t_raw, t_msk, K_raw[0], D, ratio=0.5)
    assert torch.equal(K_out, b["input_K"][0][0]) and 0 < int((msk == 0).sum()) < msk.numel()
    fed = dict(b)
    fed["input_imgs"], fed["input_K"] = [imgs[None]], [K_out[None]]
    bare = {k: val for k, val in b.items() if k not in ("input_imgs", "input_K")}
    bare.update(input_imgs_raw=[t_raw[None]], input_msks_raw=[t_msk[None]], input_K_raw=K_raw, input_D=D[None])
    both = dict(b, **{k: bare[k] for k in ("input_imgs_raw", "input_msks_raw", "input_K_raw", "input_D")})
    r = _renderer(gpu)
    with _Cfg(input_prep="batch"):
        want = {k: val.clone() for k, val in r.render_fast(fed, is_train=False).items()}
        plain = {k: val.clone() for k, val in r.render_fast(b, is_train=False).items()}
        ignored = {k: val.clone() for k, val in r.render_fast(both, is_train=False).items()}
        with pytest.raises(KeyError):
            r.render_fast(bare, is_train=False)
    keys, before = set(bare), _snapshot(bare)
    with _Cfg(input_prep="device"):
        got = {k: val.clone() for k, val in r.render_fast(bare, is_train=False).items()}
        over = {k: val.clone() for k, val in r.render_fast(both, is_train=False).items()}       # the raw keys win
        seq = [{k: val.clone() for k, val in o.items()} for o in r.render_sequence([bare, bare])]
        assert r.last_batch is bare
        tok = r.prepare_frame(bare).tokens.clone()
    with _Cfg(input_prep="nowhere"):
        with pytest.raises(ValueError, match="input_prep"):
            r.render_fast(bare, is_train=False)
    torch.cuda.synchronize()
    assert set(bare) == keys
    for (k, i), (t, old) in before.items():
        now = bare[k][i] if isinstance(bare[k], (list, tuple)) else bare[k]
        assert now is t and torch.equal(t, old)
    assert float(want["acc_map"].max()) > 0.05
    for k in ("rgb_map", "acc_map", "depth_map"):
        assert torch.equal(_bits(got[k]), _bits(want[k])), k
        assert torch.equal(_bits(over[k]), _bits(want[k])), k
        assert torch.equal(_bits(ignored[k]), _bits(plain[k])), k
        for o in seq:
            assert torch.equal(_bits(o[k]), _bits(want[k])), k           # (the frame pipeline is a re-ordering: same bits)
    assert not torch.equal(_bits(want["rgb_map"]), _bits(plain["rgb_map"]))                   # the pictures matter
    with _Cfg(input_prep="batch"):
        assert torch.equal(_bits(r.prepare_frame(fed).tokens), _bits(tok))
