"""GPU: the colour jitter of the raw frames on the device (csrc/k_jitter.hip, transhuman_amd/preprocess.py, K25).  Every operation
is integer arithmetic or single correctly rounded IEEE operations in a fixed order, so every comparison is bit for bit: against the
numpy restatement ``color_jitter_oracle`` (which tests/test_jitter_host.py holds to Pillow), and for the hue against Pillow itself on
the whole 2^24 colour cube -- the case that catches a multiply-add contracted by the compiler.  Then the C surface (workspace
contents, in place, pointer alignment, argument checks), the renderer's cfg.input_jitter and the training entry on a batch of raw
frames."""
import itertools

import numpy as np
import pytest
import torch

from transhuman_amd import config

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (2, 1, 5), (3, 5, 7), (3, 17, 33), (3, 64, 64), (1, 256, 300)]
FULL = ((2, 0, 1, 3), 1.31, 0.58, 1.62, -0.17)                       # brightness and saturation before the contrast mean
NO_CONTRAST = ((3, 2, 0, 1), 0.77, None, 0.41, 0.33)


@pytest.fixture(scope="module")
def pp(gpu):
    from transhuman_amd import hip, preprocess
    hip.load_library()
    return preprocess


def _img(V, H, W, seed=0):
    return np.random.default_rng(1000 * seed + V * H * W).integers(0, 256, (V, H, W, 3), dtype=np.uint8)


def _check(pp, gpu, img, params):
    got = pp.color_jitter(torch.from_numpy(img).to(gpu), params)
    assert got.is_cuda and got.dtype is torch.uint8 and got.shape == img.shape and got.is_contiguous()
    got, ref = got.cpu().numpy(), pp.color_jitter_oracle(img, params)
    bad = int((got != ref).sum())
    print(f"{img.shape} {tuple(params)}: {bad} bytes differ")
    assert bad == 0, (params, int(np.abs(got.astype(int) - ref).max()))
    return got


@pytest.mark.parametrize("V,H,W", SHAPES)
def test_equals_the_oracle(pp, gpu, V, H, W):
    """several shapes have H W 3 not a multiple of 16: view 1 starts unaligned, heads and tails of every length"""
    img = _img(V, H, W)
    a = _check(pp, gpu, img, FULL)
    b = _check(pp, gpu, img, NO_CONTRAST)
    assert H * W < 4 or not (np.array_equal(a, img) or np.array_equal(b, img))
    assert np.array_equal(pp.color_jitter(img[0], FULL).cpu().numpy(), pp.color_jitter_oracle(img[0], FULL))      # an ndarray, [H,W,3]


def test_all_orders(pp, gpu):
    img = _img(3, 17, 33, seed=1)
    seen = set()
    for order in itertools.permutations(range(4)):
        seen.add(_check(pp, gpu, img, (order, 1.4, 0.6, 1.7, -0.21)).tobytes())
    assert len(seen) > 12


@pytest.mark.parametrize("op,values", [(0, (0.2, 2.0, 0.0, 1.0)), (1, (0.3, 2.0, 0.0, 1.0)), (2, (0.2, 2.0, 0.0, 1.0)),
                                       (3, (-0.5, 0.5, 0.0, -0.001))])
def test_each_operation_alone_at_the_ends_of_its_range(pp, gpu, op, values):
    img = _img(3, 17, 33, seed=2)
    for f in values:
        factors = [None] * 4
        factors[op] = f
        _check(pp, gpu, img, ((0, 1, 2, 3), *factors))
    assert torch.equal(pp.color_jitter(img, ((0, 1, 2, 3), None, None, None, None)).cpu(), torch.from_numpy(img))


def test_the_contrast_mean_is_each_views_own(pp, gpu):
    rng = np.random.default_rng(5)
    img = np.stack([rng.integers(lo, lo + 50, (23, 29, 3)) for lo in (0, 100, 205)]).astype(np.uint8)
    params = ((0, 1, 2, 3), None, 0.45, None, None)
    got = _check(pp, gpu, img, params)
    pooled = pp.color_jitter_oracle(img.reshape(1, 69, 29, 3), params).reshape(img.shape)      # one mean over all views: another image
    assert all(not np.array_equal(got[v], pooled[v]) for v in (0, 2))


def test_constant_and_grey_images(pp, gpu):
    """max == min on the way into HSV, S == 0 on the way out"""
    const = np.broadcast_to(np.array([200, 31, 97], np.uint8), (2, 9, 21, 3)).copy()
    ramp = np.broadcast_to((np.arange(2 * 9 * 21) % 256).astype(np.uint8).reshape(2, 9, 21, 1), (2, 9, 21, 3)).copy()
    for img in (const, ramp):
        _check(pp, gpu, img, FULL)
        _check(pp, gpu, img, ((0, 1, 2, 3), None, None, None, 0.3))
        _check(pp, gpu, img, ((0, 1, 2, 3), None, None, 0.0, 0.3))                               # saturation 0 makes every pixel grey first


# ---- the C entry -------------------------------------------------------------------------------------------------------------
def _entry(gpu):
    from transhuman_amd import hip
    lib = hip.load_library()
    ctx, p = hip.ctx(gpu), hip._p

    def call(img, out, V, H, W, params, ws="fit", ws_bytes=None):
        (order, b, c, s, h) = params
        from transhuman_amd import preprocess
        if ws == "fit":
            ws = torch.empty(lib.th_color_jitter_workspace_bytes(V, H, W), dtype=torch.uint8, device=gpu)
        enabled = sum(1 << k for k, f in enumerate((b, c, s, h)) if f is not None)
        return lib.th_color_jitter(ctx, p(img), V, H, W, sum(op << (2 * k) for k, op in enumerate(order)), b or 0.0, c or 0.0, s or 0.0,
                                   0 if h is None else preprocess.hue_shift(h), enabled, p(out), p(ws),
                                   (0 if ws is None else ws.numel()) if ws_bytes is None else ws_bytes, hip._stream())
    return lib, call


def test_nothing_depends_on_what_output_and_workspace_held(pp, gpu):
    lib, call = _entry(gpu)
    V, H, W = 3, 64, 67
    img = _img(V, H, W, seed=3)
    t = torch.from_numpy(img).to(gpu)
    ref = torch.from_numpy(pp.color_jitter_oracle(img, FULL)).to(gpu)
    n_ws = lib.th_color_jitter_workspace_bytes(V, H, W)
    assert n_ws >= V * 8
    torch.manual_seed(8)
    results = []
    for fill in ("random", "ones"):
        for _ in range(2):
            out = torch.randint(0, 256, img.shape, dtype=torch.uint8, device=gpu) if fill == "random" else torch.full_like(t, 0xFF)
            ws = torch.randint(0, 256, (n_ws,), dtype=torch.uint8, device=gpu) if fill == "random" else \
                torch.full((n_ws,), 0xFF, dtype=torch.uint8, device=gpu)
            assert call(t, out, V, H, W, FULL, ws=ws) == 0
            results.append(out)
    assert all(torch.equal(r, ref) for r in results)
    assert torch.equal(t.cpu(), torch.from_numpy(img))                                          # the input is not written
    # without contrast no workspace is needed
    out = torch.empty_like(t)
    assert call(t, out, V, H, W, NO_CONTRAST, ws=None) == 0
    assert torch.equal(out.cpu(), torch.from_numpy(pp.color_jitter_oracle(img, NO_CONTRAST)))


def test_in_place(pp, gpu):
    _, call = _entry(gpu)
    V, H, W = 3, 17, 33
    img = _img(V, H, W, seed=4)
    for params in (FULL, NO_CONTRAST):
        t = torch.from_numpy(img).to(gpu)
        assert call(t, t, V, H, W, params) == 0
        assert torch.equal(t.cpu(), torch.from_numpy(pp.color_jitter_oracle(img, params)))


@pytest.mark.parametrize("off_in,off_out", [(3, 3), (0, 16), (5, 21), (1, 2), (0, 7)])
def test_pointers_of_any_alignment(pp, gpu, off_in, off_out):
    """img and out that agree mod 16 take the wide path behind a head; any other pair takes the narrow path for every pixel"""
    _, call = _entry(gpu)
    V, H, W = 2, 13, 37
    img = _img(V, H, W, seed=5)
    n = img.size
    src = torch.zeros(n + 32, dtype=torch.uint8, device=gpu)
    dst = torch.full((n + 32,), 0xAB, dtype=torch.uint8, device=gpu)
    src[off_in:off_in + n] = torch.from_numpy(img).to(gpu).reshape(-1)
    assert call(src[off_in:], dst[off_out:], V, H, W, FULL) == 0
    assert torch.equal(dst[off_out:off_out + n].cpu(), torch.from_numpy(pp.color_jitter_oracle(img, FULL)).reshape(-1))
    assert bool((dst[:off_out] == 0xAB).all()) and bool((dst[off_out + n:] == 0xAB).all())     # not a byte outside


def test_arguments_are_checked(pp, gpu):
    lib, call = _entry(gpu)
    V, H, W = 2, 8, 8
    img = torch.from_numpy(_img(V, H, W)).to(gpu)
    out = torch.empty_like(img)
    assert call(img, out, V, H, W, FULL) == 0
    assert call(None, out, V, H, W, FULL) < 0 and b"null" in lib.th_last_error()
    assert call(img, None, V, H, W, FULL) < 0 and b"null" in lib.th_last_error()
    for v, h, w in ((V, 0, W), (V, H, -1), (0, H, W), (V, H, 16385), (65536, H, W)):
        assert call(img, out, v, h, w, NO_CONTRAST) < 0 and b"size" in lib.th_last_error()
    assert call(img, out, V, H, W, FULL, ws=None) < 0 and b"workspace" in lib.th_last_error()
    assert call(img, out, V, H, W, FULL, ws_bytes=8) < 0 and b"workspace" in lib.th_last_error()
    assert call(img, out, V, H, W, ((0, 1, 1, 3), 1.0, 1.0, 1.0, 0.0)) < 0 and b"permutation" in lib.th_last_error()
    assert call(img, out, V, H, W, ((0, 1, 2, 3), -1.0, None, None, None)) < 0 and b"factor" in lib.th_last_error()
    assert call(img, out, V, H, W, ((0, 1, 2, 3), float("nan"), None, None, None)) < 0 and b"factor" in lib.th_last_error()
    flat = img.reshape(-1)
    assert call(flat, flat[3:], 1, H, W, NO_CONTRAST) < 0 and b"overlap" in lib.th_last_error()
    with pytest.raises(TypeError, match="uint8"):
        pp.color_jitter(img.float(), FULL)
    with pytest.raises(ValueError, match="shape"):
        pp.color_jitter(img[..., :2], FULL)
    with pytest.raises(ValueError, match="order"):
        pp.color_jitter(img, ((0, 0, 1, 2), 1.0, 1.0, 1.0, 0.0))
    assert call(img, out, V, H, W, FULL) == 0                                                   # and the context still works
    assert torch.equal(out, pp.color_jitter(img, FULL))


# ---- the hue on every colour there is --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def colour_cube():
    """all 2^24 colours as one 4096 x 4096 image, and Pillow's HSV of it"""
    from PIL import Image
    c = np.arange(256, dtype=np.uint8)
    rgb = np.stack(np.meshgrid(c, c, c, indexing="ij"), -1).reshape(4096, 4096, 3)
    return rgb, np.asarray(Image.fromarray(rgb).convert("HSV"))


@pytest.mark.parametrize("d", [0, 77, 255])
def test_hue_on_the_whole_colour_cube_equals_pillow(pp, gpu, colour_cube, d):
    from PIL import Image
    rgb, hsv = colour_cube
    shifted = hsv.copy()
    shifted[..., 0] += np.uint8(d)
    want = torch.from_numpy(np.array(Image.fromarray(shifted, "HSV").convert("RGB")))
    h = (d + 0.5) / 255.0 if d < 128 else (d - 256 - 0.5) / 255.0
    assert pp.hue_shift(h) == d
    got = pp.color_jitter(rgb, ((0, 1, 2, 3), None, None, None, h)).cpu()
    bad = int((got != want).any(-1).sum())
    print(f"d = {d}: {bad} of 2^24 colours differ from Pillow")
    assert bad == 0


# ---- the renderer ----------------------------------------------------------------------------------------------------------
def test_renderer_jitters_its_raw_input_views(pp, gpu):
    """cfg.input_prep = cfg.input_jitter = "device": a batch with only raw 128 x 128 views and a seed renders to the bits of the same
    batch fed color_jitter -> prepare_views by hand, and is not touched; under "batch" the seed is ignored; without a seed nothing
    is jittered"""
    from test_gpu_preprocess import _renderer, _snapshot, _bits
    from test_preprocess_host import D_MINUS
    from transhuman_amd import synth
    with config.override(N_samples=32, num_class=300):
        b = synth.batch_to(synth.make_batch(64, 64, 3, seed=0), gpu)
        nv = b["input_imgs"][0].shape[1]
        rng = np.random.default_rng(7)
        y, x = np.mgrid[:128, :128]
        raw = np.stack([np.stack([127.5 + 120 * np.sin(0.05 * (x + 2 * c) + v) * np.cos(0.04 * y - c) for c in range(3)], -1)
                        for v in range(nv)]) + rng.uniform(-4, 4, (nv, 128, 128, 3))
        raw = torch.from_numpy(np.clip(np.rint(raw), 0, 255).astype(np.uint8)).to(gpu)
        msk = torch.from_numpy((((y - 64) / 56.0) ** 2 + ((x - 64) / 30.0) ** 2 < 1).astype(np.uint8)[None].repeat(nv, 0)).to(gpu)
        K_raw = b["input_K"][0].clone()
        K_raw[..., :2, :] *= 2
        D = torch.from_numpy(np.stack([D_MINUS] * nv)).to(gpu)
        seed = torch.tensor([20261020], dtype=torch.int64)                                      # as a collated batch carries it: on the host
        params = pp.jitter_params(int(seed))
        assert all(f is not None for f in params[1:])

        def fed(frames):
            imgs, _, K_out = pp.prepare_views(frames, msk, K_raw[0], D, ratio=0.5)
            return dict(b, input_imgs=[imgs[None]], input_K=[K_out[None]])
        bare = {k: val for k, val in b.items() if k not in ("input_imgs", "input_K")}
        bare.update(input_imgs_raw=[raw[None]], input_msks_raw=[msk[None]], input_K_raw=K_raw, input_D=D[None], jitter_seed=seed)
        no_seed = {k: val for k, val in bare.items() if k != "jitter_seed"}
        r = _renderer(gpu)
        render = lambda batch: {k: val.clone() for k, val in r.render_fast(batch, is_train=False).items()}
        want, plain = render(fed(pp.color_jitter(raw, params))), render(fed(raw))
        keys, before = set(bare), _snapshot(bare)
        with config.override(input_prep="device", input_jitter="device"):
            got, unseeded = render(bare), render(no_seed)
        with config.override(input_prep="device"):
            assert config.cfg_get("input_jitter") == "batch"
            ignored = render(bare)
        with config.override(input_prep="device", input_jitter="host"), pytest.raises(ValueError, match="input_jitter"):
            r.render_fast(bare, is_train=False)
        torch.cuda.synchronize()
    assert set(bare) == keys and bare["jitter_seed"] is seed
    for (k, i), (t, old) in before.items():
        now = bare[k][i] if isinstance(bare[k], (list, tuple)) else bare[k]
        assert now is t and torch.equal(t, old)
    assert float(want["acc_map"].max()) > 0.05
    for k in ("rgb_map", "acc_map", "depth_map"):
        assert torch.equal(_bits(got[k]), _bits(want[k])), k
        assert torch.equal(_bits(ignored[k]), _bits(plain[k])), k
        assert torch.equal(_bits(unseeded[k]), _bits(plain[k])), k
    assert not torch.equal(_bits(want["rgb_map"]), _bits(plain["rgb_map"]))                   # the jitter matters


# ---- the training entry ----------------------------------------------------------------------------------------------------
def _raw_step(gpu, pp):
    """tests/test_gpu_train_targets.py::_setup with raw 96 x 96 frames for the three input views and the target view: the batch of
    raw keys + seed, and the same batch with the views made by hand (color_jitter -> prepare_views)"""
    from test_gpu_train_targets import _setup, _ellipse
    from test_preprocess_host import D_MINUS, picture
    cfg, net, r, base, target, _ = _setup(gpu)
    H0 = W0 = 96
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    frames, _ = picture(H0, W0, seed=11, V=4)
    y, x = np.mgrid[:H0, :W0]
    in_msk = dev((((y - 48) / 42.0) ** 2 + ((x - 48) / 24.0) ** 2 < 1).astype(np.uint8)[None].repeat(3, 0))
    K_raw = base["input_K"][0].clone()
    K_raw[..., :2, :] *= 2
    D = dev(np.stack([D_MINUS * np.float32(0.2)] * 3))
    tK_raw = target["target_K"].clone()
    tK_raw[..., :2, :] *= 2
    raw = {k: v for k, v in base.items() if k not in ("input_imgs", "input_K")}
    raw.update(input_imgs_raw=[dev(frames[:3])[None]], input_msks_raw=[in_msk[None]], input_K_raw=K_raw, input_D=D[None],
               target_img_raw=dev(frames[3:]), target_msk_raw=dev(((_ellipse(H0, W0) == 1) * 255).astype(np.uint8))[None],
               target_K_raw=tK_raw, target_D=D[:1], target_R=target["target_R"], target_T=target["target_T"],
               patch_draws=target["patch_draws"], jitter_seed=torch.tensor([77], dtype=torch.int64))
    params = pp.jitter_params(77)
    imgs, _, K_out = pp.prepare_views(pp.color_jitter(raw["input_imgs_raw"][0][0], params), in_msk, K_raw[0], D, ratio=0.5)
    m = pp.combine_masks(raw["target_msk_raw"][0], None, border=5)
    t_img, t_msk, t_K = pp.prepare_views(pp.color_jitter(raw["target_img_raw"], params), m[None], tK_raw, D[:1], ratio=0.5)
    assert torch.equal(K_out, base["input_K"][0][0]) and torch.equal(t_K, target["target_K"].to(gpu)) and (t_msk == 100).any()
    hand = {k: v for k, v in raw.items() if not k.endswith("_raw") and k not in ("input_D", "target_D", "jitter_seed")}
    hand.update(input_imgs=[imgs[None]], input_K=[K_out[None]], target_img=t_img.permute(0, 2, 3, 1).contiguous(), target_msk=t_msk,
                target_K=t_K)
    return net, r, raw, hand


def _step(net, r, batch):
    """one forward / backward through Renderer.render: the outputs and every parameter gradient"""
    net.zero_grad(set_to_none=True)
    ret = r.render(batch)
    loss = torch.mean((ret["rgb_map"] - batch["rgb"]) ** 2) + 0.1 * ret["acc_map"].mean() + 0.01 * ret["depth_map"].mean()
    loss.backward()
    out = {k: ret[k].detach().clone() for k in ("rgb_map", "acc_map", "depth_map")}
    grads = {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}
    return out, grads


RUN_TO_RUN = 1e-4


@pytest.mark.parametrize("mode", ["default", "reproducible"])
def test_training_step_on_raw_frames_and_a_seed(pp, gpu, mode):
    """Renderer.render with gradients enabled on a batch that has neither input_imgs nor ray_o -- raw input and target frames plus the
    seed -- under input_prep = target_prep = input_jitter = "device", against the pipeline made by hand: the keys added to the batch
    and the three outputs are torch.equal (torch runs on its deterministic algorithms and MIOpen on its deterministic kernels in
    both modes, as test_gpu_train_targets.py and test_gpu_train_encoder.py do for their comparisons: torch's own forward does not
    otherwise repeat itself), nothing else in the batch changes.  Gradients, "default": the backward of
    the default switches adds with float atomics in an order that changes from run to run, so the two runs -- whose inputs are
    the same bits -- are held to RUN_TO_RUN = 1e-4 of each tensor's largest gradient: a gradient is a sum of up to
    rays x samples x views ~ 2e4 fp32 terms, reordering it moves it by about sqrt(2e4) x 2^-24 ~ 1e-5 of the terms' magnitude, and
    the bar leaves a factor 10 for cancellation while staying 20 times under the 2e-3 the golden training step allows.
    "reproducible": every training switch on its device value and the ordered gather backward
    (tests/test_gpu_latgather_ordered.py::test_the_whole_step_twice_gives_the_same_bits): torch.equal."""
    from test_gpu_train_encoder import ALL_DEVICE, _reproducible_torch
    from transhuman_amd import train_targets
    switches = dict(ALL_DEVICE, train_encoder="device", train_gather_bwd="ordered") if mode == "reproducible" else {}
    cfg = config.get_cfg()
    size = cfg.patch.size
    try:
        net, r, raw, hand = _raw_step(gpu, pp)
        cfg.patch.size = 8
        keys = set(raw)
        kept = {k: (v, v.clone()) for k, v in raw.items() if torch.is_tensor(v)}
        torch.use_deterministic_algorithms(True, warn_only=True)
        with _reproducible_torch():
            with config.override(**{**switches, "target_prep": "device", "input_prep": "batch"}):
                want, want_g = _step(net, r, hand)
            with config.override(**{**switches, "target_prep": "device", "input_prep": "device", "input_jitter": "device"}):
                got, got_g = _step(net, r, raw)
                with config.override(input_jitter="batch"):                                     # the seed ignored: other targets
                    plain = dict({k: v for k, v in raw.items() if k in keys})
                    r.render(plain)
        assert set(raw) - keys == set(train_targets.REFERENCE_KEYS) and "input_imgs" not in raw and "input_K" not in raw
        for k, (t, old) in kept.items():
            assert raw[k] is t and torch.equal(t, old), k
        for k in train_targets.REFERENCE_KEYS:
            assert raw[k].shape == hand[k].shape and torch.equal(raw[k], hand[k]), k
        assert not torch.equal(plain["target_patches"], raw["target_patches"])
        for k in want:
            print(k, float((got[k] - want[k]).abs().max()))
            assert torch.equal(got[k], want[k]), k
        assert set(got_g) == set(want_g) and len(got_g) > 20
        worst = max((float((got_g[k] - want_g[k]).abs().max()) / max(float(want_g[k].abs().max()), 1e-30), k) for k in want_g)
        print(f"{mode}: largest gradient difference / largest gradient = {worst[0]:.3g} ({worst[1]}), {len(got_g)} tensors")
        assert any(float(g.abs().max()) > 0 for g in want_g.values())
        if mode == "reproducible":
            differ = [k for k in want_g if not torch.equal(got_g[k], want_g[k])]
            assert not differ, differ
        else:
            assert worst[0] <= RUN_TO_RUN, worst
    finally:
        torch.use_deterministic_algorithms(False)
        cfg.patch.size = size
        cfg.vit_depth, cfg.N_samples, cfg.perturb, cfg.raw_noise_std = 12, 64, 0.0, 0.0
