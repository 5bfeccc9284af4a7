"""K19 on the device: th_latent_gather / th_latent_gather_bwd (k_latgather.hip) and the training entry with
cfg.train_maps = "latents".

Forward: against the pinned dense device pair th_upsample_concat_nhwc -> th_pixel_gather on the same inputs.  Both evaluate
the same sum of at most 16 taps per element with at most about 12 roundings each, so the bar is derived:
|diff| <= 32 2^-24 sum_taps |coef| |x| per element, the coefficients read out of the new forward with one-hot latents (a
gather of one-hot texels returns the merged coefficients themselves, bit for bit) and, for the colour columns, the grid
weights read out of th_pixel_gather with the identity map.

Backward: the exact adjoint of those coefficients, sum_p coef[p,t] g[p,c] in float64, within (n + 18) 2^-24 sum |coef g|
(n + 2: fp32 summation of n terms in any order plus the product's rounding; 16: the merged coefficient is a sum of at most
four products of three fp32 factors that the two kernels may evaluate in different orders), and exactly 0 where nothing
contributes.

The training entry: the golden step of tests/test_train_path.py with the same bars; every executed encoder parameter against a
float64 run of the "full" torch path, bar 4 x the error of the fp32 "full" torch path (at least 2^-22 of the tensor's maximum);
peak memory."""
import numpy as np
import pytest
import torch

from transhuman_amd import config, synth
from transhuman_amd.networks import autograd_path, train_ops
from transhuman_amd.networks.encoder import SpatialEncoder
from train_step_case import STEP_CFG, check_step, golden, setup

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24
# (H, W), the three latent sizes: the shapes of tests/test_train_maps_host.py
SHAPES = {"20x28": ((20, 28), ((10, 14), (5, 7), (3, 4))), "33x17": ((33, 17), ((17, 9), (9, 5), (5, 3)))}
CH = (64, 64, 128)


@pytest.fixture(scope="module")
def hip(gpu):
    from transhuman_amd import hip as H
    H.load_library()
    return H


def _geometry(hip, gpu, H, W, V):
    b = synth.make_batch(H, W, V, seed=1)
    R, T, K = (b[k][0][0][:V] for k in ("input_R", "input_T", "input_K"))
    scale = hip.feat_scale(SpatialEncoder.feat_scale(H, W), (H, W), gpu)
    return (R, T, K), hip.pack_cams(R.to(gpu), T.to(gpu), K.to(gpu)), scale


def _points(P, seed, R, T, K, scale):
    """around the body: some project inside the image, some beyond its borders (border clamp)"""
    g = torch.Generator().manual_seed(seed)
    pts = torch.randn((P, 3), generator=g) * 0.6 + torch.tensor([0.0, 0.0, 3.0])
    if P >= 17:
        grid = autograd_path.project(pts, R, T, K) * scale.cpu() - 1.0
        outside = (grid.abs() > 1).any(-1)
        assert outside.any() and not outside.all()
    return pts


def _inputs(gpu, H, W, dims, V, seed):
    g = torch.Generator().manual_seed(seed)
    lat = [torch.randn((V, h, w, C), generator=g).to(gpu) for (h, w), C in zip(dims, CH)]       # channels-last
    img = torch.rand((V, 3, H, W), generator=g).to(gpu)
    lift_w, lift_b = torch.randn((128, 3), generator=g).to(gpu), torch.randn(128, generator=g).to(gpu)
    return lat, img, lift_w, lift_b


def _coefficients(hip, gpu, H, W, dims, V, pts, cams, scale):
    """[P,V,h w] per level (float64 numpy): the forward's merged coefficients, read with one-hot latents (channel = texel, 64 or
    128 texels of every level per pass; no image, no lift)"""
    P = pts.shape[0]
    img, zw, zb = torch.zeros((V, 3, H, W), device=gpu), torch.zeros((128, 3), device=gpu), torch.zeros(128, device=gpu)
    coef = [np.zeros((P, V, h * w)) for h, w in dims]
    for k in range(max((h * w + C - 1) // C for (h, w), C in zip(dims, CH))):
        lats = []
        for (h, w), C in zip(dims, CH):
            eye = torch.zeros((h * w, C), device=gpu)
            t = torch.arange(min(k * C, h * w), min((k + 1) * C, h * w), device=gpu)
            eye[t, t - k * C] = 1.0
            lats.append(eye.reshape(1, h, w, C).repeat(V, 1, 1, 1).contiguous())
        rows, _ = hip.latent_gather(*lats, zw, zb, img, pts, cams, scale)
        assert (rows[..., 256:] == 0).all()
        for l, ((h, w), C, c0) in enumerate(zip(dims, CH, (0, 64, 128))):
            n = min((k + 1) * C, h * w) - k * C
            if n > 0:
                coef[l][:, :, k * C:k * C + n] = rows[..., c0:c0 + n].double().cpu().numpy()
    for c in coef:
        if P:
            assert float(np.abs(c.sum(-1) - 1).max()) < 1e-5 and int((c != 0).sum(-1).max()) <= 9 and (c >= 0).all()
    return coef


def _grid_weights(hip, gpu, H, W, V, pts, cams, scale):
    """[P,V,H W] (float64 numpy): K5's bilinear weights, read with the identity map (channel = texel)"""
    n = H * W
    eye = torch.zeros((n, (n + 3) // 4 * 4), device=gpu)
    eye[torch.arange(n), torch.arange(n)] = 1.0
    eye = eye.reshape(1, H, W, -1).repeat(V, 1, 1, 1).contiguous()
    return hip.pixel_gather(eye, pts, cams, scale)[..., :n].double().cpu().numpy()


def _nchw(l):
    return l.permute(0, 3, 1, 2).contiguous()


# ---- forward ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ldo", [384, 400])
@pytest.mark.parametrize("P", [1, 17, 3000])
@pytest.mark.parametrize("V", [1, 3])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_forward_equals_the_dense_device_path(hip, gpu, shape, V, P, ldo):
    (H, W), dims = SHAPES[shape]
    (R, T, K), cams, scale = _geometry(hip, gpu, H, W, V)
    pts = _points(P, 3 + P, R, T, K, scale).to(gpu)
    lat, img, lift_w, lift_b = _inputs(gpu, H, W, dims, V, seed=7)
    dense_map = hip.upsample_concat_nhwc(img, *(_nchw(l) for l in lat), lift_w, lift_b)
    ref = hip.pixel_gather(dense_map, pts, cams, scale)                                  # [P,V,384]
    got, rgb_s = hip.latent_gather(*lat, lift_w, lift_b, img, pts, cams, scale, row_floats=ldo)
    assert got.shape == (P, V, ldo) and rgb_s.shape == (P, V, 4) and torch.isfinite(got[..., :384]).all()
    coef = _coefficients(hip, gpu, H, W, dims, V, pts, cams, scale)
    mag = np.zeros((P, V, 384))
    for l, (c0, C) in enumerate(zip((0, 64, 128), CH)):
        x = lat[l].abs().double().cpu().numpy().reshape(V, -1, C)
        mag[..., c0:c0 + C] = np.einsum("pvt,vtc->pvc", coef[l], x)
    Wt = _grid_weights(hip, gpu, H, W, V, pts, cams, scale)
    rgb = img.double().cpu().numpy().reshape(V, 3, H * W)
    lw, lb = lift_w.abs().double().cpu().numpy(), lift_b.abs().double().cpu().numpy()
    lifted = np.einsum("vkt,ck->vtc", np.abs(rgb), lw) + lb                                 # |r w0| + |g w1| + |b w2| + |bias|
    mag[..., 256:] = np.einsum("pvt,vtc->pvc", Wt, lifted)
    diff = np.abs(got[..., :384].double().cpu().numpy() - ref.double().cpu().numpy())
    tol = 32 * EPS * mag
    worst = float((diff / np.maximum(tol, 1e-300)).max())
    print(f"forward {shape} V={V} P={P} ldo={ldo}: bit-equal to the dense path: {bool((diff == 0).all())} "
          f"(latent columns {bool((diff[..., :256] == 0).all())}, colour columns {bool((diff[..., 256:] == 0).all())}); "
          f"worst difference / bound = {worst:.3f}")
    assert (diff <= tol).all(), worst
    # the blended raw colours, against the same weights
    raw = np.einsum("pvt,vkt->pvk", Wt, rgb)
    d = np.abs(rgb_s[..., :3].double().cpu().numpy() - raw)
    assert (d <= 6 * EPS * np.einsum("pvt,vkt->pvk", Wt, np.abs(rgb))).all() and (rgb_s[..., 3] == 0).all()
    if ldo > 384:                                                   # columns beyond 384 are not touched
        out = torch.full((P, V, ldo), 7.0, device=gpu)
        rs = torch.empty((P, V, 4), device=gpu)
        dims32 = hip._latent_dims([l.shape for l in lat])[1]
        p = hip._p
        hip._check(hip._lib.th_latent_gather(hip.ctx(gpu), p(lat[0]), p(lat[1]), p(lat[2]), dims32, p(img), p(lift_w), p(lift_b), V,
                                             H, W, p(pts), P, p(cams), p(scale), p(out), ldo, p(rs), None))
        torch.cuda.synchronize()
        assert torch.equal(out[..., :384], got[..., :384]) and (out[..., 384:] == 7.0).all()


def test_forward_with_a_one_by_one_level(hip, gpu):
    (H, W), dims, V, P = (12, 16), ((6, 8), (3, 4), (1, 1)), 2, 333
    (R, T, K), cams, scale = _geometry(hip, gpu, H, W, V)
    pts = _points(P, 5, R, T, K, scale).to(gpu)
    lat, img, lift_w, lift_b = _inputs(gpu, H, W, dims, V, seed=8)
    ref = hip.pixel_gather(hip.upsample_concat_nhwc(img, *(_nchw(l) for l in lat), lift_w, lift_b), pts, cams, scale)
    got, _ = hip.latent_gather(*lat, lift_w, lift_b, img, pts, cams, scale)
    coef = _coefficients(hip, gpu, H, W, dims, V, pts, cams, scale)
    assert int((coef[2] != 0).sum(-1).max()) == 1                   # the level's only texel takes every tap
    # columns 128..255: sum of the grid weights (1 up to their rounding) times the texel
    x2 = lat[2].reshape(V, 128)[None].expand(P, V, 128)
    assert float((got[..., 128:256] - x2).abs().max()) <= 8 * EPS * float(lat[2].abs().max())
    assert float((got - ref).abs().max()) <= 32 * EPS * float(ref.abs().max())


# ---- backward -----------------------------------------------------------------------------------------------------------------
def _check_adjoint(got, Wm, g, what, extra=16):
    """tests/test_gpu_train_ops.py::_check_adjoint with the K19 bound: got [V,T,C] device result, Wm [P,V,T] the forward's
    coefficients and g [P,V,C] the upstream gradient (float64)"""
    Wm, g = torch.from_numpy(np.ascontiguousarray(Wm)), torch.from_numpy(np.ascontiguousarray(g))
    spec = "pvt,pvc->vtc"
    ref = torch.einsum(spec, Wm, g).numpy()
    mag = torch.einsum(spec, Wm.abs(), g.abs()).numpy()
    n = np.rint(torch.einsum(spec, (Wm != 0).double(), torch.ones_like(g)).numpy())
    got = got.double().cpu().numpy()
    assert got.shape == ref.shape and np.isfinite(got).all()
    assert (got[n == 0] == 0).all()
    tol = (n + 2 + extra) * EPS * mag
    err = np.abs(got - ref)
    worst = float((err / np.maximum(tol, 1e-300))[n > 0].max()) if (n > 0).any() else 0.0
    print(f"adjoint {what}: n up to {int(n.max())}, worst error / bound = {worst:.3f}")
    assert (err <= tol).all(), worst
    return worst


def _backward_case(hip, gpu, H, W, dims, V, pts, ldo, what):
    (R, T, K), cams, scale = _geometry(hip, gpu, H, W, V)
    pts = pts.to(gpu)
    P = pts.shape[0]
    coef = _coefficients(hip, gpu, H, W, dims, V, pts, cams, scale)
    torch.manual_seed(5)
    g = torch.randn((P, V, ldo), device=gpu)
    shapes = [(V, h, w, C) for (h, w), C in zip(dims, CH)]
    out = tuple(torch.full(s, float("nan"), device=gpu) for s in shapes)        # the call clears the gradients itself
    got = hip.latent_gather_bwd(shapes, (H, W), pts, cams, scale, g, out=out)
    assert all(a is b for a, b in zip(got, out))
    g64 = g.double().cpu().numpy()
    for l, (c0, C) in enumerate(zip((0, 64, 128), CH)):
        _check_adjoint(got[l].reshape(V, -1, C), coef[l], g64[..., c0:c0 + C], f"{what} level {l}")
    # columns 256.. (the lift, the pad) do not reach the latents
    g2 = g.clone()
    g2[..., 256:] = float("nan")
    again = hip.latent_gather_bwd(shapes, (H, W), pts, cams, scale, g2)
    assert all(torch.isfinite(a).all() for a in again)
    return coef


@pytest.mark.parametrize("ldo", [384, 400])
@pytest.mark.parametrize("P", [1, 17, 3000])
@pytest.mark.parametrize("V", [1, 3])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_backward_is_the_adjoint_of_the_forward(hip, gpu, shape, V, P, ldo):
    (H, W), dims = SHAPES[shape]
    (R, T, K), _, scale = _geometry(hip, gpu, H, W, V)
    _backward_case(hip, gpu, H, W, dims, V, _points(P, 3 + P, R, T, K, scale), ldo, f"{shape} V={V} P={P} ldo={ldo}")


def test_backward_many_samples_inside_one_texel(hip, gpu):
    (H, W), dims = SHAPES["20x28"]
    V, P = 3, 3000
    g = torch.Generator().manual_seed(11)
    pts = torch.tensor([[0.02, -0.03, 3.0]]) + (torch.rand((P, 3), generator=g) - 0.5) * 2e-4
    (R, T, K), cams, scale = _geometry(hip, gpu, H, W, V)
    Wt = _grid_weights(hip, gpu, H, W, V, pts.to(gpu), cams, scale)
    for v in range(V):                                              # every sample inside ONE full-resolution texel cell per view
        assert int((Wt[:, v] != 0).any(0).sum()) <= 4 and int((Wt[:, v] != 0).all(0).sum()) >= 1
    coef = _backward_case(hip, gpu, H, W, dims, V, pts, 384, "one texel")
    for c in coef:
        assert int((c[:, 0] != 0).all(0).sum()) >= 1               # a latent texel that takes all 3000 samples


def test_backward_without_samples_writes_zeros(hip, gpu):
    (H, W), dims = SHAPES["33x17"]
    V = 2
    _, cams, scale = _geometry(hip, gpu, H, W, V)
    shapes = [(V, h, w, C) for (h, w), C in zip(dims, CH)]
    out = tuple(torch.full(s, float("nan"), device=gpu) for s in shapes)
    hip.latent_gather_bwd(shapes, (H, W), torch.zeros((0, 3), device=gpu), cams, scale, torch.zeros((0, V, 384), device=gpu), out=out)
    assert all((o == 0).all() for o in out)
    rows, rgb_s = hip.latent_gather(*(torch.zeros(s, device=gpu) for s in shapes), torch.zeros((128, 3), device=gpu),
                                    torch.zeros(128, device=gpu), torch.zeros((V, 3, H, W), device=gpu),
                                    torch.zeros((0, 3), device=gpu), cams, scale)
    assert rows.shape == (0, V, 384) and rgb_s.shape == (0, V, 4)


# ---- the Function: latent and lift gradients ------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,V", [(17, 1), (3000, 3)])
def test_function_gradients_of_the_latents_and_the_lift(hip, gpu, P, V):
    (H, W), dims = SHAPES["20x28"]
    (R, T, K), cams, scale = _geometry(hip, gpu, H, W, V)
    pts = _points(P, 21, R, T, K, scale).to(gpu)
    lat, img, lift_w, lift_b = _inputs(gpu, H, W, dims, V, seed=9)
    leaves = [t.clone().requires_grad_(True) for t in (*lat, lift_w.reshape(128, 3, 1, 1), lift_b)]
    rows = train_ops.LatentGatherFn.apply(*leaves, img, pts, cams, scale)
    direct, rgb_s = hip.latent_gather(*lat, lift_w, lift_b, img, pts, cams, scale)
    assert torch.equal(rows, direct)
    torch.manual_seed(6)
    g = torch.randn_like(rows)
    rows.backward(g)
    assert leaves[3].grad.shape == (128, 3, 1, 1)
    # the latents: the adjoint kernel itself (bounded above), through the Function
    coef = _coefficients(hip, gpu, H, W, dims, V, pts, cams, scale)
    g64 = g.double().cpu().numpy()
    for l, (c0, C) in enumerate(zip((0, 64, 128), CH)):
        _check_adjoint(leaves[l].grad.reshape(V, -1, C), coef[l], g64[..., c0:c0 + C], f"Function level {l}")
    # the lift: g_w = sum g[p,v,256+c] rgb_s[p,v,k], g_b = sum g[p,v,256+c] in float64 from rgb_s and g
    gl, s = g64[..., 256:].reshape(-1, 128), rgb_s.double().cpu().numpy().reshape(-1, 4)[:, :3]
    rows_n = gl.shape[0]
    for name, got, ref, mag in (("lift weight", leaves[3].grad.reshape(128, 3), gl.T @ s, np.abs(gl).T @ np.abs(s)),
                                ("lift bias", leaves[4].grad, gl.sum(0), np.abs(gl).sum(0))):
        err = np.abs(got.double().cpu().numpy() - ref)
        tol = (rows_n + 2) * EPS * mag
        print(f"{name}: {rows_n} rows, worst error / bound = {float((err / tol).max()):.4f}")
        assert (err <= tol).all()


# ---- bad arguments ---------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments(hip, gpu):
    import ctypes
    lib, ctx, p = hip._lib, hip.ctx(gpu), hip._p
    V, H, W, P = 1, 8, 8, 5
    lat = [torch.zeros((V, 4, 4, C), device=gpu) for C in CH]
    img, lw, lb = torch.zeros((V, 3, H, W), device=gpu), torch.zeros((128, 3), device=gpu), torch.zeros(128, device=gpu)
    pts, cams, sc = torch.zeros((P, 3), device=gpu), torch.zeros((V, 21), device=gpu), torch.ones(2, device=gpu)
    out, rs, g = torch.zeros((P, V, 400), device=gpu), torch.zeros((P, V, 4), device=gpu), torch.zeros((P, V, 400), device=gpu)
    dims = lambda *d: (ctypes.c_int32 * 6)(*d)
    ok = dims(4, 4, 4, 4, 4, 4)

    def fwd(d=ok, H=H, W=W, ldo=384, lat0=lat[0], pts_=pts, out_=out, rs_=rs, ctx_=ctx, img_=img):
        return lib.th_latent_gather(ctx_, p(lat0), p(lat[1]), p(lat[2]), d, p(img_), p(lw), p(lb), V, H, W, p(pts_), P, p(cams), p(sc),
                                    p(out_), ldo, p(rs_), None)

    def bwd(d=ok, H=H, W=W, ldo=384, g_=g, g0=lat[0], pts_=pts, ctx_=ctx):
        return lib.th_latent_gather_bwd(ctx_, d, V, H, W, p(pts_), P, p(cams), p(sc), p(g_), ldo, p(g0), p(lat[1]), p(lat[2]), None)

    for call in (fwd, bwd):
        for ldo in (386, 380, 256):
            assert call(ldo=ldo) < 0
            assert b"multiple of 4" in lib.th_last_error()
        for d in (dims(9, 4, 4, 4, 4, 4), dims(4, 4, 4, 9, 4, 4), dims(4, 4, 4, 4, 4, 9), dims(4, 4, 0, 4, 4, 4)):
            assert call(d=d) < 0
            assert b"latent dimensions" in lib.th_last_error()
        assert call(H=65536, W=32768) < 0
        assert b"too large" in lib.th_last_error()
        assert call(ctx_=None) < 0
        assert b"null" in lib.th_last_error()
        assert call(pts_=None) < 0
        assert b"null" in lib.th_last_error()
    for kw in ({"lat0": None}, {"out_": None}, {"rs_": None}, {"img_": None}):
        assert fwd(**kw) < 0
        assert b"null" in lib.th_last_error()
    for kw in ({"g_": None}, {"g0": None}):
        assert bwd(**kw) < 0
        assert b"null" in lib.th_last_error()
    with pytest.raises(ValueError, match="channels-last"):
        hip.latent_gather(lat[0], lat[1], lat[0], lw, lb, img, pts, cams, sc)
    with pytest.raises(ValueError, match="contiguous"):
        hip.latent_gather(lat[0].permute(0, 2, 1, 3), lat[1], lat[2], lw, lb, img, pts, cams, sc)
    torch.cuda.synchronize()


# ---- the training entry -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernels", ["torch", "device"])
def test_training_step_on_the_latents_matches_the_reference(hip, gpu, kernels):
    """tests/test_train_path.py::test_training_step_matches_the_reference with cfg.train_maps = "latents": the same golden step
    of the real reference, the same bars"""
    with config.override(**STEP_CFG, train_maps="latents", train_kernels=kernels):
        check_step(golden(), *setup(gpu))


def _tail_rows(enc, images, verts, xyz, R, T, K, maps):
    """the encoder's part of a training step as autograd_path.render runs it: encode -> painting rows [V,N,192] and pixel rows
    [P,V,384]"""
    image_shape = images.shape[-2:]
    if maps == "latents":
        from transhuman_amd import hip
        gather = autograd_path.latent_features(enc, images, hip.pack_cams(R, T, K),
                                               hip.feat_scale(enc.feat_scale(*image_shape), image_shape, images.device))
        return autograd_path._lin(enc.reduction_layer, gather(verts)).permute(1, 0, 2), gather(xyz)
    hol, pix = autograd_path.encode(enc, images)
    painted = autograd_path.sample_map(hol, autograd_path.project(verts, R, T, K), enc, image_shape).permute(0, 2, 1)
    return painted, autograd_path.sample_map(pix, autograd_path.project(xyz, R, T, K), enc, image_shape).permute(2, 0, 1)


def _encoder_grads(enc, images, verts, xyz, R, T, K, maps, g_paint, g_pix):
    enc.zero_grad(set_to_none=True)
    painted, f = _tail_rows(enc, images, verts, xyz, R, T, K, maps)
    ((painted * g_paint.to(painted)).sum() + (f * g_pix.to(f)).sum()).backward()
    return {k: p.grad.detach().double().cpu() for k, p in enc.named_parameters() if p.grad is not None}


def test_every_encoder_parameter_vs_float64(hip, gpu):
    """The encoder's part of the synthetic step (its images, input vertices, cameras and ray samples; a seeded upstream
    gradient on the painting rows and the pixel rows in place of the rest of the network, which has no float64 form): the
    gradient of every executed encoder parameter with cfg.train_maps = "latents" against a float64 run of the "full" torch path;
    bar: 4 x the error of the fp32 "full" torch path on the same device against the same float64, at least 2^-22 of the
    tensor's maximum."""
    import copy
    with config.override(**STEP_CFG) as cfg:
        net, r, b = setup(gpu)
        S = int(cfg.N_samples)
        ray_o, ray_d, near, far = b["ray_o"][0], b["ray_d"][0], b["near"][0], b["far"][0]
        z = autograd_path.sample_depths(near, far, S, False)
        xyz = (ray_o[:, None] + ray_d[:, None] * z[..., None]).reshape(-1, 3)
        images = b["input_imgs"][0].reshape(-1, *b["input_imgs"][0].shape[2:])
        V = images.shape[0]
        R, T, K = (b[k][0].reshape(V, *sh) for k, sh in (("input_R", (3, 3)), ("input_T", (3, 1)), ("input_K", (3, 3))))
        verts = b["input_smpl_vertice"][0][0]
        gen = torch.Generator().manual_seed(4)
        g_paint = torch.randn((V, verts.shape[0], 192), generator=gen)
        g_pix = torch.randn((xyz.shape[0], V, 384), generator=gen)
        enc = net.encoder
        state = copy.deepcopy(enc.state_dict())                    # (train-mode BatchNorm moves its running statistics)
        enc64 = copy.deepcopy(enc).double().cpu().train()
        cpu64 = lambda t: t.double().cpu()
        t64 = _encoder_grads(enc64, cpu64(images), cpu64(verts), cpu64(xyz), cpu64(R), cpu64(T), cpu64(K), "full",
                             g_paint.double(), g_pix.double())
        full = _encoder_grads(enc, images, verts, xyz, R, T, K, "full", g_paint.to(gpu), g_pix.to(gpu))
        enc.load_state_dict(state)
        lat = _encoder_grads(enc, images, verts, xyz, R, T, K, "latents", g_paint.to(gpu), g_pix.to(gpu))
        executed = [k for k in t64 if k.startswith("model.")] + [k for k in t64 if k.startswith(("upsample_color", "reduction_layer"))]
        assert len(executed) == len(t64) and any("layer2" in k for k in executed) and not any("layer3" in k for k in executed)
        assert set(lat) == set(t64) == set(full)
        misses = []
        for k in executed:
            scale = float(t64[k].abs().max())
            parent = float((full[k] - t64[k]).abs().max())
            err = float((lat[k] - t64[k]).abs().max())
            bar = 4.0 * max(parent, 2.0 ** -22 * scale)
            print(f"{k}: latents {err / scale:.3e}, torch fp32 full {parent / scale:.3e} of max|ref| = {scale:.3e}; err / bar = {err / bar:.3f}")
            if not err <= bar:
                misses.append((k, err / bar))
        assert not misses, misses


def test_peak_memory_is_lower_by_at_least_one_pixel_map(hip, gpu):
    """V = 3, 128 x 128, P = 4 096: forward + backward of the encoder's part of a step; the "full" path holds the pixel map, hol
    and both gradients, the "latents" path none of them"""
    V, H, W, P = 3, 128, 128, 4096
    torch.manual_seed(0)
    enc = SpatialEncoder().to(gpu).train()
    b = synth.batch_to(synth.make_batch(H, W, V, seed=0), gpu)
    images = b["input_imgs"][0].reshape(-1, *b["input_imgs"][0].shape[2:])
    R, T, K = (b[k][0].reshape(V, *sh) for k, sh in (("input_R", (3, 3)), ("input_T", (3, 1)), ("input_K", (3, 3))))
    verts = b["input_smpl_vertice"][0][0]
    xyz = verts[torch.randint(0, verts.shape[0], (P,), device=gpu)] + 0.02 * torch.randn((P, 3), device=gpu)
    g_paint, g_pix = torch.randn((V, verts.shape[0], 192), device=gpu), torch.randn((P, V, 384), device=gpu)
    peak = {}
    for maps in ("latents", "full"):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        _encoder_grads(enc, images, verts, xyz, R, T, K, maps, g_paint, g_pix)
        torch.cuda.synchronize()
        peak[maps] = torch.cuda.max_memory_allocated() - base
        enc.zero_grad(set_to_none=True)
    one_map = V * 384 * H * W * 4
    print(f"peak allocated above the inputs: full {peak['full'] / 2 ** 20:.1f} MiB, latents {peak['latents'] / 2 ** 20:.1f} MiB, "
          f"one pixel map {one_map / 2 ** 20:.1f} MiB")
    assert peak["full"] - peak["latents"] >= one_map, peak
