"""GPU: the mesh rasteriser and the two vertex-visibility rules (csrc/k_raster.hip, transhuman_amd/visibility.py) against the
float64 / int64 numpy restatement of their definition (pix_to_face equal at EVERY pixel, depth within 1 fp32 ulp, visibility
equal at every vertex -- the definition is exact, there is no cap on mismatches), the cooperative path for large triangles,
determinism, get_relative_depth against the reference's own outputs (g21), the renderer's cfg.vizmap_source == "device", and the
C surface's argument checks."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from test_visibility_host import body, body_with_arm, origin_camera, GOLD

pytestmark = pytest.mark.gpu

H = W = 512
# Device time allowed for ONE rasterise + vertex_visibility call of the cooperative-path tests (HIP events around the call).
# tools/raster_time.py measured 0.06 ms for the test body and 0.19 ms behind three image-filling quads, these two tests print 0.25
# and 0.17 ms on a first timed call; a lane that walked an image-filling triangle alone (262 144 pixels of int64 edge functions
# and float64 divisions, one after the other, at ~2 GHz) needs tens of milliseconds.  20 x the measured time sits between the two.
TIME_LIMIT_MS = 5.0


@pytest.fixture(scope="module")
def vz(gpu):
    from transhuman_amd import hip, visibility
    hip.load_library()
    return visibility


def _dev(gpu, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in arrays]


def _ulp_diff(a, b):
    """largest distance in fp32 representation steps between two arrays of positive floats (or equal zeros)"""
    ia = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    ib = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    return int(np.abs(ia - ib).max())


def _check_against_oracle(vz, gpu, verts, faces, R, T, K, h, w, background=0.0):
    d_ref, p_ref, ties = vz.rasterize_oracle(verts, faces, R, T, K, h, w, background=background, return_ties=True)
    tv, tf, tR, tT, tK = _dev(gpu, verts, faces, R, T, K)
    depth, p2f = vz.rasterize_mesh(tv, tf, tR, tT, tK, h, w, background=background)
    vis = vz.vertex_visibility(tv, tf, tR, tT, tK, h, w)
    assert depth.shape == (R.shape[0], h, w) and depth.dtype == torch.float32
    assert p2f.shape == (R.shape[0], h, w) and p2f.dtype == torch.int32
    assert vis.shape == (R.shape[0], len(verts)) and vis.dtype == torch.bool
    p2f, depth, vis = p2f.cpu().numpy(), depth.cpu().numpy(), vis.cpu().numpy()
    n_bad = int((p2f != p_ref).sum())
    ulp = _ulp_diff(np.where(p_ref >= 0, depth, 1.0), np.where(p_ref >= 0, d_ref, 1.0))
    print(f"covered pixels {[(p_ref[v] >= 0).sum() for v in range(len(p_ref))]}  pix_to_face mismatches {n_bad}  "
          f"depth max ulp {ulp}  visible {vis.sum(1)}  tie pixels {int(ties.sum())}")
    assert n_bad == 0
    assert np.array_equal(depth[p_ref < 0], d_ref[p_ref < 0])          # the background value, exactly
    assert ulp <= 1
    assert np.array_equal(vis, vz.vertex_visibility_from_faces_oracle(p_ref, faces, len(verts)))
    return depth, p2f, vis, ties


def test_body_matches_oracle(vz, gpu):
    v, f = body()
    _, p2f, vis, _ = _check_against_oracle(vz, gpu, v, f, *vz.ring_cameras(H, W), H, W)
    assert all(2796 <= c <= 2902 for c in vis.sum(1))


def test_body_and_arm_matches_oracle(vz, gpu):
    v, f, nb = body_with_arm()
    _check_against_oracle(vz, gpu, v, f, *origin_camera(), H, W, background=-1.0)


def test_coarse_body_matches_oracle(vz, gpu):
    v, f = body(True)
    _check_against_oracle(vz, gpu, v, f, *vz.ring_cameras(H, W), H, W)


def test_non_square_image_matches_oracle(vz, gpu):
    v, f = body()
    h, w = 48, 64
    _check_against_oracle(vz, gpu, v, f, *vz.ring_cameras(h, w, focal=75.0), h, w)
    _check_against_oracle(vz, gpu, v, f, *vz.ring_cameras(w, h, focal=75.0), w, h)


def _timed(fn):
    fn()                                                               # (first call: module load)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b)


def test_image_filling_quad(vz, gpu):
    """two triangles that cover all of 512 x 512 in front of the body: the cooperative path owns every pixel, no body vertex is
    visible, and the call stays within the time limit"""
    bv, bf = body()
    quad = np.array([[-1, -1, 2], [1, -1, 2], [1, 1, 2], [-1, 1, 2]], np.float32)      # u, v = 256 -+ 300 at z = 2
    v = np.concatenate([bv, quad])
    nb, nf = len(bv), len(bf)
    f = np.concatenate([bf, np.array([[nb, nb + 1, nb + 2], [nb, nb + 2, nb + 3]], np.int32)])
    R, T, K = origin_camera()
    tv, tf, tR, tT, tK = _dev(gpu, v, f, R, T, K)

    def run():
        depth, p2f = vz.rasterize_mesh(tv, tf, tR, tT, tK, H, W)
        return depth, p2f, vz.visibility_from_faces(p2f, tf, len(v))
    (depth, p2f, vis), ms = _timed(run)
    print(f"image-filling quad over the body: {ms:.3f} ms")
    assert bool((p2f >= nf).all()) and bool((depth == 2.0).all())
    assert not bool(vis[0, :nb].any()) and bool(vis[0, nb:].all())
    assert ms < TIME_LIMIT_MS
    _check_against_oracle(vz, gpu, v, f, R, T, K, H, W)


def test_long_lens_matches_oracle(vz, gpu):
    """focal 6000: triangles tens of pixels wide, all of them on the cooperative path"""
    v, f = body()
    R, T, K = vz.ring_cameras(H, W, focal=6000.0)
    tv, tf, tR, tT, tK = _dev(gpu, v, f, R, T, K)
    _, ms = _timed(lambda: vz.vertex_visibility(tv, tf, tR, tT, tK, H, W))
    print(f"long lens: {ms:.3f} ms")
    assert ms < TIME_LIMIT_MS
    _, p2f, _, _ = _check_against_oracle(vz, gpu, v, f, R, T, K, H, W)
    assert (p2f >= 0).mean() > 0.5


def test_deterministic_and_independent_of_face_order(vz, gpu):
    v, f, nb = body_with_arm()
    R, T, K = vz.ring_cameras(H, W)
    *_, ties = vz.rasterize_oracle(v, f, R, T, K, H, W, return_ties=True)
    assert not ties.any()            # (with two fragments of equal fp32 depth the owner would follow the face numbering)
    tv, tf, tR, tT, tK = _dev(gpu, v, f, R, T, K)
    d1, p1 = vz.rasterize_mesh(tv, tf, tR, tT, tK, H, W)
    d2, p2 = vz.rasterize_mesh(tv, tf, tR, tT, tK, H, W)
    assert torch.equal(p1, p2) and torch.equal(d1.view(torch.int32), d2.view(torch.int32))
    d3, p3 = vz.rasterize_mesh(tv, torch.flip(tf, [0]), tR, tT, tK, H, W)
    back = torch.where(p3 >= 0, len(f) - 1 - p3, p3)
    assert torch.equal(back, p1) and torch.equal(d3.view(torch.int32), d1.view(torch.int32))
    assert torch.equal(vz.vertex_visibility(tv, tf, tR, tT, tK, H, W),
                       vz.vertex_visibility(tv, torch.flip(tf, [0]), tR, tT, tK, H, W))


def test_depth_visibility_against_the_reference(vz, gpu):
    """get_relative_depth (if_clight_renderer.py:75-93) on g21: the reference's own outputs.
    surface_depth and relative_depth within 1e-4 (the project's parity bar); vis_mask equal on every vertex outside the band
    |relative_depth| < 1e-4 of the golden (fewer than 1 % of the vertices by the generator's assertion)."""
    g = np.load(os.path.join(GOLD, "g21_depth_vizmap.npz"))
    tv, tm, tR, tT, tK = _dev(gpu, g["verts"], g["depthmaps"], g["R"], g["T"], g["K"])
    surface, vis, rel = vz.depth_visibility(tv, tm, tR, tT, tK, det=0.07)
    assert surface.shape == (3, 2000) and vis.dtype == torch.bool and rel.dtype == torch.float32
    d_s = float(np.abs(surface.cpu().numpy() - g["surface_depth"]).max())
    d_r = float(np.abs(rel.cpu().numpy() - g["relative_depth"]).max())
    band = np.abs(g["relative_depth"]) < 1e-4
    n_mask = int((vis.cpu().numpy() != g["vis_mask"])[~band].sum())
    print(f"max|surface - ref| {d_s:.2e}  max|relative - ref| {d_r:.2e}  mask mismatches outside the band {n_mask}  "
          f"band {int(band.sum())} of {band.size}")
    assert band.mean() < 0.01
    assert d_s < 1e-4 and d_r < 1e-4
    assert n_mask == 0
    # the batch's own layout [1, V, H, W, 1] (:82) gives the same
    s5, v5, r5 = vz.depth_visibility(tv, tm[None, ..., None], tR[None], tT[None], tK[None])
    assert torch.equal(s5, surface) and torch.equal(v5, vis) and torch.equal(r5, rel)


# ---- the renderer ---------------------------------------------------------------------------------------------------------
def _renderer(gpu, faces=None):
    from transhuman_amd.networks.renderer import if_clight_renderer
    from util import make_net, synth_assign, can64
    return if_clight_renderer.Renderer(make_net(12).to(gpu), vertex_can=can64().numpy(), pc2voxel_ind=synth_assign(300),
                                       faces=faces)


def _mesh_batch(gpu, res=64):
    """the synthetic batch with the test ellipsoid (which has triangles) as the painted input body"""
    from transhuman_amd import synth
    from transhuman_amd.config import get_cfg
    get_cfg().N_samples, get_cfg().num_class = 32, 300
    b = synth.make_batch(res, res, 3, seed=0)
    v, f = body()
    b["input_smpl_vertice"] = [torch.from_numpy(v)[None]]
    return synth.batch_to(b, gpu), v, f


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


def test_renderer_device_vizmap_equals_the_oracle_mask(vz, gpu):
    b, v, f = _mesh_batch(gpu)
    res = b["input_imgs"][0].shape[-1]
    R, T, K = (b[k][0][0].cpu().numpy() for k in ("input_R", "input_T", "input_K"))
    mask = vz.vertex_visibility_oracle(v, f, R, T, K, res, res)
    assert 0 < mask.sum() < mask.size
    r = _renderer(gpu, faces=f)
    with _Cfg(vizmap_source="batch"):
        fed = dict(b)
        fed["input_vizmaps"] = [torch.from_numpy(mask)[None].to(gpu)]
        frame_b = r.prepare_frame(fed)
        tok_b, img_b = frame_b.tokens.clone(), r.render_fast(fed, is_train=False)["rgb_map"].clone()
    with _Cfg(vizmap_source="device"):
        bare = {k: val for k, val in b.items() if k != "input_vizmaps"}
        frame_d = r.prepare_frame(bare)
        tok_d, img_d = frame_d.tokens.clone(), r.render_fast(bare, is_train=False)["rgb_map"].clone()
        assert np.array_equal(r.last_vizmap.cpu().numpy().astype(bool), mask)
    torch.cuda.synchronize()
    assert torch.equal(tok_d.view(torch.int32), tok_b.view(torch.int32))
    assert torch.equal(img_d.view(torch.int32), img_b.view(torch.int32))
    # the mask matters: all-ones gives other tokens
    with _Cfg(vizmap_source="batch"):
        ones = dict(b)
        ones["input_vizmaps"] = [torch.ones_like(fed["input_vizmaps"][0])]
        assert not torch.equal(r.prepare_frame(ones).tokens, tok_b)


def test_renderer_default_is_untouched(vz, gpu):
    """default cfg (vizmap_source "batch"): a renderer that was given faces renders the synthetic batch like one that was not, to
    the bit, and like the reference (g11_render_small); the mask is read from the batch"""
    from transhuman_amd import synth
    from transhuman_amd.config import cfg_get, get_cfg
    from util import gold, maxdiff
    assert cfg_get("vizmap_source", "batch") == "batch"
    get_cfg().N_samples, get_cfg().num_class = 32, 300
    b = synth.batch_to(synth.make_batch(32, 32, 3, seed=0), gpu)
    _, f = body()
    out_f = _renderer(gpu, faces=f).render_fast(b, is_train=False)
    out_0 = _renderer(gpu).render_fast(b, is_train=False)
    for k in ("rgb_map", "acc_map", "depth_map"):
        assert torch.equal(out_f[k].view(torch.int32), out_0[k].view(torch.int32))
    g = gold("g11_render_small")
    assert maxdiff(out_f["rgb_map"][0].cpu(), g["rgb"]) < 1e-4 and maxdiff(out_f["acc_map"][0].cpu(), g["acc"]) < 1e-4
    with pytest.raises(KeyError):
        _renderer(gpu, faces=f).prepare_frame({k: val for k, val in b.items() if k != "input_vizmaps"})


def test_renderer_device_without_faces_raises(vz, gpu):
    b, _, _ = _mesh_batch(gpu, 32)
    with _Cfg(vizmap_source="device"):
        with pytest.raises(ValueError, match="faces"):
            _renderer(gpu).prepare_frame(b)


def test_renderer_depth_vizmap(vz, gpu):
    """cfg.depth_map and cfg.depth_vizmap: the mask is get_relative_depth's (:129-133) -- on the batch's depth maps when it has
    them, else on the rasterised depth"""
    b, v, f = _mesh_batch(gpu)
    res = b["input_imgs"][0].shape[-1]
    R, T, K = b["input_R"][0], b["input_T"][0], b["input_K"][0]
    tv = torch.from_numpy(v).to(gpu)
    depth, _ = vz.rasterize_mesh(tv, f, R, T, K, res, res)
    r = _renderer(gpu, faces=f)
    with _Cfg(vizmap_source="device", depth_map=True, depth_vizmap=True):
        frame = r.prepare_frame({k: val for k, val in b.items() if k != "input_vizmaps"})
        want = vz.depth_visibility(tv, depth, R, T, K)[1]
        assert torch.equal(r.last_vizmap.to(torch.bool), want) and 0 < int(want.sum()) < want.numel()
        tok_raster = frame.tokens.clone()
        given = dict(b)
        given["input_depthmaps"] = [(depth + 0.5 * (depth > 0))[None, ..., None]]       # another surface: another mask
        frame2 = r.prepare_frame(given)
        want2 = vz.depth_visibility(tv, given["input_depthmaps"][0], R, T, K)[1]
        assert torch.equal(r.last_vizmap.to(torch.bool), want2) and not torch.equal(want2, want)
        assert not torch.equal(frame2.tokens, tok_raster)
    with _Cfg(vizmap_source="batch", depth_map=True, depth_vizmap=True):                # "batch": both keys stay ignored
        tok_batch = r.prepare_frame(b).tokens.clone()
    with _Cfg(vizmap_source="batch"):
        assert torch.equal(r.prepare_frame(b).tokens, tok_batch)


# ---- the C surface --------------------------------------------------------------------------------------------------------
def test_c_surface_rejects_bad_arguments(vz, gpu):
    from transhuman_amd import hip
    lib = hip.load_library()
    v, f = body(True)
    R, T, K = vz.ring_cameras(64, 64, focal=75.0)
    tv, tf = _dev(gpu, v, f)
    cams = hip.pack_cams(*_dev(gpu, R, T, K))
    V, nv, nf, h, w = 3, len(v), len(f), 64, 64
    nbytes = lib.th_rasterize_workspace_bytes(V, nv, nf, h, w)
    assert nbytes > V * h * w * 8
    ws = torch.empty(nbytes, dtype=torch.uint8, device=gpu)
    depth = torch.empty((V, h, w), dtype=torch.float32, device=gpu)
    p2f = torch.empty((V, h, w), dtype=torch.int32, device=gpu)
    vis = torch.empty((V, nv), dtype=torch.uint8, device=gpu)
    ctx, p, s = hip.ctx(gpu), hip._p, hip._stream()

    def raster(verts=tv, faces=tf, cam=cams, d=depth, pf=p2f, work=ws, nb=nbytes, n_v=nv):
        return lib.th_rasterize_mesh(ctx, p(verts), n_v, p(faces), nf, p(cam), V, h, w, 0.0, p(d), p(pf), p(work), nb, s)
    assert raster() == 0
    for kw in ({"verts": None}, {"faces": None}, {"cam": None}, {"d": None}, {"pf": None}, {"work": None}):
        assert raster(**kw) < 0 and b"null" in lib.th_last_error()
    assert raster(nb=nbytes - 1) < 0 and b"workspace" in lib.th_last_error()
    bad = tf.clone()
    bad[len(bad) // 2, 1] = nv                                         # one index past the end
    assert raster(faces=bad) < 0 and b"face index" in lib.th_last_error()
    bad[len(bad) // 2, 1] = -1
    assert raster(faces=bad) < 0 and b"face index" in lib.th_last_error()
    assert lib.th_rasterize_workspace_bytes(V, nv, nf, 0, w) == 0 and lib.th_rasterize_workspace_bytes(0, nv, nf, h, w) == 0
    assert raster() == 0                                               # and the context still works
    assert lib.th_vertex_visibility(ctx, p(p2f), p(tf), nf, nv, V, h, w, p(vis), s) == 0
    assert lib.th_vertex_visibility(ctx, None, p(tf), nf, nv, V, h, w, p(vis), s) < 0
    assert lib.th_vertex_visibility(ctx, p(p2f), p(tf), nf, nv, V, h, w, None, s) < 0
    dm = torch.zeros((V, h, w), device=gpu)
    out = [torch.empty((V, nv), dtype=torch.float32, device=gpu), vis, torch.empty((V, nv), dtype=torch.float32, device=gpu)]
    assert lib.th_depth_visibility(ctx, p(tv), nv, p(cams), V, p(dm), h, w, C.c_float(0.07), *[p(o) for o in out], s) == 0
    assert lib.th_depth_visibility(ctx, p(tv), nv, p(cams), V, None, h, w, C.c_float(0.07), *[p(o) for o in out], s) < 0
    torch.cuda.synchronize()
