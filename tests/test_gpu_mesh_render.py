"""GPU: vertex normals and normal-coloured Phong frames (csrc/k_meshshade.hip, transhuman_amd/mesh_render.py) against the float64 /
int64 numpy restatement of their definition: the int64 normal sums equal at every vertex, normals and covered pixels within 1 fp32
ulp (or 2^-40 absolute where 0.7 n + 0.7 cancels to nearly zero), uncovered pixels exactly the background, no cap on mismatches;
bitwise determinism; marching cubes -> normals -> frame end to end; and the C surface's argument checks."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from test_mesh_render_host import awkward_mesh, octahedron

pytestmark = pytest.mark.gpu

H, W = 96, 128                       # not square: swapped strides would show
BG = (0.25, 0.5, 0.75)


@pytest.fixture(scope="module")
def mr(gpu):
    from transhuman_amd import hip, mesh_render
    hip.load_library()
    return mesh_render


def _dev(gpu, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in arrays]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _far(got, want):
    """bool: NOT within 1 fp32 ulp or 2^-40 absolute, whichever is larger"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    steps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    return (steps > 1) & (np.abs(got.astype(np.float64) - want.astype(np.float64)) > 2.0 ** -40)


@functools.lru_cache(maxsize=None)
def cameras():
    """two ring cameras of H x W; the second is pushed 2.8 m forward and 0.3 m sideways: it stands beside the body, 0.2 m in front
    of its centre plane, so vertices lie behind it, triangles cross its near plane and much of what is left is off-screen"""
    from transhuman_amd import visibility as vz
    R, T, K = vz.ring_cameras(H, W, angles=(0.0, 2.1), focal=110.0)
    T = T.copy()
    T[1, :, 0] += np.array([0.3, 0.0, -2.8], np.float32)
    return R, T, K


@functools.lru_cache(maxsize=None)
def image_oracle(pixel_centre):
    from transhuman_amd import mesh_render, visibility as vz
    v, f = vz.uv_ellipsoid()
    out = mesh_render.render_mesh_oracle(v, f, *cameras(), H, W, pixel_centre=pixel_centre, background=BG)
    for a in out:
        a.setflags(write=False)
    return out


# ---- normals --------------------------------------------------------------------------------------------------------------
def _device_sums_and_normals(mr, gpu, v, f, flip=False):
    """the C entry point with a workspace of the test's own: (int64 sums [nv,3], normals fp32 [nv,3], status)"""
    from transhuman_amd import hip
    lib = hip.load_library()
    tv, tf = _dev(gpu, v, f)
    nv, nf = len(v), len(f)
    ws = torch.empty(lib.th_vertex_normals_workspace_bytes(nv, nf), dtype=torch.uint8, device=gpu)
    n = torch.empty((nv, 3), dtype=torch.float32, device=gpu)
    st = torch.full((1,), 7, dtype=torch.int32, device=gpu)
    assert lib.th_vertex_normals(hip.ctx(gpu), hip._p(tv), nv, hip._p(tf), nf, int(flip), hip._p(n), hip._p(st), hip._p(ws),
                                 ws.numel(), hip._stream()) == 0
    return ws[:nv * 24].view(torch.int64).reshape(nv, 3).cpu().numpy(), n.cpu().numpy(), int(st.item())


@pytest.mark.parametrize("body", ["ellipsoid", "awkward", "octahedron"])
def test_normals_match_oracle(mr, gpu, body):
    from transhuman_amd import visibility as vz
    v, f = {"ellipsoid": vz.uv_ellipsoid, "awkward": lambda: awkward_mesh()[:2], "octahedron": octahedron}[body]()
    sums, n, status = _device_sums_and_normals(mr, gpu, v, f)
    assert status == 0
    assert np.array_equal(sums, mr.normal_sums_oracle(v, f))                         # exact, every vertex
    want = mr.vertex_normals_oracle(v, f)
    far = _far(n, want)
    print(f"{body}: {len(v)} vertices, normals not within 1 ulp: {int(far.sum())}, not bit-equal: {int((n != want).sum())}")
    assert not far.any()
    got = mr.vertex_normals(*_dev(gpu, v, f))
    assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy().view(np.int32), n.view(np.int32))
    flipped = mr.vertex_normals(*_dev(gpu, v, f), flip=True).cpu().numpy()
    assert np.array_equal(flipped, -n) and not _far(flipped, mr.vertex_normals_oracle(v, f, flip=True)).any()
    if body == "awkward":
        _, _, hub, iso = awkward_mesh()
        assert np.array_equal(n[iso].view(np.int32), np.zeros(3, np.int32)) and n[hub, 2] > 0.99
        assert np.array_equal(flipped[iso].view(np.int32), np.zeros(3, np.int32))   # +0.0, also when flipped
    # float64 vertices (a Mesh's) are rounded to fp32 once
    assert torch.equal(_bits(mr.vertex_normals(torch.from_numpy(v.astype(np.float64)).to(gpu), f)), _bits(got))


def test_normals_do_not_depend_on_face_order_or_run(mr, gpu):
    from transhuman_amd import visibility as vz
    for v, f in (vz.uv_ellipsoid(), awkward_mesh()[:2]):
        tv, tf = _dev(gpu, v, f)
        a = mr.vertex_normals(tv, tf)
        assert torch.equal(_bits(a), _bits(mr.vertex_normals(tv, tf)))
        assert torch.equal(_bits(a), _bits(mr.vertex_normals(tv, torch.flip(tf, [0]))))
        perm = torch.from_numpy(np.random.RandomState(1).permutation(len(f))).to(gpu)
        assert torch.equal(_bits(a), _bits(mr.vertex_normals(tv, tf[perm])))


def test_bad_face_index_is_reported_and_stays_in_bounds(mr, gpu):
    from transhuman_amd import hip, visibility as vz
    lib = hip.load_library()
    v, f = vz.uv_ellipsoid(10, 12)
    nv, nf = len(v), len(f)
    nbytes = lib.th_vertex_normals_workspace_bytes(nv, nf)
    assert nbytes >= nv * 24
    tv = torch.from_numpy(v).to(gpu)
    for bad_index in (nv, -1, 2 ** 31 - 1, -2 ** 31):
        bad = f.astype(np.int64)
        bad[nf // 2, 1] = bad_index
        tf = torch.from_numpy(bad.astype(np.int32)).to(gpu)
        with pytest.raises(ValueError, match="face index"):
            mr.vertex_normals(tv, tf)
        # guard bands around the workspace and the output: untouched
        ws_all = torch.full((nbytes + 8192,), 0x5a, dtype=torch.uint8, device=gpu)
        n_all = torch.full((nv * 3 + 2048,), -7.0, dtype=torch.float32, device=gpu)
        st = torch.zeros(1, dtype=torch.int32, device=gpu)
        ws, n = ws_all[4096:4096 + nbytes], n_all[1024:1024 + nv * 3]
        assert lib.th_vertex_normals(hip.ctx(gpu), hip._p(tv), nv, hip._p(tf), nf, 0, hip._p(n), hip._p(st), hip._p(ws), nbytes,
                                     hip._stream()) == 0
        assert int(st.item()) == 1
        assert bool((ws_all[:4096] == 0x5a).all()) and bool((ws_all[4096 + nbytes:] == 0x5a).all())
        assert bool((n_all[:1024] == -7.0).all()) and bool((n_all[1024 + nv * 3:] == -7.0).all())
        # the faulty face added nothing; every other face did
        keep = np.delete(f, nf // 2, 0)
        assert np.array_equal(ws[:nv * 24].view(torch.int64).reshape(nv, 3).cpu().numpy(), mr.normal_sums_oracle(v, keep))
    with pytest.raises((hip.HipError, ValueError), match="face index"):
        mr.render_mesh(tv, tf, *vz.ring_cameras(32, 32, angles=(0.0,), focal=40.0), 32, 32)


def test_range_check_on_the_device(mr, gpu):
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    f = np.array([[0, 1, 2]], np.int32)
    n = mr.vertex_normals(*_dev(gpu, v * 2048, f)).cpu().numpy()                     # 2^62 / 1 exactly: still in range
    assert np.array_equal(n, mr.vertex_normals_oracle(v * 2048, f)) and np.array_equal(n, [[0, 0, 1]] * 3)
    for big, faces in ((v * 2049, f), (v * 2048, np.repeat(f, 2, 0)), (v * np.float32(1e30), f)):
        with pytest.raises(ValueError, match="range"):
            mr.vertex_normals(*_dev(gpu, big, faces))
    bad = v.copy()
    bad[1, 0] = np.inf
    with pytest.raises(ValueError, match="range"):
        mr.vertex_normals(*_dev(gpu, bad, f))


# ---- the image ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pixel_centre", [0.0, 0.5])
def test_image_matches_oracle(mr, gpu, pixel_centre):
    from transhuman_amd import visibility as vz
    v, f = vz.uv_ellipsoid()
    R, T, K = cameras()
    img_ref, d_ref, p_ref = image_oracle(pixel_centre)
    # the second camera does what it was built for
    _, _, z, ok = vz.project_oracle(v, R, T, K)
    assert ok[0].all() and 0 < (~ok[1]).sum() < len(v) and (z[1][ok[1]] > 0).all()
    cov = p_ref >= 0
    assert cov[0].sum() > 500 and cov[1].sum() > 500 and not cov[0].all() and not cov[1].all()
    image, depth, p2f = mr.render_mesh(*_dev(gpu, v, f, R, T, K), H, W, pixel_centre=pixel_centre, background=BG)
    assert image.shape == (2, H, W, 3) and image.dtype == torch.float32 and image.is_contiguous()
    assert depth.shape == (2, H, W) and p2f.shape == (2, H, W) and p2f.dtype == torch.int32
    image, depth, p2f = image.cpu().numpy(), depth.cpu().numpy(), p2f.cpu().numpy()
    far = _far(image[cov], img_ref[cov])
    worst = float(np.abs(image[cov].astype(np.float64) - img_ref[cov]).max())
    print(f"pixel_centre {pixel_centre}: covered {cov.sum((1, 2))}, pix_to_face mismatches {int((p2f != p_ref).sum())}, colours "
          f"not within 1 ulp / 2^-40: {int(far.sum())}, not bit-equal: {int((image[cov] != img_ref[cov]).sum())}, max |diff| "
          f"{worst:.3e}, image range [{image[cov].min():.4f}, {image[cov].max():.4f}]")
    assert np.array_equal(p2f, p_ref)
    assert not _far(np.where(cov, depth, 1.0), np.where(cov, d_ref, 1.0)).any()
    assert not far.any()
    assert np.array_equal(image[~cov], np.broadcast_to(np.asarray(BG, np.float32), image[~cov].shape))
    assert np.isfinite(image).all()


def test_views_are_independent_and_runs_repeat(mr, gpu):
    from transhuman_amd import visibility as vz
    v, f = vz.uv_ellipsoid()
    R, T, K = vz.ring_cameras(H, W, angles=(0.0, 2.1, 4.2), focal=110.0)
    tv, tf, tR, tT, tK = _dev(gpu, v, f, R, T, K)
    a = mr.render_mesh(tv, tf, tR, tT, tK, H, W, pixel_centre=0.5)
    b = mr.render_mesh(tv, tf, tR, tT, tK, H, W, pixel_centre=0.5)
    for x, y in zip(a, b):
        assert torch.equal(_bits(x), _bits(y))
    for view in range(3):
        one = mr.render_mesh(tv, tf, tR[view:view + 1], tT[view:view + 1], tK[view:view + 1], H, W, pixel_centre=0.5)
        for x, y in zip(a, one):
            assert torch.equal(_bits(x[view:view + 1]), _bits(y))
    assert not torch.equal(a[0][0], a[0][1])
    # the light and the material reach the kernel
    c = mr.render_mesh(tv, tf, tR, tT, tK, H, W, pixel_centre=0.5, light=(1.0, -2.0, 0.5), ambient=0.4, diffuse=0.5, specular=0.3,
                       shininess=8)
    want = mr.render_mesh_oracle(v, f, R, T, K, H, W, pixel_centre=0.5, light=(1.0, -2.0, 0.5), ambient=0.4, diffuse=0.5,
                                 specular=0.3, shininess=8)
    assert np.array_equal(c[2].cpu().numpy(), want[2]) and not _far(c[0].cpu().numpy(), want[0]).any()
    assert not torch.equal(c[0], a[0])


# ---- end to end -----------------------------------------------------------------------------------------------------------
def test_marching_cubes_to_frame(mr, gpu, tmp_path):
    """an analytic ball's sigma grid at 32^3 -> hip.marching_cubes -> vertex_normals with the flip render_mesh_sequence chooses:
    every normal points outward; render_mesh of it covers a disc whose centre pixel is lit; the sequence driver writes the frame"""
    from PIL import Image
    from transhuman_amd import hip, visibility as vz
    from transhuman_amd.camera_path import gen_path_virt, synthetic_rig
    from transhuman_amd.evaluator import to_uint8
    from transhuman_amd.mesh import Mesh
    centre, voxel = np.array([0.03, 0.10, 3.0]), 0.05
    g = np.arange(32) - 15.5
    r = np.sqrt(g[:, None, None] ** 2 + g[None, :, None] ** 2 + g[None, None, :] ** 2)
    sigma = torch.from_numpy(np.clip(10.0 - r, 0.0, None).astype(np.float32)).to(gpu)      # dense inside r = 10 voxels
    verts, faces = hip.marching_cubes(sigma, 0.5, scale=(voxel,) * 3, origin=tuple(centre - 15.5 * voxel))
    assert verts.dtype == torch.float64 and verts.shape[0] > 1000
    n = mr.vertex_normals(verts, faces, flip=mr.MARCHING_CUBES_FLIP).cpu().numpy().astype(np.float64)
    radial = verts.cpu().numpy() - centre
    radius = np.linalg.norm(radial, axis=1)
    assert np.abs(radius - 9.5 * voxel).max() < 0.02
    cosine = (n * radial).sum(1) / radius
    print(f"{len(n)} vertices, {len(faces)} faces, n . radial in [{cosine.min():.4f}, {cosine.max():.4f}]")
    assert (cosine > 0).all() and cosine.min() > 0.9
    R, T, K = vz.ring_cameras(64, 64, angles=(0.0,), focal=64.0)
    image, depth, p2f = mr.render_mesh(verts, faces, R, T, K, 64, 64, flip=mr.MARCHING_CUBES_FLIP)
    cov = (p2f[0] >= 0).cpu().numpy()
    yy, xx = np.mgrid[:64, :64]
    dist = np.hypot(xx - 32.0, yy - 32.0)
    rim = 64.0 * np.tan(np.arcsin(9.5 * voxel / 3.0))                    # the silhouette of a ball of 0.475 m seen from 3 m
    assert cov[dist < rim - 1.0].all() and not cov[dist > rim + 1.0].any()
    # the point facing the camera: n = (0, 0, -1), texel (0.7, 0.7, 1.4), d = 2.5 / |(-0.03, 2.9, -2.5)| = 0.65
    px = image[0, 32, 32].cpu().numpy()
    dark = mr.render_mesh(verts, faces, R, T, K, 64, 64, flip=not mr.MARCHING_CUBES_FLIP)[0][0, 32, 32].cpu().numpy()
    print(f"centre pixel {px}, with the other flip {dark}")
    assert abs(px[2] - (0.5 + np.float32(0.3) * 0.65) * 1.4) < 0.03 and abs(px[0] - (0.5 + 0.3 * 0.65) * 0.7) < 0.03
    assert dark[2] < 0.05                                                # facing away: ambient x texel (0.7, 0.7, 0)
    assert bool((image[0][torch.from_numpy(~cov).to(gpu)] == 1.0).all())
    # the sequence driver: flip=None, pytorch3d's grid, <i>.png
    rig = synthetic_rig()
    K1 = K[0]
    frames = list(mr.render_mesh_sequence([Mesh(verts, faces)], rig, K1, 64, 64, out_dir=str(tmp_path), first_frame=5))
    cam = gen_path_virt(rig, render_views=1)[0]
    want = mr.render_mesh(verts, faces, cam[:3, :3][None].astype(np.float32), cam[:3, 3:][None].astype(np.float32), K, 64, 64,
                          pixel_centre=0.5, flip=False)[0][0]
    assert len(frames) == 1 and torch.equal(frames[0], want) and bool((want != 1.0).any())
    assert np.array_equal(np.asarray(Image.open(tmp_path / "5.png")), to_uint8(want.cpu().numpy()))


# ---- the C surface --------------------------------------------------------------------------------------------------------
def test_c_surface_rejects_bad_arguments(mr, gpu):
    from transhuman_amd import hip, visibility as vz
    lib = hip.load_library()
    v, f = vz.uv_ellipsoid(10, 12)
    R, T, K = vz.ring_cameras(32, 48, angles=(0.0, 2.1), focal=40.0)
    tv, tf = _dev(gpu, v, f)
    cams = hip.pack_cams(*_dev(gpu, R, T, K))
    V, nv, nf, h, w = 2, len(v), len(f), 32, 48
    ctx, p, s = hip.ctx(gpu), hip._p, hip._stream()
    nbytes = lib.th_vertex_normals_workspace_bytes(nv, nf)
    assert nbytes >= nv * 24
    assert lib.th_vertex_normals_workspace_bytes(0, nf) == 0 and lib.th_vertex_normals_workspace_bytes(nv, 0) == 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=gpu)
    n = torch.empty((nv, 3), dtype=torch.float32, device=gpu)
    st = torch.empty(1, dtype=torch.int32, device=gpu)

    def normals(verts=tv, faces=tf, out=n, status=st, work=ws, nb=nbytes, n_v=nv, n_f=nf):
        return lib.th_vertex_normals(ctx, p(verts), n_v, p(faces), n_f, 0, p(out), p(status), p(work), nb, s)
    assert normals() == 0 and int(st.item()) == 0
    for kw in ({"verts": None}, {"faces": None}, {"out": None}, {"status": None}, {"work": None}):
        assert normals(**kw) < 0 and b"null" in lib.th_last_error()
    assert normals(nb=nbytes - 1) < 0 and b"workspace" in lib.th_last_error()
    assert normals(n_v=0) < 0 and normals(n_f=0) < 0 and normals(n_f=-3) < 0

    depth, p2f = vz.rasterize_mesh(tv, tf, *_dev(gpu, R, T, K), h, w)
    image = torch.empty((V, h, w, 3), dtype=torch.float32, device=gpu)
    light, bg = (C.c_float * 3)(0.0, 3.0, 0.0), (C.c_float * 3)(1.0, 1.0, 1.0)

    def shade(verts=tv, nrm=n, faces=tf, cam=cams, pf=p2f, L=light, B=bg, out=image, m=64, n_v=nv, n_f=nf, views=V, hh=h, ww=w):
        return lib.th_shade_mesh(ctx, p(verts), p(nrm), n_v, p(faces), n_f, p(cam), views, hh, ww, p(pf), L, B, 0.5, 0.3, 0.2, m,
                                 p(out), s)
    assert shade() == 0
    ok = image.clone()
    for kw in ({"verts": None}, {"nrm": None}, {"faces": None}, {"cam": None}, {"pf": None}, {"L": None}, {"B": None},
               {"out": None}):
        assert shade(**kw) < 0 and b"null" in lib.th_last_error()
    for m in (0, -64, 3, 48, 65):
        assert shade(m=m) < 0 and b"power of two" in lib.th_last_error()
    for m in (1, 2, 128):
        assert shade(m=m) == 0
    for kw in ({"n_v": 0}, {"n_f": 0}, {"views": 0}, {"hh": 0}, {"ww": 0}, {"ww": -1}, {"hh": 16385}):
        assert shade(**kw) < 0
    # entries of pix_to_face that name no face shade as background and read nothing
    wild = p2f.clone()
    wild[0, :4] = nf
    wild[1, :4] = -5
    assert shade(pf=wild) == 0 and bool((image[:, :4] == 1.0).all())
    assert shade() == 0 and torch.equal(image, ok)                     # and the context still works
    torch.cuda.synchronize()
