"""CPU: the definition of the vertex normals and of the normal-coloured Phong image through its float64 / int64
numpy restatement, transhuman_amd.mesh_render.*_oracle -- hand-written normals, the exactness of the integer sums, the range
check, a triangle whose centre pixel has a closed form, the two pixel grids, a back face, and the sequence driver's cameras."""
import functools
import os

import numpy as np
import pytest

from transhuman_amd import mesh_render as mr
from transhuman_amd import visibility as vz
from transhuman_amd.camera_path import gen_path_virt, synthetic_rig

F32 = lambda x: float(np.float32(x))


# ---- bodies shared with tests/test_gpu_mesh_render.py ---------------------------------------------------------------------
def octahedron():
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)
    return v, f


@functools.lru_cache(maxsize=None)
def awkward_mesh():
    """a cone of 512 triangles around one hub vertex (valence 512), a sliver triangle (area ~1e-9), a face of exactly zero area,
    a face that names one vertex twice, and an isolated vertex -> (verts fp32, faces int32, hub index, isolated index)"""
    rs = np.random.RandomState(3)
    ang = 2 * np.pi * np.arange(512) / 512
    ring = np.stack([0.4 * np.cos(ang), 0.4 * np.sin(ang), 3.2 + 0.01 * rs.standard_normal(512)], 1)
    hub = np.array([[0.013, -0.021, 2.9]])
    extra = np.array([[0.5, 0.5, 3.0], [0.9, 0.5000001, 3.0], [0.7, 0.50000004, 3.0],          # sliver
                      [-0.5, 0.5, 3.0], [-0.25, 0.5, 3.0], [-0.125, 0.5, 3.0],                 # collinear: zero area
                      [0.123, 0.456, 2.5]])                                                    # isolated
    v = np.concatenate([hub, ring, extra]).astype(np.float32)
    f = [[0, 1 + k, 1 + (k + 1) % 512] for k in range(512)]
    f += [[513, 514, 515], [516, 517, 518], [513, 516, 516]]
    return v, np.asarray(f, np.int32), 0, 519


def big_triangle(front=True):
    """one triangle at z = 2 in front of origin_camera(focal 20) of 24 x 32: pixel (col 16, row 12) looks at (0, 0, 2)"""
    v = np.array([[-1, -1, 2], [1, -1, 2], [0, 1.5, 2]], np.float32)
    f = np.array([[0, 2, 1]] if front else [[0, 1, 2]], np.int32)         # front: (v1 - v0) x (v2 - v0) = (0, 0, -5), at the camera
    R = np.eye(3, dtype=np.float32)[None]
    T = np.zeros((1, 3, 1), np.float32)
    K = np.array([[[20, 0, 16], [0, 20, 12], [0, 0, 1]]], np.float32)
    return v, f, R, T, K


# ---- normals --------------------------------------------------------------------------------------------------------------
def test_octahedron_normals_are_the_axes():
    v, f = octahedron()
    n = mr.vertex_normals_oracle(v, f)
    assert n.dtype == np.float32 and np.array_equal(n, v)
    assert np.array_equal(mr.vertex_normals_oracle(v, f, flip=True), -v)
    assert np.array_equal(mr.normal_sums_oracle(v, f), (4 * v.astype(np.int64)) << 40)
    # float64 vertices (a Mesh's) are rounded to fp32 once
    v64 = v.astype(np.float64) * (1 + 1e-12)
    assert np.array_equal(mr.vertex_normals_oracle(v64, f), n)


def test_isolated_vertex_and_cancelling_faces_give_zero():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5]], np.float32)
    f = np.array([[0, 1, 2], [0, 2, 1]], np.int32)
    for flip in (False, True):
        n = mr.vertex_normals_oracle(v, f, flip=flip)
        assert np.array_equal(n.view(np.int32), np.zeros((4, 3), np.int32))          # +0.0, also when flipped
    v, f, hub, iso = awkward_mesh()
    n = mr.vertex_normals_oracle(v, f)
    assert np.array_equal(n[iso], [0, 0, 0]) and abs(float(np.linalg.norm(n[hub].astype(np.float64))) - 1) < 1e-6
    assert n[hub, 2] > 0.99                                                          # the cone's axis (ring walked x -> y)
    assert np.array_equal(n[516:519], np.zeros((3, 3)))                              # only zero-area faces


def test_face_order_does_not_change_a_bit():
    for v, f in (vz.uv_ellipsoid(40, 42), awkward_mesh()[:2]):
        a = mr.vertex_normals_oracle(v, f)
        assert np.array_equal(a.view(np.int32), mr.vertex_normals_oracle(v, f[::-1]).view(np.int32))
        perm = np.random.RandomState(0).permutation(len(f))
        assert np.array_equal(mr.normal_sums_oracle(v, f), mr.normal_sums_oracle(v, f[perm]))
        ref = np.cross(v[f[:, 1]].astype(np.float64) - v[f[:, 0]], v[f[:, 2]].astype(np.float64) - v[f[:, 0]])
        s = np.zeros((len(v), 3))
        for k in range(3):
            np.add.at(s, f[:, k], ref)
        # (each face's components are rounded to 2^-41: 512 faces at most per vertex here)
        assert np.abs(mr.normal_sums_oracle(v, f) / mr.SCALE - s).max() < 1e-9


def test_range_check_raises():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    f = np.array([[0, 1, 2]], np.int32)
    mr.vertex_normals_oracle(v * 2048, f)                                   # c = 2^22: 2^62 / 1 exactly, still in range
    with pytest.raises(ValueError, match="range"):
        mr.vertex_normals_oracle(v * 2049, f)
    with pytest.raises(ValueError, match="range"):
        mr.vertex_normals_oracle(v * 2048, np.repeat(f, 2, 0))              # the bound divides by the face count
    with pytest.raises(ValueError, match="range"):
        mr.vertex_normals_oracle(v * np.float32(1e30), f)                   # (c overflows fp64's integers, not fp64)
    bad = v.copy()
    bad[1, 0] = np.inf
    with pytest.raises(ValueError, match="range"):
        mr.vertex_normals_oracle(bad, f)
    with pytest.raises(ValueError, match="face index"):
        mr.vertex_normals_oracle(v, np.array([[0, 1, 3]]))
    with pytest.raises(ValueError, match="face index"):
        mr.vertex_normals_oracle(v, np.array([[0, -1, 2]]))
    # a metre-scale body is five orders of magnitude inside: the largest |c| 2^40 of the SMPL-sized ellipsoid against 2^62 / nf
    bv, bf = vz.uv_ellipsoid()
    e1, e2 = bv[bf[:, 1]].astype(np.float64) - bv[bf[:, 0]], bv[bf[:, 2]].astype(np.float64) - bv[bf[:, 0]]
    assert np.abs(np.cross(e1, e2)).max() * mr.SCALE < 1e-5 * mr.SUM_MAX / len(bf)


# ---- shading --------------------------------------------------------------------------------------------------------------
def _closed_form(light, nz):
    """the definition at the world point (0, 0, 2) of a z = 2 plane with unit normal (0, 0, nz), camera at the origin, by hand"""
    p = np.array([0.0, 0.0, 2.0])
    n = np.array([0.0, 0.0, nz])
    t = np.array([0.7 * 0.0 + 0.7, 0.7 * (0.0 - 0.0) + 0.7, 0.7 * (0.0 - nz) + 0.7])     # F R n = (0, 0, -nz)
    L = np.asarray(light, np.float32).astype(np.float64)
    lh = (L - p) / max(np.sqrt(((L - p) ** 2).sum()), 1e-6)
    vh = (0.0 - p) / 2.0
    d = float(n @ lh)
    s = max(float(vh @ (2 * d * n - lh)), 0.0) ** 64
    return (F32(0.5) + F32(0.3) * max(d, 0.0)) * t + F32(0.2) * (s if d > 0 else 0.0), d, s


def _ulps(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) / np.maximum(np.spacing(np.abs(b).astype(np.float32)).astype(np.float64), 2.0 ** -40)


@pytest.mark.parametrize("light", [mr.LIGHT, (0.0, 0.0, 0.0), (0.3, -0.4, 1.0)])
def test_centre_pixel_of_a_facing_triangle_has_the_closed_form(light):
    v, f, R, T, K = big_triangle()
    bg = (0.25, 0.5, 0.75)
    img, depth, p2f, terms = mr.render_mesh_oracle(v, f, R, T, K, 24, 32, light=light, background=bg, return_terms=True)
    assert img.shape == (1, 24, 32, 3) and img.dtype == np.float32 and depth.shape == p2f.shape == (1, 24, 32)
    assert p2f[0, 12, 16] == 0 and depth[0, 12, 16] == 2.0
    want, d, s = _closed_form(light, -1.0)
    assert d > 0 and abs(terms["d"][0, 12, 16] - d) < 1e-14
    # (the weights b_i are quotients rounded in float64: the sum of three differs from the hand value by ~1e-16 relative)
    assert _ulps(img[0, 12, 16], want).max() <= 1.0
    if tuple(light) == (0.0, 0.0, 0.0):                  # light at the eye, looking straight at the plane: the full highlight
        assert s == 1.0 and abs(terms["specular"][0, 12, 16] - F32(0.2)) < 1e-15
        assert np.allclose(img[0, 12, 16], 0.8 * np.array([0.7, 0.7, 1.4]) + 0.2, atol=1e-6)
    # uncovered pixels: exactly the background
    off = p2f[0] < 0
    assert 0 < off.sum() < off.size and not off[12, 16] and off[0, 0] and off[23, 31]
    assert np.array_equal(img[0][off], np.broadcast_to(np.asarray(bg, np.float32), (int(off.sum()), 3)))
    assert np.isnan(terms["d"][0][off]).all() and (depth[0][off] == 0).all()


def test_texel_is_the_normal_in_the_flipped_camera_frame():
    """a rotated camera: at every covered pixel (colour - specular) / (a + diffuse) = 0.7 F R n + 0.7 for the one normal n"""
    v, f = big_triangle()[:2]
    R, T, K = vz.ring_cameras(24, 32, angles=(0.5,), centre=(0.0, 0.0, 2.0), dist=2.0, focal=20.0)
    img, _, p2f, terms = mr.render_mesh_oracle(v, f, R, T, K, 24, 32, return_terms=True)
    cov = p2f[0] >= 0
    assert cov.sum() > 50
    n = np.array([0.0, 0.0, -1.0])
    want = 0.7 * (np.diag([1.0, -1.0, -1.0]) @ R[0].astype(np.float64) @ n) + 0.7
    got = (img[0][cov] - terms["specular"][0][cov][:, None]) / (F32(0.5) + terms["diffuse"][0][cov])[:, None]
    assert np.abs(got - want).max() < 1e-6


def test_pixel_centre_half_is_a_shifted_K():
    v, f = vz.uv_ellipsoid(10, 12)
    R, T, K = vz.ring_cameras(24, 32, angles=(0.0, 2.0), focal=30.0)
    a = mr.render_mesh_oracle(v, f, R, T, K, 24, 32, pixel_centre=0.5)
    Ks = K.copy()
    Ks[:, 0, 2] -= np.float32(0.5)
    Ks[:, 1, 2] -= np.float32(0.5)
    b = mr.render_mesh_oracle(v, f, R, T, Ks, 24, 32)
    c = mr.render_mesh_oracle(v, f, R, T, K, 24, 32)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert not np.array_equal(a[2], c[2]) and (a[2] >= 0).sum() > 40
    with pytest.raises(ValueError, match="pixel_centre"):
        mr.render_mesh_oracle(v, f, R, T, K, 24, 32, pixel_centre=0.25)
    with pytest.raises(ValueError, match="power of two"):
        mr.render_mesh_oracle(v, f, R, T, K, 24, 32, shininess=48)


def test_back_face_has_no_diffuse_and_no_specular():
    v, f, R, T, K = big_triangle(front=False)
    img, _, p2f, terms = mr.render_mesh_oracle(v, f, R, T, K, 24, 32, return_terms=True)
    cov = p2f[0] >= 0
    assert cov[12, 16] and (terms["d"][0][cov] < 0).all()
    assert (terms["diffuse"][0][cov] == 0).all() and (terms["specular"][0][cov] == 0).all()
    want, d, _ = _closed_form(mr.LIGHT, 1.0)
    assert d < 0 and np.allclose(want, [0.35, 0.35, 0.0], atol=1e-15)
    assert _ulps(img[0, 12, 16], want).max() <= 1.0
    # flip=True turns the same face towards the camera and the light
    lit = mr.render_mesh_oracle(v, f, R, T, K, 24, 32, flip=True)[0]
    assert np.array_equal(lit, mr.render_mesh_oracle(*big_triangle(front=True), 24, 32)[0])


def test_smooth_body_is_lit_from_above():
    """the ellipsoid under the light at (0, 3, 0): vertices whose normal points at the light are brighter than the far side"""
    v, f = vz.uv_ellipsoid(20, 22)
    R, T, K = vz.ring_cameras(48, 48, angles=(0.0,), focal=50.0)
    img, _, p2f, terms = mr.render_mesh_oracle(v, f, R, T, K, 48, 48, return_terms=True)
    d = terms["d"][0]
    rows = np.nonzero((p2f[0] >= 0).any(1))[0]
    # world +y is image-down: the light at y = 3 is below the body's centre (y = 0.1), so d grows down the image
    assert np.nanmean(d[rows[-3:]]) > 0.5 and np.nanmean(d[rows[-3:]]) > np.nanmean(d[rows[:3]]) + 0.3
    assert np.isfinite(img).all() and img.min() >= -1e-6 and img.max() <= 1.4 * 0.8 + 0.2


# ---- the sequence driver ----------------------------------------------------------------------------------------------------
def test_sequence_cameras_are_i_mod_n_along_the_orbit(tmp_path):
    from PIL import Image
    rig = synthetic_rig()
    K = np.array([[50, 0, 16], [0, 50, 12], [0, 0, 1]], np.float64)
    meshes = [vz.uv_ellipsoid(4 + k, 6) for k in range(4)]
    calls = []

    def stub(verts, faces, R, T, Kc, H, W, **kw):
        calls.append((len(verts), R, T, Kc, H, W, kw))
        return np.full((1, H, W, 3), 0.2 * len(calls), np.float32), None, None

    out = list(mr.render_mesh_sequence(meshes, rig, K, 24, 32, out_dir=str(tmp_path / "frames"), first_frame=3, render=stub))
    w2c = gen_path_virt(rig, render_views=4)
    assert len(out) == len(calls) == 4
    for k, (nv, R, T, Kc, H, W, kw) in enumerate(calls):
        cam = w2c[(3 + k) % 4]
        assert nv == len(meshes[k][0]) and (H, W) == (24, 32)
        assert R.shape == (1, 3, 3) and R.dtype == np.float32 and np.array_equal(R[0], cam[:3, :3].astype(np.float32))
        assert T.shape == (1, 3, 1) and np.array_equal(T[0], cam[:3, 3:].astype(np.float32))
        assert np.array_equal(Kc, K.astype(np.float32)[None])
        assert kw == {"pixel_centre": 0.5, "flip": mr.MARCHING_CUBES_FLIP}
        png = np.asarray(Image.open(tmp_path / "frames" / f"{3 + k}.png"))
        assert png.shape == (24, 32, 3) and (png == 51 * (k + 1)).all()
    assert mr.MARCHING_CUBES_FLIP is False
    assert sorted(os.listdir(tmp_path / "frames")) == ["3.png", "4.png", "5.png", "6.png"]
    assert list(mr.render_mesh_sequence([], rig, K, 24, 32)) == []


def test_sequence_through_the_oracle_and_ply_files(tmp_path):
    from transhuman_amd.mesh import Mesh
    rig = synthetic_rig()
    K = np.array([[40, 0, 16], [0, 40, 12], [0, 0, 1]], np.float32)
    v, f = vz.uv_ellipsoid(6, 8)
    path = Mesh(v.astype(np.float64), f).export(str(tmp_path / "0.ply"))
    frames = list(mr.render_mesh_sequence([Mesh(v.astype(np.float64), f), path], rig, K, 24, 32, render=mr.render_mesh_oracle,
                                          flip=True, light=(0.0, 1.0, 0.0)))
    w2c = gen_path_virt(rig, render_views=2)
    for i, frame in enumerate(frames):
        R, T = w2c[i][:3, :3].astype(np.float32)[None], w2c[i][:3, 3:].astype(np.float32)[None]
        want = mr.render_mesh_oracle(v, f, R, T, K[None], 24, 32, pixel_centre=0.5, flip=True, light=(0.0, 1.0, 0.0))[0][0]
        assert frame.shape == (24, 32, 3) and np.array_equal(frame, want)
        assert (frame != 1).any()
