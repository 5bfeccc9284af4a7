"""CPU: the rasteriser's definition through its float64 / int64 numpy restatement,
transhuman_amd.visibility.rasterize_oracle -- geometry facts on the 6 890-vertex test ellipsoid (back / front facing vertices,
occlusion by a second body), the top-left rule on a shared edge, the skip rules, and the layout of the g21 golden."""
import functools
import os

import numpy as np

from transhuman_amd import visibility as vz

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CENTRE = np.array([0.03, 0.10, 3.0])
H = W = 512


@functools.lru_cache(maxsize=None)
def body(coarse=False):
    return vz.uv_ellipsoid(40, 42) if coarse else vz.uv_ellipsoid()


def arm():
    """the occluder of the occlusion tests: a thin ellipsoid between the camera at the origin and the body"""
    return vz.uv_ellipsoid(30, 32, radii=(0.07, 0.35, 0.07), centre=CENTRE + np.array([0.10, 0.05, -0.45]))


def origin_camera(focal=600.0, h=H, w=W):
    R = np.eye(3, dtype=np.float32)[None]
    T = np.zeros((1, 3, 1), np.float32)
    K = np.array([[[focal, 0, w / 2.0], [0, focal, h / 2.0], [0, 0, 1]]], np.float32)
    return R, T, K


def body_with_arm():
    bv, bf = body()
    av, af = arm()
    return np.concatenate([bv, av]), np.concatenate([bf, af + len(bv)]), len(bv)


@functools.lru_cache(maxsize=None)
def body_visibility(coarse=False):
    v, f = body(coarse)
    R, T, K = vz.ring_cameras(H, W)
    return vz.vertex_visibility_oracle(v, f, R, T, K, H, W)


def facing(verts, faces, R, T):
    """per view: (min, max) over each vertex's incident faces of n . view, n the unit outward normal, view the unit vector from
    the face's centroid to the camera"""
    v = verts.astype(np.float64)
    n = np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    cen = v[faces].mean(1)
    out = []
    for view in range(R.shape[0]):
        eye = -R[view].astype(np.float64).T @ T[view].astype(np.float64).reshape(3)
        d = eye - cen
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        dot = (n * d).sum(1)
        lo, hi = np.full(len(v), np.inf), np.full(len(v), -np.inf)
        for k in range(3):
            np.minimum.at(lo, faces[:, k], dot)
            np.maximum.at(hi, faces[:, k], dot)
        out.append((lo, hi))
    return out


def test_test_body_has_smpl_counts():
    v, f = body()
    assert v.shape == (6890, 3) and f.shape == (13776, 3) and v.dtype == np.float32 and f.dtype == np.int32
    assert f.min() == 0 and f.max() == 6889


def test_ellipsoid_back_and_front_vertices():
    v, f = body()
    R, T, K = vz.ring_cameras(H, W)
    vis = body_visibility()
    for view, (lo, hi) in enumerate(facing(v, f, R, T)):
        assert not vis[view][hi < 0].any(), "a vertex whose incident faces are all back-facing is visible"
        assert (hi < 0).sum() > 2000
        front = lo > 0.3
        assert front.sum() > 1500
        assert vis[view][front].all(), "a clearly front-facing vertex is invisible"


def test_coarse_ellipsoid_front_vertices():
    v, f = body(True)
    R, T, K = vz.ring_cameras(H, W)
    vis = body_visibility(True)
    for view, (lo, hi) in enumerate(facing(v, f, R, T)):
        assert not vis[view][hi < 0].any()
        assert vis[view][lo > 0.05].all()


def test_visible_share():
    counts = body_visibility().sum(1)
    assert all(2796 <= c <= 2902 for c in counts), counts


def _in_shadow(points, centre, radii):
    """the segment from the origin to each point crosses the ellipsoid"""
    d = points.astype(np.float64) / radii
    o = -np.asarray(centre, np.float64) / radii
    a, b, c = (d * d).sum(1), 2 * (d * o).sum(1), (o * o).sum() - 1.0
    disc = b * b - 4 * a * c
    t = (-b - np.sqrt(np.maximum(disc, 0.0))) / (2 * a)
    return (disc > 0) & (t > 0) & (t < 1)


def test_occlusion_by_a_second_body():
    bv, bf = body()
    allv, allf, nb = body_with_arm()
    R, T, K = origin_camera()
    without = vz.vertex_visibility_oracle(bv, bf, R, T, K, H, W)[0]
    with_arm = vz.vertex_visibility_oracle(allv, allf, R, T, K, H, W)[0][:nb]
    shadow = _in_shadow(bv, CENTRE + np.array([0.10, 0.05, -0.45]), np.array([0.07, 0.35, 0.07]) * 0.85)
    ring_ok = shadow.copy()                          # the vertex and every neighbour across an edge lie in the shadow
    for a, b in ((0, 1), (1, 2), (2, 0)):
        np.logical_and.at(ring_ok, bf[:, a], shadow[bf[:, b]])
        np.logical_and.at(ring_ok, bf[:, b], shadow[bf[:, a]])
    assert ring_ok.sum() > 100 and (ring_ok & without).sum() > 50
    assert not with_arm[ring_ok].any(), "a body vertex behind the arm is visible"
    assert not (with_arm & ~without).any(), "the arm made a body vertex visible"


def _flat(points):
    """vertices at depth 1 under the identity camera: (u, v) = (x, y)"""
    p = np.asarray(points, np.float32)
    verts = np.concatenate([p, np.ones((len(p), 1), np.float32)], 1)
    I = np.eye(3, dtype=np.float32)[None]
    return verts, I, np.zeros((1, 3, 1), np.float32), I


def test_shared_edge_belongs_to_exactly_one_triangle():
    verts, R, T, K = _flat([(2, 2), (10, 2), (10, 10), (2, 10)])       # the diagonal (2,2)-(10,10) runs through pixel centres
    faces = np.array([[0, 1, 2], [0, 2, 3]])
    _, both = vz.rasterize_oracle(verts, faces, R, T, K, 16, 16)
    cover = [vz.rasterize_oracle(verts, faces[k:k + 1], R, T, K, 16, 16)[1][0] >= 0 for k in range(2)]
    assert not (cover[0] & cover[1]).any()
    union = cover[0] | cover[1]
    expect = np.zeros((16, 16), bool)
    expect[2:10, 2:10] = True                                          # top and left edges in, bottom and right edges out
    assert np.array_equal(union, expect)
    diag = np.arange(2, 10)
    assert (both[0][diag, diag] >= 0).all() and (cover[0][diag, diag] ^ cover[1][diag, diag]).all()
    assert np.array_equal(both[0] >= 0, expect)
    _, flipped = vz.rasterize_oracle(verts, faces[:, [0, 2, 1]], R, T, K, 16, 16)
    assert np.array_equal(flipped, both)


def test_skip_rules():
    I = np.eye(3, dtype=np.float32)[None]
    T0 = np.zeros((1, 3, 1), np.float32)
    K = np.array([[[10, 0, 8], [0, 10, 8], [0, 0, 1]]], np.float32)
    tri = np.array([[0, 1, 2]])
    front = np.array([[-0.5, -0.5, 1], [0.5, -0.5, 1], [0, 0.5, 1]], np.float32)
    d, p = vz.rasterize_oracle(front, tri, I, T0, K, 16, 16, background=-1.0)
    assert (p >= 0).sum() > 20 and np.all(d[p >= 0] == 1.0) and np.all(d[p < 0] == -1.0)
    behind = front * np.array([1, 1, -1], np.float32)
    near = front.copy()
    near[2, 2] = 2.0 ** -10                                            # one vertex inside the near limit: z <= 1e-3
    outside = front + np.array([50, 0, 0], np.float32)
    line = np.array([[-0.5, -0.5, 1], [0, 0, 1], [0.5, 0.5, 1]], np.float32)
    for verts in (behind, near, outside, line):
        d, p = vz.rasterize_oracle(verts, tri, I, T0, K, 16, 16)
        assert np.all(p == -1) and np.all(d == 0.0)
        assert not vz.vertex_visibility_oracle(verts, tri, I, T0, K, 16, 16).any()


def test_nearest_fragment_then_lowest_face_wins():
    verts, R, T, K = _flat([(1, 1), (9, 1), (1, 9)])
    far = verts.copy()
    far[:, 2] = 2.0
    far[:, :2] *= 2.0                                                  # same image, twice as far
    v = np.concatenate([far, verts, verts])
    f = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8]])
    d, p, ties = vz.rasterize_oracle(v, f, R, T, K, 12, 12, return_ties=True)
    assert set(np.unique(p)) == {-1, 1} and np.all(d[p == 1] == 1.0)
    assert np.array_equal(ties[0], p[0] == 1)                          # faces 1 and 2 coincide: every pixel is a tie


def test_golden_layout():
    g = np.load(os.path.join(GOLD, "g21_depth_vizmap.npz"))
    V, nv = 3, 2000
    shapes = {"verts": (nv, 3), "R": (V, 3, 3), "T": (V, 3, 1), "K": (V, 3, 3), "depthmaps": (V, 64, 64),
              "surface_depth": (V, nv), "relative_depth": (V, nv), "vis_mask": (V, nv)}
    for name, shape in shapes.items():
        assert g[name].shape == shape, name
        assert g[name].dtype == (np.bool_ if name == "vis_mask" else np.float32), name
    assert (np.abs(g["relative_depth"]) < 1e-4).mean() < 0.01
    assert (g["depthmaps"] == 0).any() and 0 < g["vis_mask"].sum() < V * nv
