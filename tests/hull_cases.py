"""Adversarial vertex / sample sets for K1 (transhuman_amd/csrc/k_hull.hip) and a numpy restatement of its vertex grid.

The restatement follows the kernel's own fp32 expressions (grid_build_kernel: gmin, h, inv_h, dim; cell_coord; vert_cell).  It is
used for ONE thing: to prove, on the CPU, that a case reaches the branch it is named for (a sample a few ulp from the threshold,
in the layer of cells around the grid, next to a cell of exactly 8 / 9 / 64 / 65 vertices, in a grid whose cell was enlarged by
the extent rule).  It is never the reference of a result: that is oracle.th_oracle.hull_mask, exact brute force --
(dx*dx + dy*dy) + dz*dz in fp32, correctly rounded sqrt, < fp32 thresh.

Shared by tests/test_hull_cases_host.py (preconditions) and tests/test_gpu_hull_mask.py (device against the reference)."""
import functools
from collections import namedtuple

import numpy as np
import torch

from oracle import th_oracle as O
from transhuman_amd import synth

F = np.float32
GRID_MAX_DIM = 64
GRID_MAX_CELLS = GRID_MAX_DIM ** 3
HULL_PROBE = 8
H0_FACTOR = F(1.05)
BAND = F(4e-6)

Case = namedtuple("Case", "name verts pts thresh")
# rays instead of points: the samples are O.sampling_points(ray_o, ray_d, near, far, S, t_rand) (t_rand: the jitter form, or None)
RayCase = namedtuple("RayCase", "name verts ray_o ray_d near far S t_rand thresh")
Grid = namedtuple("Grid", "gmin h inv_h dim ncell")


# ---- the grid, restated ------------------------------------------------------------------------------------------------
def cell_coord(x, gmin, inv_h):
    """cell_coord: floorf((x - gmin) * inv_h), clamped in float to [-2, GRID_MAX_DIM + 1] (NaN -> -2), then to int"""
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.floor((np.asarray(x, F) - gmin) * inv_h)
    assert c.dtype == F
    return np.fmin(np.fmax(c, F(-2)), F(GRID_MAX_DIM + 1)).astype(np.int64)


def grid_setup(verts, thresh, h0_factor=H0_FACTOR):
    """thread 0 of grid_build_kernel: box of the vertices, h = max(thresh * 1.05, ext / 62), dim = cell of the maximum + 1"""
    verts = np.asarray(verts, F)
    gmin, gmax = verts.min(0), verts.max(0)
    ext = F(max(F(0), (gmax - gmin).max()))
    h0 = F(F(thresh) * F(h0_factor))
    h = F(max(h0, F(ext / F(GRID_MAX_DIM - 2))))
    inv_h = F(F(1) / h)
    dim = np.clip(cell_coord(gmax, gmin, inv_h) + 1, 1, GRID_MAX_DIM)
    return Grid(gmin=gmin, h=h, inv_h=inv_h, dim=dim, ncell=int(np.prod(dim)))


def vert_cells(grid, verts):
    """vert_cell: [nv,3] cell coordinates, clamped into the grid"""
    return np.clip(cell_coord(verts, grid.gmin, grid.inv_h), 0, grid.dim - 1)


def sample_cells(grid, pts):
    """-> ([P,3] cell coordinates as both mask kernels compute them, [P] bool: inside the grid extended by one layer)"""
    c = cell_coord(pts, grid.gmin, grid.inv_h)
    return c, ((c >= -1) & (c <= grid.dim)).all(1)


def linear(grid, c):
    return (c[..., 2] * grid.dim[1] + c[..., 1]) * grid.dim[0] + c[..., 0]


# ---- the reference and its by-products ---------------------------------------------------------------------------------
def _t(a):
    return torch.from_numpy(np.array(a, F))          # (a copy: the cases' arrays are read-only)


def nearest(pts, verts):
    """(fp32 d2 to the nearest vertex, its index): the oracle's own expression (knn_points_exact, K = 1)"""
    d2, idx = O.knn_points_exact(_t(pts), _t(verts), 1)
    return d2[:, 0].numpy(), idx[:, 0].numpy()


def d2_min(pts, verts):
    return nearest(pts, verts)[0]


def d64_min(pts, verts, chunk=4096):
    """float64 distance to the nearest vertex"""
    p, v = np.asarray(pts, np.float64), np.asarray(verts, np.float64)
    out = np.empty(p.shape[0])
    for s in range(0, p.shape[0], chunk):
        d = p[s:s + chunk, None, :] - v[None, :, :]
        out[s:s + chunk] = np.sqrt((d * d).sum(-1).min(1))
    return out


def count_within(pts, verts, thresh, chunk=4096):
    """how many vertices pass the reference's predicate, per sample"""
    p, v = _t(pts), _t(verts)
    out = np.empty(p.shape[0], np.int64)
    for s in range(0, p.shape[0], chunk):
        pp = p[s:s + chunk]
        dx, dy, dz = (pp[:, None, a] - v[None, :, a] for a in range(3))
        d2 = dx * dx + dy * dy
        d2 = d2 + dz * dz
        out[s:s + chunk] = (d2.double().sqrt().float() < thresh).sum(1).numpy()      # (the sqrt of O.hull_mask)
    return out


def band_of(d2, thresh):
    """samples whose nearest d2 the kernel decides by the square root: t2lo <= d2 < t2hi, the kernel's fp32 expressions"""
    t = F(thresh)
    t2 = F(t * t)
    return (d2 >= F(t2 * F(F(1) - BAND))) & (d2 < F(t2 * F(F(1) + BAND)))


def sqrt_decided(d2, thresh):
    """samples where `d2 < fl(thresh * thresh)` and `sqrt(d2) < thresh` disagree: only the exact square-root rule is right"""
    t = F(thresh)
    return (d2 < F(t * t)) != (np.sqrt(d2, dtype=F) < t)


# ---- 1. threshold shell -------------------------------------------------------------------------------------------------
SHELL_K = tuple(range(-48, 49, 3))


def _directions(rs, n_random):
    """the 26 axis / edge / corner directions and n_random random ones, unit length, float64"""
    g = np.array([(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)], np.float64)
    r = rs.normal(size=(n_random, 3))
    u = np.concatenate([g, r])
    return u / np.linalg.norm(u, axis=1, keepdims=True)


def _shell_pts(verts, u, thresh, ks=SHELL_K):
    """v + u * thresh * (1 + k 2^-22) for every vertex, direction and k: formed in float64, rounded to fp32"""
    r = float(F(thresh)) * (1.0 + np.asarray(ks, np.float64) * 2.0 ** -22)
    p = verts.astype(np.float64)[:, None, None, :] + u[None, :, None, :] * r[None, None, :, None]
    return p.reshape(-1, 3).astype(F)


def _lattice(rs, thresh, origin):
    """64 isolated vertices: a 4 x 4 x 4 lattice of spacing 4 thresh, jittered by up to 0.4 thresh per axis"""
    ax = np.arange(4, dtype=np.float64) * 4.0 * thresh
    v = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3) + rs.uniform(-0.4, 0.4, (64, 3)) * thresh
    return (v + np.asarray(origin, np.float64)).astype(F)


def _shell(name, thresh, origin, seed):
    rs = np.random.RandomState(seed)
    verts = _lattice(rs, thresh, origin)
    return Case(name, verts, _shell_pts(verts, _directions(rs, 38), thresh), thresh)


SHELL_SETS = {f"shell_t{t}_o{o}": (t, (o, o, o), 100 + i) for i, (t, o) in
              enumerate((t, o) for t in (0.1, 0.05, 0.3) for o in (0, 1.0))}
SHELL_FAR = {"shell_far_a": (0.1, (37.5, -12.0, 3.0), 110), "shell_far_b": (0.1, (1000.0, 1000.0, 1000.0), 111)}


# ---- 2. cell populations ------------------------------------------------------------------------------------------------
POP_N = (1, 7, 8, 9, 63, 64, 65, 72, 73, 129, 200)
POP_THRESH = 0.1
POP_PITCH = 0.0065           # >= 0.05 thresh; 15 columns x 14 rows = 210 >= 200 fit into one 0.105 cell


def pop_layout(n):
    """-> (verts [n + 2], patch [n + 2] bool, pts [4 n], role [4 n]): n vertices in the cell (2, 2, 2) of a grid spanned by two
    anchor vertices, as a planar patch just above the cell's floor; per vertex a sample 0.999 thresh above it (same cell:
    "near_own"), one 0.999 thresh below it (the cell underneath: "near_nbr") and the same two at 1.001 thresh ("far_*")"""
    rs = np.random.RandomState(200 + n)
    h = float(F(F(POP_THRESH) * H0_FACTOR))
    k = np.arange(n)
    patch = np.stack([2 * h + 0.005 + (k % 15) * POP_PITCH, 2 * h + 0.005 + (k // 15) * POP_PITCH, np.full(n, 2 * h + 0.002)], -1)
    anchors = np.array([[0.0, 0.0, 0.0], [5 * h, 5 * h, 5 * h]])
    verts = np.concatenate([patch, anchors])
    is_patch = np.arange(n + 2) < n
    order = rs.permutation(n + 2)
    verts, is_patch = verts[order].astype(F), is_patch[order]
    pv = verts[is_patch].astype(np.float64)
    t = float(F(POP_THRESH))
    pts, role = [], []
    for sign, dist, r in ((1, 1 - 1e-3, "near_own"), (-1, 1 - 1e-3, "near_nbr"), (1, 1 + 1e-3, "far_own"), (-1, 1 + 1e-3, "far_nbr")):
        pts.append(pv + np.array([0.0, 0.0, sign * t * dist]))
        role += [r] * n
    pts, role = np.concatenate(pts).astype(F), np.array(role)
    order = rs.permutation(4 * n)
    return verts, is_patch, pts[order], role[order]


def _pop(n):
    verts, _, pts, _ = pop_layout(n)
    return Case(f"pop{n}", verts, pts, POP_THRESH)


# ---- 3. grid border ------------------------------------------------------------------------------------------------------
BORDER_BOX = np.array([1.04, 0.62, 0.83])      # the maximum corner sits near the top of its cell in x, y and z (h = 0.105)
SIDES = tuple((a, s) for a in range(3) for s in (-1, 1))


def _border():
    """vertices on the faces, edges and corners of their own box [0, BORDER_BOX]; samples in shells around them (half of those
    outside the box), in the second layer of cells outside the grid on each of the six sides, and at +-1e6"""
    rs = np.random.RandomState(300)
    L = BORDER_BOX
    corners = np.array([(x, y, z) for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float64)
    edges = []
    for a in range(3):
        for b0 in (0, 1):
            for c0 in (0, 1):
                e = np.empty((10, 3))
                e[:, a] = rs.uniform(0, 1, 10)
                e[:, (a + 1) % 3], e[:, (a + 2) % 3] = b0, c0
                edges.append(e)
    faces = []
    for a, s in SIDES:
        f = rs.uniform(0, 1, (40, 3))
        f[:, a] = 0 if s < 0 else 1
        faces.append(f)
    verts = (np.concatenate([corners] + edges + faces) * L).astype(F)
    verts = verts[rs.permutation(verts.shape[0])]
    assert (verts == verts.max(0)).all(1).any()                                     # a vertex exactly at the maximum corner
    u = _directions(rs, 14)
    r = 0.1 * np.array([0.3, 0.7, 0.95, 0.999, 1.001, 1.1])
    shell = (verts.astype(np.float64)[:, None, None, :] + u[None, :, None, :] * r[None, None, :, None]).reshape(-1, 3)
    shell = shell[rs.permutation(shell.shape[0])[:9000]]
    h = float(F(F(0.1) * H0_FACTOR))
    grid = grid_setup(verts, 0.1)
    top = grid.dim * h                                                              # where the layer `dim` begins
    second = []
    for a, s in SIDES:
        p = rs.uniform(-0.1, 0.1, (60, 3)) + rs.uniform(0, 1, (60, 3)) * L
        p[:, a] = rs.uniform(-2 * h + 1e-4, -h - 1e-4, 60) if s < 0 else top[a] + rs.uniform(h + 1e-4, 2 * h - 1e-4, 60)
        second.append(p)
    far = np.array([[s * 1e6 if a == b else 0.3 for b in range(3)] for a, s in SIDES] + [[1e6] * 3, [-1e6] * 3, [1e6, -1e6, 0.0]])
    pts = np.concatenate([shell] + second + [far]).astype(F)
    return Case("border", verts, pts[rs.permutation(pts.shape[0])], 0.1)


# ---- 4. extent rule and degenerate sets ---------------------------------------------------------------------------------
def _body_verts():
    return synth.make_batch(16, 16, 3, seed=0)["tar_smpl_vertice"][0].numpy().astype(F)


def _with_samples(name, verts, thresh, seed, n_uniform=3000):
    """a small threshold shell around 32 of the vertices + uniform points in the bounding box widened by 2 h"""
    rs = np.random.RandomState(seed)
    pick = verts[rs.permutation(verts.shape[0])[:32]]
    shell = _shell_pts(pick, _directions(rs, 6), thresh, ks=range(-48, 49, 12))
    h = float(grid_setup(verts, thresh).h)
    lo, hi = verts.min(0).astype(np.float64) - 2 * h, verts.max(0).astype(np.float64) + 2 * h
    uni = rs.uniform(lo, hi, (n_uniform, 3)).astype(F)
    pts = np.concatenate([shell, uni])
    return Case(name, verts, pts[rs.permutation(pts.shape[0])], thresh)


def _single():
    return _with_samples("single", np.array([[0.3, -0.2, 1.1]], F), 0.1, 400)


def _coincident():
    return _with_samples("coincident65", np.tile(np.array([[-0.7, 0.45, 2.0]], F), (65, 1)), 0.1, 401)


def _line(axis):
    """500 vertices on a 10 m line along one axis, both ends included"""
    rs = np.random.RandomState(402 + axis)
    t = np.concatenate([[0.0, 10.0], rs.uniform(0, 10, 498)])
    v = np.tile(np.array([[0.25, -1.5, 2.0]]), (500, 1))
    v[:, axis] += t[rs.permutation(500)]
    return _with_samples("line_" + "xyz"[axis], v.astype(F), 0.1, 405 + axis)


def _plane():
    """2000 vertices in the plane z = 1.25, 8 m x 5 m, corners included"""
    rs = np.random.RandomState(408)
    xy = np.concatenate([[[0, 0], [8, 5], [0, 5], [8, 0]], rs.uniform(0, 1, (1996, 2)) * [8, 5]])
    v = np.concatenate([xy - [4.0, 1.0], np.full((2000, 1), 1.25)], 1)
    return _with_samples("plane", v[rs.permutation(2000)].astype(F), 0.1, 409)


def _cube():
    """2000 vertices in a 20 m cube, two opposite corners included: 63^3 cells, just under GRID_MAX_CELLS"""
    rs = np.random.RandomState(410)
    v = np.concatenate([[[0, 0, 0], [20, 20, 20]], rs.uniform(0, 20, (1998, 3))]) - [10.0, 10.0, 5.0]
    return _with_samples("cube20", v[rs.permutation(2000)].astype(F), 0.1, 411)


def _body_shifted():
    v = (_body_verts().astype(np.float64) + [37.5, -12.0, 3.0]).astype(F)
    return _with_samples("body_shifted", v, 0.1, 412, n_uniform=1500)


ENLARGED = {"line_x": (63, 1, 1), "line_y": (1, 63, 1), "line_z": (1, 1, 63), "plane": (63, 39, 1), "cube20": (63, 63, 63)}


# ---- 5. sample counts and the ray form -----------------------------------------------------------------------------------
POINT_COUNTS = (1, 63, 64, 65, 255, 256, 257)


def _count(P):
    """the first P samples of one fixed set on the synthetic body (vertices pushed out by 0 .. 0.4 m in random directions)"""
    rs = np.random.RandomState(500)
    v = _body_verts()
    u = rs.normal(size=(257, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    pts = v[rs.randint(0, v.shape[0], 257)].astype(np.float64) + u * rs.uniform(0.0, 0.4, (257, 1))
    return Case(f"count{P}", v, pts[:P].astype(F), 0.1)


RAY_BATCH = dict(H=24, W=24, V=3, seed=0, focal=75.0)
RAY_SETS = {"rays_1x64": (1, 64, False), "rays_17x7": (17, 7, True), "rays_33x96": (33, 96, False), "rays_250x64": (250, 64, False),
            # (the sets of the small-frame rule only)
            "rays_15x7": (15, 7, False), "rays_16x64": (16, 64, False), "rays_17x64": (17, 64, False)}
RAY_FORM = ("rays_1x64", "rays_17x7", "rays_33x96", "rays_250x64")
RULE_SETS = ("rays_1x64", "rays_15x7", "rays_16x64", "rays_17x64", "rays_250x64")


@functools.lru_cache(maxsize=None)
def _ray_batch():
    return synth.make_batch(**RAY_BATCH)


def _rays(name):
    """R rays of the synthetic frame: the centre pixel first, then a seeded draw of the others"""
    R, S, jitter = RAY_SETS[name]
    b = _ray_batch()
    n = b["ray_o"][0].shape[0]
    centre = (RAY_BATCH["H"] // 2) * RAY_BATCH["W"] + RAY_BATCH["W"] // 2
    rest = np.random.RandomState(510).permutation(n)
    idx = np.concatenate([[centre], rest[rest != centre]])[:R]
    t_rand = torch.from_numpy(np.random.RandomState(511).uniform(0, 1, (R, S)).astype(F)) if jitter else None
    g = lambda k: b[k][0][torch.from_numpy(idx)].contiguous()
    return RayCase(name, b["tar_smpl_vertice"][0].numpy().astype(F), g("ray_o"), g("ray_d"), g("near"), g("far"), S, t_rand, 0.1)


def _rays_miss():
    """16 rays that pass the body at a distance: the frame's rays moved 3 m sideways"""
    c = _rays("rays_16x64")
    return c._replace(name="rays_miss", ray_o=c.ray_o + torch.tensor([3.0, 0.0, 0.0]))


# ---- samples that are not finite (needs the clamp in cell_coord) ---------------------------------------------------------
def _nonfinite():
    """NaN, +-inf and +-3e38 in one, two or all three coordinates, every third sample, among ordinary ones"""
    c = _count(257)
    rs = np.random.RandomState(600)
    pts = c.pts.copy()
    bad = np.array([np.nan, np.inf, -np.inf, 3e38, -3e38], F)
    rows = np.arange(0, 257, 3)
    for j, i in enumerate(rows):
        axes = [(0,), (1,), (2,), (0, 1), (1, 2), (0, 1, 2)][j % 6]
        for a in axes:
            pts[i, a] = bad[(j + a) % 5]
    return Case("nonfinite", c.verts, pts, 0.1)


# ---- registry -------------------------------------------------------------------------------------------------------------
_MAKERS = {}
_MAKERS.update({k: (lambda k=k, a=a: _shell(k, *a)) for k, a in {**SHELL_SETS, **SHELL_FAR}.items()})
_MAKERS.update({f"pop{n}": (lambda n=n: _pop(n)) for n in POP_N})
_MAKERS.update({"border": _border, "single": _single, "coincident65": _coincident, "line_x": lambda: _line(0),
                "line_y": lambda: _line(1), "line_z": lambda: _line(2), "plane": _plane, "cube20": _cube,
                "body_shifted": _body_shifted})
_MAKERS.update({f"count{P}": (lambda P=P: _count(P)) for P in POINT_COUNTS})
FINITE_CASES = tuple(_MAKERS)
_MAKERS["nonfinite"] = _nonfinite
CASES = tuple(_MAKERS)
POP_CASES = tuple(f"pop{n}" for n in POP_N)
DEGENERATE = ("single", "coincident65", "line_x", "line_y", "line_z", "plane", "cube20", "body_shifted")
_RAY_MAKERS = {k: (lambda k=k: _rays(k)) for k in RAY_SETS}
_RAY_MAKERS["rays_miss"] = _rays_miss


@functools.lru_cache(maxsize=None)
def case(name):
    c = _MAKERS[name]()
    assert c.name == name and c.verts.dtype == F and c.pts.dtype == F and c.verts.shape[1] == 3 and c.pts.shape[1] == 3
    assert np.isfinite(c.verts).all() and (name == "nonfinite" or np.isfinite(c.pts).all())
    assert c.pts.shape[0] * c.verts.shape[0] < 3e8
    c.verts.setflags(write=False); c.pts.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def ray_case(name):
    c = _RAY_MAKERS[name]()
    assert c.name == name and c.ray_o.dtype == torch.float32 and c.ray_o.shape == (c.near.shape[0], 3)
    return c


@functools.lru_cache(maxsize=None)
def ray_pts(name):
    """[R,S,3] fp32: the samples where the reference places them (bit-exact with the device: test_sampling_and_hull_mask_bit_exact)"""
    c = ray_case(name)
    pts, _ = O.sampling_points(c.ray_o, c.ray_d, c.near, c.far, c.S, c.t_rand)
    return pts


def ray_z(name):
    """[R,S] the explicit depths of the jitter form (what th_points.z_vals takes), or None"""
    c = ray_case(name)
    return None if c.t_rand is None else O.sampling_points(c.ray_o, c.ray_d, c.near, c.far, c.S, c.t_rand)[1]


@functools.lru_cache(maxsize=None)
def grid_of(name):
    c = case(name)
    return grid_setup(c.verts, c.thresh)


@functools.lru_cache(maxsize=None)
def ref_of(name):
    """bool [P] of oracle.th_oracle.hull_mask: computed once, shared by every test, never modified"""
    c = case(name)
    m = O.hull_mask(_t(c.pts), _t(c.verts), c.thresh).numpy()
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def ray_ref_of(name):
    """bool [R,S] of oracle.th_oracle.hull_mask on the reference's sample positions"""
    c = ray_case(name)
    m = O.hull_mask(ray_pts(name).reshape(-1, 3), _t(c.verts), c.thresh).view(-1, c.S).numpy()
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def nearest_of(name):
    """(fp32 d2 to the nearest vertex [P], its index [P]) of the exact oracle"""
    c = case(name)
    d2, idx = nearest(c.pts, c.verts)
    d2.setflags(write=False); idx.setflags(write=False)
    return d2, idx


def d2_of(name):
    return nearest_of(name)[0]


def describe(verts, pts, thresh, i):
    """for an assertion message: sample i, its fp32 d2 to the nearest vertex (and thresh^2), its cell and the grid"""
    g = grid_setup(verts, thresh)
    p = np.asarray(pts, F).reshape(-1, 3)[i:i + 1]
    c, inside = sample_cells(g, p)
    t = F(thresh)
    return (f"sample {i} at {p[0].tolist()}: fp32 d2 to the nearest vertex {float(d2_min(p, verts)[0])!r} (thresh^2 {float(F(t * t))!r}), "
            f"cell {c[0].tolist()} of dim {g.dim.tolist()} (h {float(g.h)!r}, in the extended grid: {bool(inside[0])})")
