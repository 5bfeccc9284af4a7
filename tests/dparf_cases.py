"""Adversarial centre sets for K4 (transhuman_amd/csrc/k_dparf.hip) and a numpy restatement of its candidate grid.

The restatement follows the kernel's own fp32 expressions (dpgrid_setup_kernel, dpgrid_fill_kernel, phase 1 of dparf_kernel).
It is used for ONE thing: to prove, on the CPU, that a case reaches the branch of the grid it is named for (growth loop,
overflowing slot, air cell, point outside the box, disabled grid).  It is never the reference of a result: the reference of
the selection is oracle.th_oracle.knn_points_exact, the reference of the values a float64 evaluation.

Shared by tests/test_dparf_cases_host.py (preconditions, superset property), tests/test_gpu_dparf_knn.py (full scan against
the oracle, grid against full scan) and tests/test_gpu_train_ops.py (the forward's weight matrix)."""
import functools
from collections import namedtuple

import numpy as np
import torch

from oracle import th_oracle as O

F = np.float32
DP_K = 7
DPG_MAXCELLS = 32768
DPG_STRIDE = 192
DPG_CELL = F(0.075)
DPG_MARGIN = F(0.25)
BODY_STD = np.array([0.18, 0.45, 0.10])

Case = namedtuple("Case", "name cen pts rot")
Grid = namedtuple("Grid", "gmin g inv_g dim ncell grown")
Cells = namedtuple("Cells", "cell kind count lists lists64")   # per point; kind: see KINDS
KINDS = ("disabled", "outside", "air", "overflow", "listed")


# ---- the grid, restated ------------------------------------------------------------------------------------------------
def grid_setup(cen):
    """dpgrid_setup_kernel: box of the centres + margin, cell size from the token density, grown until the grid fits"""
    cen = np.asarray(cen, F)
    nc = cen.shape[0]
    mn, mx = cen.min(0), cen.max(0)
    ext = (mx - mn) + F(2) * DPG_MARGIN
    g = F(min(max(DPG_CELL * np.cbrt(F(500) / F(nc), dtype=F), F(0.04)), F(0.12)))
    grown = 0
    for _ in range(32):
        n = int(np.prod(np.ceil(ext / g).astype(np.int64)))
        if n <= DPG_MAXCELLS:
            break
        g = F(g * F(1.25))
        grown += 1
    dim = np.maximum(1, np.ceil(ext / g).astype(np.int64))
    n = int(np.prod(dim))
    return Grid(gmin=(mn - DPG_MARGIN).astype(F), g=g, inv_g=F(1) / g, dim=dim,
                ncell=n if (n <= DPG_MAXCELLS and nc >= DP_K) else 0, grown=grown)


def point_cells(grid, pts):
    """phase 1 of dparf_kernel: cell index of every point, -1 outside the box (or with the grid disabled)"""
    pts = np.asarray(pts, F)
    if grid.ncell == 0:
        return np.full(pts.shape[0], -1, np.int64)
    c = np.floor((pts - grid.gmin) * grid.inv_g).astype(np.int64)
    inside = ((c >= 0) & (c < grid.dim)).all(1)
    cell = (c[:, 2] * grid.dim[1] + c[:, 1]) * grid.dim[0] + c[:, 0]
    return np.where(inside, cell, -1)


def cell_lists(grid, cen, cells):
    """dpgrid_fill_kernel for the given cells -> {cell: (kind, count, list, list64)}: `list` holds the centres within `rad` as
    the kernel computes it in fp32; `list64` the centres within d7(q) + 2h in float64 without any margin (the set the proof
    speaks of)"""
    cen = np.asarray(cen, F)
    g, dim = grid.g, grid.dim
    h = F(0.8660254) * g
    skip = F(0.30) + F(0.8660254) * g
    out = {}
    for cell in cells:
        cx, cy, cz = cell % dim[0], (cell // dim[0]) % dim[1], cell // (dim[0] * dim[1])
        q = grid.gmin + (np.array([cx, cy, cz], F) + F(0.5)) * g
        d = q[None, :] - cen
        dsq = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        if dsq.min() > skip * skip:
            out[cell] = ("air", -1, None, None)
            continue
        pv = np.partition(dsq, DP_K - 1)[DP_K - 1]
        rad = np.sqrt(pv, dtype=F) * F(1.0001) + F(2) * h * F(1.0001) + F(1e-5)
        lst = np.nonzero(dsq <= rad * rad)[0]
        d64 = np.sqrt(((q.astype(np.float64)[None, :] - cen.astype(np.float64)) ** 2).sum(1))
        lst64 = np.nonzero(d64 <= np.partition(d64, DP_K - 1)[DP_K - 1] + 2.0 * 0.8660254037844386 * float(g))[0]
        out[cell] = ("listed" if lst.size <= DPG_STRIDE else "overflow", int(lst.size) if lst.size <= DPG_STRIDE else -1, lst,
                     lst64)
    return out


def classify(cen, pts):
    """-> (Grid, Cells): which branch of phase 1 every point takes"""
    grid = grid_setup(cen)
    cell = point_cells(grid, pts)
    per_cell = cell_lists(grid, cen, np.unique(cell[cell >= 0]))
    kind, count, lists, lists64 = [], [], [], []
    for c in cell:
        if c < 0:
            k = ("disabled" if grid.ncell == 0 else "outside", -1, None, None)
        else:
            k = per_cell[int(c)]
        kind.append(k[0]); count.append(k[1]); lists.append(k[2]); lists64.append(k[3])
    return grid, Cells(cell=cell, kind=np.array(kind), count=np.array(count), lists=lists, lists64=lists64)


def fractions(cells):
    return {k: float((cells.kind == k).mean()) for k in KINDS}


# ---- the cases -----------------------------------------------------------------------------------------------------------
def _rots(rs, nc):
    """cluster-mean blend rotations: an orthogonal matrix shrunk by the averaging, spectral norm <= 1"""
    q, _ = np.linalg.qr(rs.normal(size=(nc, 3, 3)))
    return (q * rs.uniform(0.6, 1.0, (nc, 1, 1))).reshape(nc, 9).astype(F)


def _body_centres(nc, seed=0):
    return (np.random.RandomState(1000 + seed + nc).normal(size=(nc, 3)) * BODY_STD).astype(F)


def _near(rs, cen, P, std=0.05):
    return (cen[rs.randint(0, cen.shape[0], P)] + rs.normal(0, std, (P, 3))).astype(F)


def _body(nc, P):
    rs = np.random.RandomState(nc)
    cen = _body_centres(nc)
    return Case(f"body{nc}", cen, _near(rs, cen, P), _rots(rs, nc))


def _spread():
    rs = np.random.RandomState(21)
    cen = rs.uniform(-2.5, 2.5, (500, 3)).astype(F)
    return Case("spread", cen, _near(rs, cen, 3003), _rots(rs, 500))


def _tight():
    rs = np.random.RandomState(22)
    blob_at = np.array([0.05, 0.30, 0.02])
    cen = np.concatenate([_body_centres(1100), (blob_at + rs.normal(0, 0.02, (400, 3))).astype(F)])
    cen = cen[rs.permutation(1500)]
    P = 3999
    pts = np.concatenate([(blob_at + rs.normal(0, 0.02, (P // 2, 3))).astype(F), _near(rs, _body_centres(1100), P - P // 2)])
    return Case("tight", cen, pts[rs.permutation(P)], _rots(rs, 1500))


def _islands():
    rs = np.random.RandomState(23)
    a, b = np.array([-0.8, 0.0, 0.0]), np.array([0.8, 0.0, 0.0])
    cen = np.concatenate([a + rs.normal(0, 0.08, (150, 3)), b + rs.normal(0, 0.08, (150, 3))]).astype(F)
    cen = cen[rs.permutation(300)]
    lo, hi = cen.min(0).astype(np.float64), cen.max(0).astype(np.float64)
    P = 3501
    between = rs.uniform(lo, hi, (2 * P // 3, 3))
    around = rs.uniform(lo - 0.45, hi + 0.45, (P - 2 * P // 3, 3))
    pts = np.concatenate([between, around]).astype(F)
    return Case("islands", cen, pts[rs.permutation(P)], _rots(rs, 300))


def _lattice(dup):
    rs = np.random.RandomState(24 + dup)
    ax = np.arange(8, dtype=np.float64) / 8.0
    cen = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    if dup:
        cen = np.concatenate([cen, cen])
    cen = cen[rs.permutation(cen.shape[0])].astype(F)
    hx = np.arange(15, dtype=np.float64) / 16.0
    pts = np.stack(np.meshgrid(hx, hx, hx, indexing="ij"), -1).reshape(-1, 3).astype(F)
    return Case("lattice_dup" if dup else "lattice", cen, pts[rs.permutation(pts.shape[0])], _rots(rs, cen.shape[0]))


def _faces():
    """points ON the faces of the grid's cells: gmin + k g evaluated in fp32, its two fp32 neighbours, and the outer faces"""
    rs = np.random.RandomState(25)
    cen = _body_centres(500)
    grid = grid_setup(cen)
    assert grid.g == DPG_CELL and grid.grown == 0      # (cbrt(500 / 500) = 1: the cell size is the constant itself)
    P = 3003
    pts = _near(rs, cen, P)
    k = np.floor((pts - grid.gmin) * grid.inv_g).astype(np.int64) + rs.randint(0, 2, (P, 3))
    outer = rs.rand(P, 3) < 0.15                      # the nearer outer face of the box instead
    k = np.where(outer, np.where(k * 2 < grid.dim, 0, grid.dim), k)
    face = (grid.gmin + k.astype(F) * grid.g).astype(F)
    ulp = rs.randint(-1, 2, (P, 3))
    face = np.where(ulp < 0, np.nextafter(face, F(-np.inf)), np.where(ulp > 0, np.nextafter(face, F(np.inf)), face)).astype(F)
    snap = rs.rand(P, 3) < 0.6                        # one, two or all three coordinates on a face
    snap[np.arange(P), rs.randint(0, 3, P)] = True
    # (an outer face only where that keeps the point near the body: the far ends of the long axis are a metre from any centre)
    snap &= ~outer | (np.abs(face - pts) < 0.5)
    return Case("faces", cen, np.where(snap, face, pts).astype(F), _rots(rs, 500))


def _far():
    rs = np.random.RandomState(26)
    body = _body_centres(500)
    cen = np.concatenate([body[:250], np.full((1, 3), 1e5, F), body[250:]])
    return Case("far", cen, _near(rs, body, 2999), _rots(rs, 501))


def _edge():
    """the domain edge of dp_sin: 7 centres, offsets up to 2.4 m, rotations of norm <= 1 -> |a| at octave 9 just under 2^12"""
    rs = np.random.RandomState(27)
    cen = rs.normal(0, 0.005, (7, 3)).astype(F)
    P = 2049
    u = rs.normal(size=(P, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    rho = 2.38 * rs.uniform(0.0, 1.0, (P, 1)) ** (1.0 / 3.0)
    rho[: P // 4] = 2.38                               # a quarter of them on the outer sphere itself
    q, _ = np.linalg.qr(rs.normal(size=(7, 3, 3)))
    rot = (q * rs.uniform(0.97, 1.0, (7, 1, 1))).reshape(7, 9).astype(F)
    return Case("edge", cen, (u * rho).astype(F), rot)


_MAKERS = {
    "body7": lambda: _body(7, 2311), "body8": lambda: _body(8, 2050), "body13": lambda: _body(13, 2177),
    "body500": lambda: _body(500, 3001), "body4096": lambda: _body(4096, 4099),
    "spread": _spread, "tight": _tight, "islands": _islands, "lattice": lambda: _lattice(0), "lattice_dup": lambda: _lattice(1),
    "faces": _faces, "far": _far, "edge": _edge,
}
CASES = tuple(_MAKERS)
GRID_CASES = tuple(c for c in CASES if c != "edge")      # (edge: a case of the value checks, the grid sees nothing new in it)


@functools.lru_cache(maxsize=None)
def case(name):
    c = _MAKERS[name]()
    assert c.name == name and c.cen.dtype == F and c.pts.dtype == F and c.rot.shape == (c.cen.shape[0], 9)
    return c


@functools.lru_cache(maxsize=None)
def grid_of(name):
    c = case(name)
    return classify(c.cen, c.pts)


@functools.lru_cache(maxsize=None)
def knn_of(name):
    """(d2 [P,7] fp32, idx [P,7]) of the exact oracle: computed once, shared by every test, never modified"""
    c = case(name)
    d2, idx = O.knn_points_exact(torch.from_numpy(c.pts), torch.from_numpy(c.cen), DP_K)
    d2, idx = d2.numpy(), idx.numpy()
    d2.setflags(write=False); idx.setflags(write=False)
    return d2, idx


def blend_of(rot):
    """[N_c, 9] row-major rotation blocks -> the [N_c, 4, 4] blend matrices oracle.th_oracle.dparf takes"""
    b = torch.zeros((rot.shape[0], 4, 4), dtype=torch.float32)
    b[:, :3, :3] = torch.as_tensor(rot).reshape(-1, 3, 3)
    b[:, 3, 3] = 1.0
    return b


# ---- the forward's weight matrix -------------------------------------------------------------------------------------------
def dparf_forward_weights(hip, pts, cen, rot, views=1, check=True):
    """W[p,c]: what the forward kernel selected and weighted, read with one-hot tokens (a blend of one-hot rows returns the
    weights themselves, bit for bit) in passes of `views` x 192 centres: view v of a pass carries the v-th block of 192"""
    P, nc = pts.shape[0], cen.shape[0]
    Wm = torch.zeros((P, nc), dtype=torch.float64)
    step = 192 * views
    for c0 in range(0, nc, step):
        tok = torch.zeros((views, nc, 192), device=pts.device)
        spans = []
        for v in range(views):
            a = c0 + 192 * v
            n = min(192, nc - a)
            if n <= 0:
                break
            tok[v, a + torch.arange(n), torch.arange(n)] = 1.0
            spans.append((v, a, n))
        out = hip.dparf_encode(pts, cen, rot, tok)
        for v, a, n in spans:
            Wm[:, a:a + n] = out[:, v, :n].double().cpu()
    if check:
        assert ((Wm != 0).sum(1) == 7).all() and float((Wm.sum(1) - 1).abs().max()) < 1e-6
    return Wm.numpy()
