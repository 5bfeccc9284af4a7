"""K4's adversarial cases on the CPU: every case reaches the branch of the candidate grid it is named for (stated on the numpy
restatement of the grid in dparf_cases.py), and the grid's proof holds on them: the restated list of a point's cell contains
the 7 neighbours the exact oracle selects.  The device side is tests/test_gpu_dparf_knn.py."""
import numpy as np
import pytest

import dparf_cases as D


@pytest.mark.parametrize("name", D.CASES)
def test_case_shape_and_range(name):
    c = D.case(name)
    P, nc = c.pts.shape[0], c.cen.shape[0]
    assert 2000 <= P <= 4100 and P % 128 != 0 and 7 <= nc <= 4096
    assert np.isfinite(c.pts).all() and np.isfinite(c.cen).all()
    d2, idx = D.knn_of(name)
    assert (np.diff(d2, axis=1) >= 0).all() and (idx >= 0).all() and (idx < nc).all()
    # no weight can underflow: every point within 2 m of its 7th centre (the domain-edge case: 2.4 m, by construction)
    assert float(np.sqrt(d2[:, 6].astype(np.float64)).max()) < (2.4 if name == "edge" else 2.0)
    # rotations of norm <= 1, PE arguments inside dp_sin's domain
    assert float(np.linalg.norm(c.rot.reshape(-1, 3, 3).astype(np.float64), ord=2, axis=(1, 2)).max()) <= 1.0 + 1e-6
    assert np.pi * 512 * float(np.sqrt(d2[:, 6].astype(np.float64)).max()) + 1.6 < 4096


def test_body_cases_reach_the_sentinels_and_the_cap():
    for nc in (7, 13):
        # the even lane scans ceil(nc / 2) centres, the odd lane floor(nc / 2): at most 7, the odd lane fewer -- its list ends
        # in (3e38, 0x7fffffff) sentinels, which then take part in the merge
        assert nc - nc // 2 <= 7 and nc // 2 < 7 and D.case(f"body{nc}").cen.shape[0] == nc
    assert D.case("body8").cen.shape[0] == 8 and D.case("body500").cen.shape[0] == 500
    assert D.case("body4096").cen.shape[0] == 4096                  # TH_MAX_CLUSTERS, and the last N_c the grid builder admits
    for name in ("body7", "body8", "body13", "body500", "body4096"):
        grid, cells = D.grid_of(name)
        fr = D.fractions(cells)
        print(name, "g", grid.g, "dim", grid.dim, fr)
        assert grid.ncell > 0 and fr["listed"] >= 0.25


def test_spread_runs_the_growth_loop():
    grid, cells = D.grid_of("spread")
    print("spread: grew", grid.grown, "times, g", grid.g, "dim", grid.dim, D.fractions(cells))
    assert grid.grown >= 1 and 0 < grid.ncell <= D.DPG_MAXCELLS


def test_tight_overflows_the_slots():
    _, cells = D.grid_of("tight")
    fr = D.fractions(cells)
    longest = max(len(l) for l in cells.lists if l is not None)
    print("tight:", fr, "longest list", longest)
    assert fr["overflow"] >= 0.25 and fr["listed"] >= 0.25 and longest > D.DPG_STRIDE
    # both sides of `pos < DPG_STRIDE`: lists that just fit and lists that just do not
    sizes = np.array([len(l) for l in cells.lists if l is not None])
    assert (sizes <= D.DPG_STRIDE).any() and (sizes > D.DPG_STRIDE).any()


def test_islands_has_air_outside_and_listed_points():
    _, cells = D.grid_of("islands")
    fr = D.fractions(cells)
    print("islands:", fr)
    assert fr["air"] >= 0.10 and fr["outside"] >= 0.10 and fr["listed"] >= 0.25


@pytest.mark.parametrize("name", ["lattice", "lattice_dup"])
def test_lattice_distances_are_exact_and_tied(name):
    c = D.case(name)
    d = c.pts[:, None, :] - c.cen[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    assert d2.dtype == np.float32
    d64 = (c.pts.astype(np.float64)[:, None, :] - c.cen.astype(np.float64)[None, :, :])
    assert np.array_equal(d2.astype(np.float64), (d64 * d64).sum(-1))           # fp32 d2 = float64 d2, every pair
    s = np.sort(d2, axis=1)
    tie78 = float((s[:, 6] == s[:, 7]).mean())
    print(name, "points with a 7th/8th tie:", tie78)
    assert tie78 >= 0.5
    if name == "lattice_dup":
        # every centre twice: equal distances between different indices at every rank of the list
        assert all((s[:, k] == s[:, k + 1]).any() for k in range(7))
        assert (s[:, 0] == s[:, 1]).all()


def test_faces_points_sit_on_cell_faces():
    c = D.case("faces")
    grid, cells = D.grid_of("faces")
    t = np.rint((c.pts - grid.gmin) * grid.inv_g)
    face = (grid.gmin + t.astype(np.float32) * grid.g).astype(np.float32)
    on = c.pts == face
    near = (c.pts == np.nextafter(face, np.float32(-np.inf))) | (c.pts == np.nextafter(face, np.float32(np.inf)))
    outer = on & ((t == 0) | (t == grid.dim))
    fr = D.fractions(cells)
    print("faces: on a face", float(on.any(1).mean()), "one ulp off", float(near.any(1).mean()), "on an outer face",
          float(outer.any(1).mean()), fr)
    assert on.any(1).mean() > 0.3 and near.any(1).mean() > 0.3 and outer.any(1).mean() > 0.02
    assert fr["outside"] > 0.01 and fr["listed"] > 0.5
    # both neighbours of a face are taken: cell k - 1 and cell k of the same face position
    k = np.floor((c.pts - grid.gmin) * grid.inv_g)
    assert ((on | near) & (k == t)).any() and ((on | near) & (k == t - 1)).any()


def test_far_centre_disables_the_grid():
    grid, cells = D.grid_of("far")
    assert grid.ncell == 0 and grid.grown == 32 and (cells.kind == "disabled").all()


@pytest.mark.parametrize("name", D.CASES)
def test_cell_lists_hold_the_seven_neighbours(name):
    """the superset property: for a point in cell (q, h) every one of its 7 nearest centres lies within d7(q) + 2h of q.
    Checked twice: the float64 set without any margin is contained in the fp32 list the kernel's expressions give (the
    margins 1.0001 / 1e-5 cover the rounding), and the oracle's neighbours are in that list."""
    _, cells = D.grid_of(name)
    _, idx = D.knn_of(name)
    checked = 0
    for p in range(idx.shape[0]):
        lst = cells.lists[p]
        if lst is None:
            continue
        assert np.isin(cells.lists64[p], lst).all(), (name, p)
        assert np.isin(idx[p], lst).all(), (name, p, cells.kind[p])
        checked += cells.kind[p] == "listed"
    assert checked == int((cells.kind == "listed").sum())
    if name != "far":
        assert checked > 0
