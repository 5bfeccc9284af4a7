"""K1's adversarial cases on the CPU: every case is what its name says (stated on the reference, oracle.th_oracle.hull_mask, and on
the numpy restatement of the vertex grid in hull_cases.py), the fp32 reference agrees with a float64 distance wherever that one
is decisive, and the grid's premise holds on them: the nearest vertex of every hit sample lies in the 3 x 3 x 3 cells around the
sample's.  The tests that end in `_would_show` state, on the restatement, why a named way of breaking the kernel cannot pass
the device tests.  The device side is tests/test_gpu_hull_mask.py."""
import numpy as np
import pytest
import torch

import hull_cases as Hc
from oracle import th_oracle as O

F = np.float32


# ---- every case -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", Hc.FINITE_CASES)
def test_reference_agrees_with_float64_where_that_is_decisive(name):
    """fp32 reference = (float64 distance < thresh) on every sample whose float64 distance is more than 1e-5 relative away"""
    c = Hc.case(name)
    t = float(F(c.thresh))
    d64 = Hc.d64_min(c.pts, c.verts)
    clear = np.abs(d64 / t - 1.0) > 1e-5
    ref = Hc.ref_of(name)
    print(f"{name}: {c.pts.shape[0]} samples x {c.verts.shape[0]} vertices, decisive in float64: {clear.mean():.3f}, hits {ref.mean():.3f}")
    assert ref.dtype == bool and ref.shape == (c.pts.shape[0],)
    assert clear.any() and np.array_equal(ref[clear], d64[clear] < t)


@pytest.mark.parametrize("name", tuple(Hc.SHELL_SETS) + tuple(Hc.SHELL_FAR) + ("cube20", "plane"))
def test_reference_takes_the_correctly_rounded_square_root(name):
    """the reference on THIS host = numpy's fp32 sqrt (IEEE: correctly rounded) = the float64 sqrt rounded to fp32, compared with
    fp32 thresh -- on the sets that hold samples an ulp from the threshold.  (torch's own fp32 CPU sqrt is an ulp off for one
    operand in seven on some hosts; oracle.th_oracle.hull_mask does not use it.)"""
    c = Hc.case(name)
    d2 = Hc.d2_of(name)
    s32 = np.sqrt(d2, dtype=F)
    assert np.array_equal(s32, np.sqrt(d2.astype(np.float64)).astype(F))
    assert np.array_equal(Hc.ref_of(name), s32 < F(c.thresh))
    # the pairs themselves, not only the nearest one: the oracle's d2 is the fp32 expression in x, y, z order
    v = c.verts[Hc.nearest_of(name)[1]]
    d = c.pts - v
    assert np.array_equal((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2], d2)


@pytest.mark.parametrize("name", Hc.FINITE_CASES)
def test_nearest_vertex_of_a_hit_is_in_the_neighbourhood(name):
    """the premise of the pruning, on the restatement: a hit sample lies in the grid extended by one layer and the cell of its
    nearest vertex is at most one away on every axis"""
    c, g = Hc.case(name), Hc.grid_of(name)
    ref = Hc.ref_of(name)
    _, idx = Hc.nearest_of(name)
    sc, inside = Hc.sample_cells(g, c.pts)
    vc = Hc.vert_cells(g, c.verts)
    assert g.ncell <= Hc.GRID_MAX_CELLS and (g.dim >= 1).all() and (g.dim <= Hc.GRID_MAX_DIM).all()
    assert inside[ref].all()
    assert (np.abs(sc[ref] - vc[idx[ref]]) <= 1).all()


# ---- 1. threshold shell ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tuple(Hc.SHELL_SETS))
def test_shell_fills_the_band(name):
    c, g = Hc.case(name), Hc.grid_of(name)
    ref, d2 = Hc.ref_of(name), Hc.d2_of(name)
    band, decided = Hc.band_of(d2, c.thresh), Hc.sqrt_decided(d2, c.thresh)
    print(f"{name}: {c.pts.shape[0]} samples, hits {ref.mean():.3f}, in the d2 band {band.mean():.3f}, decided by the square root "
          f"alone {int(decided.sum())}")
    assert c.verts.shape[0] == 64 and c.pts.shape[0] == 64 * 64 * len(Hc.SHELL_K)
    assert 0.3 <= ref.mean() <= 0.7
    assert band.mean() >= 0.10
    if c.thresh in (0.1, 0.05):
        assert decided.sum() >= 100
    # isolated vertices: one per cell, and no sample has a second vertex anywhere near
    assert np.unique(Hc.linear(g, Hc.vert_cells(g, c.verts))).size == 64
    assert Hc.count_within(c.pts, c.verts, 2.0 * c.thresh).max() == 1
    assert g.h == F(F(c.thresh) * Hc.H0_FACTOR)


@pytest.mark.parametrize("name", tuple(Hc.SHELL_FAR))
def test_far_shells_have_both_outcomes(name):
    ref = Hc.ref_of(name)
    print(f"{name}: hits {ref.mean():.3f}, in the d2 band {Hc.band_of(Hc.d2_of(name), 0.1).mean():.3f}")
    assert ref.any() and not ref.all()


# ---- 2. cell populations -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", Hc.POP_N)
def test_population_cases(n):
    verts, is_patch, pts, role = Hc.pop_layout(n)
    c = Hc.case(f"pop{n}")
    assert np.array_equal(c.verts, verts) and np.array_equal(c.pts, pts)
    g = Hc.grid_of(c.name)
    vc = Hc.linear(g, Hc.vert_cells(g, verts))
    own = vc[is_patch][0]
    # all n vertices of the patch share ONE cell, an inner one, and nothing else is in it
    assert is_patch.sum() == n and (vc[is_patch] == own).all() and (vc == own).sum() == n
    own_c = Hc.vert_cells(g, verts)[is_patch][0]
    assert (own_c >= 1).all() and (own_c <= g.dim - 2).all()
    # spacing of the patch >= 0.05 thresh
    pv = verts[is_patch].astype(np.float64)
    if n > 1:
        d = np.sqrt(((pv[:, None] - pv[None]) ** 2).sum(-1)) + np.eye(n)
        assert d.min() >= 0.05 * c.thresh
    sc, inside = Hc.sample_cells(g, pts)
    assert inside.all()
    lin = Hc.linear(g, sc)
    for r in ("near_own", "far_own"):
        assert (lin[role == r] == own).all()
    for r in ("near_nbr", "far_nbr"):
        assert (sc[role == r] == own_c - [0, 0, 1]).all()
    within = Hc.count_within(pts, verts, c.thresh)
    near = np.char.startswith(role, "near")
    assert (within[near] == 1).all() and (within[~near] == 0).all()
    assert np.array_equal(Hc.ref_of(c.name), near)
    # every vertex of the patch is the ONE vertex in reach of a sample of its own cell and of a sample of the cell underneath:
    # whatever order the atomics leave in the cell, every position of it decides a sample of either kind
    _, idx = Hc.nearest_of(c.name)
    patch_ids = np.nonzero(is_patch)[0]
    for r in ("near_own", "near_nbr"):
        assert np.array_equal(np.sort(idx[role == r]), patch_ids)


# ---- 3. grid border ----------------------------------------------------------------------------------------------------------
def test_border_reaches_the_layer_around_the_grid():
    c, g = Hc.case("border"), Hc.grid_of("border")
    ref = Hc.ref_of("border")
    sc, inside = Hc.sample_cells(g, c.pts)
    vmax = c.verts.max(0)
    assert (c.verts == vmax).all(1).any() and (c.verts.min(0) == 0).all()
    # the vertices lie on the surface of their own box
    assert ((c.verts == 0) | (c.verts == vmax)).any(1).all()
    assert (Hc.vert_cells(g, vmax[None])[0] == g.dim - 1).all()
    for a, s in Hc.SIDES:
        layer = sc[:, a] == (-1 if s < 0 else g.dim[a])
        second = sc[:, a] == (-2 if s < 0 else g.dim[a] + 1)
        finite = np.abs(c.pts).max(1) < 1e5
        print(f"border, axis {a} side {s:+d}: in the layer {int((layer & inside).sum())} ({int((layer & ref).sum())} hits), one layer "
              f"further out {int((second & finite).sum())}")
        assert (layer & inside & ref).sum() >= 20 and (layer & inside & ~ref).sum() >= 1
        assert (second & finite).sum() >= 20
    assert not ref[~inside].any() and (~inside).sum() >= 120
    far = np.abs(c.pts).max(1) >= 1e5
    assert far.sum() == 9 and not inside[far].any() and not ref[far].any()


# ---- 4. extent rule and degenerate sets --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", Hc.DEGENERATE)
def test_degenerate_sets(name):
    c, g = Hc.case(name), Hc.grid_of(name)
    ref = Hc.ref_of(name)
    _, inside = Hc.sample_cells(g, c.pts)
    h0 = F(F(c.thresh) * Hc.H0_FACTOR)
    print(f"{name}: {c.verts.shape[0]} vertices, h {float(g.h):.6f} (h0 {float(h0):.6f}), dim {g.dim.tolist()}, hits {ref.mean():.3f}, "
          f"samples outside the extended grid {(~inside).mean():.3f}, in the d2 band {Hc.band_of(Hc.d2_of(name), c.thresh).mean():.3f}")
    assert ref.any() and not ref.all() and (~inside).any()
    assert Hc.band_of(Hc.d2_of(name), c.thresh).any()
    if name in Hc.ENLARGED:
        assert g.h > h0 and tuple(g.dim) == Hc.ENLARGED[name]
    else:
        assert g.h == h0
    if name in ("single", "coincident65"):
        assert tuple(g.dim) == (1, 1, 1) and np.unique(c.verts, axis=0).shape[0] == 1
    if name == "cube20":
        assert g.ncell == 63 ** 3 < Hc.GRID_MAX_CELLS
    if name == "body_shifted":
        assert c.verts.shape[0] == 6890 and np.abs(c.verts).max() > 37


# ---- 5. sample counts and the ray form ---------------------------------------------------------------------------------------
def test_count_cases_are_prefixes_with_both_outcomes():
    full = Hc.case("count257")
    for P in Hc.POINT_COUNTS:
        c = Hc.case(f"count{P}")
        assert c.pts.shape[0] == P and np.array_equal(c.pts, full.pts[:P])
        assert np.array_equal(Hc.ref_of(c.name), Hc.ref_of("count257")[:P])
    r = Hc.ref_of("count257")
    assert r[:63].any() and not r[:63].all() and r[0]


def test_ray_cases():
    for name, (R, S, jitter) in Hc.RAY_SETS.items():
        c, m = Hc.ray_case(name), Hc.ray_ref_of(name)
        hit = m.any(1)
        print(f"{name}: hit rays {int(hit.sum())} of {R}, valid samples {int(m.sum())}")
        assert m.shape == (R, S) and c.ray_o.shape == (R, 3) and (c.t_rand is not None) == jitter
        assert hit.sum() >= 1 and (R < 15 or not hit.all())
        assert (m.sum(1)[hit] < S).any()                       # the rule changes the count: a hit ray with a sample outside the hull
        if jitter:
            z = Hc.ray_z(name)
            plain, _ = O.sampling_points(c.ray_o, c.ray_d, c.near, c.far, S)
            assert z.shape == (R, S) and not torch.equal(plain, Hc.ray_pts(name))
            assert torch.equal(c.ray_o[:, None] + c.ray_d[:, None] * z[..., None], Hc.ray_pts(name))
    assert not Hc.ray_ref_of("rays_miss").any() and Hc.ray_ref_of("rays_miss").shape == (16, 64)


def test_nonfinite_case():
    c, full = Hc.case("nonfinite"), Hc.case("count257")
    bad = ~np.isfinite(c.pts).all(1) | (np.abs(c.pts) > 1e38).any(1)
    ref = Hc.ref_of("nonfinite")
    assert bad.sum() == 86 and np.isnan(c.pts).any() and np.isposinf(c.pts).any() and np.isneginf(c.pts).any()
    assert (c.pts == F(3e38)).any() and (c.pts == F(-3e38)).any()
    assert not ref[bad].any()                                                          # the reference: a plain miss
    assert np.array_equal(c.pts[~bad], full.pts[~bad]) and np.array_equal(ref[~bad], Hc.ref_of("count257")[~bad])
    assert ref[~bad].any() and not ref[~bad].all()
    # the restatement (with the clamp): outside the extended grid, every one of them
    _, inside = Hc.sample_cells(Hc.grid_of("nonfinite"), c.pts)
    assert not inside[bad].any()


# ---- why a broken kernel cannot pass ----------------------------------------------------------------------------------------
def test_a_smaller_box_margin_would_show():
    """`1.001f` -> `0.999f`: a cell that holds one vertex has that vertex as its box; the shells hold hits farther from it than
    0.999 thresh + 1e-6, which the screening would then drop"""
    for name in Hc.SHELL_SETS:
        c = Hc.case(name)
        t = F(c.thresh)
        d = np.sqrt(Hc.d2_of(name).astype(np.float64))
        assert (Hc.ref_of(name) & (d > float(t) * 0.999 + 1e-6 + 1e-7)).sum() >= 1000


def test_a_comparison_of_squares_would_show():
    """band 0 and `d2 < t2`: the predicate becomes d2 < fl(thresh^2); test_shell_fills_the_band counts the samples it gets wrong"""
    for name in Hc.SHELL_SETS:
        c = Hc.case(name)
        if c.thresh != 0.3:
            d2, t = Hc.d2_of(name), F(c.thresh)
            assert ((d2 < F(t * t)) != Hc.ref_of(name)).sum() >= 100


def test_a_smaller_cell_would_show():
    """`thresh * 1.05f` -> `thresh * 0.95f`: the restated grid with that factor puts the nearest vertex of some hits two cells away"""
    for name in ("shell_t0.1_o0", "shell_t0.05_o1.0"):
        c = Hc.case(name)
        g = Hc.grid_setup(c.verts, c.thresh, h0_factor=0.95)
        assert g.h < F(c.thresh)
        _, idx = Hc.nearest_of(name)
        ref = Hc.ref_of(name)
        sc, _ = Hc.sample_cells(g, c.pts)
        apart = (np.abs(sc - Hc.vert_cells(g, c.verts)[idx]) > 1).any(1)
        print(f"{name}: hits whose vertex would be two cells away: {int((apart & ref).sum())}")
        assert (apart & ref).sum() >= 50


def test_a_dropped_layer_would_show():
    """`cx >= -1` -> `cx >= 0`: hits whose x cell is -1 become misses (the six sides: test_border_reaches_the_layer_around_the_grid)"""
    for name in ("border", "shell_t0.3_o0", "shell_t0.3_o1.0"):
        sc, _ = Hc.sample_cells(Hc.grid_of(name), Hc.case(name).pts)
        assert (Hc.ref_of(name) & (sc[:, 0] == -1)).sum() >= 20


def test_skipped_positions_of_a_cell_would_show():
    """`vs + HULL_PROBE` + 1 skips position 8 of the sample's own cell, `v0 += 65` position 72 of the own cell and position 64 of
    every other; test_population_cases shows that every position of the patch's cell decides a sample of both kinds"""
    assert Hc.HULL_PROBE == 8
    assert any(n > Hc.HULL_PROBE for n in Hc.POP_N) and any(n > Hc.HULL_PROBE + 64 for n in Hc.POP_N) and any(n > 64 for n in Hc.POP_N)
    # and the sizes on either side of each of these: 8 | 9, 64 | 65, 72 | 73
    assert {8, 9, 64, 65, 72, 73} <= set(Hc.POP_N)
