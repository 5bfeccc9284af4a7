"""K4 (transhuman_amd/csrc/k_dparf.hip) on the adversarial centre sets of dparf_cases.py.

A. th_dparf_encode (the full N_c scan, no grid) against the exact restatement: the support of the forward's weight matrix is
   the index set of oracle.th_oracle.knn_points_exact for EVERY point (same fp32 expression, ties to the lower index -- on the
   lattice cases that decides the 7th/8th ties), the weights are the float64 softmax, the xyz and PE channels the float64
   oracle.th_oracle.dparf on the same selection.
B. frames (th_eval_sigma_grid, th_render_rays): with the candidate grid = with TH_DPARF_NOGRID=1, bit for bit, on the cases
   whose points reach the grid's branches (tests/test_dparf_cases_host.py asserts on the CPU that they do).
So: oracle = device full scan (A), device full scan = device grid (B).

Bounds (derived, not measured; 2^-24 = half an ulp, the relative error of one fp32 rounding; 2^-23 = one ulp):

  weights  w_k = e_k / sum_j e_j,  e_k = expf(x_k - x_max),  x_k = -sqrt(d2_k) / 0.5, d2 the oracle's own fp32 value.
    x_k          one correctly rounded sqrt; the division by 0.5 is exact ............ |dx_k| <= 2^-24 |x_k|
    t_k          = x_k - x_max: both errors above and one rounding ................... |dt_k| <= 2^-24 (|x_k| + |x_max| + |t_k|)
    e_k          exp turns the absolute error of t_k into a relative one; expf itself is good to 1 ulp (HIP's documented
                 bound) ................................................................ rho_k = |dt_k| + 2^-23
    sum, divide  seven additions and one division, each 2^-24 ......................... 8 * 2^-24
    relative error of w_k <= rho_k + max_j rho_j + 8 * 2^-24   (+ 0.1 % for the second-order terms)
    With |x| <= 4.8 that is <= 1.9e-6.  The absolute bound is the project's 2e-6 for these channels.

  xyz / PE  channel = sum_k w_k s(a_k),  a_k = fma(def_k, pi 2^o, phase),  def_k = the rotated offset (s = identity for xyz).
    Five fp32 roundings precede the sine: the subtraction p - c, the product and two fma of the rotation, the argument fma
    (four for xyz: no argument).  Each is at most one ulp of its result: |da_k| <= 5 * 2^-23 |a_k|, and |sin'| <= 1, so
    bound = sum_k w_k * 5 * 2^-23 * |a_k|  +  2e-6   (2e-6: the bar of the token / xyz channels -- weights, dp_sin's own
    < 1e-6, the seven-term fma sum).
    At the domain edge (|a| just under 2^12 at octave 9) the bound is 5 * 2^-23 * 4096 = 2.4e-3; a failed range reduction
    shows as an O(1) error.
"""
import os

import numpy as np
import pytest
import torch

import dparf_cases as D
from oracle import th_oracle as O
from transhuman_amd import synth
from util import make_net

pytestmark = pytest.mark.gpu
ULP, HALF = 2.0 ** -23, 2.0 ** -24


@pytest.fixture(scope="module")
def hip(gpu):
    from transhuman_amd import hip as H
    H.load_library()
    return H


@pytest.fixture(scope="module")
def net(gpu, hip):
    return make_net(12).to(gpu)


def _dev(name, gpu):
    c = D.case(name)
    return tuple(torch.from_numpy(a).to(gpu) for a in (c.pts, c.cen, c.rot))


# ---- A: the full scan against the exact restatement ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def runs():
    """one evaluation per case, shared by the tests of part A and dropped with the module"""
    cache = {}
    yield cache
    cache.clear()


def _run(runs, hip, gpu, name):
    """-> (points whose support of W differs from the oracle's set, a few of those supports, W at the oracle's 7 indices [P,7],
    the seeded tokens [2,N_c,192], the rows [P,2,256] for them).  W itself [P,N_c] is not kept."""
    if name not in runs:
        pts, cen, rot = _dev(name, gpu)
        W = D.dparf_forward_weights(hip, pts, cen, rot, views=8, check=False)
        _, idx = D.knn_of(name)
        want = np.zeros(W.shape, bool)
        np.put_along_axis(want, idx, True, axis=1)
        assert (want.sum(1) == 7).all()
        bad = np.nonzero(((W != 0) != want).any(1))[0]
        tok = torch.from_numpy(np.random.RandomState(5).normal(size=(2, cen.shape[0], 192)).astype(np.float32))
        out = hip.dparf_encode(pts, cen, rot, tok.to(gpu)).cpu()
        runs[name] = (bad, [np.nonzero(W[p])[0] for p in bad[:3]], np.take_along_axis(W, idx, axis=1), tok, out)
    return runs[name]


@pytest.mark.parametrize("name", D.CASES)
def test_full_scan_selects_the_oracles_neighbours(runs, hip, gpu, name):
    """support of W = index set of knn_points_exact, every point, no exclusions"""
    bad, got_sets, _, _, _ = _run(runs, hip, gpu, name)
    _, idx = D.knn_of(name)
    c = D.case(name)
    print(f"{name}: {c.pts.shape[0]} points x {c.cen.shape[0]} centres, points with a wrong neighbour set: {bad.size}")
    assert bad.size == 0, (name, bad[:5], got_sets, idx[bad[:3]])


def _weight_ref(name):
    """-> float64 softmax weights [P,7], their derived relative bound [P,7], the oracle's indices"""
    d2, idx = D.knn_of(name)
    x = -np.sqrt(d2.astype(np.float64)) / 0.5
    t = x - x.max(1, keepdims=True)
    e = np.exp(t)
    rho = HALF * (np.abs(x) + np.abs(x).min(1, keepdims=True) + np.abs(t)) + ULP      # (x_max = the x of smallest magnitude)
    rel = (rho + rho.max(1, keepdims=True) + 8 * HALF) * 1.001
    return e / e.sum(1, keepdims=True), rel, idx


@pytest.mark.parametrize("name", D.CASES)
def test_full_scan_weights_are_the_float64_softmax(runs, hip, gpu, name):
    _, _, got, _, _ = _run(runs, hip, gpu, name)
    w64, rel, idx = _weight_ref(name)
    err = np.abs(got - w64)
    r_rel, r_abs = float((err / (rel * w64)).max()), float(err.max() / 2e-6)
    print(f"{name}: weights worst error / relative bound = {r_rel:.3f} (bound up to {rel.max():.2e}), "
          f"worst error / 2e-6 = {r_abs:.3f}")
    assert (err <= rel * w64).all() and (err <= 2e-6).all(), (r_rel, r_abs)


def _pe_bounds(name):
    """per point and PE channel (63): sum_k w_k * n * 2^-23 * |a_k| + 2e-6, and the largest |a|"""
    c = D.case(name)
    w, _, idx = _weight_ref(name)
    r = c.pts.astype(np.float64)[:, None, :] - c.cen.astype(np.float64)[idx]                     # [P,7,3]
    R = c.rot.astype(np.float64).reshape(-1, 3, 3)[idx]                                          # [P,7,3,3]
    de = np.einsum("pkj,pkjc->pkc", r, R)
    f32pi, f32hpi = float(np.float32(np.pi)), float(np.float32(np.pi * 0.5))
    lit = [4 * ULP * np.abs(de)]
    amax = 0.0
    for o in range(10):
        for ph in (0.0, f32hpi):
            a = de * (f32pi * 2.0 ** o) + ph
            amax = max(amax, float(np.abs(a).max()))
            lit.append(5 * ULP * np.abs(a))
    lit = np.concatenate(lit, -1)                                                                # [P,7,63]
    return (w[..., None] * lit).sum(1) + 2e-6, amax


@pytest.mark.parametrize("name", D.CASES)
def test_full_scan_rows_match_the_float64_oracle(runs, hip, gpu, name):
    """token, xyz and PE channels against oracle.th_oracle.dparf in float64 on the same selection; column 255 is 0"""
    c = D.case(name)
    _, _, _, tok, out = _run(runs, hip, gpu, name)
    ref = O.dparf(torch.from_numpy(c.pts).double(), torch.from_numpy(c.cen), D.blend_of(c.rot), tok.double()).numpy()
    got = out.double().numpy()
    assert got.shape == (c.pts.shape[0], 2, 256) and np.isfinite(got).all()
    assert (got[..., 255] == 0).all()
    # token channels: the weights' relative bound on every term, seven roundings of the fma chain
    w64, rel, idx = _weight_ref(name)
    tmag = np.abs(tok.double().numpy()[:, idx])                                                  # [2,P,7,192]
    tol_tok = np.moveaxis((((rel + 7 * HALF) * w64)[None, :, :, None] * tmag).sum(2), 0, 1)      # [P,2,192]
    e_tok = np.abs(got[..., :192] - ref[..., :192])
    r_tok = float((e_tok / tol_tok).max())
    lit, amax = _pe_bounds(name)
    err = np.abs(got[..., 192:255] - ref[..., 192:])
    assert np.array_equal(got[:, 0, 192:], got[:, 1, 192:])                   # the PE part does not depend on the view
    r_lit = float((err / lit[:, None, :]).max())
    print(f"{name}: tokens worst error / bound {r_tok:.3f} (max error {e_tok.max():.2e}); xyz/PE worst error / bound {r_lit:.3f}; "
          f"max |a| {amax:.1f}, max error {err.max():.2e}, largest bound {lit.max():.2e}")
    assert (e_tok <= tol_tok).all(), r_tok
    if name == "edge":
        assert 3500 < amax < 4096 and 1.5e-3 < lit.max() < 2.5e-3             # just under 2^12: the edge of dp_sin's domain
    assert (err <= lit[:, None, :]).all(), r_lit


@pytest.mark.parametrize("P", [1, 127, 128, 129, 257])
def test_layout_edges(runs, hip, gpu, P):
    """sample counts around the 128-sample workgroup, rows beyond P untouched, bit-identical runs"""
    lib = hip.load_library()
    pts, cen, rot = _dev("body500", gpu)
    _, _, _, tok, full = _run(runs, hip, gpu, "body500")
    tok = tok.to(gpu)
    out = hip.dparf_encode(pts[:P].contiguous(), cen, rot, tok)
    assert torch.equal(out.cpu(), full[:P])                                    # a row depends on its own point only
    buf = torch.full((P + 3, 2, 256), float("nan"), device=gpu)
    rc = lib.th_dparf_encode(hip.ctx(gpu), hip._p(pts), None, P, hip._p(cen), hip._p(rot), hip._p(tok), 2, cen.shape[0],
                             hip._p(buf), hip._stream())
    assert rc == 0
    assert torch.equal(buf[:P].cpu(), full[:P]) and torch.isnan(buf[P:]).all()


def test_sel_indirection(runs, hip, gpu):
    """a sample list that is neither monotonic nor free of repeats"""
    pts, cen, rot = _dev("body500", gpu)
    _, _, _, tok, full = _run(runs, hip, gpu, "body500")
    rs = np.random.RandomState(9)
    sel = rs.randint(0, pts.shape[0], 389).astype(np.int32)
    sel[:6] = [2999, 0, 2999, 17, 17, 3000]
    assert (np.diff(sel) < 0).any() and np.unique(sel).size < sel.size
    out = hip.dparf_encode(pts, cen, rot, tok.to(gpu), sel=torch.from_numpy(sel).to(gpu))
    assert out.shape[0] == 389 and torch.equal(out.cpu(), full[torch.from_numpy(sel).long()])
    again = hip.dparf_encode(pts, cen, rot, tok.to(gpu), sel=torch.from_numpy(sel).to(gpu))
    assert torch.equal(out, again)


def test_refusals(hip, gpu, net):
    """host-side checks in front of any launch"""
    pts = torch.zeros((5, 3), device=gpu)

    def args(nc):
        return pts, torch.zeros((nc, 3), device=gpu), torch.zeros((nc, 9), device=gpu), torch.zeros((1, nc, 192), device=gpu)

    with pytest.raises(hip.HipError, match="at least 7 token centres"):
        hip.dparf_encode(*args(6))
    # th_dparf_launch: 4 * ((3 N_c + 3) & ~3) + 128 * sizeof(DpNbr) (140) + 4096 <= 160 KB  <=>  N_c <= 11818
    lds = lambda nc: 4 * ((3 * nc + 3) & ~3) + 128 * 140 + 4096
    assert lds(11818) <= 160 * 1024 < lds(11819)
    with pytest.raises(hip.HipError, match="too many token centres for LDS staging"):
        hip.dparf_encode(*args(11819))
    frame, world = _frame(hip, gpu, "body500", nc_override=4097)
    with pytest.raises(hip.HipError, match="too many token clusters"):
        hip.eval_sigma_grid(net, frame, world)


# ---- B: grid = full scan, where the grid's branches are reached ----------------------------------------------------------
def _frame(hip, gpu, name, nc_override=None):
    """a hip.Frame around the case: the points themselves are the hull's vertices (every point passes the hull test), the world
    points are derived from the SMPL-space points through a non-trivial Rh / Th.  `faces` and the lattices: a signed permutation
    and Th = 0, which world2smpl undoes exactly, so the points the kernel sees are still ON the faces / the 2^-4 lattice and the
    exact ties take part in the comparison."""
    c = D.case(name)
    b = synth.make_batch(32, 32, 3, seed=0)
    exact = name in ("faces", "lattice", "lattice_dup")
    if exact:
        Rh, Th = np.array([[0, 0, 1], [-1, 0, 0], [0, 1, 0]], np.float64), np.zeros((1, 3))
    else:
        Rh, Th = b["Rh"][0].numpy().astype(np.float64), b["Th"][0].numpy().astype(np.float64)
    world = torch.from_numpy((c.pts.astype(np.float64) @ np.linalg.inv(Rh) + Th).astype(np.float32)).to(gpu)
    if exact:
        assert np.array_equal((world.cpu().numpy() - Th.astype(np.float32)) @ Rh.astype(np.float32), c.pts)
    cen, rot = c.cen, c.rot
    if nc_override is not None:
        cen, rot = np.zeros((nc_override, 3), np.float32), np.zeros((nc_override, 9), np.float32)
    nc = cen.shape[0]
    cams = hip.pack_cams(b["input_R"][0][0].to(gpu), b["input_T"][0][0].to(gpu), b["input_K"][0][0].to(gpu))
    scale = hip.feat_scale(np.array([32, 32]) / (np.array([32, 32]) - 1) * 2.0, (32, 32), gpu)
    pix = torch.from_numpy(synth.smooth_noise((3, 384, 32, 32), 24)).to(gpu)
    tok = torch.from_numpy(np.random.RandomState(6).normal(size=(3, nc, 192)).astype(np.float32)).to(gpu)
    frame = hip.Frame(world, torch.from_numpy(Rh.astype(np.float32)).to(gpu), torch.from_numpy(Th.astype(np.float32)).to(gpu),
                      cams, scale, hip.nchw_to_nhwc(pix), tok, torch.from_numpy(cen).to(gpu), torch.from_numpy(rot).to(gpu))
    return frame, world


@pytest.mark.parametrize("name", D.GRID_CASES)
def test_grid_equals_full_scan_on_points(hip, gpu, net, name, monkeypatch):
    frame, world = _frame(hip, gpu, name)
    P = world.shape[0]
    sig_grid, st_grid = hip.eval_sigma_grid(net, frame, world)
    monkeypatch.setenv("TH_DPARF_NOGRID", "1")
    sig_full, st_full = hip.eval_sigma_grid(net, frame, world)
    differ = int((sig_grid != sig_full).sum())
    print(f"{name}: {P} points, sigma differs at {differ}, sigma range {float(sig_full.min()):.3f} .. {float(sig_full.max()):.3f}")
    assert st_grid == st_full and st_grid["valid_samples"] == P
    assert torch.isfinite(sig_full).all() and float(sig_full.max()) > float(sig_full.min())
    assert torch.equal(sig_grid, sig_full)


@pytest.mark.parametrize("name", ["tight", "islands", "lattice"])
def test_grid_equals_full_scan_on_rays(hip, gpu, net, name, monkeypatch):
    """short rays through every point (two samples, 1 cm on either side), through the hull prepass and the pre-gather stage,
    which builds the grid on the context's second stream"""
    frame, world = _frame(hip, gpu, name)
    P = world.shape[0]
    d = torch.from_numpy(np.random.RandomState(8).normal(size=(P, 3)).astype(np.float32))
    d = (d / d.norm(dim=1, keepdim=True)).to(gpu)
    near, far = torch.full((P,), -0.01, device=gpu), torch.full((P,), 0.01, device=gpu)

    def render():
        pts = hip.Points(world, d, near, far, n_samples=2)
        hip.render_prepass(pts, world, 3, n_clusters=frame.c.n_clusters)
        hip.render_pregather(net, frame, pts)
        return hip.render_rays(net, frame, pts)

    # the pre-gather stage does its work only on the fused path with neighbour records, and covers every valid sample
    # with one launch only up to TH_PRE_SAMPLES of them
    assert hip.mlp_is_fused(gpu) and 2 * P <= int(os.environ.get("TH_PRE_SAMPLES", 2621440))
    with_grid = render()
    assert hip.mlp_is_fused(gpu)                      # (the range guard has not switched the path under the grid render)
    monkeypatch.setenv("TH_DPARF_NOGRID", "1")
    full_scan = render()
    print(f"{name}: {P} rays, stats {with_grid[3]}")
    assert with_grid[3] == full_scan[3] and with_grid[3]["valid_samples"] == 2 * P and with_grid[3]["hit_rays"] == P
    assert float(full_scan[1].max()) > 0
    for a, b in zip(with_grid[:3], full_scan[:3]):
        assert torch.equal(a, b)
