"""K4 and K17 under cfg.KNN 1..7, cfg.KNN_FREQ 1..10 and any cfg.KNN_DIST_ALPHA > 0 (hip.set_dparf), on their own.

The selection is held to oracle.th_oracle.knn_points_exact at K (no exclusions; the lattice cases tie at the K-th / (K+1)-th
place), the weights to the float64 softmax, the rows to oracle.th_oracle.dparf in float64 on the same selection, the backward
to the exact adjoint of the forward's own weight matrix.  The frame paths and the recordings of the real reference under the
same parameters: tests/test_gpu_dparf_params_frames.py.

Bounds (derived, as in tests/test_gpu_dparf_knn.py, for a general divisor and K terms; 2^-24 = half an ulp):

  weights  w_k = e_k / sum_j e_j,  e_k = expf(x_k - x_max),  x_k = (-sqrt(d2_k)) / alpha, d2 the oracle's own fp32 value,
           alpha = fp32(KNN_DIST_ALPHA) on both sides.
    x_k          one correctly rounded sqrt and one correctly rounded division ...... |dx_k| <= 2 * 2^-24 |x_k|
    t_k          = x_k - x_max: both errors above and one rounding ................... |dt_k| <= 2^-24 (2 |x_k| + 2 |x_max| + |t_k|)
    e_k          expf is good to 1 ulp ................................................. rho_k = |dt_k| + 2^-23
    sum, divide  K additions and one division ......................................... (K + 1) * 2^-24
    relative error of w_k <= rho_k + max_j rho_j + (K + 1) * 2^-24   (+ 0.1 % for the second-order terms)
    asserted where the float64 weight is >= 2^-100 (e_k is then a normal fp32 number); a smaller one only has to come out
    <= 2^-99.  The absolute bar 2e-6 holds where max |x| <= 4.8, which is what its derivation assumes.

  rows     token channels: the weights' relative bound on every term + K roundings of the fma chain; xyz / PE channels:
           sum_k w_k * 5 * 2^-23 |a_k| + 2e-6 over the 3 + 6 F live channels (4 * 2^-23 for xyz), as in that file.
"""
import numpy as np
import pytest
import torch

import dparf_cases as D
from oracle import th_oracle as O

pytestmark = pytest.mark.gpu
ULP, HALF = 2.0 ** -23, 2.0 ** -24
DEFAULT = (7, 10, 0.5)


@pytest.fixture(scope="module")
def hip(gpu):
    from transhuman_amd import hip as H
    H.load_library()
    return H


@pytest.fixture(autouse=True)
def defaults_afterwards(hip, gpu):
    """every test leaves the context at (7, 10, 0.5): the other files' direct hip.* calls assume a new context's values"""
    yield
    hip.set_dparf(*DEFAULT, gpu)


def _dev(name, gpu):
    c = D.case(name)
    return tuple(torch.from_numpy(a).to(gpu) for a in (c.pts, c.cen, c.rot))


def _knn(name, K):
    """the oracle's K nearest: the first K of its seven (one ordering by (d2, index))"""
    d2, idx = D.knn_of(name)
    return d2[:, :K], idx[:, :K]


def _seeded_tokens(nc, V=2):
    return torch.from_numpy(np.random.RandomState(5).normal(size=(V, nc, 192)).astype(np.float32))


# ---- 1: selection ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["body7", "body8", "body13", "lattice", "lattice_dup", "faces", "edge"])
@pytest.mark.parametrize("K", [1, 2, 3, 5, 6])
def test_selection_is_the_oracles_k_nearest(hip, gpu, K, name):
    """support of the forward's weight matrix = index set of knn_points_exact(pts, cen, K), every point, no exclusions"""
    d2, idx = _knn(name, K)
    if name == "lattice":
        d7, _ = D.knn_of(name)
        ties = int((d7[:, K - 1] == d7[:, K]).sum())
        assert ties > 0, "no point of the lattice ties at the K-th / (K+1)-th place"
    pts, cen, rot = _dev(name, gpu)
    hip.set_dparf(K, 10, 0.5, gpu)
    W = D.dparf_forward_weights(hip, pts, cen, rot, views=8, check=False)
    want = np.zeros(W.shape, bool)
    np.put_along_axis(want, idx, True, axis=1)
    assert (want.sum(1) == K).all()
    bad = np.nonzero(((W != 0) != want).any(1))[0]
    print(f"{name} K={K}: {pts.shape[0]} points x {cen.shape[0]} centres, points with a wrong neighbour set: {bad.size}")
    assert bad.size == 0, (bad[:5], [np.nonzero(W[p])[0] for p in bad[:3]], idx[bad[:3]])
    assert float(np.abs(W.sum(1) - 1).max()) < 1e-6


# ---- 2: weights --------------------------------------------------------------------------------------------------------------
def _weight_ref(name, K, alpha):
    """-> float64 softmax weights [P,K], their derived relative bound [P,K], max |x| per point [P], the oracle's indices"""
    d2, idx = _knn(name, K)
    a32 = float(np.float32(alpha))
    x = -np.sqrt(d2.astype(np.float64)) / a32
    t = x - x.max(1, keepdims=True)
    e = np.exp(t)
    rho = HALF * (2 * np.abs(x) + 2 * np.abs(x).min(1, keepdims=True) + np.abs(t)) + ULP
    rel = (rho + rho.max(1, keepdims=True) + (K + 1) * HALF) * 1.001
    return e / e.sum(1, keepdims=True), rel, np.abs(x).max(1), idx


@pytest.mark.parametrize("name", ["body7", "body500", "edge"])
@pytest.mark.parametrize("K,alpha", [(7, 0.05), (7, 0.25), (7, 2.0), (7, 1000.0), (3, 0.25)])
def test_weights_are_the_float64_softmax(hip, gpu, K, alpha, name):
    pts, cen, rot = _dev(name, gpu)
    hip.set_dparf(K, 10, alpha, gpu)
    W = D.dparf_forward_weights(hip, pts, cen, rot, views=8, check=False)
    w64, rel, xmax, idx = _weight_ref(name, K, alpha)
    got = np.take_along_axis(W, idx, axis=1)
    other = W.copy()
    np.put_along_axis(other, idx, 0.0, axis=1)
    assert (other == 0).all()                                     # nothing outside the oracle's K
    big = w64 >= 2.0 ** -100
    err = np.abs(got - w64)
    r_rel = float((err[big] / (rel * w64)[big]).max())
    small_ok = bool((got[~big] <= 2.0 ** -99).all())
    calm = xmax <= 4.8
    r_abs = float(err[calm].max() / 2e-6) if calm.any() else 0.0
    print(f"{name} K={K} alpha={alpha}: worst error / relative bound = {r_rel:.3f} (bound up to {rel.max():.2e}, max |x| {xmax.max():.1f}), "
          f"{int((~big).sum())} weights under 2^-100, {int(calm.sum())} calm points with worst error / 2e-6 = {r_abs:.3f}")
    assert (err[big] <= (rel * w64)[big]).all(), r_rel
    assert small_ok
    assert (err[calm] <= 2e-6).all(), r_abs


@pytest.mark.parametrize("name", ["body13", "lattice"])
def test_one_neighbour_copies_its_token(hip, gpu, name):
    """K = 1: the weight is exactly 1.0 and the token part of a row is tokens[v, idx], bit for bit"""
    pts, cen, rot = _dev(name, gpu)
    _, idx = _knn(name, 1)
    tok = _seeded_tokens(cen.shape[0])
    hip.set_dparf(1, 10, 0.5, gpu)
    W = D.dparf_forward_weights(hip, pts, cen, rot, views=8, check=False)
    assert ((W != 0).sum(1) == 1).all() and (np.take_along_axis(W, idx, axis=1) == 1.0).all()
    out = hip.dparf_encode(pts, cen, rot, tok.to(gpu)).cpu()
    assert torch.equal(out[..., :192], tok[:, torch.from_numpy(idx[:, 0].copy())].permute(1, 0, 2))


# ---- 3: rows -----------------------------------------------------------------------------------------------------------------
def _pe_bounds(name, K, F_, w, idx):
    c = D.case(name)
    r = c.pts.astype(np.float64)[:, None, :] - c.cen.astype(np.float64)[idx]
    R = c.rot.astype(np.float64).reshape(-1, 3, 3)[idx]
    de = np.einsum("pkj,pkjc->pkc", r, R)
    f32pi, f32hpi = float(np.float32(np.pi)), float(np.float32(np.pi * 0.5))
    lit = [4 * ULP * np.abs(de)]
    for o in range(F_):
        for ph in (0.0, f32hpi):
            lit.append(5 * ULP * np.abs(de * (f32pi * 2.0 ** o) + ph))
    lit = np.concatenate(lit, -1)                                                                # [P,K,3 + 6 F]
    return (w[..., None] * lit).sum(1) + 2e-6


def _check_rows(name, K, F_, alpha, got, tok, ref):
    """got [P,V,256] float64 against ref [P,V,195 + 6 F] float64 (the oracle or a recording, on the oracle's selection)"""
    n = 195 + 6 * F_
    assert got.shape[2] == 256 and ref.shape[2] == n and np.isfinite(got).all()
    assert (got[..., n:] == 0).all()                                           # columns 195 + 6 F .. 255: exact zero
    for v in range(1, got.shape[1]):
        assert np.array_equal(got[:, 0, 192:], got[:, v, 192:])                # the PE part does not depend on the view
    w64, rel, _, idx = _weight_ref(name, K, alpha)
    tmag = np.abs(tok.double().numpy()[:, idx])                                                  # [V,P,K,192]
    tol_tok = np.moveaxis((((rel + K * HALF) * w64)[None, :, :, None] * tmag).sum(2), 0, 1)
    e_tok = np.abs(got[..., :192] - ref[..., :192])
    lit = _pe_bounds(name, K, F_, w64, idx)
    err = np.abs(got[..., 192:n] - ref[..., 192:])
    r_tok, r_lit = float((e_tok / tol_tok).max()), float((err / lit[:, None, :]).max())
    print(f"{name} K={K} F={F_}: tokens worst error / bound {r_tok:.3f}; xyz/PE worst error / bound {r_lit:.3f} "
          f"(max error {err.max():.2e}, largest bound {lit.max():.2e})")
    assert (e_tok <= tol_tok).all(), r_tok
    assert (err <= lit[:, None, :]).all(), r_lit


@pytest.mark.parametrize("name", ["body13", "body500", "edge"])
@pytest.mark.parametrize("K,F_", [(1, 1), (3, 6), (5, 10), (7, 4)])
def test_rows_match_the_float64_oracle(hip, gpu, K, F_, name):
    c = D.case(name)
    pts, cen, rot = _dev(name, gpu)
    tok = _seeded_tokens(c.cen.shape[0])
    hip.set_dparf(K, F_, 0.5, gpu)
    got = hip.dparf_encode(pts, cen, rot, tok.to(gpu)).double().cpu().numpy()
    ref = O.dparf(torch.from_numpy(c.pts).double(), torch.from_numpy(c.cen), D.blend_of(c.rot), tok.double(), K=K, n_freq=F_,
                  alpha=0.5).numpy()
    _check_rows(name, K, F_, 0.5, got, tok, ref)


# ---- 4: layout edges -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full_b(hip, gpu):
    pts, cen, rot = _dev("body500", gpu)
    tok = _seeded_tokens(cen.shape[0]).to(gpu)
    hip.set_dparf(3, 6, 0.25, gpu)
    full = hip.dparf_encode(pts, cen, rot, tok).cpu()
    hip.set_dparf(*DEFAULT, gpu)
    return full


@pytest.mark.parametrize("P", [1, 127, 128, 129, 257])
def test_layout_edges(hip, gpu, full_b, P):
    """sample counts around the 128-sample workgroup at (3, 6, 0.25): a row depends on its own point only, rows beyond P untouched"""
    lib = hip.load_library()
    pts, cen, rot = _dev("body500", gpu)
    tok = _seeded_tokens(cen.shape[0]).to(gpu)
    hip.set_dparf(3, 6, 0.25, gpu)
    out = hip.dparf_encode(pts[:P].contiguous(), cen, rot, tok)
    assert torch.equal(out.cpu(), full_b[:P])
    buf = torch.full((P + 3, 2, 256), float("nan"), device=gpu)
    rc = lib.th_dparf_encode(hip.ctx(gpu), hip._p(pts), None, P, hip._p(cen), hip._p(rot), hip._p(tok), 2, cen.shape[0],
                             hip._p(buf), hip._stream())
    assert rc == 0
    assert torch.equal(buf[:P].cpu(), full_b[:P]) and torch.isnan(buf[P:]).all()


# ---- 5: records ----------------------------------------------------------------------------------------------------------------
def test_records_mark_their_unused_pairs(hip, gpu):
    """TH_ROWS_REC at K = 3, read where the backward keeps it (the head of its workspace): words 0..2 the oracle's indices,
    3..7 0xffffffff, 8..10 the forward's weights, 11..15 zero.  (The TH_ROWS_NBR buffer lives inside the render workspace and has no
    accessor: its records are covered by the frames of tests/test_gpu_dparf_params_frames.py, whose fused kernels consume them.)"""
    lib = hip.load_library()
    name, K, V = "body500", 3, 1
    pts, cen, rot = _dev(name, gpu)
    P, nc = pts.shape[0], cen.shape[0]
    _, idx = _knn(name, K)
    hip.set_dparf(K, 6, 0.25, gpu)
    W = D.dparf_forward_weights(hip, pts, cen, rot, views=8, check=False)
    nb = int(lib.th_dparf_encode_bwd_workspace_bytes(P, V, nc))
    ws = torch.full((nb // 4 + 1,), 0x5a5a5a5a, dtype=torch.int32, device=gpu)
    g = torch.zeros((P, V, 256), device=gpu)
    out = torch.empty((V, nc, 192), device=gpu)
    assert lib.th_dparf_encode_bwd(hip.ctx(gpu), hip._p(pts), P, hip._p(cen), hip._p(rot), V, nc, hip._p(g), hip._p(out), hip._p(ws),
                                   nb, hip._stream()) == 0
    rec = ws[:P * 16].cpu().numpy().reshape(P, 16)
    assert np.array_equal(rec[:, :K], idx.astype(np.int32))
    assert (rec[:, K:8] == -1).all()                                           # 0xffffffff
    assert (rec[:, 8 + K:] == 0).all()                                         # +0.0
    w = rec[:, 8:8 + K].copy().view(np.float32).astype(np.float64)
    assert np.array_equal(w, np.take_along_axis(W, idx, axis=1))


# ---- 6: backward ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3, 6])
def test_backward_is_the_adjoint_of_the_forward(hip, gpu, K):
    """(n + 2) 2^-24 sum |W g| per element, n = the number of non-zero terms (tests/test_gpu_train_ops.py), exact zeros where
    nothing contributes; bit-identical in two runs"""
    name, V = "body500", 3
    pts, cen, rot = _dev(name, gpu)
    P, nc = pts.shape[0], cen.shape[0]
    g = torch.from_numpy(np.random.RandomState(40 + K).normal(size=(P, V, 256)).astype(np.float32)).to(gpu)
    hip.set_dparf(K, 10, 0.5, gpu)
    Wm = torch.from_numpy(D.dparf_forward_weights(hip, pts, cen, rot, views=8, check=False))
    assert ((Wm != 0).sum(1) == K).all()
    out = torch.full((V, nc, 192), float("nan"), device=gpu)
    got = hip.dparf_encode_bwd(pts, cen, rot, g, out=out)
    again = hip.dparf_encode_bwd(pts, cen, rot, g)
    assert torch.equal(got, again)
    g64 = g[..., :192].double().cpu()
    ref = torch.einsum("pc,pvj->vcj", Wm, g64).numpy()
    mag = torch.einsum("pc,pvj->vcj", Wm.abs(), g64.abs()).numpy()
    n = np.rint(torch.einsum("pc,pvj->vcj", (Wm != 0).double(), torch.ones_like(g64)).numpy())
    got = got.double().cpu().numpy()
    assert np.isfinite(got).all() and (got[n == 0] == 0).all()
    tol = (n + 2) * HALF * mag
    err = np.abs(got - ref)
    worst = float((err / np.maximum(tol, 1e-300))[n > 0].max())
    print(f"K={K}: n up to {int(n.max())}, worst error / bound = {worst:.3f}")
    assert (err <= tol).all(), worst


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_values(hip, gpu):
    for bad in ((0, 10, 0.5), (8, 10, 0.5), (7, 0, 0.5), (7, 11, 0.5), (7, 10, 0.0), (7, 10, -1.0), (7, 10, float("inf")),
                (7, 10, float("nan"))):
        with pytest.raises(hip.HipError, match="KNN = %d, KNN_FREQ = %d" % bad[:2]):
            hip.set_dparf(*bad, gpu)
    assert hip.dparf_in_force(gpu) == DEFAULT                       # a refused call changes nothing
    pts = torch.zeros((5, 3), device=gpu)
    args = lambda nc: (pts, torch.zeros((nc, 3), device=gpu), torch.zeros((nc, 9), device=gpu), torch.zeros((1, nc, 192), device=gpu))
    hip.set_dparf(3, 10, 0.5, gpu)
    with pytest.raises(hip.HipError, match="at least 3 token centres"):
        hip.dparf_encode(*args(2))
    assert hip.dparf_encode(*args(3)).shape == (5, 1, 256)          # fewer than seven centres: the full scan, no grid
