"""GPU, one process: K23's BatchNorm backward split for SyncBatchNorm sites -- th_bn_act_bwd_sums / th_bn_act_bwd_apply
(k_encoder_bwd.hip).

World 1: the launch pair equals th_bn_act_bwd bit for bit.

Simulated ranks: a batch is cut into 2 and 3 "ranks" of 1, 2 and 3 images, every rank's record is taken on its own part and the
records are concatenated here, as the all_gather of train_ops.SyncBnActFn would.  The reference is
train_ops.sync_bn_act_bwd_oracle, the float64 restatement (tied to torch float64 autograd of plain BatchNorm on the concatenated
batch by tests/test_train_dist_rank_ordered_host.py).  The bar is the one of tests/test_gpu_train_encoder.py: with d32 torch's fp32
autograd ON THE DEVICE of plain BatchNorm (+ residual) (+ ReLU) on the concatenated batch,

    parent = max|d32 - ref|,  scale = max|ref|,    bar = 4 max(parent, 2^-24 scale)

per gradient tensor; g_y is compared rank by rank (scale and parent over the whole batch), g_gamma and g_beta as the float64 sum
of the ranks' fp32 LOCAL results against the gradient of the whole batch.  In two of the four splits channel 0 has mean 1e3 and
standard deviation 1e-2, so the ranks' pivots differ by about one standard deviation of a channel whose mean is 1e5 of them
(torch's fp32 error on that channel sets the bar of those cases; the other two splits hold the ordinary channels tightly).  As in
the K23 tests, no gradient arrives where the float64 pre-activation of a ReLU lies within 1e-3 of 0."""
import numpy as np
import pytest
import torch

from test_gpu_train_encoder import FLOOR, SIZES, _bn_autograd, _f32
from transhuman_amd.networks import train_ops

pytestmark = pytest.mark.gpu

NAMES = ("g_y", "g_res", "g_gamma", "g_beta")
EPS = 1e-5
SPLITS = ((1, 3), (2, 2), (2, 1, 3), (3, 1, 1))
VARIANTS = ((1, 1, 1), (0, 0, 1), (0, 1, 0))         # residual, relu, affine
EXTREME = ((1, 3), (2, 1, 3))                        # the splits whose channel 0 has mean 1e3 and standard deviation 1e-2


@pytest.fixture(scope="module")
def hip(gpu):
    from transhuman_amd import hip as H
    H.load_library()
    return H


def _slice_elems():
    from transhuman_amd import build, hip as H
    build.build(force=False, verbose=False)
    return H.bn_act_bwd_slice_elems()


def pytest_generate_tests(metafunc):
    if "sync_size" in metafunc.fixturenames:
        sl = _slice_elems()
        assert sl == 8192
        # L_r = N_r HW with N_r in 1 .. 3: below, at and above one, two and three slices
        sizes = SIZES + ((1, sl - 1), (64, sl // 64), (3, (sl + 1) // 3))
        metafunc.parametrize("sync_size", sizes, ids=lambda s: f"{s[0]}x{s[1]}")


# ---------------------------------------------------------------------------
# world 1 IS th_bn_act_bwd
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,hw", ((3, (9, 17)), (1, (1, 1)), (3, (64, 129))), ids=("3x9x17", "1x1x1", "3x64x129"))
@pytest.mark.parametrize("residual,relu,affine", ((0, 0, 0), (1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0)))
@pytest.mark.parametrize("C", (64, 128))
def test_one_rank_equals_bn_act_bwd_bit_for_bit(hip, gpu, C, residual, relu, affine, N, hw):
    rs = np.random.RandomState(C + N + hw[1] + 2 * residual + 4 * relu + 8 * affine)
    shape = (N, C, *hw)
    y = _f32(rs.normal(size=shape) * rs.uniform(0.1, 3, (1, C, 1, 1)) + rs.uniform(-50, 50, (1, C, 1, 1))).to(gpu)
    g = _f32(rs.normal(size=shape)).to(gpu)
    out = _f32(np.maximum(rs.normal(size=shape), 0)).to(gpu) if relu else None
    gamma = _f32(rs.normal(size=C) + 1.0).to(gpu) if affine else None
    want = hip.bn_act_bwd(y, out, g, gamma, EPS, need_residual=bool(residual), need_affine=bool(affine))
    record = hip.bn_act_bwd_sums(y, out, g)
    assert record.shape == (C, 6) and record.dtype is torch.float64
    assert torch.equal(record[:, 4], y[0, :, 0, 0].double()) and bool((record[:, 5] == N * hw[0] * hw[1]).all())
    got = hip.bn_act_bwd_apply(y, out, g, gamma, EPS, record[None], 0, need_residual=bool(residual), need_affine=bool(affine))
    for k, a, b in zip(NAMES, got, want):
        assert (a is None) == (b is None), k
        assert a is None or torch.equal(a, b), f"{k}: not th_bn_act_bwd's bits"
    assert torch.equal(record, hip.bn_act_bwd_sums(y, out, g)), "the record is not bit-identical on two runs"


# ---------------------------------------------------------------------------
# simulated ranks
# ---------------------------------------------------------------------------
C_BN = 64


def _case(split, hw, residual, relu, affine):
    """the concatenated batch, made once: fp32 inputs, the site's output from the float64 forward, and the float64 reference"""
    N, (H, W) = sum(split), hw
    shape = (N, C_BN, H, W)
    rs = np.random.RandomState(N + 3 * H + 5 * W + 7 * residual + 11 * relu + 13 * affine + 17 * len(split))
    mean, std = rs.uniform(-3, 3, C_BN), np.exp(rs.uniform(-1, 1, C_BN))
    if split in EXTREME:
        mean[0], std[0] = 1e3, 1e-2
    y = _f32(mean[None, :, None, None] + std[None, :, None, None] * rs.normal(size=shape))
    g = _f32(rs.normal(size=shape))
    res = _f32(rs.normal(size=shape)) if residual else None
    gamma, beta = (_f32(rs.normal(size=C_BN) + 1.0), _f32(rs.normal(size=C_BN))) if affine else (None, None)
    d = lambda v: None if v is None else v.double()
    out = None
    if relu:
        with torch.no_grad():
            pre = torch.batch_norm(d(y), d(gamma), d(beta), None, None, True, 0.1, EPS, False) + (0 if res is None else d(res))
        near = pre.abs() < 1e-3
        assert float(near.double().mean()) < 0.05 or N * H * W < 64
        g = torch.where(near, torch.zeros_like(g), g)
        out = torch.relu(pre).float()
    cuts = np.cumsum((0,) + split)
    parts = [slice(int(a), int(b)) for a, b in zip(cuts[:-1], cuts[1:])]
    ref = train_ops.sync_bn_act_bwd_oracle([y[p] for p in parts], [None if out is None else out[p] for p in parts],
                                           [g[p] for p in parts], gamma, EPS)
    t64 = {"g_y": torch.from_numpy(np.concatenate([r[0] for r in ref]))}
    if residual:
        t64["g_res"] = torch.from_numpy(np.concatenate([r[1] for r in ref]))
    if affine:
        t64["g_gamma"] = torch.from_numpy(sum(r[2] for r in ref))
        t64["g_beta"] = torch.from_numpy(sum(r[3] for r in ref))
    return (y, res, g, gamma, beta, out), parts, t64


def _run_ranks(hip, gpu, t, parts, residual, affine):
    y, _, g, gamma, _, out = (None if v is None else v.to(gpu) for v in t)
    per = [(y[p].contiguous(), None if out is None else out[p].contiguous(), g[p].contiguous()) for p in parts]
    records = torch.stack([hip.bn_act_bwd_sums(*a) for a in per])     # what the all_gather delivers to every rank
    assert records.shape == (len(parts), C_BN, 6)
    got = [hip.bn_act_bwd_apply(*a, gamma, EPS, records, r, need_residual=residual, need_affine=affine) for r, a in enumerate(per)]
    again = [hip.bn_act_bwd_apply(*a, gamma, EPS, records, r, need_residual=residual, need_affine=affine) for r, a in enumerate(per)]
    for a, b in zip(got, again):
        assert all((u is None and v is None) or torch.equal(u, v) for u, v in zip(a, b)), "not bit-identical on two runs"
    res = {"g_y": torch.cat([a[0] for a in got]).cpu().double()}
    if residual:
        res["g_res"] = torch.cat([a[1] for a in got]).cpu().double()
    if affine:                                                         # the LOCAL sums, added as the exchange's average would
        res["g_gamma"] = sum(a[2].cpu().double() for a in got)
        res["g_beta"] = sum(a[3].cpu().double() for a in got)
    return res, records


def _bars(gpu, t, t64, relu):
    y, res, g, gamma, beta, _ = (None if v is None else v.to(gpu) for v in t)
    _, d32 = _bn_autograd(y, res, g, gamma, beta, relu, EPS)
    bars = {}
    for k, ref in t64.items():
        parent = float((d32[k].cpu().double() - ref).abs().max())
        bars[k] = (4.0 * max(parent, FLOOR * float(ref.abs().max())), parent)
    return bars


@pytest.mark.parametrize("residual,relu,affine", VARIANTS)
@pytest.mark.parametrize("split", SPLITS, ids=lambda s: "+".join(map(str, s)))
def test_simulated_ranks_vs_float64(hip, gpu, split, sync_size, residual, relu, affine):
    t, parts, t64 = _case(split, sync_size, bool(residual), bool(relu), bool(affine))
    got, records = _run_ranks(hip, gpu, t, parts, bool(residual), bool(affine))
    assert set(got) == set(t64)
    y = t[0]
    for r, p in enumerate(parts):                                      # every rank's own pivot and element count
        assert torch.equal(records[r, :, 4].cpu(), y[p][0, :, 0, 0].double())
        assert bool((records[r, :, 5] == (p.stop - p.start) * sync_size[0] * sync_size[1]).all())
    assert len({float(records[r, 0, 4]) for r in range(len(parts))}) > 1          # channel 0: the pivots differ
    worst, failed = 0.0, []
    for k, (bar, parent) in _bars(gpu, t, t64, bool(relu)).items():
        assert got[k].shape == t64[k].shape and torch.isfinite(got[k]).all(), k
        err = float((got[k] - t64[k]).abs().max())
        ratio = err / bar if bar > 0 else (0.0 if err == 0 else float("inf"))
        worst = max(worst, ratio)
        print(f"{k}: device {err:.3e}, torch fp32 {parent:.3e}, max|ref| = {float(t64[k].abs().max()):.3e}; err / bar = {ratio:.3f}")
        if not err <= bar:
            failed.append((k, err, bar))
    print(f"sync bn {split} {sync_size} res={residual} relu={relu} affine={affine}: worst err / bar = {worst:.3f}")
    assert not failed, failed


@pytest.mark.parametrize("split,hw", (((1, 2), (9, 17)), ((3, 1, 2), (33, 47)), ((1, 1), (1, 1)), ((2, 3, 1), (64, 129))))
def test_small_integers_are_exact(hip, gpu, split, hw):
    """integer inputs, a tenth of the site's outputs exactly 0 (and the ReLU's zeros on top): the gate [out > 0], the residual's
    gradient and the LOCAL g_beta -- an integer sum -- are exact on every rank; the records' four sums are integers, so they are
    exact too; g_y and the LOCAL g_gamma are held to the float64 restatement at 4 * 2^-24 (the kernel rounds once from fp64)"""
    N = sum(split)
    rs = np.random.RandomState(N + hw[0])
    shape = (N, C_BN, *hw)
    y, g = _f32(rs.randint(-3, 4, size=shape)), _f32(rs.randint(-4, 5, size=shape))
    out = np.maximum(rs.randint(-2, 6, size=shape), 0)
    out[rs.uniform(size=shape) < 0.1] = 0
    out = _f32(out)
    gamma = _f32(rs.randint(1, 4, size=C_BN))
    cuts = np.cumsum((0,) + split)
    parts = [slice(int(a), int(b)) for a, b in zip(cuts[:-1], cuts[1:])]
    want = train_ops.sync_bn_act_bwd_oracle([y[p] for p in parts], [out[p] for p in parts], [g[p] for p in parts], gamma, EPS)
    per = [(y[p].to(gpu), out[p].to(gpu), g[p].to(gpu)) for p in parts]
    records = torch.stack([hip.bn_act_bwd_sums(*a) for a in per])
    for r, (p, a, w) in enumerate(zip(parts, per, want)):
        yp, gp = y[p].double(), torch.where(out[p] > 0, g[p], torch.zeros_like(g[p])).double()
        dp = yp - yp[0, :, 0, 0][None, :, None, None]
        sums = torch.stack([dp.sum((0, 2, 3)), (dp * dp).sum((0, 2, 3)), gp.sum((0, 2, 3)), (gp * dp).sum((0, 2, 3))], 1)
        assert torch.equal(records[r, :, :4].cpu(), sums), r
        g_y, g_res, g_gamma, g_beta = hip.bn_act_bwd_apply(*a, gamma.to(gpu), EPS, records, r, need_residual=True)
        assert torch.equal(g_res.cpu().double(), gp) and np.array_equal(g_res.cpu().double().numpy(), w[1])
        assert np.array_equal(g_beta.cpu().double().numpy(), w[3])
        for v, ref, k in ((g_y, w[0], "g_y"), (g_gamma, w[2], "g_gamma")):
            err, scale = float(np.abs(v.cpu().double().numpy() - ref).max()), float(np.abs(ref).max())
            print(r, k, err, scale)
            assert err <= 4 * FLOOR * scale, (r, k, err, scale)


def test_refusals(hip, gpu):
    lib, c, p, st = hip.load_library(), hip.ctx(gpu), hip._p, hip._stream()
    x = torch.zeros(2, 64, 3, 5, device=gpu)
    rec = torch.zeros(2, 64, 6, dtype=torch.float64, device=gpu)
    out = torch.full_like(x, 7.0)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=gpu)
    sums = lambda **k: lib.th_bn_act_bwd_sums(k.get("c", c), p(k.get("y", x)), None, p(x), k.get("N", 2), 64, 15, p(k.get("rec", rec)),
                                              p(ws), k.get("ws", ws.numel()), st)
    apply = lambda **k: lib.th_bn_act_bwd_apply(k.get("c", c), p(x), None, p(x), k.get("N", 2), 64, 15, None, k.get("eps", 1e-5),
                                                p(k.get("rec", rec)), k.get("world", 2), k.get("rank", 1), p(out), None, None,
                                                None, st)
    for what, call, name in (("short workspace", lambda: sums(ws=8), b"th_bn_act_bwd_sums"), ("N", lambda: sums(N=0), b"th_bn_act_bwd_sums"),
                             ("null record", lambda: sums(rec=None), b"th_bn_act_bwd_sums"),
                             ("null context", lambda: sums(c=None), b"th_bn_act_bwd_sums"),
                             ("rank", lambda: apply(rank=2), b"th_bn_act_bwd_apply"), ("rank < 0", lambda: apply(rank=-1), b"th_bn_act_bwd_apply"),
                             ("world", lambda: apply(world=0, rank=0), b"th_bn_act_bwd_apply"),
                             ("eps", lambda: apply(eps=0.0), b"th_bn_act_bwd_apply"), ("N", lambda: apply(N=0), b"th_bn_act_bwd_apply"),
                             ("null records", lambda: apply(rec=None), b"th_bn_act_bwd_apply")):
        assert call() != 0, what
        assert name in lib.th_last_error(), (what, lib.th_last_error())
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                    # a refused call wrote nothing
    assert sums() == 0 and apply() == 0
    with pytest.raises(ValueError, match="records"):
        hip.bn_act_bwd_apply(x, None, x, None, EPS, rec.float(), 0)
    with pytest.raises(ValueError, match="records"):
        hip.bn_act_bwd_apply(x, None, x, None, EPS, rec[:, :32], 0)
