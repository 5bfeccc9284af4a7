"""CPU: the rank-ordered gradient exchange and the SyncBatchNorm backward's definition.

GradExchange(reduce="rank_ordered", backend="torch") with three gloo ranks on host tensors (one process per rank, as
test_train_dist_host.py): all_to_all_single, torch additions in rank order, all_gather_into_tensor.  Every tensor equals
train_dist.grad_exchange_oracle bit for bit, at 2 * (world - 1) * slice * 4 bytes received per rank.  The gradients hold elements
whose bits the ORDER decides: quotients (1e8, -1e8, 1) give 1 in rank order and 0 in the order (1, 2, 0).

train_ops.sync_bn_act_bwd_oracle, the float64 numpy restatement of th_bn_act_bwd_sums / _apply, against torch float64 autograd of
plain BatchNorm (+ residual, + ReLU) on the concatenated batch, for 1, 2 and 3 ranks with unequal batches; cfg.train_sync_bn."""
import numpy as np
import pytest
import torch
import torch.distributed as dist

from test_train_dist_host import _init, _spawn, bits
from transhuman_amd import config
from transhuman_amd import train_dist as TD
from transhuman_amd import trainer as TR

WORLD = 3
# tensor 2: rank 1 has no gradient; tensor 4: no rank has one.  22 live elements -> flat_elems 32 (slots 4 + 8 + 8 + 12), which
# 3 * 4 does not divide: slice 12, capacity 36, a zero tail of 4
COUNTS = [3, 7, 5, 9, 6]
STEPS = 2


def local_gradient(rank, step, i):
    if i == 4 or (i == 2 and rank == 1):
        return None
    rs = np.random.RandomState(1000 * step + 10 * rank + i)
    n = COUNTS[i]
    g = (rs.standard_normal(n) * np.exp(rs.uniform(-10, 10, n))).astype(np.float32)
    if i == 1:                                                           # (3e8, -3e8, 3) / 3: the order decides the bits
        g[:2] = np.float32((3e8, -3e8, 3.0)[rank])
    if i == 3:
        g[:3] = [(np.inf, 1.0, -0.0), (1.0, np.nan, -0.0), (-np.inf, 2.0, -0.0)][rank]
        g[3] = np.float32((4e-45, 1e-40, -3e-39)[rank])                  # subnormals, and quotients that become some
    return g


def test_the_planted_triples_tell_the_orders_apart():
    q = [np.float32(v) / np.float32(3) for v in (3e8, -3e8, 3.0)]
    assert (q[0] + q[1]) + q[2] == 1.0 and (q[1] + q[2]) + q[0] == 0.0


def _worker(rank, world, port, q):
    _init(rank, world, port)
    try:
        params = [torch.nn.Parameter(torch.zeros(n)) for n in COUNTS]
        ex = TD.GradExchange(params, reduce="rank_ordered", backend="torch")
        rec = {"reduce": ex.reduce, "backend": ex.backend, "exchanged": [], "bytes": [], "slice": [], "flat": [], "tail": []}
        for step in range(STEPS):
            for i, p in enumerate(params):
                g = local_gradient(rank, step, i)
                if step == 0 or g is None:
                    p.grad = None if g is None else torch.from_numpy(g.copy())
                else:
                    p.grad.copy_(torch.from_numpy(g))                    # the second exchange packs in place
            flat = ex.exchange()
            lay = ex.layout
            rec["exchanged"].append([None if p.grad is None else p.grad.numpy().copy() for p in params])
            rec["bytes"].append(ex.bytes_received)
            rec["slice"].append(lay.slice)
            rec["flat"].append((flat.numel(), lay.flat.numel()))
            rec["tail"].append(lay.flat[lay.flat_elems:].numpy().copy())
            ok = all(p.grad is None or p.grad.data_ptr() == flat.data_ptr() + 4 * int(lay.offsets[i])
                     for i, p in enumerate(params))
            rec["views"] = rec.get("views", True) and ok
        q.put((rank, rec))
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def run():
    return _spawn(_worker, WORLD)


def test_three_ranks_equal_the_oracle_bit_for_bit(run):
    assert all(r["reduce"] == "rank_ordered" and r["backend"] == "torch" and r["views"] for r in run)
    for step in range(STEPS):
        local = [[local_gradient(r, step, i) for i in range(len(COUNTS))] for r in range(WORLD)]
        want = TD.grad_exchange_oracle(local, WORLD)
        assert want[4] is None and want[2] is not None
        for r in range(WORLD):
            for i, (w, got) in enumerate(zip(want, run[r]["exchanged"][step])):
                assert (w is None) == (got is None), (step, r, i)
                if w is None:
                    continue
                ok = ~np.isnan(w)
                assert np.array_equal(bits(got)[ok], bits(w)[ok]) and np.isnan(got[~ok]).all(), (step, r, i)
        got = run[0]["exchanged"][step]
        assert got[1][0] == 1.0 and got[1][1] == 1.0                     # rank order, not (1, 2, 0)'s 0
        assert np.isnan(got[3][0]) and np.isnan(got[3][1]) and bits(got[3][2:3])[0] == 0x80000000      # inf - inf, NaN, -0.0


def test_traffic_is_a_ring_all_reduces(run):
    flat_elems = TD.flat_layout(COUNTS, [1, 1, 1, 1, 0])[1]
    slice_ = TD.rank_slice(flat_elems, WORLD)
    assert (flat_elems, slice_) == (32, 12) and flat_elems % (WORLD * 4) != 0
    for r in run:
        assert r["slice"] == [slice_] * STEPS and r["flat"] == [(flat_elems, WORLD * slice_)] * STEPS
        assert r["bytes"] == [2 * (WORLD - 1) * slice_ * 4 * (s + 1) for s in range(STEPS)]
        assert all(t.size == WORLD * slice_ - flat_elems and not bits(t).any() for t in r["tail"])      # the tail stays +0
    assert 2 * (WORLD - 1) * slice_ * 4 < (WORLD - 1) * flat_elems * 4                                   # (what "ordered" receives)


def test_rank_slice():
    for flat in (0, 4, 8, 32, 36, 7420812):
        for world in (1, 2, 3, 5, 8, 64):
            s = TD.rank_slice(flat, world)
            assert s % 4 == 0 and world * s >= flat and (s == 0 or world * (s - 4) < flat)
    assert TD.rank_slice(32, 1) == 32 and TD.rank_slice(32, 3) == 12 and TD.rank_slice(33, 2) == 20


def test_reduce_values():
    p = [torch.nn.Parameter(torch.zeros(3))]
    assert TD.GradExchange(p, reduce="rank_ordered").reduce == "rank_ordered"
    assert TD.GradExchange(p).reduce == "collective"                    # the default stays one all_reduce
    with pytest.raises(ValueError, match="reduce"):
        TD.GradExchange(p, reduce="rank-ordered")
    # without a process group the exchange is local, whatever the reduce: no collective, no extra capacity, nothing received
    p[0].grad = torch.tensor([3.0, 6.0, 9.0])
    ex = TD.GradExchange(p, world=3, reduce="rank_ordered")
    flat = ex.exchange()
    assert flat.tolist() == [1.0, 2.0, 3.0, 0.0] and ex.layout.flat.numel() == 4 and ex.bytes_received == 0


def test_trainer_and_fit_take_reduce():
    import inspect
    for fn in (TR.Trainer.__init__, TR.fit):
        assert inspect.signature(fn).parameters["reduce"].default is None


# ---------------------------------------------------------------------------
# the SyncBatchNorm backward's definition
# ---------------------------------------------------------------------------
def _torch64(ys, gs, res, gamma, beta, eps, relu):
    """plain BatchNorm (+ residual) (+ ReLU) on the concatenated batch, float64 autograd -> (out, g_y, g_res, g_gamma, g_beta)"""
    y = torch.from_numpy(np.concatenate(ys)).requires_grad_(True)
    r = None if res is None else torch.from_numpy(np.concatenate(res)).requires_grad_(True)
    gm, bt = torch.from_numpy(gamma).requires_grad_(True), torch.from_numpy(beta).requires_grad_(True)
    out = torch.nn.functional.batch_norm(y, None, None, gm, bt, True, 0.1, eps)
    if r is not None:
        out = out + r
    if relu:
        out = torch.relu(out)
    out.backward(torch.from_numpy(np.concatenate(gs)))
    return (out.detach().numpy(), y.grad.numpy(), None if r is None else r.grad.numpy(), gm.grad.numpy(), bt.grad.numpy())


@pytest.mark.parametrize("batches", [(2,), (1, 3), (2, 1, 3)], ids=["1", "2", "3"])
@pytest.mark.parametrize("relu, residual", [(True, True), (True, False), (False, False)])
def test_sync_bn_oracle_equals_float64_autograd_of_the_concatenated_batch(batches, relu, residual):
    from transhuman_amd.networks.train_ops import sync_bn_act_bwd_oracle
    rs = np.random.RandomState(len(batches) * 10 + relu + 2 * residual)
    C, H, W, eps = 5, 3, 7, 1e-5
    mean, std = rs.uniform(-3, 3, C), np.exp(rs.uniform(-2, 2, C))
    # (every rank's pivot is another element.  The channel with mean 1e3 and std 1e-2 belongs to the device tests: there the
    # reference is this oracle; torch's float64 BatchNorm, which subtracts an unshifted mean, is itself 1e-11 off on it)
    ys = [mean[None, :, None, None] + std[None, :, None, None] * rs.standard_normal((n, C, H, W)) for n in batches]
    gs = [rs.standard_normal(y.shape) * 7 for y in ys]
    res = [rs.standard_normal(y.shape) for y in ys] if residual else None
    gamma, beta = rs.uniform(0.5, 2, C), rs.uniform(-1, 1, C)
    out, g_y, g_res, g_gamma, g_beta = _torch64(ys, gs, res, gamma, beta, eps, relu)
    cuts = np.cumsum((0,) + batches)
    outs = [out[a:b] if relu else None for a, b in zip(cuts[:-1], cuts[1:])]
    got = sync_bn_act_bwd_oracle(ys, outs, gs, gamma, eps)
    assert len(got) == len(batches)

    worst = [0.0]

    def close(a, b):
        worst[0] = max(worst[0], float(np.abs(a - b).max()) / float(np.abs(b).max()))
        return float(np.abs(a - b).max()) <= 1e-12 * float(np.abs(b).max())

    for (a, b), (gy, gp, _, _) in zip(zip(cuts[:-1], cuts[1:]), got):
        assert gy.dtype == np.float64 and close(gy, g_y[a:b])
        if residual:
            assert np.array_equal(gp, g_res[a:b])                        # the gated gradient IS the residual's
    assert close(sum(g[2] for g in got), g_gamma) and close(sum(g[3] for g in got), g_beta)    # the LOCAL sums add up
    print(f"{len(batches)} ranks: worst relative difference {worst[0]:.2e}")
    if len(batches) == 1:
        return
    # one rank alone is NOT the answer: the statistics are those of all ranks
    alone = sync_bn_act_bwd_oracle(ys[:1], outs[:1], gs[:1], gamma, eps)[0][0]
    assert not close(alone, g_y[:batches[0]])


def test_train_sync_bn_key():
    from transhuman_amd.networks import autograd_path as AP
    assert "train_sync_bn" not in config.TRAIN_SWITCHES and config.TRAIN_SYNC_BN == ("torch", "device")
    assert config.get_cfg().train_sync_bn == "torch"
    assert AP._sync_bn_mode("torch") == "torch" and AP._sync_bn_mode("device") == "device"
    for bad in ("Device", "", "hip", None, 1):
        with pytest.raises(ValueError, match="train_sync_bn"):
            AP._sync_bn_mode(bad)


def test_sync_sites_are_recognised_without_a_device():
    """which trunks cfg.train_sync_bn speaks about: every site train-mode with a momentum, at least one a SyncBatchNorm"""
    from transhuman_amd.networks import autograd_path as AP

    class Enc:
        def __init__(self, sites):
            self.sites = sites

        def _bn_sites(self):
            return self.sites

    bn, sbn = torch.nn.BatchNorm2d(4), torch.nn.SyncBatchNorm(4)
    assert AP._trunk_sites_have_batch_statistics(Enc([bn])) and not AP._trunk_sync_sites(Enc([bn]))
    assert AP._trunk_sync_sites(Enc([sbn, bn])) and not AP._trunk_sites_have_batch_statistics(Enc([sbn, bn]))
    assert not AP._trunk_sync_sites(Enc([sbn, torch.nn.SyncBatchNorm(4).eval()]))
    assert not AP._trunk_sync_sites(Enc([torch.nn.SyncBatchNorm(4, momentum=None)]))
