"""GPU: the gradient exchange of data-parallel training -- adam_pack_kernel / adam_unpack_kernel (csrc/k_optim.hip) against numpy
bit for bit, the device back end of train_dist.GradExchange against its torch back end, DeviceAdam stepping out of the slot views,
and the distributed trainer.Trainer end to end: two and three ranks on ONE device over gloo (torch.distributed.run, as
test_gpu_multirank.py; RCCL refuses two ranks per device) and one rank over the real transport ("nccl" = RCCL).

"Bit for bit" compares the 32-bit patterns of every element that is not a NaN in the numpy result (signed zeros, subnormals and
infinities included) and requires a NaN exactly where numpy has one, as tests/test_gpu_train_optim.py does: IEEE 754 leaves the
sign and payload of a NaN an operation produces open.  At world = 1 pack copies, and there NaN payloads are compared as well.

The multi-rank checks compare the exchange with train_dist.grad_exchange_oracle ON THE LOCAL GRADIENTS EACH RANK SAVED, which keeps
MIOpen's run-to-run differences out of the comparison.  The Trainer's exchange is ONE all_reduce on every transport: two ranks
equal the oracle bit for bit; three ranks give the sum in an order of the collective's own, which cannot meet the specified
2 * 2^-24 * sum_r |g_r / 3| against the rank-ordered oracle (figures and the bound that does hold: that test's docstring).  The
specified bound is asserted on a third job whose exchange is GradExchange(reduce="ordered")."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from transhuman_amd import train_dist as TD
from transhuman_amd import train_optim as TO

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "train_dist_worker.py")
SENTINEL = 1234.5


@pytest.fixture(scope="module")
def hip(gpu):
    from transhuman_amd import hip as H
    H.load_library()
    return H


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(got, want, what, nan_payload=False):
    got, want = np.asarray(got, np.float32).reshape(-1), np.asarray(want, np.float32).reshape(-1)
    assert got.shape == want.shape, what
    ok = np.ones(want.shape, bool) if nan_payload else ~np.isnan(want)
    bad = np.nonzero(bits(got)[ok] != bits(want)[ok])[0]
    assert bad.size == 0, (what, int(bad.size), got[ok][bad[:4]], want[ok][bad[:4]])
    assert np.isnan(got[~ok]).all(), what


# ---------------------------------------------------------------------------
# the case every pack / unpack test shares
# ---------------------------------------------------------------------------
SPECIAL = np.array([np.inf, -np.inf, np.nan, 0.0, -0.0, 1e-40, -1e-39, 1.4e-45, 3.4e38, -3.4e38, 1.1754944e-38, 3e-38, -2e-38, 1.0,
                    3.0, -7.0], np.float32)     # (1.1754944e-38 / 3, 3e-38 / 8: normal numbers whose quotient is a subnormal)


def values(n, rs):
    g = (rs.standard_normal(n) * np.exp(rs.uniform(-20, 20, n))).astype(np.float32)
    k = min(n, len(SPECIAL))
    at = rs.choice(n, k, replace=False)
    g[at] = SPECIAL[rs.permutation(len(SPECIAL))[:k]]
    return g


class Case:
    """Plan order: the eight sizes around the float4 / chunk edges, a tensor whose storage starts one element off the 16-byte
    grid (the 32-bit path), a present / NULL / present triple, a tensor WITHOUT a slot between two with one."""

    def __init__(self, hip, gpu):
        c = hip.adam_chunk_elems()
        self.sizes = [1, 3, 4, 5, c - 1, c, c + 1, 2 * c + 7, 2 * c + 9, 6, 6, 6, 11, 300, 9]
        self.n = len(self.sizes)
        self.off_one, self.null, self.no_slot = 8, 10, 13
        self.live = np.ones(self.n, np.uint8)
        self.live[self.no_slot] = 0
        rs = np.random.RandomState(25)
        self.host = [values(n, rs) for n in self.sizes]
        self.dev = []
        for i, a in enumerate(self.host):
            buf = torch.full((a.size + 8,), SENTINEL, dtype=torch.float32, device=gpu)
            assert buf.data_ptr() % 16 == 0
            o = 5 if i == self.off_one else 4
            t = buf[o:o + a.size]
            t.copy_(torch.from_numpy(a))
            assert (t.data_ptr() % 16 != 0) == (i == self.off_one)
            self.dev.append((buf, t))
        self.tensors = [t for _, t in self.dev]
        self.plan = hip.AdamPlan(self.tensors)
        self.offsets, self.flat_elems = hip.adam_flat_layout(self.sizes, self.live)
        py_off, py_n = TD.flat_layout(self.sizes, self.live)
        assert np.array_equal(py_off, self.offsets) and py_n == self.flat_elems
        self.grads = [None if i == self.null else t for i, t in enumerate(self.tensors)]

    def expected(self, world, src=None):
        src = self.host if src is None else src
        want = np.zeros(self.flat_elems, np.float32)
        with np.errstate(all="ignore"):
            for i, a in enumerate(src):
                if self.live[i] and i != self.null:
                    o = int(self.offsets[i])
                    want[o:o + a.size] = a if world == 1 else np.float32(a) / np.float32(world)
        return want

    def padding(self):
        pad = np.ones(self.flat_elems, bool)
        for i, n in enumerate(self.sizes):
            if self.live[i]:
                pad[int(self.offsets[i]):int(self.offsets[i]) + n] = False
        return pad

    def guarded_flat(self, gpu, fill_nan=True):
        big = torch.full((self.flat_elems + 8,), SENTINEL, dtype=torch.float32, device=gpu)
        flat = big[4:4 + self.flat_elems]
        if fill_nan:
            flat.view(torch.int32).fill_(-1)                              # every byte 0xFF: a NaN
        return big, flat

    def guards_intact(self, big):
        h = big.cpu().numpy()
        return bool((h[:4] == SENTINEL).all() and (h[-4:] == SENTINEL).all())


@pytest.fixture(scope="module")
def case(hip, gpu):
    return Case(hip, gpu)


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_pack_equals_numpy(case, gpu, world):
    big, flat = case.guarded_flat(gpu)
    case.plan.pack(case.grads, case.offsets, world, flat, case.flat_elems)
    torch.cuda.synchronize()
    got = flat.cpu().numpy()
    want = case.expected(world)
    same_bits(got, want, f"world {world}", nan_payload=world == 1)
    pad = case.padding()
    assert pad.sum() > 10 and not bits(got)[pad].any()                    # the padding and the NULL gradient's slot: +0
    o = int(case.offsets[case.null])
    assert not bits(got)[o:o + case.sizes[case.null]].any()
    assert case.guards_intact(big)                                        # nothing outside flat[0 : flat_elems)
    # the tensor without a slot left no trace: its neighbours' slots are adjacent up to the padding
    a, b = case.no_slot - 1, case.no_slot + 1
    assert case.offsets[case.no_slot] == -1 and case.offsets[b] == (case.offsets[a] + case.sizes[a] + 3) // 4 * 4
    for (buf, t), h in zip(case.dev, case.host):                          # pack reads its sources, nothing else
        same_bits(t.cpu().numpy(), h, "source", nan_payload=True)
        hb = buf.cpu().numpy()
        assert (hb[:4] == SENTINEL).all() and (hb[-3:] == SENTINEL).all()


def test_two_packs_write_identical_bytes(case, gpu):
    outs = []
    for _ in range(2):
        big, flat = case.guarded_flat(gpu)
        case.plan.pack(case.grads, case.offsets, 3, flat, case.flat_elems)
        outs.append(flat.view(torch.int32).cpu().numpy().copy())
    assert np.array_equal(outs[0], outs[1])


@pytest.mark.parametrize("world", [1, 3])
def test_pack_in_place(case, gpu, world):
    """the steady state: gradients that already ARE their slots (every second tensor here), the others out of place"""
    big, flat = case.guarded_flat(gpu)
    grads = list(case.grads)
    for i in range(0, case.n, 2):
        if case.live[i] and i != case.null:
            o = int(case.offsets[i])
            grads[i] = flat[o:o + case.sizes[i]]
            grads[i].copy_(torch.from_numpy(case.host[i]))
            assert grads[i].data_ptr() == flat.data_ptr() + 4 * o
    case.plan.pack(grads, case.offsets, world, flat, case.flat_elems)
    torch.cuda.synchronize()
    got = flat.cpu().numpy()
    same_bits(got, case.expected(world), f"in place, world {world}", nan_payload=world == 1)
    assert not bits(got)[case.padding()].any() and case.guards_intact(big)


def test_unpack_of_pack_is_the_identity(case, hip, gpu):
    big, flat = case.guarded_flat(gpu)
    case.plan.pack(case.tensors, case.offsets, 1, flat, case.flat_elems)          # (every gradient present this time)
    dst = []
    for i, n in enumerate(case.sizes):
        buf = torch.full((n + 8,), SENTINEL, dtype=torch.float32, device=gpu)
        o = 5 if i == case.off_one else 4
        dst.append((buf, buf[o:o + n], o))
    case.plan.unpack([t for _, t, _ in dst], case.offsets, flat, case.flat_elems)
    torch.cuda.synchronize()
    for i, ((buf, t, o), h) in enumerate(zip(dst, case.host)):
        hb = buf.cpu().numpy()
        assert (hb[:o] == SENTINEL).all() and (hb[o + h.size:] == SENTINEL).all(), i   # sentinels on both sides
        if i == case.no_slot:
            assert (hb == SENTINEL).all()                                         # no slot: not touched
        else:
            same_bits(t.cpu().numpy(), h, f"tensor {i}", nan_payload=True)
    assert case.guards_intact(big)


def test_refusals(case, hip, gpu):
    big, flat = case.guarded_flat(gpu)
    wrong = case.offsets.copy()
    wrong[3] += 4
    with pytest.raises(hip.HipError, match="layout"):
        case.plan.pack(case.grads, wrong, 2, flat, case.flat_elems)
    with pytest.raises(hip.HipError):
        case.plan.pack(case.grads, case.offsets, 2, flat[:case.flat_elems - 4], case.flat_elems)      # a short buffer
    with pytest.raises(hip.HipError, match="world"):
        case.plan.pack(case.grads, case.offsets, 0, flat, case.flat_elems)
    with pytest.raises(hip.HipError):
        case.plan.pack(case.grads[:-1], case.offsets[:-1], 2, flat, case.flat_elems)
    with pytest.raises(hip.HipError):
        case.plan.pack(case.grads, case.offsets, 2, flat.cpu(), case.flat_elems)
    none = [None] * case.n
    none[case.no_slot] = case.tensors[case.no_slot]
    with pytest.raises(hip.HipError, match="destination"):
        case.plan.unpack(none, case.offsets, flat, case.flat_elems)
    torch.cuda.synchronize()
    assert bool((flat.view(torch.int32) == -1).all()) and case.guards_intact(big)                   # a refused call wrote nothing


# ---------------------------------------------------------------------------
# GradExchange on the device
# ---------------------------------------------------------------------------
def test_device_back_end_equals_the_torch_back_end_on_the_product_network(hip, gpu):
    """the product Network's parameter list, random gradients on every tensor the reference trains (layer3 / layer4, the dead
    tokens and the PE buffers get none), world = 1, no process group: slot for slot the same bytes"""
    from transhuman_amd import config
    from transhuman_amd.networks.cross_transformer import Network
    torch.manual_seed(0)
    with config.override(vit_depth=12):                                   # (Network() reads it; the product's depth)
        net = Network()
    names = [k for k, _ in net.named_parameters()]
    dead = [k.endswith(("cls_token", "mask_token")) or ".layer3." in k or ".layer4." in k or "PE" in k for k in names]
    assert (len(names), sum(dead)) == (244, 32)
    host = list(net.parameters())
    devp = [torch.nn.Parameter(p.detach().to(gpu)) for p in host]
    gen = torch.Generator().manual_seed(1)
    for p, q, d in zip(host, devp, dead):
        if not d:
            p.grad = torch.randn(p.shape, generator=gen)
            q.grad = p.grad.to(gpu)
    local = [None if p.grad is None else p.grad.numpy().copy() for p in host]
    ex_t, ex_d = TD.GradExchange(host, world=1), TD.GradExchange(devp, world=1)
    assert (ex_t.backend, ex_d.backend) == ("torch", "device")
    ex_d._layout_of(np.array([not d for d in dead], np.uint8)).flat.view(torch.int32).fill_(-1)      # NaN bytes underneath
    flat_t, flat_d = ex_t.exchange(), ex_d.exchange()
    torch.cuda.synchronize()
    assert np.array_equal(ex_t.layout.offsets, ex_d.layout.offsets) and flat_t.numel() == flat_d.numel() > 5_000_000
    assert np.array_equal(bits(flat_t.numpy()), bits(flat_d.cpu().numpy()))
    want = TD.grad_exchange_oracle([local], 1)
    for i, (p, q, w) in enumerate(zip(host, devp, want)):
        assert (p.grad is None) == (q.grad is None) == (w is None), names[i]
        if w is not None:
            assert q.grad.shape == q.shape and q.grad.data_ptr() == flat_d.data_ptr() + 4 * int(ex_d.layout.offsets[i])
            assert np.array_equal(bits(q.grad.cpu().numpy()), bits(w)), names[i]
    # once more, in place now (the gradients are the views): the cached addresses, the same bytes
    ex_d.exchange()
    ex_d.exchange()
    torch.cuda.synchronize()
    assert ex_d.layout.view_ptrs is not None and len(ex_d._layouts) == 1
    assert np.array_equal(bits(flat_t.numpy()), bits(flat_d.cpu().numpy()))


def test_device_adam_steps_out_of_the_slot_views(hip, gpu):
    """a local exchange that divides by 3, then DeviceAdam (clip, zero_grad in the kernel): the parameters are adam_step_oracle
    applied to grad_exchange_oracle's average, bit for bit -- for a first step out of autograd-style tensors and a second one that
    accumulates into the zeroed views and packs in place"""
    c = hip.adam_chunk_elems()
    sizes = [1, 5, c + 1, 300, 7]
    rs = np.random.RandomState(8)
    p0 = [rs.standard_normal(n).astype(np.float32) for n in sizes]
    params = [torch.nn.Parameter(torch.from_numpy(a.copy()).to(gpu)) for a in p0]
    opt = TO.DeviceAdam([{"params": [p]} for p in params], 1e-2, clip_value=40.0, zero_grad=True)
    ex = TD.GradExchange(params, world=3)
    state = [(a, np.zeros_like(a), np.zeros_like(a)) for a in p0]
    for step in (1, 2):
        g = [(rs.standard_normal(n) * 100).astype(np.float32) for n in sizes]
        g[3] = None if step == 1 else g[3]                                  # joins in the second step: another layout
        for p, a in zip(params, g):
            if a is None:
                continue
            if p.grad is None:
                p.grad = torch.from_numpy(a.copy()).to(gpu)
            else:
                assert not bool(p.grad.any())                               # the kernel zeroed the view
                p.grad += torch.from_numpy(a).to(gpu)                       # what AccumulateGrad does
        ex.exchange()
        opt.step()
        torch.cuda.synchronize()
        avg = TD.grad_exchange_oracle([g, [None if a is None else np.zeros_like(a) for a in g],
                                       [None if a is None else np.zeros_like(a) for a in g]], 3)
        for i, (p, a) in enumerate(zip(params, avg)):
            if a is None:
                assert p.grad is None and p not in opt.state
                continue
            t = int(opt.state[p]["step"])
            state[i] = TO.adam_step_oracle(*state[i][:1], a, *state[i][1:], lr=1e-2, step=t, clip_value=40.0)
            same_bits(p.detach().cpu().numpy(), state[i][0], f"step {step}, tensor {i}")
            assert p.grad.data_ptr() == ex.layout.flat.data_ptr() + 4 * int(ex.layout.offsets[i])
    assert len(ex._layouts) == 2


# ---------------------------------------------------------------------------
# ranks
# ---------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _job(n, out, extra=()):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), WORKER, "--out", out] + list(extra)
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    recs = []
    for k in range(n):
        d = np.load(os.path.join(out, f"rank{k}.npz"))
        recs.append({key: d[key] for key in d.files})
    return recs


@pytest.fixture(scope="module", params=[(2, None), (3, None), (3, "ordered")], ids=["2", "3", "3-ordered"])
def job(request, gpu, tmp_path_factory):
    """the distributed Trainer as it is -- one all_reduce -- with two and with three ranks, and three ranks once more with the
    exchange replaced by GradExchange(reduce="ordered")"""
    world, reduce = request.param
    recs = _job(world, str(tmp_path_factory.mktemp(f"dp{world}{reduce or ''}")), ["--reduce", reduce] if reduce else [])
    assert all(str(rec["reduce"]) == (reduce or "collective") for rec in recs)
    return world, recs


def _names(rec, prefix):
    return [k[len(prefix):] for k in rec if k.startswith(prefix)]


def test_ranks_start_from_rank_zero(job):
    world, recs = job
    names = _names(recs[0], "own:")
    assert len(names) > 100
    for r in range(1, world):
        assert sum(str(recs[r]["own:" + k]) != str(recs[0]["own:" + k]) for k in names) == len(names)
        assert all(str(recs[r]["start:" + k]) == str(recs[0]["own:" + k]) for k in names)
        assert all(str(recs[r][k]) == str(recs[0][k]) for k in recs[0] if k.startswith("startbuf:"))


def test_exchange_equals_the_oracle_on_the_saved_local_gradients(job):
    """Two ranks through one all_reduce: bit for bit.

    Three ranks: the feature was specified with |exchange - oracle| <= 2 * 2^-24 * sum_r |g_r / 3| per element.  ONE all_reduce
    CANNOT MEET THAT BOUND, and this is not hidden: measured on an MI355X over gloo, 34 199, 34 992 and 34 696 of 7 420 812 elements
    were over it in three runs (0.47 %), worst err / bound 1.590, 1.600 and 1.794.  The collective adds in an order of its own
    (gloo's ring starts every chunk at another rank), each order's result fl(fl(x + y) + z) is within 2^-24 (|x + y| + |fl(x + y)
    + z|) <= 2 * 2^-24 (1 + 2^-24) S of the exact sum, S = sum_r |g_r / 3|, so two orders lie at most 4 * 2^-24 (1 + 2^-24) S apart
    -- twice the specified bound.  The three-rank job of the Trainer as it is (one all_reduce) is held to that, which is what a
    single collective can promise, and the figure against the specified bound is printed; the specified bound itself is
    asserted on the three-rank job whose exchange adds in rank order (reduce="ordered": all_gather, world times the traffic, on
    request only), which meets it with err = 0."""
    world, recs = job
    ordered = str(recs[0]["reduce"]) == "ordered"
    worst, where, over, seen = 0.0, None, 0, 0
    for step in range(3):
        live = _names(recs[0], f"ex{step}:")
        assert len(live) > 50
        for r in range(world):
            assert sorted(_names(recs[r], f"exdig{step}:")) == sorted(live)
            assert all(str(recs[r][f"exdig{step}:{k}"]) == str(recs[0][f"exdig{step}:{k}"]) for k in live)   # one result on all ranks
        for k in live:
            local = [[recs[r].get(f"local{step}:{k}")] for r in range(world)]
            assert any(g[0] is not None for g in local)
            want = TD.grad_exchange_oracle(local, world)[0]
            got = recs[0][f"ex{step}:{k}"]
            seen += got.size
            if world == 2:
                same_bits(got, want, (step, k))
                continue
            terms = [np.abs(np.float32(g[0]) / np.float32(world)).astype(np.float64) for g in local if g[0] is not None]
            bound = 2 * 2.0 ** -24 * np.sum(np.stack(terms), 0)
            if not ordered:                                               # any order against rank order (docstring)
                looser = 2 * (1 + 2.0 ** -24) * bound + 2.0 ** -148
                assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= looser).all(), (step, k)
            err = np.abs(got.astype(np.float64) - want.astype(np.float64))
            ratio = err / np.maximum(bound, 1e-300)
            over += int((err > bound).sum())
            if float(ratio.max()) > worst:
                worst, where = float(ratio.max()), (step, k)
    print(f"world {world}, {recs[0]['reduce']}: {seen} gradient elements; worst err / specified bound = {worst:.3f} at {where}; "
          f"{over} elements over the specified bound")
    if world == 2 or ordered:
        assert over == 0 and worst <= 1.0, (worst, where, over)
    assert all(int(rec["inplace"]) == 1 for rec in recs)                  # the later exchanges packed in place


def test_every_exchanged_element_is_the_fp32_sum_of_the_quotients_in_some_order(job):
    """what the collective may choose is the ORDER of its additions, nothing else: every element is, bit for bit, the fp32 sum
    of the ranks' fp32 quotients in one of the orders there are (one with two ranks, three with three)"""
    world, recs = job
    orders = [(0, 1)] if world == 2 else [(0, 1, 2), (0, 2, 1), (1, 2, 0)]
    if str(recs[0]["reduce"]) == "ordered":
        orders = orders[:1]                                               # rank order, nothing else
    used = np.zeros(len(orders), np.int64)
    for step in range(3):
        for k in _names(recs[0], f"ex{step}:"):
            got = recs[0][f"ex{step}:{k}"]
            q = []
            for r in range(world):
                g = recs[r].get(f"local{step}:{k}")
                with np.errstate(all="ignore"):
                    q.append(np.zeros_like(got) if g is None else np.float32(g) / np.float32(world))
            hit = np.zeros(got.shape, bool)
            for j, o in enumerate(orders):
                with np.errstate(all="ignore"):
                    acc = q[o[0]] + q[o[1]]
                    for r in o[2:]:
                        acc = acc + q[r]
                same = (bits(acc) == bits(got)).reshape(got.shape) | (np.isnan(acc) & np.isnan(got))
                used[j] += int((same & ~hit).sum())
                hit |= same
            assert hit.all(), (step, k, int((~hit).sum()))
    print(f"world {world}: elements first matched by each order {orders}: {used.tolist()}")


def test_parameters_equal_across_ranks_and_differ_from_rank_zero_alone(job):
    world, recs = job
    names = _names(recs[0], "own:")
    for step in range(3):
        for r in range(1, world):
            assert all(str(recs[r][f"param{step}:{k}"]) == str(recs[0][f"param{step}:{k}"]) for k in names), (step, r)
    live = _names(recs[0], "ex0:")
    moved = [k for k in live if str(recs[0]["param2:" + k]) != str(recs[0]["start:" + k])]
    assert len(moved) > len(live) // 2                                    # (a tensor whose gradient is exactly 0 stays)
    differ = [k for k in live if str(recs[0]["solo:" + k]) != str(recs[0]["param2:" + k])]
    assert len(differ) > len(live) // 2                                   # the other ranks' gradients took part
    assert int(recs[0]["recorder_step"]) == 3 and all(int(rec["recorder_step"]) == 0 for rec in recs[1:])   # rank 0 records
    assert all(np.isfinite(rec["losses"]).all() and len(rec["losses"]) == 3 for rec in recs)


def test_dead_tensors_have_neither_gradient_nor_state(job):
    world, recs = job
    names = _names(recs[0], "own:")
    live = set(_names(recs[0], "ex2:"))
    dead = [k for k in names if k not in live]
    assert any(".layer3." in k for k in dead) and any(".layer4." in k for k in dead)
    for rec in recs:
        assert sorted(rec["no_grad"].tolist()) == sorted(dead) and sorted(rec["state"].tolist()) == sorted(live)
        assert all(str(rec["param2:" + k]) == str(rec["start:" + k]) for k in dead)


def test_two_ranks_with_sync_bn(gpu, tmp_path):
    """SyncBatchNorm after the reference trainer's conversion (the trunk then runs under torch autograd): finite losses, and the
    parameters of the ranks stay equal"""
    recs = _job(2, str(tmp_path), ["--sync-bn"])
    names = _names(recs[0], "own:")
    assert all(np.isfinite(rec["losses"]).all() and len(rec["losses"]) == 3 for rec in recs)
    for step in range(3):
        assert all(str(recs[1][f"param{step}:{k}"]) == str(recs[0][f"param{step}:{k}"]) for k in names), step
    assert any(str(recs[0]["param2:" + k]) != str(recs[0]["start:" + k]) for k in names)


def test_one_rank_over_rccl(gpu, tmp_path):
    """the transport the gloo jobs above replace: the flat device buffer through all_reduce on "nccl" with one rank -- the
    exchanged gradients are the local ones, bit for bit"""
    env = dict(os.environ, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()),
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, WORKER, "--out", str(tmp_path), "--rccl"], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.load(open(os.path.join(str(tmp_path), "rccl.json")))
    assert res["ok"] is True and res["flat_elems"] == 4 + 4 + 4096 + 4100 + 300
