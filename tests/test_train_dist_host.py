"""CPU: data-parallel training (transhuman_amd/train_dist.py, the distributed side of trainer.py) -- the sampler against a
recording of the reference's own class (tests/golden/g25_dist_sampler.npz, tools/gen_golden_dist_sampler.py), the layout rule in
Python and in C, the oracle's properties, and the exchange over gloo with two and three ranks (one process per rank, as
test_dist_gloo.py) on a toy module with torch.optim.Adam: DeviceAdam has no host path, and the torch back end of GradExchange
is what the device back end is held against (tests/test_gpu_train_dist.py).

What "equal" means for the exchanged gradients.  Every rank divides in fp32 (one rounding, the oracle's own) and ONE all_reduce
adds the ranks, in an order of its own.  Two ranks: one addition, which has no order -- bit for bit.  Three ranks: the feature
was specified with |sum - oracle| <= 2 * 2^-24 * sum_r |g_r / 3| per element against the rank-ordered oracle.  A single
all_reduce cannot promise that: two orders of one three-term sum are each two roundings from the exact sum, so they can lie
4 * 2^-24 * sum_r |g_r / 3| apart (measured on a device job over gloo, 7.4 M gradient elements: 0.47 % beyond the specified
bound, the worst by 1.79 x; tests/test_gpu_train_dist.py).  Here, on the toy's small host tensors, gloo happens to add in rank
order and the specified bound is met and asserted; what one all_reduce promises on any transport -- one result on all ranks, each
element the fp32 sum in one of the three orders -- is asserted beside it.  reduce="ordered" (all_gather, additions in rank
order: on request only) is run as a third job and equals the oracle bit for bit.
"""
import datetime
import os
import socket
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from transhuman_amd import hip
from transhuman_amd import train_dist as TD
from transhuman_amd import trainer as TR

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g25_dist_sampler.npz")
STEPS = 3


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------------------
# sampler
# ---------------------------------------------------------------------------
def test_sampler_equals_the_reference_recording():
    g = np.load(GOLD)
    cases = g["cases"]
    assert len(cases) >= 8 and any(n % w for n, w, _, _ in cases) and any(not s for _, _, _, s in cases)
    for k, (n, world, epoch, shuffle) in enumerate(cases):
        want = g[f"idx_{k}"]
        assert want.shape == (world, -(-n // world))
        for rank in range(world):
            s = TD.DistributedSampler(int(n), num_replicas=int(world), rank=rank, shuffle=bool(shuffle))
            s.set_epoch(int(epoch))
            got = list(s)
            assert len(s) == len(got) and got == want[rank].tolist(), (k, rank)
    for max_iter, world, want in g["iters"]:
        assert TD.iterations_per_rank(int(max_iter), int(world)) == int(want)


def test_sampler_partitions_the_padded_permutation_and_follows_the_epoch():
    n, world = 23, 4
    per_epoch = []
    for epoch in (0, 1):
        blocks = []
        for rank in range(world):
            s = TD.DistributedSampler(range(n), world, rank)             # (a sized object in the place of its length)
            s.set_epoch(epoch)
            blocks.append(list(s))
        padded = sum(blocks, [])
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(epoch)).tolist()
        assert padded == perm + perm[:1] and sorted(padded[:n]) == list(range(n))      # 24 = 23 + the first index again
        per_epoch.append(padded)
    assert per_epoch[0] != per_epoch[1]
    assert list(TD.DistributedSampler(5, 2, 1, shuffle=False)) == [3, 4, 0]
    with pytest.raises(ValueError):
        TD.DistributedSampler(5, 2, 2)


# ---------------------------------------------------------------------------
# layout, oracle
# ---------------------------------------------------------------------------
def test_layout_rule_in_python_and_in_c():
    hip.load_library()
    rs = np.random.RandomState(25)
    c = hip.adam_chunk_elems()
    for trial in range(40):
        n = int(rs.randint(1, 40))
        counts = [int(x) for x in rs.choice([1, 2, 3, 4, 5, 7, 8, 255, c - 1, c, c + 1, 2 * c + 7], n)]
        live = (rs.uniform(size=n) < 0.7).astype(np.uint8) if trial else np.ones(n, np.uint8)
        off, total = TD.flat_layout(counts, live)
        off_c, total_c = hip.adam_flat_layout(counts, live)
        assert np.array_equal(off, off_c) and total == total_c
        assert all(o % 4 == 0 for o in off[live != 0]) and all(o == -1 for o in off[live == 0]) and total % 4 == 0
        end = 0
        for o, k, l in zip(off, counts, live):                         # plan order, no overlap, at most 3 elements of padding
            if l:
                assert end <= o < end + 4 and o == (end + 3) // 4 * 4
                end = o + k
        assert total == (end + 3) // 4 * 4
        again, total2 = TD.flat_layout(list(counts), live.copy())       # a pure function of (counts, bitmap)
        assert np.array_equal(off, again) and total == total2
    assert TD.flat_layout([5, 6], None)[1] == hip.adam_flat_layout([5, 6])[1] == 16
    assert TD.flat_layout([5, 6], [0, 0])[1] == hip.adam_flat_layout([5, 6], [0, 0])[1] == 0
    with pytest.raises(hip.HipError):
        hip.adam_flat_layout([4, 0])
    with pytest.raises(ValueError):
        TD.flat_layout([4, 0])


def test_oracle_properties():
    rs = np.random.RandomState(3)
    g = [rs.standard_normal((3, 5)).astype(np.float32) * 1e3 for _ in range(3)]
    g[0][0, :4] = [np.inf, -np.inf, np.nan, -0.0]
    # world 1 hands the gradient through, bit for bit
    one = TD.grad_exchange_oracle([[g[0], None]], 1)
    assert one[1] is None and np.array_equal(bits(one[0]), bits(g[0]))
    # a division and a sum in fp32, ranks in rank order; None where no rank has a gradient, zeros from a rank without one
    three = TD.grad_exchange_oracle([[g[0], None, g[0]], [g[1], None, None], [g[2], None, g[2]]], 3)
    w = np.float32(3)
    with np.errstate(all="ignore"):
        want = (g[0] / w + g[1] / w) + g[2] / w
        want2 = (g[0] / w + np.zeros_like(g[0])) + g[2] / w
    assert three[1] is None and three[0].dtype == np.float32
    ok = ~np.isnan(want)
    assert np.array_equal(bits(three[0])[ok], bits(want)[ok]) and np.isnan(three[0][~ok]).all()
    ok = ~np.isnan(want2)
    assert np.array_equal(bits(three[2])[ok], bits(want2)[ok]) and np.isnan(three[2][~ok]).all()
    assert np.isposinf(three[0][0, 0]) and np.isneginf(three[0][0, 1]) and np.isnan(three[0][0, 2])
    # equal gradients average to themselves when the division is exact
    p2 = [np.float32(2.0) ** rs.randint(-20, 20, (4, 4)).astype(np.float32) for _ in range(1)] * 2
    assert np.array_equal(TD.grad_exchange_oracle([[p2[0]], [p2[1]]], 2)[0], p2[0])
    with pytest.raises(ValueError):
        TD.grad_exchange_oracle([[g[0]]], 2)


def test_torch_back_end_packs_like_the_definition():
    """a local exchange (no process group) at world 3: the slots hold np.float32(g) / np.float32(3) bit for bit, a tensor without
    a gradient keeps none, the padding is zero although the buffer started as NaN, and a second exchange divides in place"""
    rs = np.random.RandomState(4)
    counts = [1, 3, 4, 5, 9, 6]
    params = [torch.nn.Parameter(torch.zeros(n)) for n in counts]
    grads = [(rs.standard_normal(n) * np.exp(rs.uniform(-30, 30, n))).astype(np.float32) for n in counts]
    grads[3][:] = [np.inf, -np.inf, np.nan, -0.0, 1e-42]
    for i, (p, g) in enumerate(zip(params, grads)):
        p.grad = None if i == 2 else torch.from_numpy(g.copy())
    ex = TD.GradExchange(params, world=3)
    assert ex.backend == "torch" and ex.dist is None
    lay = ex._layout_of(np.array([1, 1, 0, 1, 1, 1], np.uint8))
    lay.flat.fill_(float("nan"))
    flat = ex.exchange()
    assert ex.layout is lay and flat.numel() == 4 + 4 + 8 + 12 + 8
    with np.errstate(all="ignore"):
        want = [None if i == 2 else g / np.float32(3) for i, g in enumerate(grads)]
    for i, (p, w) in enumerate(zip(params, want)):
        if w is None:
            assert p.grad is None
            continue
        assert p.grad is lay.views[i] and p.grad.data_ptr() == flat.data_ptr() + 4 * int(lay.offsets[i])
        ok = ~np.isnan(w)
        assert np.array_equal(bits(p.grad.numpy())[ok], bits(w)[ok]) and np.isnan(p.grad.numpy()[~ok]).all(), i
    covered = np.zeros(flat.numel(), bool)
    for i in lay.live:
        covered[int(lay.offsets[i]):int(lay.offsets[i]) + counts[i]] = True
    assert (~covered).sum() == 3 + 1 + 3 + 3 + 2 and np.array_equal(bits(flat.numpy()[~covered]), np.zeros((~covered).sum(), np.uint32))
    first = [None if p.grad is None else p.grad.numpy().copy() for p in params]
    ex.exchange()                                                       # the gradients ARE the slots now
    for p, f in zip(params, first):
        if f is not None:
            with np.errstate(all="ignore"):
                w = f / np.float32(3)
            ok = ~np.isnan(w)
            assert np.array_equal(bits(p.grad.numpy())[ok], bits(w)[ok])


# ---------------------------------------------------------------------------
# gloo worlds
# ---------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _init(rank, world, port):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    # (a rank that dies ends the job through this timeout instead of stalling the others for torch's default half hour)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))


class Toy(torch.nn.Module):
    """main: every rank, every step.  side: rank 1 skips it; nobody runs it in the last step.  late: from step 1 on.  dead: never."""

    def __init__(self):
        super().__init__()
        self.a = torch.nn.Linear(5, 9)
        self.b = torch.nn.Linear(9, 3)
        self.side = torch.nn.Linear(5, 3)
        self.late = torch.nn.Linear(5, 3, bias=False)
        self.dead = torch.nn.Linear(5, 3)

    def forward(self, x, side, late):
        y = self.b(torch.tanh(self.a(x)))
        if side:
            y = y + self.side(x)
        if late:
            y = y + self.late(x)
        return y


def toy_input(rank, step):
    return torch.randn((6, 5), generator=torch.Generator().manual_seed(100 * step + rank)) * 3.0


def branches(rank, step):
    return (rank != 1 and step < STEPS - 1), step >= 1


def _exchange_worker(rank, world, port, q, reduce=None):
    _init(rank, world, port)
    try:
        torch.manual_seed(10 + rank)                                    # every rank starts somewhere else ...
        m = Toy()
        own = [p.detach().numpy().copy() for p in m.parameters()]
        params = list(m.parameters())
        ex = TD.GradExchange(params, reduce=reduce)
        rec_reduce = ex.reduce
        ex.broadcast_parameters(m)                                      # ... and continues from rank 0's
        start = [p.detach().numpy().copy() for p in params]
        opt = torch.optim.Adam([{"params": [p]} for p in params], 1e-2)
        rec = {"own": own, "start": start, "local": [], "exchanged": [], "params": [], "layouts": []}
        for step in range(STEPS):
            side, late = branches(rank, step)
            loss = (m(toy_input(rank, step), side, late) ** 2).mean()
            opt.zero_grad()
            loss.backward()
            rec["local"].append([None if p.grad is None else p.grad.numpy().copy() for p in params])
            ex.exchange()
            rec["exchanged"].append([None if p.grad is None else p.grad.numpy().copy() for p in params])
            rec["layouts"].append(ex.layout.offsets.tolist())
            opt.step()
            rec["params"].append([p.detach().numpy().copy() for p in params])
        rec["state"] = [len(opt.state.get(p, {})) for p in params]
        rec["n_layouts"] = len(ex._layouts)
        rec["reduce"] = rec_reduce
        q.put((rank, rec))
    finally:
        dist.destroy_process_group()


def _spawn(target, world, *args):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, world, port, q) + args) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert sorted(res) == list(range(world))
    return [res[r] for r in range(world)]


@pytest.fixture(scope="module", params=[(2, None), (3, None), (3, "ordered")], ids=["2", "3", "3-ordered"])
def toy_run(request):
    world, reduce = request.param
    recs = _spawn(_exchange_worker, world, reduce)
    assert all(r["reduce"] == (reduce or "collective") for r in recs)   # one all_reduce unless asked otherwise
    return world, recs


def test_every_element_is_the_sum_in_some_order(toy_run):
    """what one all_reduce promises with any number of ranks: one result on all ranks, and every element is, bit for bit, the fp32
    sum of the ranks' fp32 quotients in one of the orders there are -- the order is the collective's choice"""
    world, recs = toy_run
    orders = ((0, 1),) if world == 2 else ((0, 1, 2), (0, 2, 1), (1, 2, 0))
    for step in range(STEPS):
        for i, got in enumerate(recs[0]["exchanged"][step]):
            assert all((got is None) == (r["exchanged"][step][i] is None) for r in recs)
            if got is None:
                continue
            assert all(np.array_equal(bits(got), bits(r["exchanged"][step][i])) for r in recs)
            q = [np.zeros_like(got) if r["local"][step][i] is None else r["local"][step][i] / np.float32(world) for r in recs]
            hit = np.zeros(got.shape, bool)
            for o in orders:
                acc = q[o[0]] + q[o[1]]
                for k in o[2:]:
                    acc = acc + q[k]
                hit |= bits(acc) == bits(got)
                if recs[0]["reduce"] == "ordered":
                    break                                               # (rank order, nothing else)
            assert hit.all(), (step, i)


def test_broadcast_makes_every_rank_rank_zeros(toy_run):
    world, recs = toy_run
    for r in range(1, world):
        assert any(not np.array_equal(a, b) for a, b in zip(recs[r]["own"], recs[0]["own"]))
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(recs[r]["start"], recs[0]["own"]))


def test_exchanged_gradients_equal_the_oracle(toy_run):
    world, recs = toy_run
    names = [k for k, _ in Toy().named_parameters()]
    worst = 0.0
    for step in range(STEPS):
        want = TD.grad_exchange_oracle([recs[r]["local"][step] for r in range(world)], world)
        for r in range(world):
            for name, w, got in zip(names, want, recs[r]["exchanged"][step]):
                assert (w is None) == (got is None), (step, r, name)
                if w is None:
                    continue
                if world == 2:
                    assert np.array_equal(bits(got), bits(w)), (step, r, name)
                else:
                    terms = [np.zeros_like(w) if recs[k]["local"][step][names.index(name)] is None
                             else np.abs(recs[k]["local"][step][names.index(name)] / np.float32(world)) for k in range(world)]
                    bound = 2 * 2.0 ** -24 * np.sum(np.stack(terms).astype(np.float64), 0)
                    err = np.abs(got.astype(np.float64) - w.astype(np.float64))
                    worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
                    assert (err <= bound).all(), (step, r, name, float(err.max()))
            assert all((a is None and b is None) or np.array_equal(bits(a), bits(b))
                       for a, b in zip(recs[r]["exchanged"][step], recs[0]["exchanged"][step]))     # one result on all ranks
    print(f"world {world}: worst err / bound = {worst:.3f}")


def test_skipped_branches(toy_run):
    world, recs = toy_run
    names = [k for k, _ in Toy().named_parameters()]
    sw, dw, lw = names.index("side.weight"), names.index("dead.weight"), names.index("late.weight")
    # rank 1 skips `side` in step 0: zeros from rank 1 (the oracle's reading of None), and the tensor steps on rank 1 too
    assert recs[1]["local"][0][sw] is None and recs[0]["local"][0][sw] is not None
    others = [[recs[r]["local"][0][sw]] for r in range(world)]
    others[1] = [np.zeros_like(recs[0]["local"][0][sw])]
    assert np.array_equal(bits(TD.grad_exchange_oracle(others, world)[0]),
                          bits(TD.grad_exchange_oracle([[recs[r]["local"][0][sw]] for r in range(world)], world)[0]))
    assert recs[1]["exchanged"][0][sw] is not None and not np.array_equal(recs[1]["params"][0][sw], recs[1]["start"][sw])
    # a branch every rank skips: no gradient, no optimiser state, the parameter as broadcast
    for r in range(world):
        assert all(recs[r]["exchanged"][s][dw] is None for s in range(STEPS))
        assert recs[r]["state"][dw] == 0 and recs[r]["state"][sw] > 0
        assert np.array_equal(bits(recs[r]["params"][-1][dw]), bits(recs[0]["start"][dw]))
        # the bitmap changes from step to step -- late joins, then side leaves -- and every rank follows in the same step
        assert recs[r]["exchanged"][0][lw] is None and recs[r]["exchanged"][1][lw] is not None
        assert recs[r]["exchanged"][2][sw] is None
        assert recs[r]["n_layouts"] == 3 and recs[r]["layouts"] == recs[0]["layouts"]
        assert recs[r]["layouts"][0] != recs[r]["layouts"][1] != recs[r]["layouts"][2]


def test_parameters_stay_equal_and_match_a_single_process(toy_run):
    """Across ranks: torch.equal after every step.  Against ONE process that starts from rank 0's parameters and steps
    torch.optim.Adam on grad_exchange_oracle of the recorded per-rank gradients: bit for bit wherever the exchange IS the oracle
    -- two ranks, and three ranks with reduce="ordered".  Three ranks through one all_reduce are not compared with the single
    process: the sum may be another order's, and Adam's normalisation (m / sqrt(v): a gradient near zero can flip its sign on the
    last bit) leaves no bound on the parameters worth asserting; that run is held to its gradients above."""
    world, recs = toy_run
    for step in range(STEPS):
        for r in range(1, world):
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(recs[r]["params"][step], recs[0]["params"][step]))
    if world > 2 and recs[0]["reduce"] != "ordered":
        return
    m = Toy()
    params = list(m.parameters())
    with torch.no_grad():
        for p, a in zip(params, recs[0]["start"]):
            p.copy_(torch.from_numpy(a))
    opt = torch.optim.Adam([{"params": [p]} for p in params], 1e-2)
    for step in range(STEPS):
        avg = TD.grad_exchange_oracle([recs[r]["local"][step] for r in range(world)], world)
        for p, g in zip(params, avg):
            p.grad = None if g is None else torch.from_numpy(g.copy())
        opt.step()
        for p, want in zip(params, recs[0]["params"][step]):
            assert np.array_equal(bits(p.detach().numpy()), bits(want)), step


# ---------------------------------------------------------------------------
# fit with two ranks
# ---------------------------------------------------------------------------
class ToyWrapper(torch.nn.Module):
    """what trainer.Trainer drives: batch -> (output, loss, loss_stats, image_stats); ``net`` holds the trained parameters"""

    def __init__(self):
        super().__init__()
        self.net = torch.nn.Sequential(torch.nn.Linear(5, 4), torch.nn.BatchNorm1d(4), torch.nn.Linear(4, 2))

    def forward(self, batch):
        out = self.net(batch["x"])
        loss = ((out - batch["y"]) ** 2).mean()
        return out, loss, {"loss": loss}, {}


class _Loader(list):
    """a sized iterable of batches with a sampler, as a torch DataLoader has one"""

    def __init__(self, batches, sampler):
        super().__init__(batches)
        self.sampler = sampler


def _fit_cfg(model_dir, epochs):
    return SimpleNamespace(train=SimpleNamespace(optim="adam", lr=1e-2, weight_decay=0.0, epoch=epochs, scheduler=SimpleNamespace(
        type="cosine", warmup_epochs=1, decay_epochs=6, end_lr=1e-6)), trained_model_dir=model_dir, resume=True, save_freq=1,
        save_latest_ep=1, log_interval=1)


def _fit_worker(rank, world, port, q, model_dir, epochs):
    _init(rank, world, port)
    try:
        # (fit builds a DeviceAdam, which has no host path: the host test drives the same loop with torch.optim.Adam)
        TR.make_optimizer = lambda cfg, net: torch.optim.Adam([{"params": [p]} for p in net.parameters()], cfg.train.lr)
        saves, begins, epochs_seen, lines = [], [], [], []
        save, load = TR.save_model, TR.load_model
        TR.save_model = lambda *a, **k: (saves.append(1), save(*a, **k))[1]
        TR.load_model = lambda *a, **k: (begins.append(load(*a, **k)), begins[-1])[1]
        torch.manual_seed(50 + rank)
        wrapper = ToyWrapper()
        sampler = TD.DistributedSampler(8, world, rank)
        sampler.set_epoch = lambda e, f=sampler.set_epoch: (epochs_seen.append(e), f(e))[1]
        gen = torch.Generator().manual_seed(7 + rank)
        loader = _Loader([{"x": torch.randn((6, 5), generator=gen), "y": torch.randn((6, 2), generator=gen)} for _ in range(2)],
                         sampler)
        TR.fit(_fit_cfg(model_dir, epochs), wrapper, loader, log=lines.append, group=dist.group.WORLD)
        q.put((rank, {"saves": len(saves), "begin": begins, "epochs": epochs_seen, "lines": len(lines),
                      "state": {k: v.numpy().copy() for k, v in wrapper.state_dict().items()}}))
    finally:
        dist.destroy_process_group()


def test_fit_with_two_ranks_checkpoints_from_rank_zero_and_resumes_on_both(tmp_path):
    model_dir = str(tmp_path / "model")
    first = _spawn(_fit_worker, 2, model_dir, 2)
    assert [r["saves"] for r in first] == [4, 0] and sorted(os.listdir(model_dir)) == ["1.pth", "2.pth", "latest.pth"]
    assert [r["begin"] for r in first] == [[0], [0]] and [r["epochs"] for r in first] == [[0, 1], [0, 1]]
    assert first[0]["lines"] > 0 and first[1]["lines"] == 0             # rank 0 alone logs
    ck = torch.load(os.path.join(model_dir, "latest.pth"), map_location="cpu", weights_only=True)
    assert ck["epoch"] == 1 and ck["recorder"] == {"step": 4}
    for k, v in first[0]["state"].items():                              # parameters AND buffers of the ranks agree where they
        if "running" not in k:                                          # are exchanged or broadcast (BatchNorm's running
            assert np.array_equal(v, first[1]["state"][k]), k           # statistics are rank-local without sync_bn)
        assert np.array_equal(v, ck["net"][k[len("net."):]].numpy()), k   # ... and rank 0's are the checkpoint's (of wrapper.net)
    second = _spawn(_fit_worker, 2, model_dir, 3)
    assert [r["begin"] for r in second] == [[2], [2]] and [r["epochs"] for r in second] == [[2], [2]]
    assert [r["saves"] for r in second] == [2, 0] and "3.pth" in os.listdir(model_dir)
    for k, v in second[0]["state"].items():
        if "running" not in k:
            assert np.array_equal(v, second[1]["state"][k]), k
    assert any(not np.array_equal(v, first[0]["state"][k]) for k, v in second[0]["state"].items())


def test_single_process_callers_see_no_change(monkeypatch):
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    assert TR.init_distributed() == (None, None)                        # no launcher, no group
    t = TR.Trainer(ToyWrapper(), device="cpu")
    assert t.group is None and t.exchange is None and t.rank == 0
    assert not any(isinstance(m, torch.nn.SyncBatchNorm) for m in t.network.modules())
    with pytest.raises(ValueError, match="process group"):
        TR.Trainer(ToyWrapper(), device="cpu", sync_bn=True)
