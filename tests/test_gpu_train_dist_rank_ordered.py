"""GPU: data-parallel steps whose result does not depend on a collective's order -- ranks over gloo on ONE device
(torch.distributed.run, as tests/test_gpu_train_dist.py; at most three processes at a time).

1. The distributed Trainer's job of tests/train_dist_worker.py with three ranks and GradExchange(reduce="rank_ordered"): the
   exchanged gradients equal train_dist.grad_exchange_oracle ON THE LOCAL GRADIENTS EACH RANK SAVED bit for bit at every step -- no
   element over the specified 2 * 2^-24 * sum_r |g_r / 3|, err = 0 -- at the traffic of a ring all-reduce.  (One all_reduce leaves
   0.47 % of the elements over that bound; reduce="ordered" meets it at world times the traffic.)
2. The encoder trunk alone with two and three ranks (tests/train_dist_sync_worker.py --trunk): SyncBatchNorm sites on
   train_ops.SyncBnActFn.  The reference is the float64 stock trunk with PLAIN BatchNorm on the concatenated batch, computed here;
   with d32 torch's fp32 autograd of the same on the device, per gradient tensor

       parent = max|d32 - t64|,  scale = max|t64|,    bar = 4 max(parent, 2^-24 scale)

   as in tests/test_gpu_train_encoder.py.  Held to it: each rank's gradient at conv1's output against its slice of the batch's (the
   finest per-rank quantity: the images have no gradient on the device path, K23 builds conv1's weight gradient only), and the sum
   over the ranks of the 30 LOCAL parameter gradients (fp32 results added in float64) against the batch's.
3. The full Trainer with three ranks, SyncBatchNorm, cfg.train_sync_bn = "device", reduce = "rank_ordered" and every training switch
   on the device, run twice: finite losses, equal parameters on all ranks after every step, identical digests in both runs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_gpu_train_dist import _free_port, _names, same_bits
from train_dist_sync_worker import make_encoder, rank_parts, trunk_inputs, trunk_names
from transhuman_amd import train_dist as TD

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR = 2.0 ** -24
STEPS = 3


def _run(worker, n, out, extra):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "tests", worker), "--out", out] + list(extra)
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]


def _load(out, prefix, n):
    recs = []
    for k in range(n):
        d = np.load(os.path.join(out, f"{prefix}{k}.npz"))
        recs.append({key: d[key] for key in d.files})
    return recs


# ---------------------------------------------------------------------------
# 1: the Trainer's exchange, rank-ordered
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ordered_job(gpu, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dp3rank_ordered"))
    _run("train_dist_worker.py", 3, out, ["--reduce", "rank_ordered"])
    recs = _load(out, "rank", 3)
    assert all(str(rec["reduce"]) == "rank_ordered" for rec in recs)
    return recs


def test_three_ranks_equal_the_oracle_bit_for_bit_at_every_step(ordered_job):
    recs = ordered_job
    world, seen, over, worst = 3, 0, 0, 0.0
    for step in range(STEPS):
        live = _names(recs[0], f"ex{step}:")
        assert len(live) > 50
        for r in range(world):
            assert sorted(_names(recs[r], f"exdig{step}:")) == sorted(live)
            assert all(str(recs[r][f"exdig{step}:{k}"]) == str(recs[0][f"exdig{step}:{k}"]) for k in live)   # one result on all ranks
        for k in live:
            local = [[recs[r].get(f"local{step}:{k}")] for r in range(world)]
            want = TD.grad_exchange_oracle(local, world)[0]
            got = recs[0][f"ex{step}:{k}"]
            seen += got.size
            terms = [np.abs(np.float32(g[0]) / np.float32(world)).astype(np.float64) for g in local if g[0] is not None]
            err = np.abs(got.astype(np.float64) - want.astype(np.float64))
            over += int((err > 2 * FLOOR * np.sum(np.stack(terms), 0)).sum())
            worst = max(worst, float(err.max()))
            same_bits(got, want, (step, k))
    print(f"world 3, rank_ordered: {seen} gradient elements; {over} over the specified bound; max err = {worst:.3e}")
    assert over == 0 and worst == 0.0 and seen > 1_000_000
    assert all(int(rec["inplace"]) == 1 for rec in recs)                  # the later exchanges packed in place


def test_ordered_job_trains(ordered_job):
    recs = ordered_job
    names = _names(recs[0], "own:")
    for step in range(STEPS):
        for r in range(1, 3):
            assert all(str(recs[r][f"param{step}:{k}"]) == str(recs[0][f"param{step}:{k}"]) for k in names), (step, r)
    assert all(np.isfinite(rec["losses"]).all() and len(rec["losses"]) == STEPS for rec in recs)
    assert any(str(recs[0]["param2:" + k]) != str(recs[0]["start:" + k]) for k in names)


# ---------------------------------------------------------------------------
# 2: the trunk alone
# ---------------------------------------------------------------------------
def _reference(enc, images, seeds):
    """the stock trunk with plain BatchNorm on the whole batch -> the parameter gradients and the gradient at conv1's output"""
    kept = []
    h = enc.model.conv1.register_forward_hook(lambda m, i, o: (o.retain_grad(), kept.append(o))[0])
    lat = enc.trunk(images, fused_bn=False)
    torch.autograd.backward(lat, [s.to(l) for s, l in zip(seeds, lat)])
    h.remove()
    grads = {k: p.grad.detach().cpu().double() for k, p in enc.named_parameters() if p.grad is not None}
    grads["g_conv1"] = kept[0].grad.detach().cpu().double()
    return grads


@pytest.fixture(scope="module", params=[2, 3], ids=["2", "3"])
def trunk_job(request, gpu, tmp_path_factory):
    world = request.param
    out = str(tmp_path_factory.mktemp(f"trunk{world}"))
    _run("train_dist_sync_worker.py", world, out, ["--trunk"])
    recs = _load(out, "trunk", world)
    images, seeds = trunk_inputs(world)
    t64 = _reference(make_encoder(torch.float64), images.double(), [s.double() for s in seeds])
    d32 = _reference(make_encoder().to(gpu), images.to(gpu), seeds)
    return world, recs, t64, d32


def test_sync_sites_ran_on_the_device(trunk_job):
    world, recs, _, _ = trunk_job
    for rec in recs:
        assert str(rec["site"]) == "SyncBnActFnBackward" and int(rec["sync_calls"]) == 10     # the ten BatchNorm sites, once each
    stats = [k for k in recs[0] if k.startswith("stat:")]
    assert len(stats) >= 30
    for rec in recs[1:]:                                                  # the forward is the module's own: one statistic for all
        assert all(np.array_equal(rec[k], recs[0][k]) for k in stats)
    assert int(recs[0]["stat:model.bn1.num_batches_tracked"]) == 1
    assert float(np.abs(recs[0]["stat:model.bn1.running_mean"]).max()) > 0


def test_trunk_gradients_vs_the_float64_trunk_on_the_concatenated_batch(trunk_job):
    world, recs, t64, d32 = trunk_job
    names = trunk_names(make_encoder())
    assert len(names) == 30 and set(names) | {"g_conv1"} == set(t64)
    parts = rank_parts(world)
    got = {k: sum(torch.from_numpy(rec["grad:" + k]).double() for rec in recs) for k in names}
    for rec in recs:
        assert sorted(_names(rec, "grad:")) == sorted(names)
    got["g_conv1"] = torch.cat([torch.from_numpy(rec["g_conv1"]).double() for rec in recs])
    assert [rec["g_conv1"].shape[0] for rec in recs] == [p.stop - p.start for p in parts]
    worst, failed = 0.0, []
    for k, ref in t64.items():
        assert got[k].shape == ref.shape and torch.isfinite(got[k]).all(), k
        parent, scale = float((d32[k] - ref).abs().max()), float(ref.abs().max())
        bar = 4.0 * max(parent, FLOOR * scale)
        err = float((got[k] - ref).abs().max())
        worst = max(worst, err / bar)
        print(f"world {world} {k}: device {err:.3e}, torch fp32 {parent:.3e}, max|ref| = {scale:.3e}; err / bar = {err / bar:.3f}")
        if not err <= bar:
            failed.append((k, err, bar))
    print(f"world {world}: worst err / bar = {worst:.3f}")
    assert not failed, failed


# ---------------------------------------------------------------------------
# 3: the full Trainer, twice
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full_jobs(gpu, tmp_path_factory):
    runs = []
    for i in range(2):
        out = str(tmp_path_factory.mktemp(f"full{i}"))
        _run("train_dist_sync_worker.py", 3, out, ["--sync-bn", "--reduce", "rank_ordered"])
        recs = _load(out, "rank", 3)
        for r, rec in enumerate(recs):
            rec["sync_calls"] = json.load(open(os.path.join(out, f"sync{r}.json")))["sync_calls"]
        runs.append(recs)
    return runs


def test_full_trainer_three_ranks(full_jobs):
    for recs in full_jobs:
        names = _names(recs[0], "own:")
        assert len(names) > 100 and all(str(rec["reduce"]) == "rank_ordered" for rec in recs)
        assert all(np.isfinite(rec["losses"]).all() and len(rec["losses"]) == STEPS for rec in recs)
        for step in range(STEPS):
            for r in range(1, 3):
                assert all(str(recs[r][f"param{step}:{k}"]) == str(recs[0][f"param{step}:{k}"]) for k in names), (step, r)
        assert any(str(recs[0]["param2:" + k]) != str(recs[0]["start:" + k]) for k in names)
        # the ten sites of the trunk, once per step, on every rank
        assert all(rec["sync_calls"] >= 10 * STEPS and rec["sync_calls"] % 10 == 0 for rec in recs), [r["sync_calls"] for r in recs]


def test_full_trainer_repeats_itself_bit_for_bit(full_jobs):
    a, b = full_jobs
    names = _names(a[0], "own:")
    for r in range(3):
        assert all(str(a[r]["start:" + k]) == str(b[r]["start:" + k]) for k in names)
        for step in range(STEPS):
            differ = [k for k in names if str(a[r][f"param{step}:{k}"]) != str(b[r][f"param{step}:{k}"])]
            assert not differ, (r, step, len(differ), differ[:5])
