"""Time one optimiser step on the real Network (every parameter holding a seeded gradient), four forms in one process:

    timeout -k 10 600 python tools/optim_step_time.py [--rounds 5] [--steps 20] [--warmup 3] [--rocprof DIR]

  "reference"      torch.optim.Adam over one parameter group per tensor + clip_grad_value_(., 40): the reference's loop
                   (lib/train/optimizer.py:16-19, lib/train/trainers/trainer.py:85-86)
  "reference_fused" the same groups with fused=True
  "one_group_fused" torch's best case: ONE group, fused=True, + clip_grad_value_
  "device"         transhuman_amd.train_optim.DeviceAdam(clip_value=40): one table copy + one launch of adam_step_kernel (K22)
Prints one JSON line.  Per form, the median of --rounds alternating rounds with the lowest and the highest, each round being
--steps steps: host ms per step (wall time with a synchronisation at both ends of every step; and the part until step()
returns) and device ms per step (events around the step).  With --rocprof DIR: kernel launches per step from `rocprofv3 --kernel-trace --stats` over a short run of
that form in a fresh child process behind `--` (DIR keeps the traces).  No threshold on any figure."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time
from collections import defaultdict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORMS = ("reference", "reference_fused", "one_group_fused", "device")
CLIP, LR = 40.0, 7e-4


def setup(dev):
    import torch
    from transhuman_amd import synth
    from transhuman_amd.networks.cross_transformer import Network
    torch.manual_seed(0)
    net = Network()
    net.load_state_dict(synth.det_state_dict(net.state_dict(), seed=0, sigma_bias=-1.7))
    net = net.train().to(dev)
    gen = torch.Generator().manual_seed(1)
    for p in net.parameters():
        if p.requires_grad:
            p.grad = (torch.randn(p.shape, generator=gen) * 30).to(dev)      # (some elements beyond the clip value)
    return net


def make(form, net):
    import torch
    from transhuman_amd.train_optim import DeviceAdam
    params = [p for p in net.parameters() if p.requires_grad]
    groups = [{"params": [p], "lr": LR, "weight_decay": 0} for p in params]
    if form == "reference":
        opt = torch.optim.Adam(groups, LR)
    elif form == "reference_fused":
        opt = torch.optim.Adam(groups, LR, fused=True)
    elif form == "one_group_fused":
        opt = torch.optim.Adam(params, LR, fused=True)
    else:
        opt = DeviceAdam(groups, LR, clip_value=CLIP)
        return opt, opt.step

    def step():
        torch.nn.utils.clip_grad_value_(params, CLIP)
        opt.step()
    return opt, step


def _traced_run(out_dir, form, steps):
    d = os.path.join(out_dir, f"{form}_{steps}")
    os.makedirs(d, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "optim", "--",
           sys.executable, os.path.abspath(__file__), "--forms", form, "--rounds", "1", "--steps", str(steps), "--warmup", "0"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        return None, p.stderr[-400:]
    agg = defaultdict(lambda: [0, 0])
    for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            key = row["Kernel_Name"].split("(")[0][:70]
            agg[key][0] += 1
            agg[key][1] += int(row["End_Timestamp"]) - int(row["Start_Timestamp"])
    return agg, None


def trace(out_dir, form, steps=(4, 12)):
    """kernel launches per step from two traced child runs of one form that differ only in their step count: the set-up
    (seeded weights and gradients, the moments' first allocation) launches too, and the difference leaves it out"""
    a, err = _traced_run(out_dir, form, steps[0])
    if a is None:
        return {"error": err}
    b, err = _traced_run(out_dir, form, steps[1])
    if b is None:
        return {"error": err}
    extra = steps[1] - steps[0]
    per = {k: ((b[k][0] - a[k][0]) / extra, (b[k][1] - a[k][1]) / 1e6 / extra) for k in b if b[k][0] != a[k][0]}
    top = sorted(per.items(), key=lambda kv: -kv[1][1])[:6]
    return {"launches_per_step": round(sum(c for c, _ in per.values()), 2),
            "kernel_ms_per_step": round(sum(t for _, t in per.values()), 4),
            "top": {k: {"calls_per_step": round(c, 2), "ms_per_step": round(t, 4)} for k, (c, t) in top}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--forms", default=",".join(FORMS))
    ap.add_argument("--rocprof", default=None, metavar="DIR", help="also trace a short run of every form under rocprofv3 into DIR")
    args = ap.parse_args()
    forms = tuple(args.forms.split(","))
    res = {}
    if args.rocprof:
        # (first, before this process opens the GPU; each traced program is a fresh child behind `--`)
        res["trace"] = {f: trace(args.rocprof, f) for f in forms}
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("optim_step_time.py needs an MI355X: a time taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    res["gpu"] = torch.cuda.get_device_name(0)
    # one net per form (each optimiser moves its own copy), the same seeded weights and gradients
    steps_of = {}
    for f in forms:
        net = setup(dev)
        opt, step = make(f, net)
        steps_of[f] = (net, opt, step)
        for _ in range(args.warmup):
            step()
    n_par = [p for p in steps_of[forms[0]][0].parameters() if p.requires_grad]
    res["tensors"], res["elements"] = len(n_par), int(sum(p.numel() for p in n_par))
    torch.cuda.synchronize()
    wall, queue, devt = ({f: [] for f in forms} for _ in range(3))
    for r in range(args.rounds):
        for f in (forms if r % 2 == 0 else forms[::-1]):
            step = steps_of[f][2]
            w, q, d = 0.0, 0.0, 0.0
            for _ in range(args.steps):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                w0 = time.perf_counter()
                t0.record()
                step()
                t1.record()
                w1 = time.perf_counter()
                torch.cuda.synchronize()
                w += time.perf_counter() - w0
                q += w1 - w0
                d += t0.elapsed_time(t1)
            wall[f].append(w * 1e3 / args.steps)
            queue[f].append(q * 1e3 / args.steps)
            devt[f].append(d / args.steps)
    for f in forms:
        # host_sync: wall time of a step with a synchronisation at both ends; host_queue: until step() returns; device: between
        # events recorded around the step
        res[f] = {k + "_ms_per_step": {"median": round(float(np.median(v[f])), 4), "min": round(float(np.min(v[f])), 4),
                                       "max": round(float(np.max(v[f])), 4)}
                  for k, v in (("host_sync", wall), ("host_queue", queue), ("device", devt))}
    res["rounds"], res["steps_per_round"] = args.rounds, args.steps
    print(json.dumps(res))


if __name__ == "__main__":
    main()
