"""Time the per-point network alone -- forward + backward of MLP_forward_ori -- in both modes of cfg.train_point_net on the same
box in the same process, at the chunk of a training step: P = 32 768 samples, V = 3 views, seeded rows.

    timeout -k 10 600 python tools/point_net_time.py [--rounds 5] [--warmup 2] [--points 32768] [--rocprof DIR]

One call = raw = network(h [P,V,256], f [P,V,384], viewdir [P,27]); raw.backward(seeded g) with h and f asking for their gradients
(they come from K4 and K5 in a step) and every parameter getting its own.
  "torch"   autograd_path.point_network under torch autograd (h without its pad column)
  "device"  autograd_path.point_network_device (K20: train_ops.ReluLinearFn / LinearFn / CrossViewAttentionFn)
Prints one JSON line.  Per mode: the median of --rounds alternating rounds with the lowest and the highest (device events around
the call, one synchronisation after the closing event), torch.cuda.max_memory_allocated of a call above what is allocated before
it (the inputs, the parameters), and the largest difference of raw and of every gradient between the modes.  With --rocprof DIR:
per mode the kernel launches per call and the launches that carry the time, from `rocprofv3 --kernel-trace --stats` over a
short run of that mode in a fresh child process behind `--` (DIR keeps the traces).  No threshold on any figure."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
from collections import defaultdict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VIEWS = 3
MODES = ("torch", "device")


def setup(dev, points):
    import torch
    from transhuman_amd import synth
    from transhuman_amd.config import get_cfg
    from transhuman_amd.networks.cross_transformer import Network
    get_cfg().vit_depth = 2                                # (TransHE is not run here)
    torch.manual_seed(0)
    net = Network()
    net.load_state_dict(synth.det_state_dict(net.state_dict(), seed=0, sigma_bias=-1.7))
    net = net.train().to(dev)
    gen = torch.Generator().manual_seed(1)
    h = torch.randn((points, VIEWS, 256), generator=gen)
    h[..., 255] = 0.0                                      # K4's pad column
    f = torch.randn((points, VIEWS, 384), generator=gen)
    vd = torch.randn((points, 27), generator=gen)
    g = torch.randn((points, 4), generator=gen)
    return net, h.to(dev), f.to(dev), vd.to(dev), g.to(dev)


def call(mode, net, h, f, vd, g):
    from transhuman_amd.networks import autograd_path as A
    net.zero_grad(set_to_none=True)
    h, f = h.detach().requires_grad_(True), f.detach().requires_grad_(True)
    raw = A.point_network_device(net, h, f, vd) if mode == "device" else A.point_network(net, h[..., :255], f, vd)
    raw.backward(g)
    return raw.detach(), h.grad[..., :255], f.grad


def trace(out_dir, mode, points, calls=3):
    """kernel launches per call and the ten launches with the most device time, from a traced child run of one mode"""
    d = os.path.join(out_dir, mode)
    os.makedirs(d, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "point_net", "--",
           sys.executable, os.path.abspath(__file__), "--modes", mode, "--rounds", str(calls), "--warmup", "0", "--points", str(points)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        return {"error": p.stderr[-400:]}
    agg, n = defaultdict(lambda: [0, 0]), 0
    for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            key = row["Kernel_Name"].split("(")[0][:70]
            agg[key][0] += 1
            agg[key][1] += int(row["End_Timestamp"]) - int(row["Start_Timestamp"])
            n += 1
    top = sorted(agg.items(), key=lambda kv: -kv[1][1])[:10]
    return {"launches_per_call": round(n / calls, 1), "kernel_ms_per_call": round(sum(t for _, t in agg.values()) / 1e6 / calls, 3),
            "top": {k: {"calls_per_call": round(c / calls, 1), "ms_per_call": round(t / 1e6 / calls, 3)} for k, (c, t) in top}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--points", type=int, default=32768)
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--rocprof", default=None, metavar="DIR", help="also trace a short run of every mode under rocprofv3 into DIR")
    args = ap.parse_args()
    modes = tuple(args.modes.split(","))
    res = {"shape": {"points": args.points, "views": VIEWS}}
    if args.rocprof:
        # (first, before this process opens the GPU; each traced program is a fresh child behind `--`)
        res["trace"] = {m: trace(args.rocprof, m, args.points) for m in modes}
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("point_net_time.py needs an MI355X: a time taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    res["device"] = torch.cuda.get_device_name(0)
    net, h, f, vd, g = setup(dev, args.points)
    seen = {}
    for m in modes:
        for _ in range(max(args.warmup, 1) if len(modes) > 1 else args.warmup):
            out = call(m, net, h, f, vd, g)
            seen[m] = dict(zip(("raw", "g_h", "g_f"), out))
            seen[m].update({k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None})
    net.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    ms, peak = {m: [] for m in modes}, {m: 0 for m in modes}
    for r in range(args.rounds):
        for m in (modes if r % 2 == 0 else modes[::-1]):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            out = call(m, net, h, f, vd, g)
            t1.record()
            torch.cuda.synchronize()
            ms[m].append(t0.elapsed_time(t1))
            peak[m] = max(peak[m], torch.cuda.max_memory_allocated() - base)
            del out
            net.zero_grad(set_to_none=True)
    for m in modes:
        res[m] = {"call_ms_median": round(float(np.median(ms[m])), 2), "call_ms_min": round(float(np.min(ms[m])), 2),
                  "call_ms_max": round(float(np.max(ms[m])), 2), "rounds": args.rounds,
                  "peak_allocated_MiB": round(peak[m] / 2 ** 20, 1)}
    if len(seen) == 2:
        a, b = (seen[m] for m in MODES)
        assert set(a) == set(b) and len(a) == 3 + 32
        # (the exact gradient of the pixel branch's key bias is 0 -- the softmax cancels it: both modes leave rounding there)
        res["device_vs_torch"] = {"max_rel_to_own_max": max(
            float((a[k] - b[k]).abs().max()) / max(float(a[k].abs().max()), 1e-30) for k in a
            if k != "spatial_key_value_0.key_embed.bias")}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
