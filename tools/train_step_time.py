"""Time one training step (forward + loss.backward() of Renderer.render under autograd) at the reference's training shape --
2 400 rays x 64 samples, V = 3 input views of 512 x 512, N_c = 500 -- in both modes of cfg.train_kernels on the same box in
the same job: "torch" (every stage composed from torch operators) and "device" (K4, K5 and K7 through the HIP forwards with
the HIP adjoints of K17, transhuman_amd/networks/train_ops.py).

    timeout -k 10 900 python tools/train_step_time.py [--steps 10] [--warmup 2] [--rocprof DIR]

--maps full,latents repeats every mode with cfg.train_maps = "latents" (K19: the encoder's latents sampled directly) in the same
process; --point-net torch,device does the same with cfg.train_point_net = "device" (K20: the per-point network layer by layer
on the device; keys gain '+pointnet'); --encoder torch,device with cfg.train_encoder = "device" (K23: the encoder trunk's backward as
HIP kernels; keys gain '+encoder'); --encoder-fwd torch,device with cfg.train_encoder_fwd = "device" for the runs with the encoder on
the device (K29: the trunk's forward as HIP kernels too; keys gain '+fwd' after '+encoder'); --gather-bwd atomic,ordered with cfg.train_gather_bwd = "ordered" for the "latents" runs (K19's
backward without float atomics, k_latgather_ord.hip; keys gain '+ordered' after '+latents'); --rounds N repeats the whole sweep N
times in alternating order, so the forms are timed in turn in one process (per key then: the median of the rounds' medians with
the lowest and the highest); --attention / --vit-dense set cfg.train_attention / cfg.train_vit_dense for the whole run.
Prints one JSON line.  Per mode: median and minimum wall time of a step over --steps steps after --warmup (host clock around
forward + backward with a device synchronisation at both ends) and torch.cuda.max_memory_allocated of the timed steps; the
largest difference of the outputs and of every parameter gradient between the two modes; and, with --rocprof DIR, the device
time of the K17 kernels per step from `rocprofv3 --kernel-trace --stats` over a short run of the "device" mode in a fresh child
process (DIR keeps the trace).  --optim torch,device adds the optimiser step (the reference's torch.optim.Adam form with
clip_grad_value_, or train_optim.DeviceAdam) to what is timed.  No threshold on any figure."""
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

RAYS, SAMPLES, VIEWS, NC, SIZE = 2400, 64, 3, 500, 512
K17 = ("dpb_", "dparf_kernel<false, -2>", "dparf_kernelILb0ELin2E", "pixgather_bwd_kernel", "composite_bwd_kernel")


def setup(dev):
    import torch
    from transhuman_amd import synth
    from transhuman_amd.config import get_cfg
    from transhuman_amd.networks.cross_transformer import Network
    from transhuman_amd.networks.renderer.if_clight_renderer import Renderer
    cfg = get_cfg()
    cfg.N_samples, cfg.num_class, cfg.vit_depth, cfg.perturb, cfg.raw_noise_std = SAMPLES, NC, 12, 0.0, 0.0
    torch.manual_seed(0)
    net = Network()
    net.load_state_dict(synth.det_state_dict(net.state_dict(), seed=0, sigma_bias=-1.7))
    net.train()
    net = net.to(dev)
    body, _ = synth.make_body(0)
    d = np.load(os.path.join(ROOT, "tests", "golden", "synth_assign.npz"))
    assign = d[f"assign_{NC}"].astype(np.int64) if f"assign_{NC}" in d.files else synth.kmeans_assign(body, NC).astype(np.int64)
    r = Renderer(net, vertex_can=body.astype(np.float64) * 1.02 + 0.001, pc2voxel_ind=assign)
    b = synth.make_batch(SIZE, SIZE, VIEWS, seed=0, all_rays=False)
    n = b["ray_o"].shape[1]
    pick = torch.from_numpy(np.sort(np.random.RandomState(0).choice(n, RAYS, replace=n < RAYS)))
    for k in ("ray_o", "ray_d", "near", "far"):
        b[k] = b[k][:, pick].contiguous()
    return net, r, synth.batch_to(b, dev)


def step(net, r, b, target):
    import torch
    for p in net.parameters():
        p.grad = None
    ret = r.render(b)
    loss = torch.mean((ret["rgb_map"] - target) ** 2) + 0.1 * ret["acc_map"].mean() + 0.01 * ret["depth_map"].mean()
    loss.backward()
    return ret


def run_mode(net, r, b, target, steps, warmup):
    """in whatever mode cfg is in"""
    import torch
    for _ in range(warmup):
        step(net, r, b, target)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    ms = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ret = step(net, r, b, target)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    peak = torch.cuda.max_memory_allocated()
    outs = {k: v.detach().clone() for k, v in ret.items()}
    grads = {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}
    return {"step_ms_median": round(float(np.median(ms)), 2), "step_ms_min": round(float(np.min(ms)), 2), "steps": steps,
            "peak_allocated_MiB": round(peak / 2 ** 20, 1)}, outs, grads


def run_optim(kind, net, r, b, target, steps, warmup):
    """forward + backward + clip at 40 + optimiser step, in whatever mode cfg is in; the weights are put back"""
    import torch
    from transhuman_amd.train_optim import DeviceAdam
    saved = {k: v.detach().clone() for k, v in net.state_dict().items()}
    params = [p for p in net.parameters() if p.requires_grad]
    groups = [{"params": [p], "lr": 7e-4, "weight_decay": 0} for p in params]
    if kind == "device":
        opt = DeviceAdam(groups, 7e-4, clip_value=40.0)
    elif kind == "torch":
        opt = torch.optim.Adam(groups, 7e-4)
    else:
        raise SystemExit(f"--optim: {kind!r} is neither 'torch' nor 'device'")
    ms, opt_ms = [], []
    for i in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step(net, r, b, target)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if kind == "torch":
            torch.nn.utils.clip_grad_value_(params, 40.0)
        opt.step()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if i >= warmup:
            ms.append((t2 - t0) * 1e3)
            opt_ms.append((t2 - t1) * 1e3)
    net.load_state_dict(saved)
    return {"step_ms_median": round(float(np.median(ms)), 2), "step_ms_min": round(float(np.min(ms)), 2),
            "optim_ms_median": round(float(np.median(opt_ms)), 3), "optim_ms_min": round(float(np.min(opt_ms)), 3), "steps": steps}


def kernel_times(out_dir, steps):
    """per-step device time of the K17 kernels from the child's kernel trace"""
    agg = defaultdict(lambda: [0, 0])
    for path in glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            name = row["Kernel_Name"]
            if any(t in name for t in K17):
                key = name.split("(")[0][:60]
                agg[key][0] += 1
                agg[key][1] += int(row["End_Timestamp"]) - int(row["Start_Timestamp"])
    return {k: {"calls_per_step": round(c / steps, 2), "us_per_step": round(t / 1e3 / steps, 1)} for k, (c, t) in sorted(agg.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--modes", default="torch,device")
    ap.add_argument("--maps", default="full", help="comma list of cfg.train_maps values; every mode runs once per value "
                                                   "(results of a value other than 'full' are keyed '<mode>+<value>')")
    ap.add_argument("--point-net", default="torch", help="comma list of cfg.train_point_net values; every mode runs once per value "
                                                         "(results of 'device' are keyed '<mode>[+<maps>]+pointnet')")
    ap.add_argument("--encoder", default="torch", help="comma list of cfg.train_encoder values; every mode runs once per value "
                                                       "(results of 'device' are keyed '<mode>[+<maps>][+pointnet]+encoder')")
    ap.add_argument("--encoder-fwd", default="torch", help="comma list of cfg.train_encoder_fwd values; every run with the encoder on "
                                                           "the device runs once per value (results of 'device' are keyed "
                                                           "'...+encoder+fwd')")
    ap.add_argument("--gather-bwd", default="atomic", help="comma list of cfg.train_gather_bwd values; every 'latents' mode runs once "
                                                           "per value (results of 'ordered' are keyed '<mode>+latents+ordered...')")
    ap.add_argument("--rounds", type=int, default=1, help="repeat the sweep this many times, in alternating order")
    ap.add_argument("--attention", default="torch", help="cfg.train_attention of every run")
    ap.add_argument("--vit-dense", default="torch", help="cfg.train_vit_dense of every run")
    ap.add_argument("--rocprof", default=None, metavar="DIR", help="also trace a short 'device' run under rocprofv3 into DIR")
    ap.add_argument("--optim", default="", help="comma list of 'torch' (the reference's form: torch.optim.Adam, one group per "
                                                "parameter, + clip_grad_value_(., 40)) and 'device' (train_optim.DeviceAdam, "
                                                "K22): adds the optimiser step to what is timed, in the last mode run "
                                                "(results keyed 'step+optim:<value>'; the weights are restored afterwards)")
    args = ap.parse_args()
    res = {"shape": {"rays": RAYS, "samples": SAMPLES, "views": VIEWS, "n_clusters": NC, "image": [SIZE, SIZE]}}
    if args.rocprof:
        # (first, before this process opens the GPU; the traced program is a fresh child behind `--`)
        os.makedirs(args.rocprof, exist_ok=True)
        n = 3
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", args.rocprof, "-o", "train_step", "--",
               sys.executable, os.path.abspath(__file__), "--modes", "device", "--steps", str(n), "--warmup", "0"]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        res["k17_kernels"] = kernel_times(args.rocprof, n) if p.returncode == 0 else {"error": p.stderr[-400:]}
    import torch
    from transhuman_amd.config import override
    dev = torch.device("cuda:0")
    res["device"] = torch.cuda.get_device_name(0)
    net, r, b = setup(dev)
    target = torch.rand((1, RAYS, 3), device=dev)
    seen = {}
    with override(train_attention=args.attention, train_vit_dense=args.vit_dense):
        sweep = []
        for maps in args.maps.split(","):
            for gather_bwd in (args.gather_bwd.split(",") if maps == "latents" else ["atomic"]):
                for point_net in args.point_net.split(","):
                    for encoder in args.encoder.split(","):
                        for fwd in (args.encoder_fwd.split(",") if encoder == "device" else ["torch"]):
                            for mode in args.modes.split(","):
                                key = (mode if maps == "full" else f"{mode}+{maps}") + ("" if gather_bwd == "atomic" else "+ordered") + \
                                    ("" if point_net == "torch" else "+pointnet") + ("" if encoder == "torch" else "+encoder") + \
                                    ("" if fwd == "torch" else "+fwd")
                                sweep.append((key, dict(train_kernels=mode, train_maps=maps, train_gather_bwd=gather_bwd,
                                                        train_point_net=point_net, train_encoder=encoder, train_encoder_fwd=fwd)))
        rounds = {}
        for rnd in range(max(args.rounds, 1)):
            for key, switches in (sweep if rnd % 2 == 0 else sweep[::-1]):
                with override(**switches):
                    res[key], outs, grads = run_mode(net, r, b, target, args.steps, args.warmup)
                rounds.setdefault(key, []).append(res[key])
                seen[key] = (outs, grads)
        if args.rounds > 1:
            for key, rr in rounds.items():
                med = [x["step_ms_median"] for x in rr]
                res[key] = {"step_ms_median": round(float(np.median(med)), 2), "step_ms_lowest_round": min(med),
                            "step_ms_highest_round": max(med), "step_ms_min": min(x["step_ms_min"] for x in rr),
                            "rounds": len(rr), "steps": args.steps,
                            "peak_allocated_MiB": max(x["peak_allocated_MiB"] for x in rr)}
        with override(**switches):                                  # (the optimiser runs in the last mode run)
            for kind in [k for k in args.optim.split(",") if k]:
                res[f"step+optim:{kind}"] = run_optim(kind, net, r, b, target, args.steps, args.warmup)
    if "torch" in seen and "device" in seen:
        (o0, g0), (o1, g1) = seen["torch"], seen["device"]
        res["device_vs_torch"] = {
            "outputs_max_abs": max(float((o0[k] - o1[k]).abs().max()) for k in o0),
            "grads_max_rel_to_own_max": max(float((g0[k] - g1[k]).abs().max()) / max(float(g0[k].abs().max()), 1e-30) for k in g0)}
    for key in [k for k in seen if k.endswith("+encoder") and k[:-8] in seen]:
        (o0, g0), (o1, g1) = seen[key[:-8]], seen[key]
        res[key + "_vs_torch_encoder"] = {
            "outputs_max_abs": max(float((o0[k] - o1[k]).abs().max()) for k in o0),
            "grads_max_rel_to_own_max": max(float((g0[k] - g1[k]).abs().max()) / max(float(g0[k].abs().max()), 1e-30) for k in g0
                                            if not k.endswith("spatial_key_value_0.key_embed.bias"))}
    for key in [k for k in seen if k.endswith("+fwd") and k[:-4] in seen]:
        (o0, g0), (o1, g1) = seen[key[:-4]], seen[key]
        res[key + "_vs_torch_forward"] = {
            "outputs_max_abs": max(float((o0[k] - o1[k]).abs().max()) for k in o0),
            "grads_max_rel_to_own_max": max(float((g0[k] - g1[k]).abs().max()) / max(float(g0[k].abs().max()), 1e-30) for k in g0
                                            if not k.endswith("spatial_key_value_0.key_embed.bias"))}
    for key in [k for k in seen if k.endswith("+pointnet") and k[:-9] in seen]:
        (o0, g0), (o1, g1) = seen[key[:-9]], seen[key]
        res[key + "_vs_torch_point_net"] = {
            "outputs_max_abs": max(float((o0[k] - o1[k]).abs().max()) for k in o0),
            "grads_max_rel_to_own_max": max(float((g0[k] - g1[k]).abs().max()) / max(float(g0[k].abs().max()), 1e-30) for k in g0
                                            if not k.endswith("spatial_key_value_0.key_embed.bias"))}
    for key in [k for k in seen if "+ordered" in k and k.replace("+ordered", "") in seen]:
        (o0, g0), (o1, g1) = seen[key.replace("+ordered", "")], seen[key]
        res[key + "_vs_atomic"] = {
            "outputs_max_abs": max(float((o0[k] - o1[k]).abs().max()) for k in o0),
            "grads_max_rel_to_own_max": max(float((g0[k] - g1[k]).abs().max()) / max(float(g0[k].abs().max()), 1e-30) for k in g0)}
    for key in [k for k in seen if "+" in k and not k.endswith(("+pointnet", "+encoder", "+ordered", "+fwd")) and k.split("+")[0] in seen]:
        (o0, g0), (o1, g1) = seen[key.split("+")[0]], seen[key]
        res[key + "_vs_full"] = {
            "outputs_max_abs": max(float((o0[k] - o1[k]).abs().max()) for k in o0),
            "grads_max_rel_to_own_max": max(float((g0[k] - g1[k]).abs().max()) / max(float(g0[k].abs().max()), 1e-30) for k in g0)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
