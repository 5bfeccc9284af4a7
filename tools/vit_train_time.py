"""Time and size one TransHE forward + backward of the training entry (autograd_path.vit_forward, depth 12, V = 3 views) in the
four combinations of cfg.train_attention x cfg.train_vit_dense, on the same box in the same job, at N_c = 500 and 1500:

    timeout -k 10 900 python tools/vit_train_time.py [--reps 10] [--rounds 5] [--warmup 3] [--nc 500,1500]

Prints one JSON line.  Per N_c and combination "attention/dense":
  * ms: device time of one forward + backward (gradients of the input and of every parameter), from a pair of device events
    around --reps repetitions after --warmup; the four combinations' windows alternate, --rounds rounds; the median round is
    reported with the lowest and highest round beside it (the run-to-run spread);
  * launches: device kernels of one forward + backward, counted by torch.profiler in a pass of its own after the timed
    windows (null where the profiler gives nothing);
  * peak_allocated_MiB: torch.cuda.max_memory_allocated of one forward + backward after a warm-up call;
  * grad_max_diff_rel: the largest difference of any gradient from the torch/torch combination's, relative to that gradient's
    largest value.
No threshold on any figure; without an MI355X it fails (there is no CPU form)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VIEWS, DIM, DEPTH = 3, 192, 12
COMBOS = (("torch", "torch"), ("device", "torch"), ("torch", "device"), ("device", "device"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nc", default="500,1500")
    args = ap.parse_args()
    import torch
    from transhuman_amd import hip, synth
    from transhuman_amd.config import get_cfg
    from transhuman_amd.networks import autograd_path
    from transhuman_amd.networks.cross_transformer import Network
    if not torch.cuda.is_available():
        raise hip.HipError("tools/vit_train_time.py needs an MI355X")
    dev = torch.device("cuda:0")
    hip.load_library()
    cfg = get_cfg()
    cfg.vit_depth = DEPTH
    torch.manual_seed(0)
    net = Network()
    net.load_state_dict(synth.det_state_dict(net.state_dict(), seed=0, sigma_bias=-1.7))
    vit = net.ViT.to(dev).train()
    params = [p for k, p in vit.named_parameters() if k.startswith(("blocks.", "norm."))]

    def step(x, pe, w, combo):
        for p in params:
            p.grad = None
        x.grad = None
        (autograd_path.vit_forward(vit, x, pe, attention=combo[0], dense=combo[1]) * w).sum().backward()

    def window(x, pe, w, combo, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            step(x, pe, w, combo)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    def launches(x, pe, w, combo):
        try:
            from torch.profiler import ProfilerActivity, profile
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                step(x, pe, w, combo)
                torch.cuda.synchronize()
            n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
            return n or None
        except Exception:                                   # noqa: BLE001 (a figure that cannot be had is reported as null)
            return None

    res = {"device": torch.cuda.get_device_name(0), "views": VIEWS, "depth": DEPTH, "reps": args.reps, "rounds": args.rounds,
           "shapes": {}}
    for N in (int(n) for n in args.nc.split(",")):
        x = torch.from_numpy(synth.smooth_noise((VIEWS, N, DIM), N, passes=0)).to(dev).requires_grad_(True)
        pe = (torch.rand(VIEWS, N, 3, generator=torch.Generator().manual_seed(N)) * 2 - 1).to(dev)
        w = torch.randn(VIEWS, N, DIM, generator=torch.Generator().manual_seed(N + 1)).to(dev)
        out, grads = {}, {}
        for combo in COMBOS:
            window(x, pe, w, combo, args.warmup)
            grads[combo] = [x.grad.detach().clone()] + [p.grad.detach().clone() for p in params]
        rounds = {combo: [] for combo in COMBOS}
        for _ in range(args.rounds):
            for combo in COMBOS:
                rounds[combo].append(window(x, pe, w, combo, args.reps))
        for combo in COMBOS:
            r = rounds[combo]
            ent = {"ms": round(float(np.median(r)), 3), "ms_min": round(min(r), 3), "ms_max": round(max(r), 3)}
            step(x, pe, w, combo)
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            step(x, pe, w, combo)
            torch.cuda.synchronize()
            ent["peak_allocated_MiB"] = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)
            ent["grad_max_diff_rel"] = max(float((a - b).abs().max() / b.abs().max())
                                           for a, b in zip(grads[combo], grads[COMBOS[0]]))
            out["/".join(combo)] = ent
        for combo in COMBOS:
            out["/".join(combo)]["launches"] = launches(x, pe, w, combo)
        res["shapes"][str(N)] = out
    print(json.dumps(res))


if __name__ == "__main__":
    main()
