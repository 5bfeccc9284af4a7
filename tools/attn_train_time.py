"""Time and size the training form of TransHE's attention (cfg.train_attention) against the torch form, on the same box in the
same job, at V = 3 views, 3 heads and N_c = 500 and 1500 tokens:

    timeout -k 10 600 python tools/attn_train_time.py [--reps 50] [--warmup 5] [--nc 500,1500]

Prints one JSON line.  Per N_c and mode ("torch": the three lines of autograd_path.vit_forward -- q k^T / 8, softmax, the
product with v -- under torch autograd; "device": train_ops.AttentionFn):
  * layer_ms: device time of ONE layer's attention forward + backward on a given qkv [V, N_c, 576] and upstream gradient, from
    a pair of device events around --reps repetitions after --warmup (the two modes' windows alternate, three rounds, the
    median round is reported);
  * peak_allocated_MiB: torch.cuda.max_memory_allocated of autograd_path.vit_forward + backward at depth 12;
  * the largest difference of the two modes' qkv gradients, relative to the torch form's largest.
No threshold on any figure; without an MI355X it fails (there is no CPU form)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VIEWS, HEADS, DIM = 3, 3, 192


def attention_torch(qkv):
    V, N, _ = qkv.shape
    r = qkv.reshape(V, N, 3, HEADS, DIM // HEADS).permute(2, 0, 3, 1, 4)
    a = (r[0] @ r[1].transpose(-2, -1)) * 0.125
    return (a.softmax(dim=-1) @ r[2]).transpose(1, 2).reshape(V, N, DIM)


def layer_window(fn, qkv, g, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        qkv.grad = None
        fn(qkv).backward(g)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--nc", default="500,1500")
    args = ap.parse_args()
    import torch
    from transhuman_amd import hip, synth
    from transhuman_amd.config import get_cfg
    from transhuman_amd.networks import autograd_path, train_ops
    from transhuman_amd.networks.cross_transformer import Network
    if not torch.cuda.is_available():
        raise hip.HipError("tools/attn_train_time.py needs an MI355X")
    dev = torch.device("cuda:0")
    hip.load_library()
    cfg = get_cfg()
    cfg.vit_depth = 12
    torch.manual_seed(0)
    net = Network()
    net.load_state_dict(synth.det_state_dict(net.state_dict(), seed=0, sigma_bias=-1.7))
    vit = net.ViT.to(dev).train()
    fns = {"torch": attention_torch, "device": lambda t: train_ops.AttentionFn.apply(t, HEADS)}
    res = {"device": torch.cuda.get_device_name(0), "views": VIEWS, "heads": HEADS, "reps": args.reps, "shapes": {}}
    for N in (int(n) for n in args.nc.split(",")):
        rs = np.random.RandomState(N)
        qkv = torch.from_numpy(rs.normal(scale=3.0, size=(VIEWS, N, 3 * DIM)).astype(np.float32)).to(dev).requires_grad_(True)
        g = torch.from_numpy(rs.normal(size=(VIEWS, N, DIM)).astype(np.float32)).to(dev)
        out = {m: {} for m in fns}
        grads = {}
        for m, fn in fns.items():
            layer_window(fn, qkv, g, args.warmup)
            grads[m] = qkv.grad.detach().clone()
        rounds = {m: [] for m in fns}
        for _ in range(3):
            for m, fn in fns.items():
                rounds[m].append(layer_window(fn, qkv, g, args.reps))
        for m in fns:
            out[m]["layer_ms"] = round(float(np.median(rounds[m])), 4)
            out[m]["layer_ms_rounds"] = [round(t, 4) for t in rounds[m]]
        x = torch.from_numpy(synth.smooth_noise((VIEWS, N, DIM), N, passes=0)).to(dev)
        pe = (torch.rand(VIEWS, N, 3, generator=torch.Generator().manual_seed(N)) * 2 - 1).to(dev)
        for m in fns:
            for timed in (False, True):
                for p in vit.parameters():
                    p.grad = None
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                autograd_path.vit_forward(vit, x, pe, attention=m).square().mean().backward()
                torch.cuda.synchronize()
            out[m]["peak_allocated_MiB"] = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)
        out["qkv_grad_max_diff_rel"] = float((grads["torch"] - grads["device"]).abs().max() / grads["torch"].abs().max())
        res["shapes"][str(N)] = out
    print(json.dumps(res))


if __name__ == "__main__":
    main()
