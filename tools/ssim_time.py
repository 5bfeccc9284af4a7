"""Time th_ssim (csrc/k_metrics.hip) on a 512 x 512 x 3 fp32 crop -- the evaluator's largest crop at ratio = 0.5 --
taken as a strided view of a 1024 x 1024 frame.

    timeout -k 10 120 python tools/ssim_time.py [--iters N]

Prints one JSON line: device time per call (HIP events around N back-to-back calls of the C entry point with a
preallocated workspace: the two launches, nothing else) and host wall time per hip.ssim() call (allocation, launches,
the read-back of the result)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from transhuman_amd import hip  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = hip.load_library()
    g = torch.Generator(device=dev).manual_seed(0)
    fa = torch.rand((1024, 1024, 3), generator=g, device=dev)
    fb = (fa + 0.05 * torch.randn((1024, 1024, 3), generator=g, device=dev)).clamp(0, 1)
    a, b = fa[256:768, 256:768], fb[256:768, 256:768]
    H, W, C = a.shape
    ws = torch.empty(max(int(lib.th_ssim_workspace_bytes(H, W, C)), 256), dtype=torch.uint8, device=dev)
    out = torch.empty(1, dtype=torch.float64, device=dev)
    h = hip.ctx(dev)

    def call():
        hip._check(lib.th_ssim(h, hip._p(a), hip._p(b), H, W, C, int(a.stride(0)), hip._p(out), hip._p(ws), ws.numel(),
                               hip._stream()))

    for _ in range(20):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.iters):
        call()
    e1.record()
    torch.cuda.synchronize()
    dev_ms = e0.elapsed_time(e1) / args.iters
    first = float(out.item())

    walls = []
    for _ in range(50):
        t0 = time.perf_counter()
        v = hip.ssim(a, b)
        walls.append((time.perf_counter() - t0) * 1e3)
    assert v == first, (v, first)
    print(json.dumps({"shape": [H, W, C], "pitch": int(a.stride(0)), "ssim": first, "iters": args.iters,
                      "device_ms_per_call": round(dev_ms, 4), "wall_ms_per_hip_ssim_median": round(float(np.median(walls)), 4),
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
