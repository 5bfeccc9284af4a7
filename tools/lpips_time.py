"""Time th_lpips (csrc/k_lpips.hip): one image pair (N = 1) at 512 x 512 and at the S-real frame's crop (the body box's
bounding rectangle of the 512 x 512 synthetic frame: 414 x 360), seeded He-normal VGG16 weights.

    timeout -k 10 300 python tools/lpips_time.py [--iters N]

Prints one JSON line per size: device time per pair (HIP events around N back-to-back calls of the C entry point with a
preallocated workspace: the 23 launches, nothing else) and host wall time per hip.lpips() call (allocation, launches,
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
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = hip.load_library()
    g = torch.Generator(device=dev).manual_seed(0)
    conv_w = [torch.randn((co, ci, 3, 3), generator=g, device=dev) * (2.0 / (9 * ci)) ** 0.5
              for co, ci in hip.LPIPS_CONV_SHAPES]
    conv_b = [0.05 * torch.rand((co,), generator=g, device=dev) for co, _ in hip.LPIPS_CONV_SHAPES]
    lin_w = [torch.rand((1, c, 1, 1), generator=g, device=dev) * 0.1 for c in hip.LPIPS_TAP_CHANNELS]
    packed = hip.lpips_pack(conv_w, conv_b, lin_w, dev)
    h_ctx = hip.ctx(dev)
    for H, W in ((512, 512), (414, 360)):
        a = torch.rand((1, 3, H, W), generator=g, device=dev) * 2 - 1
        b = (a + 0.05 * torch.randn((1, 3, H, W), generator=g, device=dev)).clamp(-1, 1)
        ws = torch.empty(max(int(lib.th_lpips_workspace_bytes(1, H, W)), 256), dtype=torch.uint8, device=dev)
        out = torch.empty((1, 6), dtype=torch.float64, device=dev)

        def call():
            hip._check(lib.th_lpips(h_ctx, hip._p(a), hip._p(b), 1, H, W, hip._p(packed), hip._p(out), hip._p(ws),
                                    ws.numel(), hip._stream()))

        for _ in range(3):
            call()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            call()
        e1.record()
        torch.cuda.synchronize()
        dev_ms = e0.elapsed_time(e1) / args.iters
        first = out.clone()
        walls = []
        for _ in range(5):
            t0 = time.perf_counter()
            v = hip.lpips(a, b, packed)
            torch.cuda.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
        assert torch.equal(v, first), (v, first)
        hl, wl = [H], [W]
        for _ in range(4):
            hl.append(hl[-1] // 2)
            wl.append(wl[-1] // 2)
        levels = ((0, 1), (2, 3), (4, 5, 6), (7, 8, 9), (10, 11, 12))
        macs = sum(co * ci * 9 * hl[lev] * wl[lev] for lev, layers in enumerate(levels) for l in layers
                   for co, ci in [hip.LPIPS_CONV_SHAPES[l]])
        conv_flop = 2 * 2 * macs                             # two images, two flops per multiply-add
        print(json.dumps({"shape": [H, W], "lpips": float(first[0, 5]), "iters": args.iters,
                          "device_ms_per_pair": round(dev_ms, 4), "conv_gflop": round(conv_flop / 1e9, 1),
                          "conv_tflops": round(conv_flop / (dev_ms * 1e-3) / 1e12, 1),
                          "wall_ms_per_hip_lpips_median": round(float(np.median(walls)), 4),
                          "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
