"""Time the LPIPS (VGG16) loss forward + backward on the device (th_lpips_train + th_lpips_bwd, csrc/k_lpips.hip) against
torch autograd through the same chain (F.conv2d / relu / max_pool2d and the head in fp32) on the same GPU.

    timeout -k 10 400 python tools/lpips_grad_time.py [--window-ms 400] [--rounds 5]

Shapes: N = 6 at 20 x 20 (the training shape: cfg.patch N_patches x size) and N = 1 at 512 x 512; seeded He-normal VGG16
weights.  The baseline does the work the loss needs and no more, like the vendored module (lpips.py:88 runs the two images
through the network separately): the features of the target in1 are computed under torch.no_grad(), so autograd keeps
activations and runs backward for the N images of in0 only -- what th_lpips_bwd does.  Device time from HIP events around
back-to-back forward + backward pairs with preallocated buffers, as many per round as fill --window-ms for the faster of the
two, the two implementations alternating round by round in one process; per shape one JSON line with the median of the rounds
and the lowest and highest.  At 20 x 20 the device form is bound by its nearly empty tiles at the deep levels, not by its 45
launches."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from transhuman_amd import hip  # noqa: E402

LEVELS = ((0, 1), (2, 3), (4, 5, 6), (7, 8, 9), (10, 11, 12))


def torch_features(x, conv_w, conv_b):
    """the five normalised taps of a batch"""
    shift = torch.tensor([-.030, -.088, -.188], device=x.device)[None, :, None, None]
    scale = torch.tensor([.458, .448, .450], device=x.device)[None, :, None, None]
    h = (x - shift) / scale
    taps = []
    for k, layers in enumerate(LEVELS):
        if k:
            h = F.max_pool2d(h, 2, 2)
        for l in layers:
            h = F.relu(F.conv2d(h, conv_w[l], conv_b[l], padding=1))
        taps.append(h / (torch.sqrt((h * h).sum(1, keepdim=True) + 1e-10) + 1e-10))
    return taps


def torch_chain(x0, x1, conv_w, conv_b, lin_w):
    """LPIPS totals [N]; only the x0 branch carries a graph (the target's features are constants of the loss)"""
    with torch.no_grad():
        f1 = torch_features(x1, conv_w, conv_b)
    f0 = torch_features(x0, conv_w, conv_b)
    total = 0
    for k in range(5):
        total = total + (((f0[k] - f1[k]) ** 2) * lin_w[k].reshape(1, -1, 1, 1)).sum(1).mean((1, 2))
    return total


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window-ms", type=float, default=400.0, help="least device time of one timed round")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = hip.load_library()
    g = torch.Generator(device=dev).manual_seed(0)
    conv_w = [torch.randn((co, ci, 3, 3), generator=g, device=dev) * (2.0 / (9 * ci)) ** 0.5
              for co, ci in hip.LPIPS_CONV_SHAPES]
    conv_b = [0.05 * torch.rand((co,), generator=g, device=dev) for co, _ in hip.LPIPS_CONV_SHAPES]
    lin_w = [torch.rand((1, c, 1, 1), generator=g, device=dev) * 0.1 for c in hip.LPIPS_TAP_CHANNELS]
    packed = hip.lpips_pack(conv_w, conv_b, lin_w, dev)
    packed_bwd = hip.lpips_pack_bwd(conv_w, dev)
    h_ctx = hip.ctx(dev)
    for N, H, W in ((6, 20, 20), (1, 512, 512)):
        a = torch.rand((N, 3, H, W), generator=g, device=dev) * 2 - 1
        b = (a + 0.05 * torch.randn((N, 3, H, W), generator=g, device=dev)).clamp(-1, 1)
        state = torch.empty(int(lib.th_lpips_train_state_bytes(N, H, W)), dtype=torch.uint8, device=dev)
        ws = torch.empty(int(lib.th_lpips_bwd_workspace_bytes(N, H, W)), dtype=torch.uint8, device=dev)
        out = torch.empty((N, 6), dtype=torch.float64, device=dev)
        g_out = torch.full((N,), 1.0 / N, dtype=torch.float64, device=dev)
        g_in = torch.empty((N, 3, H, W), dtype=torch.float32, device=dev)

        def device_pair():
            hip._check(lib.th_lpips_train(h_ctx, hip._p(a), hip._p(b), N, H, W, hip._p(packed), hip._p(out), hip._p(state),
                                          state.numel(), hip._stream()))
            hip._check(lib.th_lpips_bwd(h_ctx, hip._p(g_out), hip._p(a), N, H, W, hip._p(packed), hip._p(packed_bwd),
                                        hip._p(state), state.numel(), hip._p(g_in), hip._p(ws), ws.numel(), hip._stream()))

        leaf = a.clone().requires_grad_(True)

        def torch_pair():
            leaf.grad = None
            torch_chain(leaf, b, conv_w, conv_b, lin_w).mean().backward()

        for _ in range(2):
            device_pair()
            torch_pair()
        torch.cuda.synchronize()
        scale = float(leaf.grad.abs().max())
        diff = float((g_in - leaf.grad).abs().max())
        iters = max(10, int(args.window_ms / min(timed(device_pair, 5), timed(torch_pair, 5))) + 1)
        dev_ms, torch_ms = [], []
        for _ in range(args.rounds):
            dev_ms.append(timed(device_pair, iters))
            torch_ms.append(timed(torch_pair, iters))
        stat = lambda v: {"median": round(float(np.median(v)), 4), "lowest": round(min(v), 4), "highest": round(max(v), 4)}
        print(json.dumps({"shape": [N, H, W], "iters": iters, "rounds": args.rounds, "device_ms": stat(dev_ms),
                          "torch_autograd_ms": stat(torch_ms), "state_mib": round(state.numel() / 2 ** 20, 1),
                          "max_abs_diff_to_torch": diff, "max_abs_grad": scale, "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
