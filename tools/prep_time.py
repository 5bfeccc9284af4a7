"""Time the preparation of a frame's input views on the device (csrc/k_prep.hip, K16): combine_masks (two raw masks, border 5) +
prepare_views (undistort, area resize, background) for V = 3 camera frames of 1024 x 1024 -> 512 x 512, the reference's
process_loaded / get_mask for one frame of a moving subject.

    timeout -k 10 300 python tools/prep_time.py [--iters N] [--windows M]

Prints one JSON line.  Device time: HIP events around N back-to-back calls through the C entry points with preallocated buffers
(neither call waits on the host, so the calls queue behind each other; one window of N = 200 calls is tens of milliseconds of
device work), per call; median and minimum over M windows after a warm-up window -- for the pair and for each entry point alone --
and, from the shapes, the bytes a call must move (uint8 pictures and masks in, fp32 planes and uint8 masks out) with the rate that
makes of the median.  The inputs stay in the chip's caches between calls (V x 4 MiB): the figure is the steady state of a loop over
resident frames, not of frames that arrive over PCIe.  Also the host wall time per preprocess.combine_masks + prepare_views call
pair, and -- once, on view 0 -- equality with the numpy restatement.  There is no predecessor to compare with and no threshold on
the figures."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from transhuman_amd import hip, preprocess  # noqa: E402

V, H0, W0, N = 3, 1024, 1024, 2
D = np.array([[-0.21, 0.08, 0.0008, -0.0005, 0.01], [-0.19, 0.07, -0.0006, 0.0007, 0.008], [0.04, -0.02, 0.0003, 0.0002, 0.0]],
             np.float32)


def frames(seed=0):
    """smooth pictures with sensor noise under a body-sized mask and a second, slightly different mask"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:H0, :W0]
    img = np.stack([np.stack([127.5 + 110 * np.sin(0.011 * (x + 40 * c) + v) * np.cos(0.009 * y - c) for c in range(3)], -1)
                    for v in range(V)]) + rng.normal(0, 3, (V, H0, W0, 3))
    body = ((y - 540) / 420.0) ** 2 + ((x - 512) / 170.0) ** 2 < 1
    arm = ((y - 400) / 60.0) ** 2 + ((x - 700) / 190.0) ** 2 < 1
    K = np.array([[1080.0, 0, 509.3], [0, 1079.0, 515.6], [0, 0, 1]], np.float32)
    return (np.clip(np.rint(img), 0, 255).astype(np.uint8), np.stack([body] * V).astype(np.uint8) * 255,
            np.stack([body | arm] * V).astype(np.uint8), np.stack([K] * V))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--windows", type=int, default=9)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "prep_time.py needs an MI355X"
    dev = torch.device("cuda:0")
    lib = hip.load_library()
    img, m_a, m_b, K = frames()
    t_img, t_a, t_b, t_K, t_D = (torch.from_numpy(a).to(dev) for a in (img, m_a, m_b, K, D))
    lut = torch.from_numpy(preprocess.unit_table()).to(dev)
    msk = torch.empty((V, H0, W0), dtype=torch.uint8, device=dev)
    out = torch.empty((V, 3, H0 // N, W0 // N), dtype=torch.float32, device=dev)
    out_m = torch.empty((V, H0 // N, W0 // N), dtype=torch.uint8, device=dev)
    h, p = hip.ctx(dev), hip._p

    def f_mask():
        hip._check(lib.th_prep_mask(h, p(t_a), p(t_b), V, H0, W0, 5, p(msk), hip._stream()))

    def f_views():
        hip._check(lib.th_prep_views(h, p(t_img), p(msk), V, H0, W0, p(t_K), p(t_D), N, 1, 0, p(lut), p(out), p(out_m), hip._stream()))

    def pair():
        f_mask(), f_views()

    def timed(fn):
        ms = []
        for w in range(args.windows + 1):                               # (window 0: warm-up)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if w:
                ms.append(e0.elapsed_time(e1) / args.iters)
        return {"median": round(float(np.median(ms)), 5), "min": round(float(np.min(ms)), 5), "max": round(float(np.max(ms)), 5)}

    device_ms = {"pair": timed(pair), "combine_masks": timed(f_mask), "prepare_views": timed(f_views)}
    px0, px = V * H0 * W0, V * (H0 // N) * (W0 // N)
    nbytes = {"combine_masks": 3 * px0, "prepare_views": 4 * px0 + 13 * px}
    nbytes["pair"] = nbytes["combine_masks"] + nbytes["prepare_views"]
    rate = {k: round(nbytes[k] / (device_ms[k]["median"] * 1e-3) / 1e9, 1) for k in nbytes}
    # the library path, and what it computes
    walls = []
    for _ in range(30):
        t0 = time.perf_counter()
        m = preprocess.combine_masks(t_a, t_b, border=5)
        got = preprocess.prepare_views(t_img, m, t_K, t_D, ratio=1.0 / N, mask_bkgd=True, white_bkgd=False)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    assert torch.equal(got[0], out) and torch.equal(got[1], out_m) and torch.equal(m, msk)
    ref_m = preprocess.combine_masks_oracle(m_a[:1], m_b[:1], border=5)
    ref = preprocess.prepare_views_oracle(img[:1], ref_m, K[:1], D[:1], ratio=1.0 / N, mask_bkgd=True, white_bkgd=False)
    equal = bool(np.array_equal(ref_m[0], msk[0].cpu().numpy()) and np.array_equal(ref[0][0].view(np.int32), out[0].cpu().numpy().view(np.int32))
                 and np.array_equal(ref[1][0], out_m[0].cpu().numpy()))
    print(json.dumps({"views": V, "raw": [H0, W0], "out": [H0 // N, W0 // N], "border": 5, "iters_per_window": args.iters,
                      "windows": args.windows, "device": torch.cuda.get_device_name(0), "device_ms_per_call": device_ms,
                      "bytes_per_call": nbytes, "GB_per_s_at_median": rate,
                      "wall_ms_per_library_call_pair_median": round(float(np.median(walls)), 4),
                      "view0_equals_numpy_restatement": equal}))
    assert equal


if __name__ == "__main__":
    main()
