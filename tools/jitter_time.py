"""Time the colour jitter of a training item's raw frames on the device (csrc/k_jitter.hip, K25): V = 4 camera frames of
1024 x 1024 (three input views and the target view), the reference's ColorJitter in process_loaded for one item.

    timeout -k 10 300 python tools/jitter_time.py [--iters N] [--windows M]

Prints one JSON line.  Device time: HIP events around N back-to-back calls through the C entry points with preallocated buffers
(no call waits on the host, so the calls queue behind each other), per call; median, minimum and maximum over M = 20 windows after
a warm-up window -- the jitter alone and the jitter followed by prepare_views (K16, 1024 -> 512), each with contrast in the order
(two launches: the mean of every frame first) and without it (one launch); beside them prepare_views alone, the bytes a jitter
call must move (with contrast: two reads and one write of the frames) and the rate that makes of the median.  The frames stay in
the chip's caches between calls (4 x 3 MiB): the figure is the steady state of a loop over resident frames, not of frames that
arrive over PCIe.  For context only, the host wall time of the same four frames through Pillow's ImageEnhance / HSV chain
(median of 5), which the device's result is also compared with, byte for byte.  There is no predecessor to compare with and no
threshold on the figures."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from transhuman_amd import hip, preprocess  # noqa: E402
from tools.prep_time import D, frames  # noqa: E402

V, H0, W0, N = 4, 1024, 1024, 2
WITH = preprocess.JitterParams((2, 0, 1, 3), 1.31, 0.58, 1.62, -0.17)
WITHOUT = preprocess.JitterParams((2, 0, 1, 3), 1.31, None, 1.62, -0.17)


def pil_chain(img, params):
    """one frame through Pillow, as torchvision's PIL path runs it"""
    from PIL import Image, ImageEnhance
    enhancers = (ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color)
    im = Image.fromarray(img)
    for op in params.order:
        f = params[1 + op]
        if f is None:
            continue
        if op == preprocess.HUE:
            hsv = np.array(im.convert("HSV"))
            hsv[..., 0] += np.uint8(preprocess.hue_shift(f))
            im = Image.fromarray(hsv, "HSV").convert("RGB")
        else:
            im = enhancers[op](im).enhance(f)
    return np.asarray(im)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--windows", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "jitter_time.py needs an MI355X"
    dev = torch.device("cuda:0")
    lib = hip.load_library()
    img3, m_a, _, K3 = frames()
    img = np.concatenate([img3, img3[:1, ::-1].copy()])                # the fourth frame: the first one upside down
    msk, K, Dv = np.concatenate([m_a, m_a[:1]]), np.concatenate([K3, K3[:1]]), np.concatenate([D, D[:1]])
    t_img, t_msk, t_K, t_D = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (img, msk, K, Dv))
    lut = torch.from_numpy(preprocess.unit_table()).to(dev)
    jit = torch.empty_like(t_img)
    ws = torch.empty(lib.th_color_jitter_workspace_bytes(V, H0, W0), dtype=torch.uint8, device=dev)
    out = torch.empty((V, 3, H0 // N, W0 // N), dtype=torch.float32, device=dev)
    out_m = torch.empty((V, H0 // N, W0 // N), dtype=torch.uint8, device=dev)
    h, p = hip.ctx(dev), hip._p

    def f_jitter(params):
        order, factors, d = preprocess._jitter_args(params)
        enabled = sum(1 << op for op, f in enumerate(factors + [d]) if f is not None)
        b, c, s = (0.0 if f is None else float(f) for f in factors)
        packed = sum(op << (2 * k) for k, op in enumerate(order))
        return lambda: hip._check(lib.th_color_jitter(h, p(t_img), V, H0, W0, packed, b, c, s, d or 0, enabled, p(jit), p(ws), ws.numel(),
                                                      hip._stream()))

    def f_views(src):
        return lambda: hip._check(lib.th_prep_views(h, p(src), p(t_msk), V, H0, W0, p(t_K), p(t_D), N, 1, 0, p(lut), p(out), p(out_m),
                                                    hip._stream()))

    def both(a, b):
        return lambda: (a(), b())

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

    device_ms = {"jitter_with_contrast": timed(f_jitter(WITH)), "jitter_without_contrast": timed(f_jitter(WITHOUT)),
                 "prepare_views": timed(f_views(t_img)),
                 "jitter_with_contrast+prepare_views": timed(both(f_jitter(WITH), f_views(jit))),
                 "jitter_without_contrast+prepare_views": timed(both(f_jitter(WITHOUT), f_views(jit)))}
    frame_bytes = V * H0 * W0 * 3
    nbytes = {"jitter_with_contrast": 3 * frame_bytes, "jitter_without_contrast": 2 * frame_bytes}
    rate = {k: round(nbytes[k] / (device_ms[k]["median"] * 1e-3) / 1e9, 1) for k in nbytes}
    # what it computes, and what the host takes for the same
    host_ms, equal = {}, {}
    for name, params in (("with_contrast", WITH), ("without_contrast", WITHOUT)):
        got = preprocess.color_jitter(t_img, params).cpu().numpy()
        walls = []
        for _ in range(5):
            t0 = time.perf_counter()
            ref = np.stack([pil_chain(f, params) for f in img])
            walls.append((time.perf_counter() - t0) * 1e3)
        host_ms[name] = round(float(np.median(walls)), 2)
        equal[name] = bool(np.array_equal(got, ref))
    print(json.dumps({"frames": V, "raw": [H0, W0], "out": [H0 // N, W0 // N], "iters_per_window": args.iters, "windows": args.windows,
                      "device": torch.cuda.get_device_name(0), "device_ms_per_call": device_ms, "bytes_per_call": nbytes,
                      "GB_per_s_at_median": rate, "host_pillow_ms_for_the_four_frames_median_of_5": host_ms,
                      "equals_pillow": equal}))
    assert all(equal.values())


if __name__ == "__main__":
    main()
