"""Time the training targets of a step made on the device (csrc/k_rays.hip + csrc/k_patch.hip, K9 + K18): the dense rays and the 2-D
bound mask of a 512 x 512 target view, then N = 6 patches of 20 x 20 -- what the train split of the reference's sample_ray_patch
does per step in numpy.

    timeout -k 10 300 python tools/patch_rays_time.py [--iters N] [--windows M]

Prints one JSON line.  Device time: HIP events around N back-to-back runs of the three entry points with preallocated buffers
(none of them waits on the host), per run; median / minimum / maximum over M windows after a warm-up window -- for the whole stage
and for th_patch_rays alone.  The host read: wall time of ``counts.cpu()`` on an idle stream.  The library call
(train_targets.sample_patch_rays, allocation, launches, the read and the slicing included): wall time per call.  Beside them the
numpy restatement on the same machine for the same input (sample_patch_rays_oracle, which starts from the dense rays) and numpy's
dense rays and box test (synth.pixel_rays + synth.box_interval, the operations of get_rays / get_near_far): together what a
DataLoader worker spends today, short of cv2.fillPoly.  Also, once, equality of the device result with the restatement.  There is no
predecessor to compare with and no threshold on the figures."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from transhuman_amd import hip, synth, train_targets  # noqa: E402

H = W = 512
N, P, RATIO = 6, 20, 0.8


def view(seed=0):
    rs = np.random.RandomState(seed)
    K = np.array([[600.0, 0, 256.0], [0, 600.0, 256.0], [0, 0, 1]], np.float32)
    bounds = np.array([[-0.35, -0.9, 2.6], [0.4, 0.85, 3.3]], np.float32)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    r = np.sqrt(((y - 0.5 * H) / (0.33 * H)) ** 2 + ((x - 0.45 * W) / (0.22 * W)) ** 2)
    msk = np.zeros((H, W), np.uint8)
    msk[r <= 1.15] = 100
    msk[r <= 1.0] = 1
    return (rs.uniform(size=(H, W, 3)).astype(np.float32), msk, K, np.eye(3, dtype=np.float32), np.zeros((3, 1), np.float32), bounds,
            rs.uniform(size=(N, 2)))


def stats(ms):
    return {"median": round(float(np.median(ms)), 5), "min": round(float(np.min(ms)), 5), "max": round(float(np.max(ms)), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--windows", type=int, default=9)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "patch_rays_time.py needs an MI355X"
    dev = torch.device("cuda:0")
    lib = hip.load_library()
    img, msk, K, R, T, bounds, draws = view()
    t_img, t_msk, t_draws = (torch.from_numpy(a).to(dev) for a in (img, msk, draws))
    h, p, C = hip.ctx(dev), hip._p, hip.C
    k_, r_, t_, b_ = (np.ascontiguousarray(a, np.float32).reshape(-1) for a in (K, R, T, bounds))
    corners = np.ascontiguousarray(hip.bound_corners_2d(bounds, K, np.concatenate([R, T], axis=1)), dtype=np.int32)
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
    n = H * W
    ray_o, ray_d, near, far, rm, bm = e((n, 3), torch.float32), e((n, 3), torch.float32), e(n, torch.float32), e(n, torch.float32), \
        e(n, torch.uint8), e((H, W), torch.uint8)
    rows = N * P * P
    outs = [e((N, P, P), torch.uint8), e((N, P, P), torch.uint8), e((N, P, P, 3), torch.float32), e((N, 2), torch.int32),
            e((2, N), torch.int32), e((rows, 3), torch.float32), e((rows, 3), torch.float32), e((rows, 3), torch.float32),
            e(rows, torch.float32), e(rows, torch.float32), e(rows, torch.uint8), e(rows, torch.int64)]
    ws = e(int(lib.th_patch_workspace_bytes(H, W)), torch.uint8)

    def f_rays():
        hip._check(lib.th_gen_rays(h, k_.ctypes.data_as(hip.c_float_p), r_.ctypes.data_as(hip.c_float_p), t_.ctypes.data_as(hip.c_float_p),
                                   b_.ctypes.data_as(hip.c_float_p), H, W, p(ray_o), p(ray_d), p(near), p(far), p(rm), hip._stream()))
        hip._check(lib.th_bound_mask(h, corners.ctypes.data_as(C.POINTER(C.c_int32)), H, W, p(bm), hip._stream()))

    def f_patch():
        hip._check(lib.th_patch_rays(h, p(ray_o), p(ray_d), p(near), p(far), p(rm), p(t_msk), p(bm), p(t_img), 3, 1, H, W, p(t_draws),
                                     RATIO, N, P, *(p(o) for o in outs), p(ws), ws.numel(), hip._stream()))

    def stage():
        f_rays(), f_patch()

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
        return stats(ms)

    device_ms = {"stage": timed(stage), "patch_rays": timed(f_patch), "rays_and_bound_mask": timed(f_rays)}
    reads, walls = [], []
    for _ in range(50):
        stage()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs[4].cpu()
        reads.append((time.perf_counter() - t0) * 1e3)
    for _ in range(30):
        t0 = time.perf_counter()
        got = train_targets.sample_patch_rays(t_img, t_msk, K, R, T, bounds, draws=t_draws, patch_size=P, subject_ratio=RATIO)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    # the numpy side: the restatement from the device's dense rays, and numpy's own dense rays
    dense = {k: v.cpu().numpy() for k, v in dict(ray_o=ray_o, ray_d=ray_d, near=near, far=far, mask_at_box=rm).items()}
    bm_h = bm.cpu().numpy()
    host, host_rays = [], []
    for _ in range(10):
        t0 = time.perf_counter()
        want = train_targets.sample_patch_rays_oracle(img, msk, bm_h, dense, draws, patch_size=P, subject_ratio=RATIO)
        host.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        o, d = synth.pixel_rays(H, W, K, R, T)
        synth.box_interval(bounds.astype(np.float64), o.reshape(-1, 3).astype(np.float64), d.reshape(-1, 3).astype(np.float64))
        host_rays.append((time.perf_counter() - t0) * 1e3)
    equal = all(np.asarray(want[k]).tobytes() == got[k].cpu().numpy().tobytes() for k in want)
    print(json.dumps({"view": [H, W], "patches": N, "patch_size": P, "rays": int(want["patch_div_indices"][-1]),
                      "iters_per_window": args.iters, "windows": args.windows, "device": torch.cuda.get_device_name(0),
                      "device_ms_per_call": device_ms, "host_read_ms": stats(reads), "wall_ms_per_library_call": stats(walls),
                      "numpy_restatement_ms": stats(host), "numpy_dense_rays_ms": stats(host_rays),
                      "device_equals_numpy_restatement": equal}))
    assert equal


if __name__ == "__main__":
    main()
