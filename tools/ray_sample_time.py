"""Time the dataset's other targets made on the device (csrc/k_raysample.hip, K26): sample_ray_h36m's train split (512 x 512 target
view, nrays = 1024) and its test split (the full 512 x 512 S-real frame of synth.make_batch), each followed by get_acc.

    timeout -k 10 300 python tools/ray_sample_time.py [--iters N] [--rounds M]

Prints one JSON line.  Per split, in M alternating rounds (every round measures each figure once, one after the other; reported:
the median with the lowest and the highest):
  device_ms        HIP events around N back-to-back runs of the split's entry point + th_ray_acc with preallocated buffers, on
                   dense rays that are already there (none of them waits on the host), per run
  host_read_ms     wall time of the one ``info.cpu()`` on an idle stream
  library_call_ms  wall time of train_targets.sample_rays_h36m (dense rays, bound mask, allocation, launches, the read, slicing)
  numpy_ms         the numpy restatement on the same machine from the same dense rays (sample_rays_h36m_oracle)
  gen_rays_compact_ms (test split) wall time of hip.gen_rays(compact=True) on the same camera: the boolean indexing this split's
                   compaction replaces, which waits on the host once per array
Also, once, equality of the device result with the restatement.  There is no predecessor to compare with and no threshold on the
figures."""
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
NRAYS, BODY, FACE = 1024, 0.5, 0.0


def ellipse(H, W):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    r = np.sqrt(((y - 0.5 * H) / (0.33 * H)) ** 2 + ((x - 0.45 * W) / (0.22 * W)) ** 2)
    msk = np.zeros((H, W), np.uint8)
    msk[r <= 1.15] = 100
    msk[r <= 1.0] = 1
    return msk


def train_view():
    """the view of tools/patch_rays_time.py"""
    K = np.array([[600.0, 0, 256.0], [0, 600.0, 256.0], [0, 0, 1]], np.float32)
    bounds = np.array([[-0.35, -0.9, 2.6], [0.4, 0.85, 3.3]], np.float32)
    return K, np.eye(3, dtype=np.float32), np.zeros((3, 1), np.float32), bounds


def test_view():
    """the target camera and the body box of the S-real frame"""
    b = synth.make_batch(H, W, 3, seed=0)
    cams = synth.make_cameras(H, W, 3, center=tuple(b["Th"][0, 0].tolist()))
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return f(cams["K"]), f(cams["R"]), f(cams["T"]), f(b["can_bounds"][0].numpy())


def stats(ms):
    return {"median": round(float(np.median(ms)), 5), "lowest": round(float(np.min(ms)), 5), "highest": round(float(np.max(ms)), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ray_sample_time.py needs an MI355X"
    dev = torch.device("cuda:0")
    lib = hip.load_library()
    h, p = hip.ctx(dev), hip._p
    rs = np.random.RandomState(0)
    img, msk, draws = rs.uniform(size=(H, W, 3)).astype(np.float32), ellipse(H, W), rs.uniform(size=(train_targets.MAX_ITERS, 3, NRAYS))
    t_img, t_msk, t_draws = (torch.from_numpy(a).to(dev) for a in (img, msk, draws))
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
    ws = e(int(lib.th_ray_sample_workspace_bytes(H, W, NRAYS)), torch.uint8)
    info = e(4, torch.int32)
    fig = {"train": {k: [] for k in ("device_ms", "host_read_ms", "library_call_ms", "numpy_ms")},
           "test": {k: [] for k in ("device_ms", "host_read_ms", "library_call_ms", "numpy_ms", "gen_rays_compact_ms")}}
    side, rays = {}, {}
    for split, cam in (("train", train_view()), ("test", test_view())):
        K, R, T, bounds = cam
        dense = hip.gen_rays(K, R, T, bounds, H, W, device=dev, compact=False)
        bound = hip.bound_2d_mask(bounds, K, np.concatenate([R, T], axis=1), H, W, device=dev)
        rm = dense["mask_at_box"].view(torch.uint8)
        rows = NRAYS + train_targets.MAX_ITERS if split == "train" else H * W
        outs = [e((rows, 3), torch.float32), e((rows, 3), torch.float32), e((rows, 3), torch.float32), e(rows, torch.float32),
                e(rows, torch.float32)]
        coord = e((rows, 2), torch.int64) if split == "train" else torch.zeros((1, 2), dtype=torch.int64, device=dev)
        acc = e(rows, torch.uint8)
        common = (h, p(dense["ray_o"]), p(dense["ray_d"]), p(dense["near"]), p(dense["far"]), p(rm))

        def run(split=split, common=common, bound=bound, outs=outs, coord=coord, acc=acc):
            if split == "train":
                hip._check(lib.th_ray_sample_train(*common, p(t_msk), p(bound), p(t_img), 3, 1, H, W, p(t_draws), NRAYS, BODY, FACE,
                                                   *(p(o) for o in outs), p(coord), p(info), p(ws), ws.numel(), hip._stream()))
                n_acc = NRAYS                                                # (a finished loop has written at least nrays rows)
            else:
                hip._check(lib.th_ray_sample_test(*common, p(t_img), 3, 1, H, W, *(p(o) for o in outs), p(info), p(ws), ws.numel(),
                                                  hip._stream()))
                n_acc = 1                                                    # (coord is all zeros: one window)
            hip._check(lib.th_ray_acc(h, p(coord), n_acc, p(t_msk), H, W, p(acc), hip._stream()))
        kw = dict(nrays=NRAYS, draws=t_draws, body_ratio=BODY, face_ratio=FACE) if split == "train" else {}
        side[split] = (cam, run, kw, {k: v.cpu().numpy() for k, v in dense.items()}, bound.cpu().numpy())
    for rnd in range(args.rounds + 1):                                       # (round 0: warm-up)
        for split, (cam, run, kw, dense_h, bound_h) in side.items():
            cur = {}
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            run()
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.iters):
                run()
            e1.record()
            torch.cuda.synchronize()
            cur["device_ms"] = e0.elapsed_time(e1) / args.iters
            t0 = time.perf_counter()
            info.cpu()
            cur["host_read_ms"] = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            got = train_targets.sample_rays_h36m(t_img, t_msk, *cam, split, **kw)
            torch.cuda.synchronize()
            cur["library_call_ms"] = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            want = train_targets.sample_rays_h36m_oracle(img, msk, bound_h, dense_h, split, **{**kw, **({"draws": draws} if kw else {})})
            cur["numpy_ms"] = (time.perf_counter() - t0) * 1e3
            if split == "test":
                t0 = time.perf_counter()
                hip.gen_rays(*cam, H, W, device=dev, compact=True)
                torch.cuda.synchronize()
                cur["gen_rays_compact_ms"] = (time.perf_counter() - t0) * 1e3
            rays[split] = int(want["rgb"].shape[0])
            assert all(np.asarray(want[k]).tobytes() == got[k].cpu().numpy().tobytes() for k in got), split
            if rnd:
                for k, v in cur.items():
                    fig[split][k].append(v)
    print(json.dumps({"view": [H, W], "nrays": NRAYS, "rays": rays, "iters_per_round": args.iters, "rounds": args.rounds,
                      "device": torch.cuda.get_device_name(0),
                      **{split: {k: stats(v) for k, v in f.items()} for split, f in fig.items()},
                      "device_equals_numpy_restatement": True}))


if __name__ == "__main__":
    main()
