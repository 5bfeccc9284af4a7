"""Time th_rasterize_mesh + th_vertex_visibility (csrc/k_raster.hip) for V = 3 views of 512 x 512 on the 6 890-vertex /
13 776-face test ellipsoid (transhuman_amd.visibility.uv_ellipsoid: SMPL's counts, ~6 px^2 per projected triangle), and on the
worst case of the cooperative path: two triangles that fill every pixel of the three images, in front of that body.

    timeout -k 10 120 python tools/raster_time.py [--iters N]

Prints one JSON line.  Per case: device time per call -- HIP events around EACH call of the two C entry points with a
preallocated workspace (th_rasterize_mesh ends in a host wait for its face-index check, so calls cannot be queued back to
back; the events bracket the memset, the four kernels of the rasteriser and the memset + kernel of the visibility pass), median
and minimum over N calls after 20 warm-up calls -- and the host wall time per visibility.vertex_visibility() call (allocations,
launches, the wait)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from transhuman_amd import hip, visibility  # noqa: E402

H = W = 512


def measure(name, verts, faces, R, T, K, iters, dev):
    lib = hip.load_library()
    tv = torch.from_numpy(verts).to(dev)
    tf = torch.from_numpy(faces.astype(np.int32)).to(dev)
    cams = hip.pack_cams(*(torch.from_numpy(x).to(dev) for x in (R, T, K)))
    V, nv, nf = cams.shape[0], tv.shape[0], tf.shape[0]
    ws = torch.empty(int(lib.th_rasterize_workspace_bytes(V, nv, nf, H, W)), dtype=torch.uint8, device=dev)
    depth = torch.empty((V, H, W), dtype=torch.float32, device=dev)
    p2f = torch.empty((V, H, W), dtype=torch.int32, device=dev)
    vis = torch.empty((V, nv), dtype=torch.uint8, device=dev)
    h = hip.ctx(dev)

    def call():
        hip._check(lib.th_rasterize_mesh(h, hip._p(tv), nv, hip._p(tf), nf, hip._p(cams), V, H, W, 0.0, hip._p(depth),
                                         hip._p(p2f), hip._p(ws), ws.numel(), hip._stream()))
        hip._check(lib.th_vertex_visibility(h, hip._p(p2f), hip._p(tf), nf, nv, V, H, W, hip._p(vis), hip._stream()))

    for _ in range(20):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    walls = []
    for _ in range(50):
        t0 = time.perf_counter()
        out = visibility.vertex_visibility(tv, tf, R, T, K, H, W)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    assert torch.equal(out, vis.to(torch.bool))
    return {"case": name, "views": V, "verts": nv, "faces": nf, "covered_pixels": [int((p2f[v] >= 0).sum()) for v in range(V)],
            "visible_vertices": [int(x) for x in vis.sum(1)], "iters": iters,
            "device_ms_per_call_median": round(float(np.median(ms)), 4), "device_ms_per_call_min": round(float(np.min(ms)), 4),
            "wall_ms_per_vertex_visibility_median": round(float(np.median(walls)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=500)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    bv, bf = visibility.uv_ellipsoid()
    R, T, K = visibility.ring_cameras(H, W)
    rows = [measure("body", bv, bf, R, T, K, args.iters, dev)]
    # a quad 2 m in front of every camera, 3 m wide: 600 px / m * 1.5 m / 2 m = 450 px to each side of the centre
    nb = len(bv)
    quads_v, quads_f = [], []
    for v in range(R.shape[0]):
        Rm, Tm = R[v].astype(np.float64), T[v].astype(np.float64).reshape(3)
        cam_pts = np.array([[-1.5, -1.5, 2.0], [1.5, -1.5, 2.0], [1.5, 1.5, 2.0], [-1.5, 1.5, 2.0]])
        quads_v.append(((cam_pts - Tm) @ Rm).astype(np.float32))                  # x_world = R^T (x_cam - T)
        o = nb + 4 * v
        quads_f += [[o, o + 1, o + 2], [o, o + 2, o + 3]]
    rows.append(measure("body behind three image-filling quads", np.concatenate([bv] + quads_v),
                        np.concatenate([bf, np.asarray(quads_f, np.int32)]), R, T, K, args.iters, dev))
    assert all(c == H * W for c in rows[1]["covered_pixels"])
    print(json.dumps({"image": [H, W], "device": torch.cuda.get_device_name(0), "cases": rows}))


if __name__ == "__main__":
    main()
