"""Time one normal-coloured Phong frame of a mesh (csrc/k_meshshade.hip on top of csrc/k_raster.hip): th_vertex_normals +
th_rasterize_mesh + th_shade_mesh for ONE view of 512 x 512 on pytorch3d's pixel grid, of

  ball    a synthetic ball of radius 100 voxels extracted by hip.marching_cubes from a 256^3 sigma grid (voxel 5 mm: the size of
          mesh the reconstruction workflow renders -- a few hundred thousand vertices and faces)
  body    the 6 890-vertex / 13 776-face test ellipsoid (transhuman_amd.visibility.uv_ellipsoid: SMPL's counts)

    timeout -k 10 300 python tools/mesh_shade_time.py [--iters N]

Prints one JSON line.  Per case: device time -- HIP events around each of the three C entry points with preallocated buffers
(th_rasterize_mesh ends in a host wait for its face-index check, so frames cannot be queued back to back; the events bracket the
memsets and kernels of each call), and around the three together; median and minimum over N frames after 20 warm-up frames -- and
the host wall time per mesh_render.render_mesh() call (allocations, launches, the two waits).  There is no predecessor to compare
with and no threshold on the figures."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from transhuman_amd import hip, mesh_render, visibility  # noqa: E402

H = W = 512


def ball_mesh(dev, n=256, radius=100.0, voxel=0.005, centre=(0.03, 0.10, 3.0)):
    g = torch.arange(n, device=dev, dtype=torch.float32) - (n - 1) / 2.0
    r = torch.sqrt(g[:, None, None] ** 2 + g[None, :, None] ** 2 + g[None, None, :] ** 2)
    sigma = torch.clamp(radius + 0.5 - r, min=0.0)                      # level 0.5 at r = radius
    origin = tuple(float(c) - (n - 1) / 2.0 * voxel for c in centre)
    verts, faces = hip.marching_cubes(sigma, 0.5, scale=(voxel,) * 3, origin=origin)
    return verts.to(torch.float32), faces


def measure(name, tv, tf, R, T, K, iters, dev):
    lib = hip.load_library()
    tK = mesh_render._shift_K(K, 0.5, dev)
    cams = hip.pack_cams(torch.from_numpy(R).to(dev), torch.from_numpy(T).to(dev), tK)
    V, nv, nf = cams.shape[0], tv.shape[0], tf.shape[0]
    ws_n = torch.empty(int(lib.th_vertex_normals_workspace_bytes(nv, nf)), dtype=torch.uint8, device=dev)
    ws_r = torch.empty(int(lib.th_rasterize_workspace_bytes(V, nv, nf, H, W)), dtype=torch.uint8, device=dev)
    normals = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    depth = torch.empty((V, H, W), dtype=torch.float32, device=dev)
    p2f = torch.empty((V, H, W), dtype=torch.int32, device=dev)
    image = torch.empty((V, H, W, 3), dtype=torch.float32, device=dev)
    light, bg = (C.c_float * 3)(*mesh_render.LIGHT), (C.c_float * 3)(*mesh_render.BACKGROUND)
    h, p = hip.ctx(dev), hip._p

    def f_normals():
        hip._check(lib.th_vertex_normals(h, p(tv), nv, p(tf), nf, 0, p(normals), p(status), p(ws_n), ws_n.numel(), hip._stream()))

    def f_raster():
        hip._check(lib.th_rasterize_mesh(h, p(tv), nv, p(tf), nf, p(cams), V, H, W, 0.0, p(depth), p(p2f), p(ws_r), ws_r.numel(),
                                         hip._stream()))

    def f_shade():
        hip._check(lib.th_shade_mesh(h, p(tv), p(normals), nv, p(tf), nf, p(cams), V, H, W, p(p2f), light, bg, mesh_render.AMBIENT,
                                     mesh_render.DIFFUSE, mesh_render.SPECULAR, mesh_render.SHININESS, p(image), hip._stream()))

    def frame():
        f_normals(), f_raster(), f_shade()

    def timed(fn):
        ms = []
        for _ in range(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return {"median": round(float(np.median(ms)), 4), "min": round(float(np.min(ms)), 4)}

    for _ in range(20):
        frame()
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    row = {"case": name, "verts": nv, "faces": nf, "iters": iters, "device_ms": {
        "frame": timed(frame), "vertex_normals": timed(f_normals), "rasterize": timed(f_raster), "shade": timed(f_shade)}}
    walls = []
    for _ in range(30):
        t0 = time.perf_counter()
        out = mesh_render.render_mesh(tv, tf, R, T, K, H, W, pixel_centre=0.5)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    assert torch.equal(out[0], image) and torch.equal(out[2], p2f)
    row["covered_pixels"] = int((p2f >= 0).sum())
    row["wall_ms_per_render_mesh_median"] = round(float(np.median(walls)), 4)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    R, T, K = visibility.ring_cameras(H, W, angles=(0.0,))
    bv, bf = ball_mesh(dev)
    rows = [measure("ball 256^3", bv, bf, R, T, K, args.iters, dev)]
    ev, ef = visibility.uv_ellipsoid()
    rows.append(measure("body", torch.from_numpy(ev).to(dev), torch.from_numpy(ef).to(dev), R, T, K, args.iters, dev))
    print(json.dumps({"image": [H, W], "views": 1, "device": torch.cuda.get_device_name(0), "cases": rows}))


if __name__ == "__main__":
    main()
