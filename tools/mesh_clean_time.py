"""Time the two steps behind marching cubes: K24 (components + component filter, csrc/k_meshcc.hip) and the point query with
colours (th_eval_points, transhuman_amd/mesh_color.py).

  case 1  components + filter("largest") of a 256^3 marching-cubes ball of radius 90 voxels with a few hundred satellite balls
          of radius 2.5 voxels on a 32-voxel lattice around it: sweeps, host reads of the sweep flags, what was removed
  case 2  eval_points + colours at the SMPL-sized body (6 890 points) and at the ball's vertex count, with the sigma-only
          eval_sigma_grid on the same points beside it, from the same process (synthetic 64 x 64 x 3 frame, N_c = 300)

    timeout -k 10 300 python tools/mesh_clean_time.py [--iters N] [--scipy]

Prints one JSON line.  Device time: HIP events on the stream around each call (the calls' own host waits -- the sweep flags, the
counts, the range guard -- are inside the bracket), median and minimum of N calls after 5 warm-up calls.  --scipy adds
scipy.sparse.csgraph.connected_components on the host for context (not a reference, not a threshold).  Nothing here has a target."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from transhuman_amd import hip, mesh_clean, mesh_color, synth  # noqa: E402


def ball_with_satellites(dev, n=256, radius=90.0, sat_radius=2.5, pitch=32):
    g = torch.arange(n, device=dev, dtype=torch.float32)
    c = g - (n - 1) / 2.0
    r = torch.sqrt(c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2)
    d = torch.remainder(g, pitch) - pitch / 2.0                               # offset from the lattice point of the cell
    rs = torch.sqrt(d[:, None, None] ** 2 + d[None, :, None] ** 2 + d[None, None, :] ** 2)
    cc = torch.floor(g / pitch) * pitch + pitch / 2.0 - (n - 1) / 2.0         # the lattice point itself, from the cube's centre
    far = torch.sqrt(cc[:, None, None] ** 2 + cc[None, :, None] ** 2 + cc[None, None, :] ** 2) > radius + 4 * sat_radius
    field = torch.maximum(radius - r, torch.where(far, sat_radius - rs, torch.full_like(rs, -1e3)))
    sigma = torch.clamp(field + 0.5, min=0.0)                                 # level 0.5 at the surfaces
    return hip.marching_cubes(sigma, 0.5, scale=(0.005,) * 3, origin=(-0.64, -0.64, 2.36))


def timed(fn, iters, warm=5):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"median": round(float(np.median(ms)), 4), "min": round(float(np.min(ms)), 4)}


def case_components(dev, iters, with_scipy):
    v, f = ball_with_satellites(dev)
    nv, nf = v.shape[0], f.shape[0]
    labels, info = mesh_clean.components(f, nv)
    v2, f2, finfo = mesh_clean.filter_components(v, f, "largest")
    row = {"case": "ball 256^3 + satellites", "verts": nv, "faces": nf, "components": info["n_components"],
           "sweeps": info["sweeps"], "flag_reads": info["flag_reads"], "kept_faces": finfo["kept_faces"],
           "removed_faces": finfo["removed_faces"], "iters": iters,
           "device_ms": {"components": timed(lambda: mesh_clean.components(f, nv), iters),
                         "components+filter": timed(lambda: mesh_clean.filter_components(v, f, "largest"), iters)}}
    if with_scipy:
        try:
            import scipy.sparse as sp
            from scipy.sparse.csgraph import connected_components
            fh = f.cpu().numpy().astype(np.int64)
            t0 = time.perf_counter()
            e = np.concatenate([fh[:, [0, 1]], fh[:, [1, 2]]])
            n, _ = connected_components(sp.coo_matrix((np.ones(len(e), np.int8), (e[:, 0], e[:, 1])), shape=(nv, nv)), directed=False)
            row["scipy_host_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
            row["scipy_components"] = int(n)
        except ImportError:
            row["scipy_host_ms"] = None
    return row, nv


def case_points(dev, iters, n_ball):
    from transhuman_amd.config import get_cfg
    from transhuman_amd.networks.cross_transformer import Network
    from transhuman_amd.networks.renderer import if_mesh_renderer
    cfg = get_cfg()
    cfg.N_samples, cfg.num_class = 32, 300
    torch.manual_seed(0)
    net = Network()
    net.load_state_dict(synth.det_state_dict(net.state_dict(), seed=0, sigma_bias=-1.7))
    net.train()
    bc = synth.make_batch(64, 64, 3, seed=0)
    body = bc["tar_smpl_vertice_smplcoord"][0].numpy()
    gold = os.path.join(ROOT, "tests", "golden", "synth_assign.npz")
    assign = np.load(gold)["assign_300"].astype(np.int64) if os.path.exists(gold) else synth.kmeans_assign(body, 300)
    r = if_mesh_renderer.Renderer(net.to(dev), vertex_can=body.astype(np.float64) * 1.02 + 0.001, pc2voxel_ind=assign)
    b = synth.batch_to(bc, dev)
    frame = r.prepare_frame(b)
    verts = b["tar_smpl_vertice"][0].to(torch.float32)
    gen = torch.Generator().manual_seed(1)
    rows = []
    for name, n in (("body", verts.shape[0]), ("ball's vertex count", n_ball)):
        reps = (n + verts.shape[0] - 1) // verts.shape[0]
        pts = (verts.repeat(reps, 1)[:n] + (0.02 * (torch.rand((n, 3), generator=gen) - 0.5)).to(dev)).contiguous()
        d = torch.randn((n, 3), generator=gen).to(dev)
        raw, st = hip.eval_points(net, frame, pts, d)
        col, grey = mesh_color.colors_from_raw(raw)

        def f_points():
            mesh_color.colors_from_raw(hip.eval_points(net, frame, pts, d)[0])

        rows.append({"case": name, "points": n, "inside_hull": int(st["valid_samples"]), "without_rgb": grey, "iters": iters,
                     "device_ms": {"eval_points+colours": timed(f_points, iters),
                                   "eval_points": timed(lambda: hip.eval_points(net, frame, pts, d), iters),
                                   "eval_sigma_grid": timed(lambda: hip.eval_sigma_grid(net, frame, pts), iters)}})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--scipy", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    hip.load_library()
    row, n_ball = case_components(dev, args.iters, args.scipy)
    rows = [row] + case_points(dev, args.iters, n_ball)
    print(json.dumps({"device": torch.cuda.get_device_name(0), "cases": rows}))


if __name__ == "__main__":
    main()
