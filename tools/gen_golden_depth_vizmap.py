"""Write tests/golden/g21_depth_vizmap.npz: the reference's own Renderer.get_relative_depth
(lib/networks/renderer/if_clight_renderer.py:75-93), called as paint_neural_human calls it (:123-133), on a seeded input:
V = 3 cameras, smooth synthetic 64 x 64 depth maps with a zero background region, 2 000 vertices of which some project outside
the image.  Arrays only: the inputs (verts, R, T, K, depthmaps), the reference's projection (depth, uv) and its three outputs
(surface_depth, vis_mask, relative_depth).

    python tools/gen_golden_depth_vizmap.py [--seed 21]

Runs on the CPU, only where the reference checkout exists (oracle/ref_harness.py).  The mask flips where relative_depth crosses
zero, so tests/test_gpu_visibility.py leaves the band |relative_depth| < 1e-4 (the project's parity bar) out of the mask
comparison; this script asserts, on the reference itself, that the band holds fewer than 1 % of the vertices."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_harness  # noqa: E402
from transhuman_amd import visibility  # noqa: E402

V, H, W, NV = 3, 64, 64, 2000
BAND = 1e-4


def make_inputs(seed):
    rs = np.random.RandomState(seed)
    centre = np.array([0.03, 0.10, 3.0])
    R, T, K = visibility.ring_cameras(H, W, angles=(0.0, 2.1, 4.2), centre=centre, dist=3.0, focal=75.0)
    # a cloud around the body's centre, wide enough that some of it leaves the 64 x 64 window (75 px per metre of offset at 3 m)
    verts = (centre + rs.normal(0.0, 1.0, size=(NV, 3)) * np.array([0.55, 0.55, 0.30])).astype(np.float32)
    rows, cols = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    maps = []
    for v in range(V):
        smooth = 3.0 + 0.25 * np.sin(0.11 * cols + 0.7 * v) * np.cos(0.09 * rows - 0.4 * v) + 0.002 * (cols - rows)
        inside = ((cols - 31.0 - 2 * v) / 24.0) ** 2 + ((rows - 33.0 + v) / 29.0) ** 2 < 1.0
        maps.append(np.where(inside, smooth, 0.0))
    depthmaps = np.stack(maps).astype(np.float32)
    return verts, R, T, K, depthmaps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=21)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "g21_depth_vizmap.npz"))
    args = ap.parse_args()
    verts, R, T, K, depthmaps = make_inputs(args.seed)
    mods = ref_harness.load_reference()
    Renderer = mods["if_clight_renderer"].Renderer
    t = torch.from_numpy
    smpl_vertice = t(verts)[None]                                                   # batch['input_smpl_vertice'][t]
    input_R, input_T, input_K = t(R).reshape(-1, 3, 3), t(T).reshape(-1, 3, 1), t(K).reshape(-1, 3, 3)
    # :123-126, the reference's own expressions
    vertice_rot = torch.matmul(input_R[:, None], smpl_vertice.unsqueeze(-1))[..., 0]
    vertice = vertice_rot + input_T[:, None, :3, 0]
    vertice = torch.matmul(input_K[:, None], vertice.unsqueeze(-1))[..., 0]
    uv = vertice[:, :, :2] / vertice[:, :, 2:]
    depth = vertice[:, :, 2:]                                                       # :131
    batch = {"input_depthmaps": [t(depthmaps)[None, ..., None]]}                    # [1, V, H, W, 1] (:82)
    with torch.no_grad():
        surface, vis, rel = Renderer.get_relative_depth(None, depth, uv, batch, det=0.07, t=0)   # :132
    surface, vis, rel = surface[..., 0].numpy(), vis.numpy(), rel[..., 0].numpy()
    assert surface.shape == (V, NV) and vis.shape == (V, NV) and rel.shape == (V, NV)
    outside = ((uv[..., 0] < 0) | (uv[..., 0] > W - 1) | (uv[..., 1] < 0) | (uv[..., 1] > H - 1)).numpy()
    band = np.abs(rel) < BAND
    print(f"vertices outside the image: {outside.sum(1)} of {NV}; on the zero background: {(surface == 0).sum(1)}; "
          f"visible: {vis.sum(1)}; |relative_depth| < {BAND}: {band.sum()} of {band.size}")
    assert outside.sum() > 0 and (~outside).sum() > 0
    assert 0 < vis.sum() < vis.size
    assert band.mean() < 0.01, "more than 1 % of the vertices sit on the mask's threshold: choose another seed"
    np.savez_compressed(args.out, seed=np.int64(args.seed), verts=verts, R=R, T=T, K=K, depthmaps=depthmaps,
                        depth=depth[..., 0].numpy().astype(np.float32), uv=uv.numpy().astype(np.float32),
                        surface_depth=surface.astype(np.float32), vis_mask=vis.astype(bool),
                        relative_depth=rel.astype(np.float32), det=np.float32(0.07))
    print(f"wrote {args.out} ({os.path.getsize(args.out)} bytes)")


if __name__ == "__main__":
    main()
