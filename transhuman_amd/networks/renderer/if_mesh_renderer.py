"""Mesh-reconstruction renderer: density cube over a voxel grid, then the iso-surface.

Drop-in for /root/reference/lib/networks/renderer/if_mesh_renderer.py
(`Renderer.render`, :46-113).  The hull mask, DPaRF, pixel gather and the
sigma branch of the MLP run through th_eval_sigma_grid; the reference also
evaluates (and discards) RGB for sigma>0 voxels (:84-99) -- `cube` only needs
sigma_raw, which is what is produced here.  Marching cubes (:103, PyMCubes in the reference) runs on the device too
(th_marching_cubes_*, K13): the padded cube never leaves HBM before the mesh exists; `mesh` is a
transhuman_amd.mesh.Mesh (vertices / faces / export(path) like the trimesh object the visualiser uses,
lib/visualizers/if_nerf_mesh.py:25-35).  Two options of ours act on that mesh, both off by default: cfg.mesh_components
("all" | "largest" | n: drop the floaters, mesh_clean.py) and cfg.mesh_colors ("none" | "normal": the field's RGB at the vertices,
mesh_color.py).
"""
import os
import sys

# Drop-in loading: the reference instantiates this file through imp.load_source(cfg.<x>_module, cfg.<x>_path)
# (lib/networks/make_network.py:4-11, renderer/make_renderer.py:4-8) under WHATEVER module name the YAML gives --
# 'lib.networks.cross_transformer' if only the path key is changed.  Relative imports would then resolve inside the
# reference's `lib` package, so the package is imported absolutely, found through this file's own location.
_REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
if _REPO not in sys.path:
    sys.path.insert(0, _REPO)

import numpy as np                                                  # noqa: E402

from transhuman_amd.config import get_cfg, cfg_get                  # noqa: E402
from transhuman_amd import hip                                      # noqa: E402
from transhuman_amd.truncation import sigma_in_force               # noqa: E402
from transhuman_amd.dparf_params import params_in_force            # noqa: E402
from transhuman_amd.networks.renderer.if_clight_renderer import Renderer as Base_Renderer   # noqa: E402


class Renderer(Base_Renderer):
    def render(self, batch, frame=None, pts_slice=None):
        cfg = get_cfg()
        pts = batch["pts"]                                           # [1,X,Y,Z,3]
        sh = pts.shape
        frame = frame if frame is not None else self.prepare_frame(batch)
        flat = pts.reshape(-1, 3)
        if pts_slice is not None:
            flat = flat[pts_slice]
        hip.set_truncation(sigma_in_force(cfg), flat.device)         # cfg.use_truncation / cfg.KNN_SIGMA in force (K27)
        hip.set_dparf(*params_in_force(self.net, cfg), flat.device)  # cfg.KNN / KNN_FREQ / KNN_DIST_ALPHA in force (K4)
        sigma, stats = hip.eval_sigma_grid(self.net, frame, flat)
        self.last_stats = stats
        if pts_slice is not None:
            return {"sigma": sigma}
        import torch
        from transhuman_amd.mesh import Mesh
        cube_d = torch.nn.functional.pad(sigma.view(*sh[1:4]), (10, 10, 10, 10, 10, 10))     # :99-101 (np.pad 10, zeros)
        voxel = np.array(cfg.voxel_size, dtype=np.float64)
        can_bounds = batch["can_bounds"][0].cpu().numpy().astype(np.float64)
        LB = can_bounds[0] - 10 * voxel                                                        # :107
        verts, tris = hip.marching_cubes(cube_d, cfg.mesh_th, scale=voxel, origin=LB)         # :103-108
        mesh = Mesh(verts, tris.to(torch.int64))
        # ours, off by default (cfg_get: the reference's cfg has neither key): drop the floaters, then colour the vertices.  `cube`
        # is never touched.
        comps, colors = cfg_get("mesh_components", "all"), cfg_get("mesh_colors", "none")
        if comps != "all":
            mesh = mesh.filter_components(comps)
        if colors != "none":
            if colors != "normal":
                raise ValueError(f"cfg.mesh_colors is {colors!r}: 'none' or 'normal'")
            from transhuman_amd import mesh_color
            mesh.vertex_colors = mesh_color.vertex_colors(self, batch, mesh, view="normal", frame=frame)
        # the reference hands the cube back as a numpy array (:99-109): copy it through a pinned staging buffer (a
        # pageable 276^3 fp32 copy takes 10+ ms of a 55 ms frame)
        key = (tuple(cube_d.shape), str(cube_d.device))
        pin = getattr(self, "_cube_pin", None)
        if pin is None or pin[0] != key:
            pin = self._cube_pin = (key, torch.empty(cube_d.shape, dtype=torch.float32, pin_memory=True))
        pin[1].copy_(cube_d.detach(), non_blocking=True)
        torch.cuda.current_stream(cube_d.device).synchronize()
        cube = pin[1].numpy().copy()
        return {"cube": cube, "mesh": mesh}
