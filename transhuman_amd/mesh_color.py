"""Vertex colours of an extracted mesh: the radiance field's RGB queried at the vertices (th_eval_points).

The reference evaluates the network's RGB at every sigma > 0 voxel of the grid and throws it away (if_mesh_renderer.py:61,
:84-99); its meshes are grey.  Here the field is asked at the mesh's own vertices -- they lie on the sigma = cfg.mesh_th > 0
surface, hence inside the hull and in the RGB branch -- with a viewing direction per vertex:

  view="normal"          d = -n, n the area-weighted vertex normal of mesh_render.vertex_normals in the orientation
                         render_mesh_sequence uses for marching-cubes meshes (outward): every vertex is looked at head-on from
                         outside.  A vertex without a normal (no face, or cancelling ones) is looked at along (0, 0, -1).
  view=camera_centre[3]  d = normalize(v - c)

  colour = clip(floor(255 sigmoid(rgb) + 0.5), 0, 255) as uint8, computed with torch (not hot).  A vertex whose row came back
  without RGB -- outside the hull, or sigma <= 0 -- has rgb = 0 and gets 128 (sigmoid(0) = 0.5); such vertices are counted.

K15's frames stay normal-shaded: there is no colour mode of shade_mesh / render_mesh.
"""
import numpy as np
import torch

from . import hip
from . import mesh_render
from .truncation import sigma_in_force
from .dparf_params import params_in_force


def colors_from_raw(raw, as_float=False):
    """raw [P,4] (rgb logits, sigma_raw) as th_eval_points returns it -> (colours uint8 [P,3], or fp32 sigmoid(rgb) with
    ``as_float``; the number of rows without RGB: sigma <= 0, which includes every row outside the hull).  Pure torch."""
    raw = torch.as_tensor(raw)
    c = torch.sigmoid(raw[:, :3].to(torch.float32))
    n_default = int((raw[:, 3] <= 0).sum())
    if as_float:
        return c, n_default
    return torch.clamp(torch.floor(255.0 * c + 0.5), 0.0, 255.0).to(torch.uint8), n_default


def view_directions(verts, faces, view="normal"):
    """the viewing direction per vertex, fp32 [nv,3] on the device (unit length)"""
    v = mesh_render._verts_dev(verts)
    if isinstance(view, str):
        if view != "normal":
            raise ValueError(f"view is {view!r}: 'normal' or a camera centre [3]")
        n = mesh_render.vertex_normals(v, faces, flip=mesh_render.MARCHING_CUBES_FLIP)
        d = 0.0 - n
        none = (n == 0).all(dim=1)
        if bool(none.any()):
            d[none] = torch.tensor([0.0, 0.0, -1.0], device=d.device)
        return d
    c = torch.as_tensor(np.asarray(view, dtype=np.float32).reshape(1, 3), device=v.device)
    d = v - c
    return d / torch.clamp(d.norm(dim=1, keepdim=True), min=1e-12)


def vertex_colors(renderer, batch, mesh_or_verts, faces=None, view="normal", frame=None, as_float=False, return_info=False):
    """-> uint8 [nv,3] on the device (fp32 sigmoid(rgb) with ``as_float``).  ``mesh_or_verts``: a Mesh, or vertices [nv,3] with
    ``faces``.  ``frame``: the renderer's prepared frame of ``batch`` (made here when None).  ``return_info=True`` ->
    (colours, dict(no_rgb=vertices that came back without RGB and are 128 grey, valid_samples=vertices inside the hull))."""
    if faces is None and hasattr(mesh_or_verts, "vertices"):
        verts, faces = mesh_or_verts.vertices, mesh_or_verts.faces
    else:
        verts = mesh_or_verts
    if isinstance(view, str) and (view != "normal" or faces is None):
        raise ValueError(f"view is {view!r}: 'normal' (needs the faces) or a camera centre [3]")
    v = mesh_render._verts_dev(verts)
    frame = frame if frame is not None else renderer.prepare_frame(batch)
    if v.shape[0] == 0:
        out = torch.empty((0, 3), dtype=torch.float32 if as_float else torch.uint8, device=v.device)
        return (out, dict(no_rgb=0, valid_samples=0)) if return_info else out
    d = view_directions(v, faces, view)
    hip.set_truncation(sigma_in_force(), v.device)                   # cfg.use_truncation / cfg.KNN_SIGMA in force (K27)
    hip.set_dparf(*params_in_force(renderer.net), v.device)          # cfg.KNN / KNN_FREQ / KNN_DIST_ALPHA in force (K4)
    raw, stats = hip.eval_points(renderer.net, frame, v, d)
    col, n_default = colors_from_raw(raw, as_float=as_float)
    return (col, dict(no_rgb=n_default, valid_samples=int(stats["valid_samples"]))) if return_info else col
