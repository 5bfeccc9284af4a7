"""Triangle mesh container + binary PLY writer + the evaluator's PSNR -- the consumers of the mesh / eval workloads
(SURVEY 8f-4).

The reference hands `mcubes.marching_cubes`' output to `trimesh.Trimesh(vertices_world, triangles)`
(lib/networks/renderer/if_mesh_renderer.py:109) and the visualiser calls `mesh.export('<frame>.ply')`
(lib/visualizers/if_nerf_mesh.py:25-35); neither package is installed here.  ``Mesh`` keeps the two attributes the
reference's code touches (``vertices`` float64 [nv,3], ``faces`` int64 [nt,3]) and ``export`` writes the same file
layout trimesh's PLY exporter produces (binary little-endian, float x/y/z per vertex, uchar-counted int32 index
lists per face), so downstream tools read either.  Ours on top: optional ``vertex_colors`` (uint8 [nv,3], written as
``uchar red, green, blue, alpha`` behind x y z -- this project's layout, unpinned against trimesh) and ``largest_component`` /
``filter_components`` (mesh_clean.py, K24).  ``psnr_metric`` is lib/evaluators/if_nerf.py:34-37 on device
tensors (one reduction kernel, no host copy of the image).
"""
import numpy as np
import torch


class Mesh:
    def __init__(self, vertices, faces, vertex_colors=None):
        self.vertices = vertices        # [nv,3] float64 (device tensor or ndarray)
        self.faces = faces              # [nt,3] integer
        self.vertex_colors = vertex_colors      # None, or [nv,3] uint8 (device tensor or ndarray): mesh_color.vertex_colors

    def _host(self):
        v = self.vertices.detach().cpu().numpy() if torch.is_tensor(self.vertices) else np.asarray(self.vertices)
        f = self.faces.detach().cpu().numpy() if torch.is_tensor(self.faces) else np.asarray(self.faces)
        return np.asarray(v, dtype=np.float64).reshape(-1, 3), np.asarray(f).reshape(-1, 3)

    @property
    def is_watertight(self):
        """every undirected edge is shared by exactly two triangles"""
        _, f = self._host()
        if f.shape[0] == 0:
            return False
        e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]).astype(np.int64)
        e.sort(axis=1)
        _, counts = np.unique(e, axis=0, return_counts=True)
        return bool((counts == 2).all())

    def _host_colors(self):
        if self.vertex_colors is None:
            return None
        c = self.vertex_colors
        c = c.detach().cpu().numpy() if torch.is_tensor(c) else np.asarray(c)
        return np.asarray(c, dtype=np.uint8).reshape(-1, 3)

    def export(self, path):
        """binary little-endian PLY (trimesh's layout: float32 positions, `list uchar int` faces).  With ``vertex_colors`` every
        vertex record is x y z followed by `uchar red, green, blue, alpha` (alpha 255) -- this project's definition of the
        coloured file; without colours the file is what it always was, byte for byte."""
        v, f = self._host()
        col = self._host_colors()
        if col is not None and col.shape[0] != v.shape[0]:
            raise ValueError(f"vertex_colors has {col.shape[0]} rows for {v.shape[0]} vertices")
        cprops = "" if col is None else "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\n"
        header = ("ply\nformat binary_little_endian 1.0\ncomment transhuman_amd marching cubes\n"
                  f"element vertex {v.shape[0]}\nproperty float x\nproperty float y\nproperty float z\n{cprops}"
                  f"element face {f.shape[0]}\nproperty list uchar int vertex_indices\nend_header\n")
        face_rec = np.empty(f.shape[0], dtype=[("n", "u1"), ("idx", "<i4", (3,))])
        face_rec["n"] = 3
        face_rec["idx"] = f.astype("<i4")
        if col is None:
            vert_bytes = v.astype("<f4").tobytes()
        else:
            vert_rec = np.empty(v.shape[0], dtype=[("xyz", "<f4", (3,)), ("rgba", "u1", (4,))])
            vert_rec["xyz"] = v.astype("<f4")
            vert_rec["rgba"][:, :3] = col
            vert_rec["rgba"][:, 3] = 255
            vert_bytes = vert_rec.tobytes()
        with open(path, "wb") as fh:
            fh.write(header.encode("ascii"))
            fh.write(vert_bytes)
            fh.write(face_rec.tobytes())
        return path

    def filter_components(self, keep="largest"):
        """A new Mesh of the kept components (mesh_clean.filter_components, K24): "largest" or an int, the least number of
        faces of a kept component.  Order-preserving; colours follow their vertices; faces keep their dtype."""
        from . import mesh_clean
        v, f, info = mesh_clean.filter_components(self.vertices, self.faces, keep=keep, colors=self.vertex_colors)
        if torch.is_tensor(self.faces):
            f = f.to(self.faces.dtype)
        out = Mesh(v, f, info.get("colors"))
        out.filter_info = info
        return out

    def largest_component(self):
        return self.filter_components("largest")


def read_ply(path, colors=False):
    """reader for the files Mesh.export writes (tests / tools) -> (vertices float32 [nv,3], faces int32 [nt,3]); the colour
    bytes of a coloured file are skipped.  ``colors=True`` -> (vertices, faces, colours uint8 [nv,3] or None without them)."""
    with open(path, "rb") as fh:
        nv = nt = 0
        uchars = 0
        while True:
            line = fh.readline().decode("ascii").strip()
            if line.startswith("element vertex"):
                nv = int(line.split()[-1])
            elif line.startswith("element face"):
                nt = int(line.split()[-1])
            elif line.startswith("property uchar"):
                uchars += 1
            elif line == "end_header":
                break
        assert uchars in (0, 4), "vertex records: x y z, optionally red green blue alpha"
        if uchars:
            vrec = np.frombuffer(fh.read(16 * nv), dtype=[("xyz", "<f4", (3,)), ("rgba", "u1", (4,))])
            v, col = np.ascontiguousarray(vrec["xyz"]), np.ascontiguousarray(vrec["rgba"][:, :3])
        else:
            v, col = np.frombuffer(fh.read(12 * nv), dtype="<f4").reshape(nv, 3), None
        rec = np.frombuffer(fh.read(13 * nt), dtype=[("n", "u1"), ("idx", "<i4", (3,))])
    assert (rec["n"] == 3).all()
    return (v, rec["idx"], col) if colors else (v, rec["idx"])


def psnr_metric(img_pred, img_gt):
    """lib/evaluators/if_nerf.py:34-37: -10 log10(mean((pred - gt)^2)) -- tensors (any device) or ndarrays"""
    if torch.is_tensor(img_pred):
        d = img_pred.to(torch.float64) - torch.as_tensor(img_gt, device=img_pred.device).to(torch.float64)
        mse = float((d * d).mean())
    else:
        mse = float(np.mean((np.asarray(img_pred, np.float64) - np.asarray(img_gt, np.float64)) ** 2))
    return -10.0 * np.log(mse) / np.log(10.0)
