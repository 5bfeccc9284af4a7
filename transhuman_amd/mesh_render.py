"""Normal-coloured, Phong-lit frames of an extracted mesh, on the device (csrc/k_meshshade.hip, K15, on top of K14's rasteriser).

The reference's reconstruction workflow extracts one mesh per frame (scripts/mesh.sh), renders each with
``render_mesh_dynamic.py`` along the ``gen_path_virt`` orbit and strings the frames into a video.  The script renders with
pytorch3d (:182-276: ``MeshRasterizer(image_size=512, blur_radius=0, faces_per_pixel=1)``, ``SoftPhongShader`` with
``PointLights(location=(0, 3, 0))``, default ``Materials``, white background, ``verts_rgb = 0.7 n + 0.7`` with n the vertex
normals of the mesh in the camera frame with y and z flipped).  pytorch3d is third-party and absent, so no frame of the
reference's own exists to compare with -- the situation visibility.py describes for the vizmap archive.  The image is
therefore DEFINED BY THIS PROJECT, after those settings; parity with pytorch3d itself is unpinned:

  arithmetic      float64 on the exactly promoted fp32 inputs, no contraction, in the order written; every output (normals, image)
                  rounded once to fp32.  float64 vertices (a ``Mesh``'s) are rounded to fp32 once, first.
  vertex normals  pytorch3d's area-weighted rule: every corner of face (i0, i1, i2) receives c = (v1 - v0) x (v2 - v0) -- as the
                  int64 q = rint(c 2^40), so that the per-vertex sum is exact and independent of the order of the faces;
                  n = s / max(|s|, 1e-6), (0, 0, 0) without faces or with cancelling ones; ``flip`` negates.  Faces the rasteriser
                  skips count: normals belong to the mesh, not to a view.  In range while every |c_k| 2^40 <= 2^62 / nf (no sum
                  can then leave int64; metre-scale bodies are five orders of magnitude inside); a mesh outside raises.
  pixel grid      ``pixel_centre`` is the (u, v) of the centre of pixel (0, 0): 0.0 (this project's grid, OpenCV's, the vizmaps')
                  or 0.5 (pytorch3d's, the grid the reference's frames are on); subtracted in fp32 from K[0,2] and K[1,2].
  fragments       depth / pix_to_face of visibility.rasterize_mesh; at a covered pixel w_i = e_i / 2A from the same snapped int64
                  edge functions, b_i = (w_i / z_i) / ((w_0 / z_0 + w_1 / z_1) + w_2 / z_2); sums over corners ((b_0 x_0 + b_1 x_1) + b_2 x_2)
  shading         p = sum b_i v_i, nh = unit(sum b_i n_i), texel t = sum b_i (0.7 (F R n_i) + 0.7), F = diag(1, -1, -1);
                  lh = unit(L - p), vh = unit(C - p), C = -R^T T, unit(x) = x / max(|x|, 1e-6); d = nh . lh;
                  colour = (a + k_d max(d, 0)) t + k_s [d > 0] max(vh . (2 d nh - lh), 0)^m, m a power of two taken by squaring
                  (a, k_d, k_s, m = 0.5, 0.3, 0.2, 64: ambient 0.5 x 1, diffuse 0.3 x 1, specular 0.2 x 1, shininess 64; with one
                  face per pixel and no blur the soft blend is the nearest face's colour to below fp32 resolution).  L, a, k_d,
                  k_s and the background are taken as fp32.  Unclamped; uncovered pixels are ``background`` exactly.

``vertex_normals_oracle`` / ``render_mesh_oracle`` restate this in float64 / int64 numpy (importable without a GPU); the device
is held to them: normals and covered pixels within 1 fp32 ulp, uncovered pixels exactly (tests/test_gpu_mesh_render.py).

Meshes from ``hip.marching_cubes`` over a sigma grid (dense inside) have outward face normals under this rule, like PyMCubes'
that the reference's script renders unflipped: ``MARCHING_CUBES_FLIP`` is False, and that is what ``flip=None`` means in
``render_mesh_sequence`` (pinned end to end by tests/test_gpu_mesh_render.py on an analytic ball).
"""
import os

import numpy as np
import torch

from . import hip
from . import visibility as vz
from .camera_path import gen_path_virt

SHIFT = 40                                   # fixed-point fraction bits of the normal sums
SCALE = float(1 << SHIFT)
SUM_MAX = float(1 << 62)
EPS = 1e-6
LIGHT = (0.0, 3.0, 0.0)                      # render_mesh_dynamic.py:245
BACKGROUND = (1.0, 1.0, 1.0)                 # :240
AMBIENT, DIFFUSE, SPECULAR, SHININESS = 0.5, 0.3, 0.2, 64      # pytorch3d's default PointLights x Materials
MARCHING_CUBES_FLIP = False


def _check_pixel_centre(pixel_centre):
    if float(pixel_centre) not in (0.0, 0.5):
        raise ValueError(f"pixel_centre is {pixel_centre}: 0.0 (OpenCV's grid, the default) or 0.5 (pytorch3d's)")
    return np.float32(pixel_centre)


def _squarings(shininess):
    m = int(shininess)
    if m != shininess or m < 1 or m & (m - 1):
        raise ValueError(f"shininess is {shininess}: a power of two (the power is taken by squaring)")
    return m.bit_length() - 1


# ---------------------------------------------------------------------------
# device
# ---------------------------------------------------------------------------
def _verts_dev(verts, device=None):
    v = verts if torch.is_tensor(verts) else torch.from_numpy(np.ascontiguousarray(np.asarray(verts)))
    if not v.is_cuda:
        v = v.to(device if device is not None else torch.device("cuda", torch.cuda.current_device()))
    return hip._f32(v).reshape(-1, 3)


def _normals_launch(v, f, flip):
    """th_vertex_normals without the wait: (normals fp32 [nv,3], status int32 [1]) on the device"""
    lib = hip.load_library()
    dev = v.device
    nv, nf = v.shape[0], f.shape[0]
    nbytes = lib.th_vertex_normals_workspace_bytes(nv, nf)
    if nbytes == 0:
        raise ValueError(f"vertex_normals: unsupported sizes nv={nv} nf={nf}")
    ws = hip._ws(nbytes, dev)
    normals = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    hip._check(lib.th_vertex_normals(hip.ctx(dev), hip._p(v), nv, hip._p(f), nf, int(bool(flip)), hip._p(normals),
                                     hip._p(status), hip._p(ws), ws.numel(), hip._stream()))
    return normals, status


def _raise_status(status):
    code = int(status.item())
    if code & 1:
        raise ValueError("a face index is outside [0, n_verts)")
    if code & 2:
        raise ValueError(f"the mesh is outside the range of the exact normal sums: a face has |(v1 - v0) x (v2 - v0)| 2^{SHIFT} "
                         "above 2^62 / n_faces, or is not finite")


def vertex_normals(verts, faces, flip=False):
    """th_vertex_normals: verts [nv,3] (fp32 or a Mesh's float64; device tensor or ndarray), faces [nf,3] integer
    -> area-weighted unit vertex normals fp32 [nv,3] on the device.  Waits once for the stream (the status word): a face index
    outside the mesh or a mesh outside the range raises ValueError."""
    v = _verts_dev(verts)
    normals, status = _normals_launch(v, vz._faces_dev(faces, v.device), flip)
    _raise_status(status)
    return normals


def shade_mesh(verts, normals, faces, R, T, K, pix_to_face, light=LIGHT, background=BACKGROUND, ambient=AMBIENT,
               diffuse=DIFFUSE, specular=SPECULAR, shininess=SHININESS):
    """th_shade_mesh: image fp32 [V,H,W,3] from pix_to_face int32 [V,H,W] of rasterize_mesh for the same mesh and cameras.
    No host wait."""
    import ctypes as C
    lib = hip.load_library()
    _squarings(shininess)
    v = _verts_dev(verts)
    dev = v.device
    n = hip._f32(normals).reshape(-1, 3)
    f = vz._faces_dev(faces, dev)
    cams = vz._cams(R, T, K, dev)
    p2f = pix_to_face.to(torch.int32).contiguous()
    V, H, W = p2f.shape
    if cams.shape[0] != V or n.shape[0] != v.shape[0]:
        raise ValueError(f"shade_mesh: {cams.shape[0]} cameras / {V} images, {n.shape[0]} normals / {v.shape[0]} vertices")
    image = torch.empty((V, H, W, 3), dtype=torch.float32, device=dev)
    L = (C.c_float * 3)(*[float(x) for x in light])
    B = (C.c_float * 3)(*[float(x) for x in background])
    hip._check(lib.th_shade_mesh(hip.ctx(dev), hip._p(v), hip._p(n), v.shape[0], hip._p(f), f.shape[0], hip._p(cams), V, H, W,
                                 hip._p(p2f), L, B, float(ambient), float(diffuse), float(specular), int(shininess),
                                 hip._p(image), hip._stream()))
    return image


def _shift_K(K, pixel_centre, device):
    """K fp32 [V,3,3] with the principal point moved by -pixel_centre, in fp32"""
    pc = _check_pixel_centre(pixel_centre)
    K = torch.as_tensor(K).to(device=device, dtype=torch.float32).reshape(-1, 3, 3).clone()
    K[:, 0, 2] -= float(pc)
    K[:, 1, 2] -= float(pc)
    return K


def render_mesh(verts, faces, R, T, K, H, W, pixel_centre=0.0, light=LIGHT, background=BACKGROUND, flip=False,
                ambient=AMBIENT, diffuse=DIFFUSE, specular=SPECULAR, shininess=SHININESS):
    """verts [nv,3], faces [nf,3], R [V,3,3], T [V,3,1], K [V,3,3] -> (image fp32 [V,H,W,3] unclamped, ``background`` where nothing
    landed; depth fp32 [V,H,W], 0 there; pix_to_face int32 [V,H,W], -1 there), all on the device.
    ``evaluator.to_uint8(image)`` is the 8-bit frame."""
    _squarings(shininess)
    v = _verts_dev(verts)
    f = vz._faces_dev(faces, v.device)
    K = _shift_K(K, pixel_centre, v.device)
    normals = vertex_normals(v, f, flip=flip)
    depth, p2f = vz.rasterize_mesh(v, f, R, T, K, H, W)
    image = shade_mesh(v, normals, f, R, T, K, p2f, light=light, background=background, ambient=ambient, diffuse=diffuse,
                       specular=specular, shininess=shininess)
    return image, depth, p2f


def _load_mesh(m):
    if isinstance(m, (str, os.PathLike)):
        from .mesh import read_ply
        return read_ply(os.fspath(m))
    if hasattr(m, "vertices") and hasattr(m, "faces"):
        return m.vertices, m.faces
    v, f = m
    return v, f


def render_mesh_sequence(meshes, RT, K, H, W, out_dir=None, flip=None, first_frame=0, render=None, **kw):
    """The frames of render_mesh_dynamic.py:319-353, a generator.  meshes: a sequence of ``Mesh`` objects, (verts, faces) pairs
    or paths of PLY files (``Mesh.export``'s); RT: the rig's world-to-camera 4x4 matrices; K: ONE [3,3] intrinsic matrix (the
    script uses the first camera's).  With n = len(meshes), frame i = first_frame + k shows meshes[k] from
    ``gen_path_virt(RT, render_views=n)[i % n]`` (:319, :335) on pytorch3d's pixel grid (pixel_centre 0.5) and yields its image
    fp32 [H,W,3]; with ``out_dir`` it is also written to ``<out_dir>/<i>.png`` (evaluator.to_uint8 + PIL, like the evaluator's
    crops).  flip=None: what meshes from hip.marching_cubes need (MARCHING_CUBES_FLIP = False).  ``render`` (default render_mesh)
    is called as render(verts, faces, R [1,3,3], T [1,3,1], K [1,3,3], H, W, pixel_centre=0.5, flip=flip, **kw)."""
    meshes = list(meshes)
    n = len(meshes)
    if n == 0:
        return
    render = render_mesh if render is None else render
    flip = MARCHING_CUBES_FLIP if flip is None else flip
    w2c = gen_path_virt(RT, render_views=n)
    K1 = np.asarray(K, np.float32).reshape(1, 3, 3)
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
    for k, m in enumerate(meshes):
        i = int(first_frame) + k
        cam = np.asarray(w2c[i % n], np.float64)
        R = cam[:3, :3].astype(np.float32).reshape(1, 3, 3)
        T = cam[:3, 3:].astype(np.float32).reshape(1, 3, 1)
        v, f = _load_mesh(m)
        image = render(v, f, R, T, K1, H, W, pixel_centre=0.5, flip=flip, **kw)[0][0]
        if out_dir is not None:
            from PIL import Image
            from .evaluator import to_uint8
            Image.fromarray(to_uint8(vz._np(image, np.float32))).save(os.path.join(out_dir, f"{i}.png"))
        yield image


# ---------------------------------------------------------------------------
# float64 / int64 numpy restatement of the definition
# ---------------------------------------------------------------------------
def _f64(x, shape=None):
    a = vz._np(x, np.float32).astype(np.float64)
    return a if shape is None else a.reshape(shape)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _unit(x):
    return x / np.maximum(np.sqrt(_dot(x, x)), EPS)[..., None]


def normal_sums_oracle(verts, faces):
    """int64 [nv,3]: the exact sums of q = rint(c 2^40) over each vertex's faces.  Raises ValueError on a face index outside
    the mesh or a mesh outside the range."""
    v = _f64(verts, (-1, 3))
    f = vz._np(faces, np.int64).reshape(-1, 3)
    if f.size and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError("a face index is outside [0, n_verts)")
    e1, e2 = v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
    with np.errstate(all="ignore"):
        c = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
        t = c * SCALE
        if not (np.abs(t) <= SUM_MAX / float(max(len(f), 1))).all():
            raise ValueError(f"the mesh is outside the range of the exact normal sums: a face has |(v1 - v0) x (v2 - v0)| "
                             f"2^{SHIFT} above 2^62 / n_faces, or is not finite")
    q = np.rint(t).astype(np.int64)
    sums = np.zeros((len(v), 3), np.int64)
    for k in range(3):
        np.add.at(sums, f[:, k], q)
    return sums


def vertex_normals_oracle(verts, faces, flip=False):
    """The definition's vertex normals on the host: fp32 [nv,3] (numpy)."""
    s = normal_sums_oracle(verts, faces).astype(np.float64) / SCALE
    n = _unit(s)
    if flip:
        n = 0.0 - n
    return n.astype(np.float32)


def render_mesh_oracle(verts, faces, R, T, K, H, W, pixel_centre=0.0, light=LIGHT, background=BACKGROUND, flip=False,
                       ambient=AMBIENT, diffuse=DIFFUSE, specular=SPECULAR, shininess=SHININESS, return_terms=False):
    """The definition on the host: (image fp32 [V,H,W,3], depth fp32 [V,H,W], pix_to_face int32 [V,H,W]) as numpy arrays; with
    ``return_terms`` also a dict of float64 [V,H,W] maps "d" (nh . lh), "diffuse" (k_d max(d, 0)) and "specular" (the whole
    specular term), NaN where nothing landed."""
    pc = _check_pixel_centre(pixel_centre)
    nsq = _squarings(shininess)
    v32 = vz._np(verts, np.float32).reshape(-1, 3)
    f = vz._np(faces, np.int64).reshape(-1, 3)
    K32 = vz._np(K, np.float32).reshape(-1, 3, 3).copy()
    K32[:, 0, 2] -= pc
    K32[:, 1, 2] -= pc
    n32 = vertex_normals_oracle(v32, f, flip=flip)
    H, W = int(H), int(W)
    depth, p2f = vz.rasterize_oracle(v32, f, R, T, K32, H, W)
    X, Y, Z, _ = vz.project_oracle(v32, R, T, K32)
    v, nrm = v32.astype(np.float64), n32.astype(np.float64)
    Rm, Tm = _f64(R, (-1, 3, 3)), _f64(T, (-1, 3))
    L, a, kd, ks = _f64(light, (3,)), float(np.float32(ambient)), float(np.float32(diffuse)), float(np.float32(specular))
    V = p2f.shape[0]
    image = np.empty((V, H, W, 3), np.float32)
    image[...] = vz._np(background, np.float32).reshape(3)
    terms = {k: np.full((V, H, W), np.nan) for k in ("d", "diffuse", "specular")}
    for view in range(V):
        row, col = np.nonzero(p2f[view] >= 0)
        if not len(row):
            continue
        idx = f[p2f[view, row, col]]                                       # [n,3]
        tx, ty, tz = X[view][idx], Y[view][idx], Z[view][idx]
        area2 = vz._edge(tx[:, 0], ty[:, 0], tx[:, 1], ty[:, 1], tx[:, 2], ty[:, 2])
        swap = area2 < 0                                                   # orient to positive area: swap the 2nd and 3rd corner
        order = np.where(swap[:, None], np.array([0, 2, 1]), np.array([0, 1, 2]))
        take = lambda x: np.take_along_axis(x, order, 1)
        idx, tx, ty, tz = take(idx), take(tx), take(ty), take(tz)
        area = np.abs(area2).astype(np.float64)
        px, py = col.astype(np.int64) * 256, row.astype(np.int64) * 256
        e = [vz._edge(tx[:, 1], ty[:, 1], tx[:, 2], ty[:, 2], px, py), vz._edge(tx[:, 2], ty[:, 2], tx[:, 0], ty[:, 0], px, py),
             vz._edge(tx[:, 0], ty[:, 0], tx[:, 1], ty[:, 1], px, py)]
        wz = [(e[k].astype(np.float64) / area) / tz[:, k] for k in range(3)]
        den = (wz[0] + wz[1]) + wz[2]
        b = [wz[k] / den for k in range(3)]
        mix = lambda x: (b[0][:, None] * x[0] + b[1][:, None] * x[1]) + b[2][:, None] * x[2]
        Rv = Rm[view]
        tex = []
        for k in range(3):
            nk = nrm[idx[:, k]]
            m = [(Rv[a_, 0] * nk[:, 0] + Rv[a_, 1] * nk[:, 1]) + Rv[a_, 2] * nk[:, 2] for a_ in range(3)]
            tex.append(np.stack([0.7 * m[0] + 0.7, 0.7 * (0.0 - m[1]) + 0.7, 0.7 * (0.0 - m[2]) + 0.7], 1))
        p = mix([v[idx[:, k]] for k in range(3)])
        nh = _unit(mix([nrm[idx[:, k]] for k in range(3)]))
        t = mix(tex)
        eye = np.array([0.0 - ((Rv[0, a_] * Tm[view, 0] + Rv[1, a_] * Tm[view, 1]) + Rv[2, a_] * Tm[view, 2]) for a_ in range(3)])
        lh, vh = _unit(L[None] - p), _unit(eye[None] - p)
        d = _dot(nh, lh)
        r = (2.0 * d)[:, None] * nh - lh
        s = np.maximum(_dot(vh, r), 0.0)
        for _ in range(nsq):
            s = s * s
        shade = a + kd * np.maximum(d, 0.0)
        spec = ks * np.where(d > 0.0, s, 0.0)
        image[view, row, col] = (shade[:, None] * t + spec[:, None]).astype(np.float32)
        terms["d"][view, row, col] = d
        terms["diffuse"][view, row, col] = kd * np.maximum(d, 0.0)
        terms["specular"][view, row, col] = spec
    out = (image, depth, p2f)
    return out + (terms,) if return_terms else out
