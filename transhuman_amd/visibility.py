"""Vertex visibility maps and SMPL depth maps, rasterised on the device (csrc/k_raster.hip, K14).

``batch['input_vizmaps']`` ([1, V, 6890]: the SMPL vertices visible from each input camera, applied by paint_neural_human at
if_clight_renderer.py:176-182) and ``batch['input_depthmaps']`` are only LOADED by the reference, from the .npy files of
``rasterize_root/<human>/{visibility,depth}`` (can_smpl.py:439-475); no program of the reference writes them and the archive's
generator is unknown to us.  The rasteriser here is therefore defined by this project:

  projection   float64 on the exactly promoted fp32 inputs, no contraction: cam_i = ((R_i0 x + R_i1 y) + R_i2 z) + T_i,
               p_i = (K_i0 cam_0 + K_i1 cam_1) + K_i2 cam_2, u = p_0 / p_2, v = p_1 / p_2, z = cam_2
  pixel grid   the centre of pixel (col, row) is (u, v) = (col, row)
  snapping     X = rint(256 u), Y = rint(256 v) (round-half-even)
  skipped      triangles with a vertex at z <= 1e-3, or |u| or |v| not below 2^20, or zero snapped area; NO clipping
  coverage     either winding (oriented to positive area by swapping the 2nd and 3rd corner), int64 edge functions at the pixel
               centres (256 col, 256 row), inside where all three are > 0, or = 0 on a top or left edge (y down)
  depth        w_i = e_i / 2A, zf = 1 / ((w_0 / z_0 + w_1 / z_1) + w_2 / z_2) in float64, rounded once to fp32
  z-buffer     uint64 key (fp32 bits of zf) << 32 | face index, minimum wins: nearest, then the lower face index

``rasterize_oracle`` / ``vertex_visibility_oracle`` restate this in float64 / int64 numpy (importable without a GPU); the
device reproduces their ``pix_to_face`` at every pixel and their depth to the last bit of the float64 reciprocal chain.
"""
import numpy as np
import torch

from . import hip

NEAR = 1e-3
UV_MAX = float(1 << 20)


# ---------------------------------------------------------------------------
# device
# ---------------------------------------------------------------------------
def _faces_dev(faces, device):
    if torch.is_tensor(faces):
        f = faces.detach()
    else:
        f = torch.from_numpy(np.ascontiguousarray(np.asarray(faces).astype(np.int64)))
    return f.to(device=device, dtype=torch.int32).reshape(-1, 3).contiguous()


def _cams(R, T, K, device):
    to = lambda x: torch.as_tensor(x).to(device)
    R, T, K = to(R).reshape(-1, 3, 3), to(T).reshape(-1, 3, 1), to(K).reshape(-1, 3, 3)
    return hip.pack_cams(R, T, K)


def rasterize_mesh(verts, faces, R, T, K, H, W, background=0.0):
    """th_rasterize_mesh: verts [nv,3] (device), faces [nf,3] integer, R [V,3,3], T [V,3,1], K [V,3,3]
    -> (depth fp32 [V,H,W], ``background`` where nothing landed; pix_to_face int32 [V,H,W], -1 there).
    Waits once for the stream (the face-index check's answer)."""
    lib = hip.load_library()
    v = hip._f32(verts).reshape(-1, 3)
    dev = v.device
    f = _faces_dev(faces, dev)
    cams = _cams(R, T, K, dev)
    V, nv, nf, H, W = cams.shape[0], v.shape[0], f.shape[0], int(H), int(W)
    nbytes = lib.th_rasterize_workspace_bytes(V, nv, nf, H, W)
    if nbytes == 0:
        raise ValueError(f"rasterize_mesh: unsupported sizes V={V} nv={nv} nf={nf} H={H} W={W}")
    ws = hip._ws(nbytes, dev)
    depth = torch.empty((V, H, W), dtype=torch.float32, device=dev)
    p2f = torch.empty((V, H, W), dtype=torch.int32, device=dev)
    hip._check(lib.th_rasterize_mesh(hip.ctx(dev), hip._p(v), nv, hip._p(f), nf, hip._p(cams), V, H, W, float(background),
                                     hip._p(depth), hip._p(p2f), hip._p(ws), ws.numel(), hip._stream()))
    return depth, p2f


def visibility_from_faces(pix_to_face, faces, nv):
    """th_vertex_visibility: uint8 [V, nv], 1 where the vertex is a corner of a face that owns a pixel of pix_to_face[v]."""
    lib = hip.load_library()
    dev = pix_to_face.device
    p2f = pix_to_face.to(torch.int32).contiguous()
    f = _faces_dev(faces, dev)
    V, H, W = p2f.shape
    vis = torch.empty((V, int(nv)), dtype=torch.uint8, device=dev)
    hip._check(lib.th_vertex_visibility(hip.ctx(dev), hip._p(p2f), hip._p(f), f.shape[0], int(nv), V, H, W, hip._p(vis),
                                        hip._stream()))
    return vis


def vertex_visibility(verts, faces, R, T, K, H, W):
    """bool [V, nv]: the vertices visible from each camera (the reference's batch['input_vizmaps'][t][0])."""
    v = hip._f32(verts).reshape(-1, 3)
    f = _faces_dev(faces, v.device)
    _, p2f = rasterize_mesh(v, f, R, T, K, H, W)
    return visibility_from_faces(p2f, f, v.shape[0]).to(torch.bool)


def depth_visibility(verts, depthmaps, R, T, K, det=0.07):
    """th_depth_visibility (get_relative_depth, if_clight_renderer.py:75-93 as :129-133 calls it): depthmaps [V,H,W] (a
    trailing / leading axis of 1 as in batch['input_depthmaps'][t] is accepted) -> (surface_depth fp32 [V,nv], vis_mask bool
    [V,nv], relative_depth fp32 [V,nv])."""
    lib = hip.load_library()
    v = hip._f32(verts).reshape(-1, 3)
    dev = v.device
    cams = _cams(R, T, K, dev)
    V, nv = cams.shape[0], v.shape[0]
    d = torch.as_tensor(depthmaps).to(dev)
    if d.dim() == 5:                                   # [1, V, H, W, 1]
        d = d[0, ..., 0]
    elif d.dim() == 4:                                 # [V, H, W, 1]
        d = d[..., 0]
    if d.dim() != 3 or d.shape[0] != V:
        raise ValueError(f"depth_visibility: depthmaps of shape {tuple(depthmaps.shape)} do not match {V} cameras")
    d = hip._f32(d)
    H, W = int(d.shape[1]), int(d.shape[2])
    surface = torch.empty((V, nv), dtype=torch.float32, device=dev)
    vis = torch.empty((V, nv), dtype=torch.uint8, device=dev)
    rel = torch.empty((V, nv), dtype=torch.float32, device=dev)
    hip._check(lib.th_depth_visibility(hip.ctx(dev), hip._p(v), nv, hip._p(cams), V, hip._p(d), H, W, float(det),
                                       hip._p(surface), hip._p(vis), hip._p(rel), hip._stream()))
    return surface, vis.to(torch.bool), rel


# ---------------------------------------------------------------------------
# float64 / int64 numpy restatement of the definition
# ---------------------------------------------------------------------------
def _np(x, dtype):
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(x).astype(dtype))


def project_oracle(verts, R, T, K):
    """(X, Y int64 [V,nv] snapped to 1/256 pixel, z float64 [V,nv], ok bool [V,nv]) of the definition's projection."""
    v = _np(verts, np.float32).reshape(-1, 3).astype(np.float64)
    R = _np(R, np.float32).reshape(-1, 3, 3).astype(np.float64)
    T = _np(T, np.float32).reshape(-1, 3).astype(np.float64)
    K = _np(K, np.float32).reshape(-1, 3, 3).astype(np.float64)
    x, y, z = v[None, :, 0], v[None, :, 1], v[None, :, 2]
    cam = [((R[:, i, 0, None] * x + R[:, i, 1, None] * y) + R[:, i, 2, None] * z) + T[:, i, None] for i in range(3)]
    p = [(K[:, i, 0, None] * cam[0] + K[:, i, 1, None] * cam[1]) + K[:, i, 2, None] * cam[2] for i in range(3)]
    with np.errstate(all="ignore"):
        u, w = p[0] / p[2], p[1] / p[2]
        ok = (cam[2] > NEAR) & (np.abs(u) < UV_MAX) & (np.abs(w) < UV_MAX)
        X = np.where(ok, np.rint(np.where(ok, u, 0.0) * 256.0), 0.0).astype(np.int64)
        Y = np.where(ok, np.rint(np.where(ok, w, 0.0) * 256.0), 0.0).astype(np.int64)
    return X, Y, np.where(ok, cam[2], 0.0), ok


def _edge(ax, ay, bx, by, px, py):
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def _top_left(ax, ay, bx, by):
    return ((by == ay) & (bx > ax)) | (by < ay)


def rasterize_oracle(verts, faces, R, T, K, H, W, background=0.0, return_ties=False, chunk_pixels=1 << 21):
    """The definition, on the host: (depth fp32 [V,H,W], pix_to_face int32 [V,H,W]) as numpy arrays; with
    ``return_ties`` also bool [V,H,W], the pixels whose two nearest fragments have equal fp32 depth (where the owner is decided
    by the face index alone)."""
    faces = _np(faces, np.int64).reshape(-1, 3)
    X, Y, Z, ok = project_oracle(verts, R, T, K)
    V, nv = X.shape
    if faces.size and (faces.min() < 0 or faces.max() >= nv):
        raise ValueError("a face index is outside [0, n_verts)")
    H, W = int(H), int(W)
    zbuf = np.full((V, H * W), np.iinfo(np.uint64).max, np.uint64)
    frags = []
    for view in range(V):
        i0, i1, i2 = faces[:, 0], faces[:, 1], faces[:, 2]
        good = ok[view, i0] & ok[view, i1] & ok[view, i2]
        area2 = _edge(X[view, i0], Y[view, i0], X[view, i1], Y[view, i1], X[view, i2], Y[view, i2])
        good &= area2 != 0
        swap = area2 < 0                                     # orient to positive area: swap the 2nd and 3rd corner
        j1, j2 = np.where(swap, i2, i1), np.where(swap, i1, i2)
        area2 = np.abs(area2)
        tx = np.stack([X[view, i0], X[view, j1], X[view, j2]], 1)
        ty = np.stack([Y[view, i0], Y[view, j1], Y[view, j2]], 1)
        tz = np.stack([Z[view, i0], Z[view, j1], Z[view, j2]], 1)
        x0 = np.maximum((tx.min(1) + 255) >> 8, 0)
        x1 = np.minimum(tx.max(1) >> 8, W - 1)
        y0 = np.maximum((ty.min(1) + 255) >> 8, 0)
        y1 = np.minimum(ty.max(1) >> 8, H - 1)
        good &= (x0 <= x1) & (y0 <= y1)
        ids = np.nonzero(good)[0]
        bw, bh = (x1 - x0 + 1)[ids], (y1 - y0 + 1)[ids]
        npix = bw * bh
        start = 0
        while start < len(ids):
            # a run of triangles whose boxes hold at most chunk_pixels pixels (one at least)
            csum = np.cumsum(npix[start:])
            stop = start + max(1, int(np.searchsorted(csum, chunk_pixels, side="right")))
            sel, n_sel, w_sel = ids[start:stop], npix[start:stop], bw[start:stop]
            tri = np.repeat(np.arange(len(sel)), n_sel)
            local = np.arange(int(n_sel.sum())) - np.repeat(np.cumsum(n_sel) - n_sel, n_sel)
            col = x0[sel][tri] + local % w_sel[tri]
            row = y0[sel][tri] + local // w_sel[tri]
            px, py = col * 256, row * 256
            ax, ay = tx[sel][tri], ty[sel][tri]
            e = [_edge(ax[:, 1], ay[:, 1], ax[:, 2], ay[:, 2], px, py),
                 _edge(ax[:, 2], ay[:, 2], ax[:, 0], ay[:, 0], px, py),
                 _edge(ax[:, 0], ay[:, 0], ax[:, 1], ay[:, 1], px, py)]
            tl = [_top_left(ax[:, 1], ay[:, 1], ax[:, 2], ay[:, 2]), _top_left(ax[:, 2], ay[:, 2], ax[:, 0], ay[:, 0]),
                  _top_left(ax[:, 0], ay[:, 0], ax[:, 1], ay[:, 1])]
            inside = np.ones(len(tri), bool)
            for k in range(3):
                inside &= (e[k] > 0) | ((e[k] == 0) & tl[k])
            tri, col, row = tri[inside], col[inside], row[inside]
            area = area2[sel][tri].astype(np.float64)
            zz = tz[sel][tri]
            w = [e[k][inside].astype(np.float64) / area for k in range(3)]
            zf = 1.0 / ((w[0] / zz[:, 0] + w[1] / zz[:, 1]) + w[2] / zz[:, 2])
            bits = zf.astype(np.float32).view(np.uint32).astype(np.uint64)
            key = (bits << np.uint64(32)) | sel[tri].astype(np.uint64)
            pix = row * W + col
            np.minimum.at(zbuf[view], pix, key)
            if return_ties:
                frags.append((view, pix, key))
            start = stop
    hit = zbuf != np.iinfo(np.uint64).max
    depth = np.where(hit, (zbuf >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(background))
    p2f = np.where(hit, (zbuf & np.uint64(0xffffffff)).astype(np.int64), -1).astype(np.int32)
    out = (depth.astype(np.float32).reshape(V, H, W), p2f.reshape(V, H, W))
    if return_ties:
        ties = np.zeros((V, H * W), bool)
        for view, pix, key in frags:
            same_depth = (key >> np.uint64(32)) == (zbuf[view, pix] >> np.uint64(32))
            other_face = key != zbuf[view, pix]
            ties[view, pix[same_depth & other_face]] = True
        out += (ties.reshape(V, H, W),)
    return out


def vertex_visibility_from_faces_oracle(pix_to_face, faces, nv):
    faces = _np(faces, np.int64).reshape(-1, 3)
    p2f = np.asarray(pix_to_face)
    vis = np.zeros((p2f.shape[0], int(nv)), bool)
    for view in range(p2f.shape[0]):
        owners = np.unique(p2f[view][p2f[view] >= 0])
        vis[view, faces[owners].reshape(-1)] = True
    return vis


def vertex_visibility_oracle(verts, faces, R, T, K, H, W):
    """bool [V, nv] (numpy): vertex n is visible in view v iff it is a corner of a face that owns a pixel of view v."""
    _, p2f = rasterize_oracle(verts, faces, R, T, K, H, W)
    nv = _np(verts, np.float32).reshape(-1, 3).shape[0]
    return vertex_visibility_from_faces_oracle(p2f, faces, nv)


# ---------------------------------------------------------------------------
# test bodies (tests/test_visibility_host.py, tests/test_gpu_visibility.py, tools/raster_time.py)
# ---------------------------------------------------------------------------
def uv_ellipsoid(n_lat=82, n_lon=84, radii=(0.25, 0.85, 0.18), centre=(0.03, 0.10, 3.0)):
    """UV ellipsoid with the pole along y: n_lat latitude rings x n_lon longitudes + the two poles, faces oriented outward.
    82 x 84 gives 6 890 vertices and 13 776 faces, SMPL's counts.  -> (verts fp32 [nv,3], faces int32 [nf,3])"""
    th = np.pi * (np.arange(n_lat) + 1) / (n_lat + 1)
    ph = 2 * np.pi * np.arange(n_lon) / n_lon
    ring = np.stack([np.sin(th)[:, None] * np.cos(ph)[None], np.broadcast_to(np.cos(th)[:, None], (n_lat, n_lon)),
                     np.sin(th)[:, None] * np.sin(ph)[None]], -1).reshape(-1, 3)
    unit = np.concatenate([[[0.0, 1.0, 0.0]], ring, [[0.0, -1.0, 0.0]]])
    verts = unit * np.asarray(radii) + np.asarray(centre)
    idx = lambda i, j: 1 + i * n_lon + (j % n_lon)
    south = 1 + n_lat * n_lon
    faces = []
    for j in range(n_lon):
        faces.append((0, idx(0, j), idx(0, j + 1)))
        faces.append((south, idx(n_lat - 1, j + 1), idx(n_lat - 1, j)))
    for i in range(n_lat - 1):
        for j in range(n_lon):
            a, b, c, d = idx(i, j), idx(i, j + 1), idx(i + 1, j), idx(i + 1, j + 1)
            faces.append((a, c, d))
            faces.append((a, d, b))
    faces = np.asarray(faces, np.int64)
    # outward: the normal points away from the centre
    v = verts - np.asarray(centre)
    n = np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]])
    flip = (n * v[faces].mean(1)).sum(1) < 0
    faces[flip] = faces[flip][:, [0, 2, 1]]
    return verts.astype(np.float32), faces.astype(np.int32)


def ring_cameras(H=512, W=512, angles=(0.0, 2.1, 4.2), centre=(0.03, 0.10, 3.0), dist=3.0, focal=600.0):
    """Cameras on a ring of radius ``dist`` around ``centre`` looking at it (x_cam = R x + T), K = [[f,0,W/2],[0,f,H/2],[0,0,1]].
    -> (R [V,3,3], T [V,3,1], K [V,3,3]) fp32"""
    c = np.asarray(centre, np.float64)
    Rs, Ts, Ks = [], [], []
    for a in angles:
        ca, sa = np.cos(a), np.sin(a)
        R = np.array([[ca, 0, sa], [0, 1, 0], [-sa, 0, ca]])
        Rs.append(R)
        Ts.append((-R @ c + np.array([0, 0, dist])).reshape(3, 1))
        Ks.append(np.array([[focal, 0, W / 2.0], [0, focal, H / 2.0], [0, 0, 1]]))
    return np.stack(Rs).astype(np.float32), np.stack(Ts).astype(np.float32), np.stack(Ks).astype(np.float32)
