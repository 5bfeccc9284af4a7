"""CPU ORACLE for the TransHuman rendering hot path -- TEST INFRASTRUCTURE ONLY.

This file is a from-scratch CPU (torch fp32 / numpy) restatement of the
reference's algorithm for the path named by BASELINE.json:north_star.  It is
the checker for the HIP kernels and the timed "cpu_baseline" in bench.py.
Nothing under ``transhuman_amd/`` (the product) may import it: only
``tests/``, ``__graft_entry__.smoke()`` and ``bench.py``'s cpu_baseline leg do.

Parity pinning: every function below is checked in tests/test_oracle_golden.py
against golden vectors produced by importing the *real* reference modules in
the survey container (oracle/gen_golden.py -> tests/golden/*.npz).
The one place the reference's own arithmetic is NOT available is
``pytorch3d.ops.knn_points`` (third-party, un-vendored, version unpinned,
/root/reference/README.md:63-64): its semantics are restated from its
documented contract (squared L2, K smallest ascending, ties -> lower index)
in ``knn_points_exact`` and the goldens use that same stand-in, so parity at
the KNN boundary is "unpinned by the reference" (DESIGN.md section 3).

All file:line citations are relative to /root/reference/.
Weights are addressed by the reference's state-dict key names.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

def widen(obj, dtype=torch.float64):
    """Every floating tensor of a batch dict / state dict / list as ``dtype`` (values unchanged: fp32 -> fp64 is exact).
    With float64 inputs every function below evaluates the SAME graph in double precision -- the 'truth' the fp32
    evaluations (this oracle's own and the HIP path's) are both approximations of; discrete decisions (hull mask, 7-NN
    sets, the ViT's 32-octave PE table, which is defined by fp32 argument rounding) stay those of the fp32 pass."""
    if torch.is_tensor(obj):
        return obj.to(dtype) if obj.is_floating_point() else obj
    if isinstance(obj, dict):
        return {k: widen(v, dtype) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(widen(v, dtype) for v in obj)
    return obj


# ---------------------------------------------------------------------------
# a-1  sample placement   lib/networks/renderer/if_clight_renderer.py:271-287
# ---------------------------------------------------------------------------
def sampling_points(ray_o, ray_d, near, far, n_samples, t_rand=None):
    """ray_o,ray_d [R,3]; near,far [R] -> pts [R,S,3], z [R,S].
    t_rand [R,S] (the draws of torch.rand, :282): the stratified jitter of cfg.perturb > 0 in train() mode, :276-283."""
    t = torch.linspace(0.0, 1.0, steps=n_samples).to(near)
    z = near[..., None] * (1.0 - t) + far[..., None] * t          # :274
    if t_rand is not None:
        mids = .5 * (z[..., 1:] + z[..., :-1])                    # :278
        upper = torch.cat([mids, z[..., -1:]], -1)
        lower = torch.cat([z[..., :1], mids], -1)
        z = lower + (upper - lower) * t_rand.to(upper)            # :283
    pts = ray_o[:, None] + ray_d[:, None] * z[..., None]          # :285
    return pts, z


# ---------------------------------------------------------------------------
# third-party boundary: pytorch3d.ops.knn_points  (call sites
# if_clight_renderer.py:440, if_mesh_renderer.py:53, cross_transformer.py:170)
# ---------------------------------------------------------------------------
def knn_points_exact(p, q, K, chunk=4096):
    """Exact brute force.  p [P,3], q [N,3] fp32 -> (d2 [P,K] ascending squared
    L2 computed as (dx*dx + dy*dy) + dz*dz in fp32, idx [P,K] int64; ties go to
    the lower index)."""
    P = p.shape[0]
    d2o = torch.empty((P, K), dtype=p.dtype, device=p.device)
    ido = torch.empty((P, K), dtype=torch.int64, device=p.device)
    for s in range(0, P, chunk):
        pp = p[s:s + chunk]
        dx = pp[:, None, 0] - q[None, :, 0]
        dy = pp[:, None, 1] - q[None, :, 1]
        dz = pp[:, None, 2] - q[None, :, 2]
        d2 = dx * dx + dy * dy
        d2 = d2 + dz * dz
        if K == 1:
            v, i = d2.min(dim=1)                # first occurrence on CPU
            d2o[s:s + chunk, 0] = v
            ido[s:s + chunk, 0] = i
        else:
            v, i = torch.sort(d2, dim=1, stable=True)
            d2o[s:s + chunk] = v[:, :K]
            ido[s:s + chunk] = i[:, :K]
    return d2o, ido


def hull_mask(pts, verts, thresh=0.1):
    """if_clight_renderer.py:440-442 -- sqrt(min d2) < 0.1 per sample.
    pts [P,3], verts [NV,3] (both world space) -> bool [P].
    The square root is the CORRECTLY ROUNDED one of d2's own precision, as IEEE 754 and the reference's CUDA sqrt give it.  For
    fp32 it is taken in float64 and rounded back (53 >= 2 * 24 + 2 bits: the double rounding is exact for a square root): the
    fp32 sqrt of torch's CPU kernels is an ulp off on some hosts (one x86 server CPU: 14 % of the operands, 176 samples of
    tests/hull_cases.py's thresh-0.3 shells decided the other way), and a sample an ulp from the threshold flips with it."""
    d2, _ = knn_points_exact(pts, verts, 1)
    d2 = d2[:, 0]
    if d2.dtype == torch.float32:
        return d2.double().sqrt().float() < thresh
    return d2.sqrt() < thresh


# ---------------------------------------------------------------------------
# a-3 helpers
# ---------------------------------------------------------------------------
def world2smpl(pts, Rh, Th):
    """if_clight_renderer.py:289-295: q = (p - Th) @ Rh.  pts [...,3], Rh [3,3], Th [1,3]."""
    sh = pts.shape
    return torch.matmul(pts.reshape(-1, 3) - Th.reshape(1, 3), Rh).reshape(sh)


def view_embed(ray_d, view_res=4):
    """if_clight_renderer.py:525-526 + lib/networks/embedder.py:9-35:
    v=d/|d|; [v, sin(2^k v), cos(2^k v)] k<view_res -> [R, 3+6*view_res]."""
    v = ray_d / torch.norm(ray_d, dim=-1, keepdim=True)
    out = [v]
    freqs = (2.0 ** torch.linspace(0.0, view_res - 1, steps=view_res)).to(ray_d.dtype)
    for f in freqs.tolist():
        out.append(torch.sin(v * f))
        out.append(torch.cos(v * f))
    return torch.cat(out, -1)


def pe_encode(x, num_freqs, include_input=True):
    """pixelNeRF PE, lib/networks/vision_transformer.py:100-136.
    x [N,3] -> [N, 6F (+3)]; arg = addcmul(phase, x, freq) (single-rounding
    FMA), layout per octave: sin(f x) xyz, cos(f x) xyz."""
    freqs = np.pi * 2.0 ** torch.arange(0, num_freqs)             # :109 (fp32 tensor)
    _freqs = torch.repeat_interleave(freqs, 2).view(1, -1, 1)     # :116
    _phases = torch.zeros(2 * num_freqs)
    _phases[1::2] = np.pi * 0.5                                   # :121
    _phases = _phases.view(1, -1, 1)
    e = x.unsqueeze(1).repeat(1, num_freqs * 2, 1)
    # (the fp32 constants of the reference, widened when the oracle runs in float64: see render_fast(dtype=...))
    e = torch.sin(torch.addcmul(_phases.to(x), e, _freqs.to(x)))              # :132
    e = e.view(x.shape[0], -1)
    if include_input:
        e = torch.cat((x, e), dim=-1)
    return e


def normalize_pe(pe, cr=(-1.5, -1.5, -1.5, 1.5, 1.5, 1.5)):
    """if_clight_renderer.py:373-383 (float64 in, float32 out)."""
    cr = torch.tensor(cr).to(pe.device)
    mn, mx = cr[:3][None, None, :], cr[3:][None, None, :]
    out = (((pe - mn) / (mx - mn)) - 0.5) * 2
    return out.type(torch.float32)


# ---------------------------------------------------------------------------
# a-4 / a-9  projection + bilinear sampling
# ---------------------------------------------------------------------------
def project_uv(x, R, T, K):
    """if_clight_renderer.py:123-126 / :228-232.  x [N,3]; R [V,3,3]; T [V,3,1];
    K [V,3,3] -> uv [V,N,2]."""
    rot = torch.matmul(R[:, None], x[None, :, :, None])[..., 0]
    cam = rot + T[:, None, :3, 0]
    pix = torch.matmul(K[:, None], cam.unsqueeze(-1))[..., 0]
    return pix[:, :, :2] / pix[:, :, 2:]


def feat_scale(H, W):
    """lib/networks/encoder.py:148-153 then if_clight_renderer.py:193-195:
    scale = [W,H]/([W,H]-1)*2 / [H,W] as float32 (note the H/W mix of the
    reference, harmless for square images)."""
    s = np.array([W, H]) / (np.array([W, H]) - 1) * 2.0
    s = s / np.array([H, W])
    return torch.tensor(s).to(dtype=torch.float32)


def bilinear_border(feat, uv, scale):
    """Explicit restatement of F.grid_sample(bilinear, align_corners=True,
    padding_mode='border') as used at if_clight_renderer.py:197-206.
    feat [V,C,H,W]; uv [V,N,2] pixel coords; scale [2] -> [V,C,N]."""
    V, C, H, W = feat.shape
    g = uv * scale.to(uv.device) - 1.0                                          # :197
    ix = ((g[..., 0] + 1.0) / 2.0) * (W - 1)
    iy = ((g[..., 1] + 1.0) / 2.0) * (H - 1)
    ix = ix.clamp(0.0, float(W - 1))
    iy = iy.clamp(0.0, float(H - 1))
    x0 = torch.floor(ix); y0 = torch.floor(iy)
    x1 = x0 + 1; y1 = y0 + 1
    w_nw = (x1 - ix) * (y1 - iy)
    w_ne = (ix - x0) * (y1 - iy)
    w_sw = (x1 - ix) * (iy - y0)
    w_se = (ix - x0) * (iy - y0)
    out = torch.zeros((V, C, uv.shape[1]), dtype=feat.dtype, device=feat.device)
    fl = feat.reshape(V, C, H * W)
    for (xx, yy, ww) in ((x0, y0, w_nw), (x1, y0, w_ne), (x0, y1, w_sw), (x1, y1, w_se)):
        inb = (xx >= 0) & (xx <= W - 1) & (yy >= 0) & (yy <= H - 1)
        lin = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).long()
        val = torch.gather(fl, 2, lin[:, None, :].expand(V, C, -1))
        out = out + val * (ww * inb.to(ww.dtype))[:, None, :]
    return out


def paint(holder_feat_map, verts_w, in_R, in_T, in_K, vizmap):
    """paint_neural_human, if_clight_renderer.py:95-184 (rasterize=True path).
    holder_feat_map [V,192,H,W]; verts_w [NV,3]; vizmap bool [V,NV]
    -> big_holder [V,NV,192] with invisible vertices zeroed (:181-182)."""
    V, C, H, W = holder_feat_map.shape
    uv = project_uv(verts_w, in_R, in_T, in_K)
    lat = bilinear_border(holder_feat_map, uv, feat_scale(H, W)).permute(0, 2, 1)
    return lat * vizmap[..., None].to(lat.dtype)


def segment_mean(src, offsets, members):
    """voxelization, if_clight_renderer.py:356-371: per-cluster arithmetic mean
    over the member list in stored order.  src [NV,...] -> [N_c,...] (dtype kept)."""
    out = []
    for c in range(len(offsets) - 1):
        idx = torch.as_tensor(members[offsets[c]:offsets[c + 1]], dtype=torch.long, device=src.device)
        out.append(src[idx].mean(0))
    return torch.stack(out)


# ---------------------------------------------------------------------------
# a-6  TransHE  lib/networks/vision_transformer.py:257-383
# ---------------------------------------------------------------------------
def attention(qkv, heads):
    """Attention.forward, :271-278, on the output of the fused qkv layer: qkv [V,N,3C] with column = which C + head hd + d
    -> [V,N,C] (dtype kept: float64 in, float64 out)."""
    V, N, C3 = qkv.shape
    C = C3 // 3
    hd = C // heads
    qkv = qkv.reshape(V, N, 3, heads, hd).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0], qkv[1], qkv[2]
    a = (q @ k.transpose(-2, -1)) * (hd ** -0.5)                   # :274
    a = a.softmax(dim=-1)
    return (a @ v).transpose(1, 2).reshape(V, N, C)


def vit_forward(x, pe_xyz, sd, depth, prefix="ViT.", heads=3):
    """x [V,N,192] tokens; pe_xyz [V,N,3] normalised canonical centres."""
    V, N, C = x.shape
    # (32 octaves: the top ones are sin(pi 2^31 x) -- DEFINED by the fp32 rounding of the argument, a hash of x; the table
    # is therefore always the fp32 one, widened when the oracle runs in float64)
    # ... and always evaluated on the HOST: sin() of arguments up to pi 2^31 depends on the library's argument reduction, and
    # the goldens (the reference imported on the host) pin the host's table -- the oracle may run on a device (tools/dense_tail.py)
    pe = pe_encode(pe_xyz.float().cpu().reshape(-1, 3), C // 6, include_input=False).view(V, N, C).to(x)
    x = x + pe                                                     # :366-367
    for i in range(depth):
        p = f"{prefix}blocks.{i}."
        y = F.layer_norm(x, (C,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], 1e-6)
        qkv = F.linear(y, sd[p + "attn.qkv.weight"], sd[p + "attn.qkv.bias"])
        y = attention(qkv, heads)
        y = F.linear(y, sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"])
        x = x + y
        y = F.layer_norm(x, (C,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], 1e-6)
        y = F.linear(y, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"])
        y = F.gelu(y)                                              # nn.GELU (erf)
        y = F.linear(y, sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"])
        x = x + y
    return F.layer_norm(x, (C,), sd[prefix + "norm.weight"], sd[prefix + "norm.bias"], 1e-6)


# ---------------------------------------------------------------------------
# a-7  DPaRF  lib/networks/cross_transformer.py:151-205
# ---------------------------------------------------------------------------
def dparf(pts_s, centres, blend, tokens, K=7, n_freq=10, alpha=0.5):
    """pts_s [P,3] (SMPL coords); centres [N_c,3]; blend [N_c,4,4] (any float
    dtype, cast to fp32 like :185); tokens [V,N_c,192]
    -> human_rep [P,V,255] (token part then PE part, as torch.cat at :199)."""
    d2, idx = knn_points_exact(pts_s.float(), centres.float(), K)
    if pts_s.dtype != torch.float32:
        # float64 "truth" mode: the neighbour SET is a discrete decision and stays the fp32 pass's; distances are recomputed
        dd = pts_s.unsqueeze(1) - centres.to(pts_s.dtype)[idx]
        d2 = (dd * dd).sum(-1)
    d = d2.sqrt()                                                  # :171
    w = F.softmax(-d / alpha, dim=1)                               # :153-154
    rel = pts_s.unsqueeze(1) - centres.to(pts_s.dtype)[idx]        # :183-184
    rot = blend[..., :3, :3].type(torch.float32).to(pts_s.dtype)[idx]   # :185-186 (the fp32 cast is the reference's)
    de = torch.matmul(rel.unsqueeze(-2), rot).squeeze(-2)          # :187-188
    P = pts_s.shape[0]
    pe = pe_encode(de.reshape(-1, 3), n_freq, True).view(P, K, -1)
    out = []
    for v in range(tokens.shape[0]):
        f = torch.cat([tokens[v][idx].to(pe.dtype), pe], dim=-1)   # :198-199
        out.append(torch.sum(w.unsqueeze(-1) * f, dim=1))          # :200
    return torch.stack(out, dim=1)


# ---------------------------------------------------------------------------
# a-8  per-point MLP  lib/networks/cross_transformer.py:128-149, 273-353
# ---------------------------------------------------------------------------
def _lin(sd, name, x):
    w = sd[name + ".weight"]
    return F.linear(x, w.reshape(w.shape[0], -1), sd[name + ".bias"])


def multiview_agg(sd, h, f):
    """h [P,V,255] human rep, f [P,V,384] pixel feats -> inter [P,V,256]."""
    s = F.relu(_lin(sd, "fc_0", h))                                # :315
    p = F.relu(_lin(sd, "alpha_res_0", f))                         # :316
    kp = _lin(sd, "spatial_key_value_0.key_embed", p)              # :134
    vp = _lin(sd, "spatial_key_value_0.value_embed", p)
    ks = _lin(sd, "spatial_key_value_1.key_embed", s)              # :137
    vs = _lin(sd, "spatial_key_value_1.value_embed", s)
    A = torch.einsum("pjc,pic->pji", kp, ks) / math.sqrt(kp.shape[-1])   # :141-142
    A = F.softmax(A, dim=1)                                        # :144 (over pixel views j)
    n = vs + torch.einsum("pjc,pji->pic", vp, A)                   # :145-147
    n = F.relu(_lin(sd, "fc_1", n))
    return F.relu(_lin(sd, "fc_2", n))                             # :319-320


def alpha_forward(sd, inter):
    o = F.relu(_lin(sd, "fc_3", inter.mean(dim=1)))                # :325-326
    return _lin(sd, "alpha_fc", o)                                 # [P,1]


def rgb_forward(sd, inter, f, viewdir):
    """inter [P,V,256]; f [P,V,384]; viewdir [P,27] -> [P,3]."""
    V = inter.shape[1]
    feat = _lin(sd, "feature_fc", inter) + _lin(sd, "rgb_res_0", f)   # :333-335
    feat = torch.cat([feat, viewdir[:, None, :].expand(-1, V, -1)], dim=-1)
    net = F.relu(_lin(sd, "view_fc", feat)) + _lin(sd, "rgb_res_1", f)   # :341-344
    net = F.relu(_lin(sd, "fc_4", net.mean(dim=1)))                # :347-350
    return _lin(sd, "rgb_fc", net)


def network_forward(sd, pixel_feat, viewdir, pts_s, centres, blend, tokens, pts_mask=None,
                    K=7, n_freq=10, alpha=0.5):
    """Network.forward, cross_transformer.py:207-311.
    pixel_feat [V,384,P]; viewdir [P,27]; pts_s [P,3]; pts_mask bool [P] | None
    -> raw [P,4] (rgb logits, sigma_raw).  With a mask: progressive RGB (only
    sigma_raw > 0, :298) and zeros on masked-out points (:231,:268)."""
    P = pts_s.shape[0]
    f_all = pixel_feat.permute(2, 0, 1)
    if pts_mask is not None:
        raw = torch.zeros((P, 4), dtype=pts_s.dtype, device=pts_s.device)
        if pts_mask.sum() == 0:
            return raw
        sel = pts_mask
    else:
        sel = torch.ones(P, dtype=torch.bool, device=pts_s.device)
    ps, f, vd = pts_s[sel], f_all[sel], viewdir[sel]
    h = dparf(ps, centres, blend, tokens, K, n_freq, alpha)
    inter = multiview_agg(sd, h, f)
    sig = alpha_forward(sd, inter)
    if pts_mask is not None:
        rgb = torch.zeros((ps.shape[0], 3), dtype=pts_s.dtype, device=pts_s.device)
        dm = sig[:, 0] > 0
        if dm.sum() > 0:
            rgb[dm] = rgb_forward(sd, inter[dm], f[dm], vd[dm])
        raw[sel] = torch.cat([rgb, sig], dim=1)
        return raw
    return torch.cat([rgb_forward(sd, inter, f, vd), sig], dim=1)


# ---------------------------------------------------------------------------
# a-10  compositing  lib/networks/renderer/nerf_net_utils.py:14-59
# ---------------------------------------------------------------------------
def raw2outputs(raw, z, ray_d, white_bkgd=False, noise=None):
    """raw [R,S,4]; z [R,S]; ray_d [R,3] -> rgb [R,3], acc [R], depth [R], weights [R,S].
    noise [R,S]: randn * raw_noise_std, :39-41 (added to sigma in front of the relu)."""
    d = z[..., 1:] - z[..., :-1]
    d = torch.cat([d, torch.full_like(d[..., :1], 1e10)], -1)      # :31-35
    d = d * torch.norm(ray_d[..., None, :], dim=-1)                # :37
    c = torch.sigmoid(raw[..., :3])
    sig = raw[..., 3] if noise is None else raw[..., 3] + noise.to(raw)     # :44
    a = 1.0 - torch.exp(-F.relu(sig) * d)                          # :27-28,:44
    T = torch.cumprod(torch.cat([torch.ones((a.shape[0], 1), dtype=a.dtype, device=a.device), 1.0 - a + 1e-10], -1), -1)[:, :-1]
    w = a * T                                                      # :46-49
    rgb = torch.sum(w[..., None] * c, -2)
    depth = torch.sum(w * z, -1)
    acc = torch.sum(w, -1)
    if white_bkgd:
        rgb = rgb + (1.0 - acc[..., None])
    return rgb, acc, depth, w


# ---------------------------------------------------------------------------
# frame constants shared by render_fast and the mesh renderer
# ---------------------------------------------------------------------------
def frame_constants(sd, batch, holder_feat_map, offsets, members, can_centres64, vit_depth):
    """if_clight_renderer.py:531-547: paint -> group -> ViT, plus DPaRF tables.
    can_centres64: float64 [N_c,3] cluster means of the canonical template
    (Renderer.__init__ :73)."""
    t = 0
    V = holder_feat_map.shape[0]
    big = paint(holder_feat_map, batch["input_smpl_vertice"][t][0],
                batch["input_R"][t].reshape(-1, 3, 3), batch["input_T"][t].reshape(-1, 3, 1),
                batch["input_K"][t].reshape(-1, 3, 3), batch["input_vizmaps"][t][0])
    grouped = torch.stack([segment_mean(big[v], offsets, members) for v in range(V)])
    pe_xyz = normalize_pe(can_centres64.unsqueeze(0).repeat(V, 1, 1)).to(grouped.dtype)      # (fp32 cast: the reference's)
    tokens = vit_forward(grouped, pe_xyz, sd, vit_depth)
    centres = segment_mean(batch["tar_smpl_vertice_smplcoord"][0], offsets, members)
    blend = segment_mean(batch["blend_mtx"][0], offsets, members)
    return dict(grouped=grouped, tokens=tokens, centres=centres, blend=blend)


def pixel_aligned(pixel_feat_map, xyz_w, batch):
    """get_pixel_aligned_feature, if_clight_renderer.py:210-269 -> [V,384,P]."""
    t = 0
    V, C, H, W = pixel_feat_map.shape
    uv = project_uv(xyz_w, batch["input_R"][t].reshape(-1, 3, 3),
                    batch["input_T"][t].reshape(-1, 3, 1), batch["input_K"][t].reshape(-1, 3, 3))
    return bilinear_border(pixel_feat_map, uv, feat_scale(H, W))


def render_fast(sd, batch, holder_feat_map, pixel_feat_map, offsets, members, can_centres64,
                n_samples=64, vit_depth=12, small_frame_rays=2400, hull=0.1, chunk=32768, white_bkgd=False,
                t_rand=None, sigma_noise=None):
    """Renderer.render_fast, if_clight_renderer.py:429-484 (+ _render :500-605,
    batchify_rays :607-656).  Encoder outputs are inputs here.
    t_rand [R,S]: the draws of the depth jitter (:276-283); sigma_noise [R,S]: randn * raw_noise_std of raw2outputs, indexed
    by the frame's rays (the reference draws it for the hit rays only; the rows of the other rays are not used).
    Returns dict rgb_map [1,R,3], acc_map [1,R], depth_map [1,R]."""
    ray_o, ray_d = batch["ray_o"][0], batch["ray_d"][0]
    near, far = batch["near"][0], batch["far"][0]
    R = ray_o.shape[0]
    dt = ray_o.dtype
    pts, z = sampling_points(ray_o, ray_d, near, far, n_samples, t_rand)
    # float64 "truth" mode (every floating tensor of `batch` / `sd` / the feature maps handed in as float64: the exact
    # arithmetic of the same graph on the same fp32 inputs): discrete decisions -- this hull mask, the 7-NN sets of
    # dparf -- are taken from the fp32 pass, as the reference would take them
    pts32 = pts if dt == torch.float32 else sampling_points(ray_o.float(), ray_d.float(), near.float(), far.float(), n_samples,
                                                            None if t_rand is None else t_rand.float())[0]
    vm = hull_mask(pts32.reshape(-1, 3), batch["tar_smpl_vertice"][0].float(), hull).view(R, n_samples)
    hit = vm.sum(-1) > 0                                           # :443
    dv = ray_o.device
    out = dict(rgb_map=torch.zeros(1, R, 3, dtype=dt, device=dv), acc_map=torch.zeros(1, R, dtype=dt, device=dv),
               depth_map=torch.zeros(1, R, dtype=dt, device=dv))
    Rp = int(hit.sum())
    fc = frame_constants(sd, batch, holder_feat_map, offsets, members, can_centres64, vit_depth)
    if Rp == 0:
        return out, fc
    o, d, zz, pw, m = ray_o[hit], ray_d[hit], z[hit], pts[hit], vm[hit]
    ps = world2smpl(pw, batch["Rh"][0], batch["Th"][0]).reshape(-1, 3)
    vd = view_embed(d)[:, None, :].expand(-1, n_samples, -1).reshape(-1, 27)
    xyz = pw.reshape(-1, 3)
    if Rp <= small_frame_rays:                                     # :551 un-masked branch
        pf = pixel_aligned(pixel_feat_map, xyz, batch)
        raw = network_forward(sd, pf, vd, ps, fc["centres"], fc["blend"], fc["tokens"], None)
    else:
        mm = m.reshape(-1)
        raws = []
        for s in range(0, xyz.shape[0], chunk):
            pf = pixel_aligned(pixel_feat_map, xyz[s:s + chunk], batch)
            raws.append(network_forward(sd, pf, vd[s:s + chunk], ps[s:s + chunk], fc["centres"],
                                        fc["blend"], fc["tokens"], mm[s:s + chunk]))
        raw = torch.cat(raws, 0)
    rgb, acc, depth, _ = raw2outputs(raw.view(Rp, n_samples, 4), zz, d, white_bkgd,       # :593 (hit rays only)
                                     None if sigma_noise is None else sigma_noise[hit])
    fc = dict(fc, hit=hit, raw=raw.view(Rp, n_samples, 4), mask=m)      # (test diagnostics: per-sample outputs of the hit rays)
    out["rgb_map"][0, hit] = rgb
    out["acc_map"][0, hit] = acc
    out["depth_map"][0, hit] = depth
    return out, fc


def render_sigma_grid(sd, batch, pts_grid, holder_feat_map, pixel_feat_map, offsets, members,
                      can_centres64, vit_depth=12, hull=0.1, chunk=32768):
    """if_mesh_renderer.Renderer.render :46-100 up to ``cube`` (before np.pad
    and marching cubes).  pts_grid [1,X,Y,Z,3] -> sigma_raw cube [X,Y,Z]."""
    sh = pts_grid.shape
    xyz = pts_grid.reshape(-1, 3)
    m = hull_mask(xyz, batch["tar_smpl_vertice"][0], hull)
    ps = world2smpl(xyz, batch["Rh"][0], batch["Th"][0])
    vd = torch.zeros((xyz.shape[0], 27))                           # :62
    fc = frame_constants(sd, batch, holder_feat_map, offsets, members, can_centres64, vit_depth)
    raws = []
    for s in range(0, xyz.shape[0], chunk):
        pf = pixel_aligned(pixel_feat_map, xyz[s:s + chunk], batch)
        raws.append(network_forward(sd, pf, vd[s:s + chunk], ps[s:s + chunk], fc["centres"],
                                    fc["blend"], fc["tokens"], m[s:s + chunk]))
    raw = torch.cat(raws, 0)
    return raw[:, 3].view(*sh[1:4])


# ---------------------------------------------------------------------------
# f-1 (feeds the path)  SpatialEncoder.forward  lib/networks/encoder.py:97-155
# ---------------------------------------------------------------------------
def _bn_train(x, w, b, eps=1e-5):
    """BatchNorm2d in *train mode* (run.py:29 leaves the net in train())."""
    return F.batch_norm(x, None, None, w, b, True, 0.0, eps)


def _basic_block(sd, p, x, stride, has_down):
    idt = x
    y = F.conv2d(x, sd[p + "conv1.weight"], None, stride, 1)
    y = F.relu(_bn_train(y, sd[p + "bn1.weight"], sd[p + "bn1.bias"]))
    y = F.conv2d(y, sd[p + "conv2.weight"], None, 1, 1)
    y = _bn_train(y, sd[p + "bn2.weight"], sd[p + "bn2.bias"])
    if has_down:
        idt = F.conv2d(x, sd[p + "downsample.0.weight"], None, stride, 0)
        idt = _bn_train(idt, sd[p + "downsample.1.weight"], sd[p + "downsample.1.bias"])
    return F.relu(y + idt)


def encoder_forward(sd, images, prefix="encoder."):
    """images [V,3,H,W] -> holder_feat_map [V,192,H,W], pixel_feat_map [V,384,H,W]."""
    m = prefix + "model."
    H, W = images.shape[2:]
    x = F.conv2d(images, sd[m + "conv1.weight"], None, 2, 3)
    x = F.relu(_bn_train(x, sd[m + "bn1.weight"], sd[m + "bn1.bias"]))
    lat = [x]
    x = F.max_pool2d(x, 3, 2, 1)
    x = _basic_block(sd, m + "layer1.0.", x, 1, False)
    x = _basic_block(sd, m + "layer1.1.", x, 1, False)
    lat.append(x)
    x = _basic_block(sd, m + "layer2.0.", x, 2, True)
    x = _basic_block(sd, m + "layer2.1.", x, 1, False)
    lat.append(x)
    lat = [F.interpolate(l, (H, W), mode="bilinear", align_corners=True) for l in lat]
    pix = torch.cat(lat, dim=1)
    col = F.conv2d(images, sd[prefix + "upsample_color.weight"], sd[prefix + "upsample_color.bias"])
    pix = torch.cat([pix, col], dim=1)
    hol = F.conv2d(pix, sd[prefix + "reduction_layer.weight"], sd[prefix + "reduction_layer.bias"])
    return hol, pix


# ---------------------------------------------------------------------------
# ray generation (numpy, the reference's dtypes)
# ---------------------------------------------------------------------------
def gen_rays(H, W, K, R, T, bounds):
    """lib/utils/if_nerf/if_nerf_data_utils.py:11-30 (get_rays), :65-97 (get_near_far) chained as the test split
    of sample_ray_h36m does (:271-283).  K, R, T, bounds float32 (can_smpl.py:640-645, :216-232).
    Returns the dense per-pixel arrays {ray_o, ray_d [H*W,3] f32 (ray_d with the :70 clamp), near, far [H*W] f32
    (0 outside), mask_at_box bool [H*W]}."""
    rays_o = -np.dot(R.T, T).ravel()                                                   # :14
    i, j = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32), indexing="xy")
    xy1 = np.stack([i, j, np.ones_like(i)], axis=2)
    pixel_camera = np.dot(xy1, np.linalg.inv(K).T)                                     # :25
    pixel_world = np.dot(pixel_camera - T.ravel(), R)                                  # :26
    rays_d = pixel_world - rays_o[None, None]
    ray_o = np.broadcast_to(rays_o, rays_d.shape).reshape(-1, 3).astype(np.float32)    # :273
    ray_d = rays_d.reshape(-1, 3).astype(np.float32)                                   # :274
    b = bounds + np.array([-0.01, 0.01])[:, None]                                      # :67 (promotes to float64)
    nominator = b[None] - ray_o[:, None]
    ray_d[np.abs(ray_d) < 1e-5] = 1e-5                                                 # :70 (in place)
    d_intersect = (nominator / ray_d[:, None]).reshape(-1, 6)
    p_intersect = d_intersect[..., None] * ray_d[:, None] + ray_o[:, None]
    min_x, min_y, min_z, max_x, max_y, max_z = b.ravel()
    eps = 1e-6
    hit = (p_intersect[..., 0] >= (min_x - eps)) * (p_intersect[..., 0] <= (max_x + eps)) * \
          (p_intersect[..., 1] >= (min_y - eps)) * (p_intersect[..., 1] <= (max_y + eps)) * \
          (p_intersect[..., 2] >= (min_z - eps)) * (p_intersect[..., 2] <= (max_z + eps))
    mask = hit.sum(-1) == 2                                                            # :84
    p_int = p_intersect[mask][hit[mask]].reshape(-1, 2, 3)
    o, d = ray_o[mask], ray_d[mask]
    norm_ray = np.linalg.norm(d, axis=1)                                               # float32 (:92)
    d0 = np.linalg.norm(p_int[:, 0] - o, axis=1) / norm_ray
    d1 = np.linalg.norm(p_int[:, 1] - o, axis=1) / norm_ray
    near = np.zeros(H * W, np.float32)
    far = np.zeros(H * W, np.float32)
    near[mask] = np.minimum(d0, d1).astype(np.float32)
    far[mask] = np.maximum(d0, d1).astype(np.float32)
    return dict(ray_o=ray_o, ray_d=ray_d, near=near, far=far, mask_at_box=mask)


def bound_2d_mask(bounds, K, pose, H, W):
    """lib/utils/if_nerf/if_nerf_data_utils.py:49-62 (get_bound_2d_mask).  The corner projection / rounding are the
    reference's numpy expressions (:33-53, base_utils.py:178-187).  cv2.fillPoly is THIRD-PARTY and absent here
    (PARITY UNPINNED against OpenCV itself): its scan conversion for integer vertices is restated from the
    published source (imgproc/src/drawing.cpp: CollectPolyEdges draws every edge as an 8-connected line,
    FillEdgeCollection fills each scanline between consecutive pairs of edge crossings, an edge active for
    y0 <= y < y1, crossing x rounded half up, ends inclusive).  Plain loops: 6 polygons x 5 edges."""
    mn, mx = np.asarray(bounds)[0], np.asarray(bounds)[1]
    corners = np.array([[mn[0], mn[1], mn[2]], [mn[0], mn[1], mx[2]], [mn[0], mx[1], mn[2]], [mn[0], mx[1], mx[2]],
                        [mx[0], mn[1], mn[2]], [mx[0], mn[1], mx[2]], [mx[0], mx[1], mn[2]], [mx[0], mx[1], mx[2]]])
    xyz = np.dot(corners, np.asarray(pose)[:, :3].T) + np.asarray(pose)[:, 3:].T     # base_utils.project
    xyz = np.dot(xyz, np.asarray(K).T)
    c2 = np.round(xyz[:, :2] / xyz[:, 2:]).astype(int)                                 # :52
    mask = np.zeros((H, W), dtype=np.uint8)
    ys, xs = np.mgrid[0:H, 0:W]
    for face in ([0, 1, 3, 2, 0], [4, 5, 7, 6, 5], [0, 1, 5, 4, 0], [2, 3, 7, 6, 2], [0, 2, 6, 4, 0], [1, 3, 7, 5, 1]):
        pts = [(int(c2[v, 0]), int(c2[v, 1])) for v in face]
        cross = [[] for _ in range(H)]
        for e in range(5):
            (x0, y0), (x1, y1) = pts[e], pts[(e + 1) % 5]
            dx, dy = x1 - x0, y1 - y0
            # the edge as an 8-connected line
            if dx == 0 and dy == 0:
                if 0 <= x0 < W and 0 <= y0 < H:
                    mask[y0, x0] = 1
            elif abs(dx) >= abs(dy):
                for x in range(max(min(x0, x1), 0), min(max(x0, x1), W - 1) + 1):
                    y = int(np.floor(float(y0) + float(x - x0) * (float(dy) / float(dx)) + 0.5))
                    if 0 <= y < H:
                        mask[y, x] = 1
            else:
                for y in range(max(min(y0, y1), 0), min(max(y0, y1), H - 1) + 1):
                    x = int(np.floor(float(x0) + float(y - y0) * (float(dx) / float(dy)) + 0.5))
                    if 0 <= x < W:
                        mask[y, x] = 1
            # scanline crossings
            if y0 == y1:
                continue
            if y0 > y1:
                x0, y0, x1, y1 = x1, y1, x0, y0
            for y in range(max(y0, 0), min(y1, H)):
                cross[y].append(int(np.floor(float(x0) + float(y - y0) * (float(x1 - x0) / float(y1 - y0)) + 0.5)))
        for y in range(H):
            c = sorted(cross[y])
            for i in range(0, len(c) - 1, 2):
                a, b = max(c[i], 0), min(c[i + 1], W - 1)
                if a <= b:
                    mask[y, a:b + 1] = 1
    return mask


# ---------------------------------------------------------------------------
# marching cubes (consumer of the sigma cube), PLY, PSNR
# ---------------------------------------------------------------------------
_MC_EDGE_PT = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 0], [0, 0, 1], [1, 0, 1], [0, 1, 1], [0, 0, 1],
                        [0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]])
_MC_EDGE_AX = np.array([0, 1, 0, 1, 0, 1, 0, 1, 2, 2, 2, 2])


def mc_case_table():
    """the published 256 x 16 triangle table (Lorensen & Cline 1987, Bourke / Bloyd numbering), tests/golden/mc_case_table.npz"""
    import os
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return np.load(os.path.join(here, "tests", "golden", "mc_case_table.npz"))["tri"].astype(np.int64)


def marching_cubes(cube, iso, scale=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0)):
    """mcubes.marching_cubes(cube, iso) as if_mesh_renderer.py:103 calls it, followed by the index -> world transform
    of :106-108.  PyMCubes is THIRD-PARTY and absent (PARITY UNPINNED against mcubes itself): its published algorithm
    (marchingcubes.h: corner m of cell (i,j,k) in the Bourke numbering sets bit m when value <= iso; one vertex per
    cut edge at x1 + (x2 - x1) (iso - f1) / (f2 - f1), float64, midpoint if f1 == f2; triangles from the case table)
    is restated with numpy.  Vertex order: owning grid point row-major, +x / +y / +z edge; triangle order: cell
    row-major, table order (the device kernel's order; PyMCubes' own order follows from its traversal).
    -> (vertices float64 [nv,3], triangles int64 [nt,3])"""
    c = np.asarray(cube, dtype=np.float32)
    X, Y, Z = c.shape
    inside = c <= np.float32(iso)
    f = c.astype(np.float64)
    flags = np.zeros((X, Y, Z), dtype=np.int64)
    flags[:-1] |= (inside[:-1] != inside[1:]) * 1
    flags[:, :-1] |= (inside[:, :-1] != inside[:, 1:]) * 2
    flags[:, :, :-1] |= (inside[:, :, :-1] != inside[:, :, 1:]) * 4
    pop = (flags & 1) + ((flags >> 1) & 1) + ((flags >> 2) & 1)
    vbase = np.cumsum(pop.reshape(-1)) - pop.reshape(-1)
    nv = int(pop.sum())
    verts = np.zeros((nv, 3), dtype=np.float64)
    idx = np.stack(np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing="ij"), -1).astype(np.float64)
    vb = vbase.reshape(X, Y, Z)
    for a in range(3):
        sel = (flags >> a) & 1 == 1
        f0 = f[sel]
        f1 = np.roll(f, -1, axis=a)[sel]
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(f1 == f0, 0.5, (float(np.float32(iso)) - f0) / (f1 - f0))
        p = idx[sel].copy()
        p[:, a] = p[:, a] + t
        rank = np.zeros_like(flags)
        for b in range(a):
            rank = rank + ((flags >> b) & 1)
        verts[vb[sel] + rank[sel]] = p
    verts = verts * np.asarray(scale, dtype=np.float64)[None] + np.asarray(origin, dtype=np.float64)[None]
    # cells
    ins = inside.astype(np.int64)
    case = (ins[:-1, :-1, :-1] | ins[1:, :-1, :-1] << 1 | ins[1:, 1:, :-1] << 2 | ins[:-1, 1:, :-1] << 3 |
            ins[:-1, :-1, 1:] << 4 | ins[1:, :-1, 1:] << 5 | ins[1:, 1:, 1:] << 6 | ins[:-1, 1:, 1:] << 7)
    table = mc_case_table()
    ntri = (table >= 0).sum(1) // 3
    cells = np.argwhere((case != 0) & (case != 255))                      # row-major order
    cs = case[cells[:, 0], cells[:, 1], cells[:, 2]]
    counts = ntri[cs]
    tbase = np.cumsum(counts) - counts
    tris = np.zeros((int(counts.sum()), 3), dtype=np.int64)
    for k in range(15):                                                   # k-th edge slot of the table row
        has = table[cs, k] >= 0
        e = table[cs[has], k]
        pt = cells[has] + _MC_EDGE_PT[e]
        ax = _MC_EDGE_AX[e]
        fl = flags[pt[:, 0], pt[:, 1], pt[:, 2]]
        rank = np.where(ax >= 1, fl & 1, 0) + np.where(ax >= 2, (fl >> 1) & 1, 0)
        tris[tbase[has] + k // 3, k % 3] = vb[pt[:, 0], pt[:, 1], pt[:, 2]] + rank
    return verts, tris


def psnr_metric(img_pred, img_gt):
    """lib/evaluators/if_nerf.py:34-37"""
    mse = np.mean((img_pred - img_gt) ** 2)
    return -10 * np.log(mse) / np.log(10)


# ---------------------------------------------------------------------------
# SMPL linear blend skinning (numpy float64, lib/utils/SMPL.py:114-186)
# ---------------------------------------------------------------------------
def rodrigues(r):
    """cv2.Rodrigues(rotation vector) -> 3x3 (third-party, absent here: OpenCV's documented formula
    R = cos(t) I + (1 - cos(t)) n n^T + sin(t) [n]x with t = |r|, n = r / t; identity for t = 0).
    Parity unpinned against cv2 itself; tests pin it against scipy's Rotation.from_rotvec."""
    r = np.asarray(r, np.float64).reshape(3)
    t = np.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
    if t < np.finfo(np.float64).eps:
        return np.eye(3)
    n = r / t
    c, s = np.cos(t), np.sin(t)
    K = np.array([[0, -n[2], n[1]], [n[2], 0, -n[0]], [-n[1], n[0], 0]])
    return c * np.eye(3) + (1 - c) * np.outer(n, n) + s * K


def smpl_lbs(model, pose, beta):
    """SMPL._call, lib/utils/SMPL.py:114-186.  model: dict of float64 arrays (synth.make_smpl_model layout,
    parent[0] = -1); pose: [24,3,3] rotation matrices or 72 axis-angle values; beta [10].
    Returns (v [nv,3], joints [24,3], T [nv,4,4]) float64."""
    nv = model["v_template"].shape[0]
    shapedirs = model["shapedirs"].reshape(-1, 10)
    v_shaped = shapedirs.dot(np.asarray(beta, np.float64)[:, None]).reshape(nv, 3) + model["v_template"]   # :122
    J = model["J_regressor"].dot(v_shaped)                                                                  # :127
    pose = np.asarray(pose)
    if pose.shape == (24, 3, 3):
        R = pose
    else:
        R = np.array([rodrigues(p) for p in pose.reshape(-1, 3)], dtype="float32")                          # :135-139
    Is = np.eye(3, dtype="float32")[None, :]
    lrotmin = (R[1:, :] - Is).reshape(-1, 1)                                                                # :147
    v_posed = v_shaped + model["posedirs"].reshape(-1, 207).dot(lrotmin).reshape(nv, 3)                     # :149
    parent = model["parent"][1:]
    J_ = J.copy()
    J_[1:, :] = J[1:, :] - J[parent, :]                                                                     # :153
    G_ = np.concatenate([R, J_[:, :, None]], axis=-1)
    pad = np.repeat(np.array([[0, 0, 0, 1]], dtype="float32"), 24, axis=0).reshape(-1, 1, 4)
    G_ = np.concatenate([G_, pad], axis=1)
    G = [G_[0].copy()]
    for i in range(1, 24):
        G.append(G[parent[i - 1]].dot(G_[i, :, :]))                                                         # :160-161
    G = np.stack(G, axis=0)
    joints = G[:, :3, 3]
    rest = np.concatenate([J, np.zeros((24, 1))], axis=-1)[:, :, None]
    rest_mtx = np.concatenate([np.zeros((24, 4, 3), dtype="float32"), rest], axis=-1)
    G = G - np.matmul(G, rest_mtx)                                                                          # :169-170
    rest_h = np.concatenate([v_posed, np.ones(nv)[:, None]], axis=-1)
    T = model["weights"].dot(G.reshape(24, -1)).reshape(nv, 4, 4)                                           # :176
    v = np.matmul(T, rest_h[:, :, None])[:, :3, 0]                                                          # :177,:186
    return v, joints, T
