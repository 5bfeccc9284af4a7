"""The training entry of the boundary: ``Renderer.render`` with gradients.

The reference trains through ``Renderer.render(batch)`` (lib/train/trainers/if_nerf_clight.py:45, trainer.py:79-86:
``loss.backward()`` through the whole path, patches of <= 2400 rays).  The HIP kernels of this repository carry no
autograd, so a call with gradients enabled (or with the training-time randomisations ``cfg.perturb`` /
``cfg.raw_noise_std``) is served by this module instead: the same forward composed from differentiable torch operators
on the module's own parameters, on the device the batch lives on (torch's ROCm kernels on an MI355X).  It is NOT the
rendering hot path and not a fallback of it -- inference calls (``render_fast``, ``render_sequence``, ``render`` under
``no_grad``) never come here; SURVEY 7 hard-part 6 planned exactly this split.

``cfg.train_kernels`` selects how the three non-GEMM stages around the per-point network run: "torch" (default) composes
them from torch operators like everything else; "device" runs the token blend (K4), the pixel-aligned gather (K5) and the
compositing (K7) through the HIP forwards with HIP adjoints (``train_ops``), once over all samples before
the chunk loop.  The encoder trunk follows ``cfg.train_encoder`` and the per-point network ``cfg.train_point_net`` (both below).

``cfg.train_maps`` selects what the image features are sampled from: "full" (default) builds the reference's two full-size maps
(``encode``); "latents" runs the trunk as before and samples its three latents and the images directly at the input vertices
and at the ray samples (``train_ops.LatentGatherFn``) -- no [V,384,H,W] map, no [V,192,H,W] map, and no gradient
of either.  It needs the batch on the device, whatever ``cfg.train_kernels`` says.

``cfg.train_attention`` selects, independently, how the attention inside TransHE's blocks runs: "torch" (default) as three
torch operators whose autograd keeps a [V, heads, N, N] probability tensor per layer; "device" through the attention kernels
of the inference path with a HIP backward that recomputes the probabilities tile by tile (``train_ops.AttentionFn``,
DESIGN.md "K3 training form").

``cfg.train_vit_dense`` selects, independently again, how everything else inside TransHE runs -- the dense layers, LayerNorm
and GELU: "torch" (default) as torch modules under torch autograd; "device" through the fp32 MFMA GEMMs of the inference
path with HIP backwards that recompute LN(x) and gelu(u) instead of keeping them and add their partial sums in a fixed order
(``train_ops.NormLinearFn`` / ``LinearFn`` / ``GeluLinearFn`` / ``LayerNormFn``): with both switches on "device" TransHE's
gradient is bit-identical from run to run.  The residual adds and the positional table stay torch operators.

``cfg.train_point_net`` selects, independently of the other four, how the per-point network runs: "torch" (default) is
``point_network`` under torch autograd; "device" is ``point_network_device``: the layer-by-layer form of the inference path
(th_mlp_forward) on the fp32 MFMA GEMMs, every ReLU in its layer's epilogue, with HIP backwards (``train_ops.ReluLinearFn`` /
``LinearFn`` / ``CrossViewAttentionFn``).  View means and residual adds stay torch operators.

``cfg.train_encoder`` selects, independently of the other five, how the ResNet18 trunk of the encoder is differentiated: "torch"
(default) is ``SpatialEncoder.trunk(fused_bn=False)`` under torch autograd; "device" is ``trunk_device``: the same torch
operators in the forward, site by site without a graph -- latents, running statistics and num_batches_tracked are the "torch"
mode's bit for bit --, and HIP backwards with fixed-order sums (``train_ops.ConvFn`` / ``BnActFn`` / ``MaxPoolFn``, DESIGN.md
K23).  ``cfg.train_encoder_fwd`` = "device" (default "torch"; read only under ``cfg.train_encoder`` = "device"; its own check,
``encoder_fwd_mode``) replaces those torch operators by HIP forwards: ``hip.conv2d_fwd32`` (K29: exact fp32 operands on the MFMA,
fixed-order sums), ``hip.bn_act`` (K11) and ``hip.maxpool3x3s2``; the backwards are the same.
The upsamples, ``upsample_color`` and ``reduction_layer`` stay what ``cfg.train_maps`` makes them.  A trunk converted to
SyncBatchNorm (data-parallel training) runs under torch autograd as a whole under "device" too, unless ``cfg.train_sync_bn`` =
"device" (default "torch"; its own check, ``_sync_bn_mode``: the key is not in the table below), which runs the converted sites
on ``train_ops.SyncBnActFn``: the BatchNorm backward split around one all_gather of a [C, 6] float64 record per site.

The allowed values of these six and of ``cfg.train_gather_bwd`` (the form of the latent gather's adjoint) are one table,
``config.TRAIN_SWITCHES``, and ``_switch`` is their one reader: a value outside the table is a ValueError, a value other than
the first on CPU tensors a HipError.

``cfg.use_truncation`` (the reference's key, with ``cfg.KNN_SIGMA``; cross_transformer.py:175-180, :247-264) is honoured under every
combination of the switches: the samples whose nearest token centre is KNN_SIGMA or farther away are taken out once, in front of
the token blend, the pixel rows and the per-point network, and get raw = 0 (``truncation_lists``).

Pinned by ``oracle/gen_golden_train.py`` (the real reference imported in the survey container: outputs and parameter
gradients of one training step's forward/backward on a synthetic patch -> ``tests/golden/g18_train_step.npz``) and
``tests/test_train_path.py``.  Every function cites the reference lines it follows.
"""
import math

import torch
import torch.nn.functional as F

from ..config import TRAIN_ENCODER_FWD, TRAIN_SWITCHES, TRAIN_SYNC_BN, get_cfg
from ..truncation import sigma_in_force
from ..dparf_params import check_centres, params_in_force


# ---- the switches ------------------------------------------------------------------------------------------------------
def _switch(key, value, on_device, noun="batch"):
    """The one reader of config.TRAIN_SWITCHES: ``value`` of cfg.<key> as a str, one of the key's allowed values; any but the
    first runs HIP kernels, so it is refused unless the tensors (the ``noun`` of the message) are on the device."""
    allowed = TRAIN_SWITCHES[key]
    mode = str(value)
    if mode not in allowed:
        raise ValueError(f"cfg.{key} must be {allowed[0]!r} or {allowed[1]!r}, not {mode!r}")
    if mode != allowed[0] and not on_device:
        from .. import hip
        raise hip.HipError(f"cfg.{key} = '{mode}' needs the {noun} on an MI355X (the HIP kernels have no CPU form); "
                           f"use '{allowed[0]}' for a CPU batch")
    return mode


def _sync_bn_mode(value):
    """cfg.train_sync_bn, which is not one of TRAIN_SWITCHES (it selects nothing in a single process): one of config.TRAIN_SYNC_BN"""
    mode = str(value)
    if mode not in TRAIN_SYNC_BN:
        raise ValueError(f"cfg.train_sync_bn must be {TRAIN_SYNC_BN[0]!r} or {TRAIN_SYNC_BN[1]!r}, not {mode!r}")
    return mode


def encoder_fwd_mode(value=None):
    """cfg.train_encoder_fwd, which is not one of TRAIN_SWITCHES (it selects nothing unless cfg.train_encoder = "device"): one of
    config.TRAIN_ENCODER_FWD.  Without an argument the live cfg's value, the default where the key is absent.  Read by
    ``trunk_device`` and by the trunk's Functions of train_ops in their forward, nowhere else."""
    if value is None:
        value = getattr(get_cfg(), "train_encoder_fwd", TRAIN_ENCODER_FWD[0])
    mode = str(value)
    if mode not in TRAIN_ENCODER_FWD:
        raise ValueError(f"cfg.train_encoder_fwd must be {TRAIN_ENCODER_FWD[0]!r} or {TRAIN_ENCODER_FWD[1]!r}, not {mode!r}")
    return mode


# ---- sampling ----------------------------------------------------------------------------------------------------------
def sample_depths(near, far, n_samples, perturb):
    """if_clight_renderer.py:271-287: z = near (1 - t) + far t; with ``perturb`` one uniform sample per stratum."""
    t = torch.linspace(0.0, 1.0, steps=n_samples).to(near)
    z = near[..., None] * (1.0 - t) + far[..., None] * t
    if perturb:
        mids = 0.5 * (z[..., 1:] + z[..., :-1])
        upper = torch.cat([mids, z[..., -1:]], -1)
        lower = torch.cat([z[..., :1], mids], -1)
        z = lower + (upper - lower) * torch.rand(z.shape).to(upper)
    return z


def embed_view(ray_d, view_res):
    """if_clight_renderer.py:525-526 + embedder.py:9-35: [v, sin(2^k v), cos(2^k v)], k < view_res."""
    v = ray_d / torch.norm(ray_d, dim=-1, keepdim=True)
    out = [v]
    for k in range(view_res):
        out += [torch.sin(v * (2.0 ** k)), torch.cos(v * (2.0 ** k))]
    return torch.cat(out, -1)


# ---- encoder, painting, grouping ----------------------------------------------------------------------------------------
def _trunk_sites_have_batch_statistics(enc):
    """every BatchNorm site of the trunk is a train-mode nn.BatchNorm2d with a momentum: what th_bn_act_bwd is the backward of
    (eval mode normalises with the running statistics; SyncBatchNorm, after the reference trainer's conversion, with the
    statistics of all ranks: ``_trunk_sync_sites``)"""
    return all(isinstance(b, torch.nn.BatchNorm2d) and b.training and b.momentum is not None for b in enc._bn_sites())


def _trunk_sync_sites(enc):
    """every BatchNorm site is a train-mode BatchNorm2d or SyncBatchNorm with a momentum, and at least one is a SyncBatchNorm:
    the trunk th_bn_act_bwd_sums / _apply are the backward of at the converted sites"""
    sites = list(enc._bn_sites())
    return (all(isinstance(b, (torch.nn.BatchNorm2d, torch.nn.SyncBatchNorm)) and b.training and b.momentum is not None
                for b in sites) and any(isinstance(b, torch.nn.SyncBatchNorm) for b in sites))


def trunk_device(enc, images):
    """SpatialEncoder.trunk(images, fused_bn=False) (encoder.walk_trunk) on the per-site Functions of train_ops: the same torch
    operators in the forward, called without recording a graph -- or, under cfg.train_encoder_fwd = "device", k_encoder_fwd.hip
    (K29), th_bn_act and th_maxpool3x3s2 --, and k_encoder_bwd.hip in the backward (K23).  A trunk whose
    BatchNorm sites do not all use batch statistics runs under torch autograd as a whole; so does one with SyncBatchNorm sites,
    unless cfg.train_sync_bn = "device" (read only then), which runs them on train_ops.SyncBnActFn."""
    from .. import hip
    from . import train_ops as T
    from .encoder import walk_trunk
    _switch("train_encoder", "device", images.is_cuda)
    if not _trunk_sites_have_batch_statistics(enc):
        if not (_trunk_sync_sites(enc) and _sync_bn_mode(getattr(get_cfg(), "train_sync_bn", TRAIN_SYNC_BN[0])) == "device"):
            return enc.trunk(images, fused_bn=False)
    encoder_fwd_mode()                                       # (a bad value raises here, before the first site)

    def conv_bn(conv, bn, t, residual=None, relu=True):
        if conv.bias is not None:
            raise hip.HipError("cfg.train_encoder = 'device': the trunk's convolutions have no bias in the HIP backward")
        site = T.SyncBnActFn if isinstance(bn, torch.nn.SyncBatchNorm) else T.BnActFn
        return site.apply(T.ConvFn.apply(t, conv.weight, conv.stride[0]), bn, residual, relu, bn.weight, bn.bias)

    return walk_trunk(enc.model, images, conv_bn, T.MaxPoolFn.apply)


def _trunk(enc, images, encoder):
    if _switch("train_encoder", encoder, images.is_cuda) == "device":
        return trunk_device(enc, images)
    return enc.trunk(images, fused_bn=False)


def encode(enc, images, encoder="torch"):
    """SpatialEncoder.forward (encoder.py:97-155) through torch's own modules (autograd); encoder = "device": the trunk through
    ``trunk_device``."""
    H, W = images.shape[2:]
    lat = _trunk(enc, images, encoder)
    lat = [F.interpolate(l, (H, W), mode="bilinear", align_corners=True) for l in lat]
    pix = torch.cat(lat + [enc.upsample_color(images)], dim=1)
    return enc.reduction_layer(pix), pix


def latent_features(enc, images, cams, scale, encoder="torch", gather_bwd="atomic"):
    """cfg.train_maps = "latents": the trunk as in ``encode`` (stock modules; torch autograd, or ``trunk_device``), each latent
    channels-last once; returns ``gather(points [N,3]) -> [N,V,384]``, the rows ``sample_map(pix, ...)`` would give (K19);
    ``gather_bwd``: the form of its adjoint (cfg.train_gather_bwd)"""
    from . import train_ops
    gather_bwd = _switch("train_gather_bwd", gather_bwd, True)         # (the key has no CPU refusal of its own)
    lat = [l.permute(0, 2, 3, 1).contiguous() for l in _trunk(enc, images, encoder)]
    lift = enc.upsample_color
    return lambda pts: train_ops.LatentGatherFn.apply(*lat, lift.weight, lift.bias, images, pts, cams, scale, gather_bwd)


def project(x, R, T, K):
    """x [N,3] -> uv [V,N,2] (if_clight_renderer.py:123-126, :228-232)."""
    cam = torch.einsum("vij,nj->vni", R, x) + T[:, None, :, 0]
    pix = torch.einsum("vij,vnj->vni", K, cam)
    return pix[..., :2] / pix[..., 2:]


def sample_map(feat, uv, enc, image_shape):
    """sample_from_feature_map (:186-208): grid_sample, bilinear, align_corners, border.  feat [V,C,H,W] -> [V,C,N]."""
    from .. import hip
    H, W = feat.shape[2:]
    scale = hip.feat_scale(enc.feat_scale(H, W), image_shape, feat.device)       # :193-195 (float64 divide, fp32 cast)
    g = (uv * scale - 1.0).unsqueeze(2)
    return F.grid_sample(feat, g, align_corners=True, mode="bilinear", padding_mode="border")[:, :, :, 0]


_pool_cache = {}


def pooling_matrix_cached(renderer, n_verts, device, dtype):
    """pooling_matrix of the renderer's clustering, built once per (renderer, device, dtype): the dense [N_c, 6890] matrix is
    a constant of the renderer, not of the call"""
    key = (id(renderer), int(n_verts), str(device), dtype)
    ent = _pool_cache.get(key)
    if ent is None or ent[0]() is not renderer:
        import weakref
        if len(_pool_cache) > 16:
            _pool_cache.clear()
        ent = (weakref.ref(renderer), pooling_matrix(renderer.csr_offsets, renderer.csr_members, n_verts, device, dtype))
        _pool_cache[key] = ent
    return ent[1]


def pooling_matrix(offsets, members, n_verts, device, dtype):
    """voxelization (:356-371) as one matrix: row c holds 1 / |cluster c| at the cluster's vertices"""
    rows = torch.repeat_interleave(torch.arange(len(offsets) - 1), torch.as_tensor(offsets[1:] - offsets[:-1]))
    cols = torch.as_tensor(members, dtype=torch.long)
    M = torch.zeros((len(offsets) - 1, n_verts), dtype=dtype)
    M[rows, cols] = 1.0
    return (M / M.sum(1, keepdim=True)).to(device)


# ---- TransHE -------------------------------------------------------------------------------------------------------------
def _torch_attention(qkv, heads, scale):
    """softmax(q k^T scale) v of a block from its qkv rows [V,N,3C] as torch operators -> [V,N,C]"""
    V, N, C3 = qkv.shape
    qkv = qkv.reshape(V, N, 3, heads, C3 // 3 // heads).permute(2, 0, 3, 1, 4)
    s = (qkv[0] @ qkv[1].transpose(-2, -1)) * scale
    return (s.softmax(dim=-1) @ qkv[2]).transpose(1, 2).reshape(V, N, C3 // 3)


def _layer_norm(x, w, b, eps):
    return F.layer_norm(x, w.shape, w, b, eps)


def _vit_ops(dense):
    """the four operators vit_forward is composed from: the modules' own torch operators, or the HIP Functions of train_ops"""
    if dense == "device":
        from . import train_ops as T
        return {"norm_linear": T.NormLinearFn.apply, "linear": T.LinearFn.apply, "gelu_linear": T.GeluLinearFn.apply,
                "layernorm": T.LayerNormFn.apply}
    return {"norm_linear": lambda x, lw, lb, W, b, eps: F.linear(_layer_norm(x, lw, lb, eps), W, b), "linear": F.linear,
            "gelu_linear": lambda u, W, b: F.linear(F.gelu(u), W, b), "layernorm": _layer_norm}


def _device_attention(qkv, heads, scale):
    """_torch_attention's result through train_ops.AttentionFn (the kernels have the blocks' own scale, 1 / 8, built in)"""
    from . import train_ops
    return train_ops.AttentionFn.apply(qkv, heads)


def vit_forward(vit, x, pe_xyz, attention="torch", dense="torch"):
    """VisionTransformer.forward (vision_transformer.py:257-307, :362-383), mask = None.  attention = "device": every block's
    softmax(q k^T / 8) v through train_ops.AttentionFn (HIP forward and backward, no N x N tensor) instead of torch operators.
    dense = "device": every dense layer, LayerNorm and GELU through the HIP Functions of train_ops (k_vit_dense_bwd.hip)."""
    attention = _switch("train_attention", attention, True)          # (both values are checked before either refusal)
    dense = _switch("train_vit_dense", dense, x.is_cuda, "tokens")
    _switch("train_attention", attention, x.is_cuda, "tokens")
    ops = _vit_ops(dense)
    attend = _device_attention if attention == "device" else _torch_attention
    x = x + vit.get_PE(pe_xyz).to(x.dtype)
    if dense == "device":
        x = x.contiguous()                       # (the HIP Functions take contiguous rows; the sum keeps the strides of the pooled tokens)
    for blk in vit.blocks:
        a, m = blk.attn, blk.mlp
        qkv = ops["norm_linear"](x, blk.norm1.weight, blk.norm1.bias, a.qkv.weight, a.qkv.bias, blk.norm1.eps)
        # (for the HIP Functions again: neither call copies here, a Linear's rows and _torch_attention's reshape are contiguous)
        y = attend(qkv.contiguous(), vit.num_heads, a.scale).contiguous()
        x = x + ops["linear"](y, a.proj.weight, a.proj.bias)
        u = ops["norm_linear"](x, blk.norm2.weight, blk.norm2.bias, m.fc1.weight, m.fc1.bias, blk.norm2.eps)
        x = x + ops["gelu_linear"](u, m.fc2.weight, m.fc2.bias)
    return ops["layernorm"](x, vit.norm.weight, vit.norm.bias, vit.norm.eps)


# ---- per-point network ---------------------------------------------------------------------------------------------------
def _lin(mod, x):
    """a Conv1d(k = 1) applied to rows: x [..., in] -> [..., out]"""
    return F.linear(x, mod.weight.reshape(mod.weight.shape[0], -1), mod.bias)


def human_representation(net, pts_s, centres, rot, tokens, K, alpha):
    """get_human_representation (cross_transformer.py:158-205) -> [P,V,195 + 6 KNN_FREQ] (255 at the default 10 octaves)"""
    d2 = ((pts_s[:, None, :] - centres[None]) ** 2).sum(-1)
    d2k, idx = torch.topk(d2, K, dim=1, largest=False)
    w = F.softmax(-d2k.clamp_min(0).sqrt() / alpha, dim=1)
    rel = pts_s[:, None, :] - centres[idx]
    de = torch.matmul(rel.unsqueeze(-2), rot[idx]).squeeze(-2)
    pe = net.PE_relative(de.reshape(-1, 3)).view(pts_s.shape[0], K, -1)
    out = [torch.sum(w.unsqueeze(-1) * torch.cat([tokens[v][idx], pe], -1), dim=1) for v in range(tokens.shape[0])]
    return torch.stack(out, dim=1)


def point_network(net, h, f, viewdir):
    """MLP_forward_ori (cross_transformer.py:273-353): h [P,V,255], f [P,V,384], viewdir [P,27] -> raw [P,4]"""
    V = h.shape[1]
    s = F.relu(_lin(net.fc_0, h))
    p = F.relu(_lin(net.alpha_res_0, f))
    kp, vp = _lin(net.spatial_key_value_0.key_embed, p), _lin(net.spatial_key_value_0.value_embed, p)
    ks, vs = _lin(net.spatial_key_value_1.key_embed, s), _lin(net.spatial_key_value_1.value_embed, s)
    A = F.softmax(torch.einsum("pjc,pic->pji", kp, ks) / math.sqrt(kp.shape[-1]), dim=1)          # :141-144
    n = vs + torch.einsum("pjc,pji->pic", vp, A)
    inter = F.relu(_lin(net.fc_2, F.relu(_lin(net.fc_1, n))))
    sigma = _lin(net.alpha_fc, F.relu(_lin(net.fc_3, inter.mean(dim=1))))
    feat = _lin(net.feature_fc, inter) + _lin(net.rgb_res_0, f)
    feat = torch.cat([feat, viewdir[:, None, :].expand(-1, V, -1)], dim=-1)
    c = F.relu(_lin(net.view_fc, feat)) + _lin(net.rgb_res_1, f)
    rgb = _lin(net.rgb_fc, F.relu(_lin(net.fc_4, c.mean(dim=1))))
    return torch.cat([rgb, sigma], dim=1)


def _point_net_device_ops():
    """the three operators point_network_device is composed from, on the HIP Functions of train_ops"""
    from . import train_ops as T
    return {"linear": T.LinearFn.apply, "relu_linear": T.ReluLinearFn.apply, "xattn": T.CrossViewAttentionFn.apply}


def point_network_torch_ops():
    """the same three operators as plain torch (any dtype, any device): what point_network_device computes, for the tests"""
    def xattn(kvp, kvs):
        A = F.softmax(torch.einsum("pjc,pic->pji", kvp[..., :128], kvs[..., :128]) / math.sqrt(128), dim=1)
        return kvs[..., 128:] + torch.einsum("pjc,pji->pic", kvp[..., 128:], A)
    return {"linear": F.linear, "relu_linear": lambda a, W, b: F.relu(F.linear(a, W, b)), "xattn": xattn}


def point_network_device(net, h, f, viewdir, ops=None):
    """point_network (same arguments, same result) as th_mlp_forward composes it (k_mlp.hip): one GEMM per layer with the ReLU
    in its epilogue, the key and value embeddings of a branch as one 384-row layer, the cross-view attention as one kernel.
    h is [P,V,195 + 6 KNN_FREQ] or K4's zero-padded [P,V,256] row.  The GEMMs take multiples of 16: the odd layers are padded with zeros here,
    by differentiable operators, so autograd slices the gradients of the Parameters back.  ``ops``: the three operators
    (default: the HIP Functions of train_ops)."""
    ops = ops or _point_net_device_ops()
    lin, rlin = ops["linear"], ops["relu_linear"]
    w = lambda m: m.weight.reshape(m.weight.shape[0], -1)
    P, V = f.shape[:2]
    n_in = net.fc_0.weight.shape[1]                                # 195 + 6 KNN_FREQ
    if h.shape[-1] == n_in:
        h = F.pad(h, (0, 256 - n_in))
    h, f = h.contiguous(), f.contiguous()
    kv0, kv1 = net.spatial_key_value_0, net.spatial_key_value_1
    s = rlin(h, F.pad(w(net.fc_0), (0, 256 - n_in)), net.fc_0.bias)                             # 195 + 6 F -> 256 columns
    p = rlin(f, w(net.alpha_res_0), net.alpha_res_0.bias)
    kvp = lin(p, torch.cat([w(kv0.key_embed), w(kv0.value_embed)]), torch.cat([kv0.key_embed.bias, kv0.value_embed.bias]))
    kvs = lin(s, torch.cat([w(kv1.key_embed), w(kv1.value_embed)]), torch.cat([kv1.key_embed.bias, kv1.value_embed.bias]))
    n = ops["xattn"](kvp, kvs)
    inter = rlin(rlin(n, w(net.fc_1), net.fc_1.bias), w(net.fc_2), net.fc_2.bias)
    a = rlin(inter.mean(dim=1), w(net.fc_3), net.fc_3.bias)
    sigma = lin(a, F.pad(w(net.alpha_fc), (0, 0, 0, 15)), F.pad(net.alpha_fc.bias, (0, 15)))[:, :1]       # 1 -> 16 rows
    feat = lin(inter, w(net.feature_fc), net.feature_fc.bias) + lin(f, w(net.rgb_res_0), net.rgb_res_0.bias)
    feat = torch.cat([feat, viewdir[:, None, :].expand(-1, V, -1), feat.new_zeros((P, V, 5))], dim=-1)    # 283 -> 288 columns
    c = rlin(feat, F.pad(w(net.view_fc), (0, 5)), net.view_fc.bias) + lin(f, w(net.rgb_res_1), net.rgb_res_1.bias)
    c = rlin(c.mean(dim=1), w(net.fc_4), net.fc_4.bias)
    rgb = lin(c, F.pad(w(net.rgb_fc), (0, 0, 0, 13)), F.pad(net.rgb_fc.bias, (0, 13)))[:, :3]              # 3 -> 16 rows
    return torch.cat([rgb, sigma], dim=1)


def composite(raw, z, ray_d, raw_noise_std, white_bkgd):
    """raw2outputs (nerf_net_utils.py:14-59)"""
    d = torch.cat([z[..., 1:] - z[..., :-1], torch.full_like(z[..., :1], 1e10)], -1)
    d = d * torch.norm(ray_d[..., None, :], dim=-1)
    noise = torch.randn(raw[..., 3].shape).to(raw) * raw_noise_std if raw_noise_std > 0.0 else 0.0
    a = 1.0 - torch.exp(-F.relu(raw[..., 3] + noise) * d)
    T = torch.cumprod(torch.cat([torch.ones_like(a[:, :1]), 1.0 - a + 1e-10], -1), -1)[:, :-1]
    w = a * T
    rgb = torch.sum(w[..., None] * torch.sigmoid(raw[..., :3]), -2)
    acc = torch.sum(w, -1)
    if white_bkgd:
        rgb = rgb + (1.0 - acc[..., None])
    return rgb, acc, torch.sum(w * z, -1)


# ---- cfg.use_truncation --------------------------------------------------------------------------------------------------
class _Truncation:
    """the kept samples of a step: ``index`` selects their rows from a [P, ...] tensor, ``scatter`` puts raw rows back"""
    def __init__(self, index, n, scatter):
        self.index, self.n, self.scatter = index, n, scatter


def truncation_lists(pts_s, centres, sigma, mode):
    """mask_preserve = knn_dist.min(-1) < cfg.KNN_SIGMA (cross_transformer.py:175-180) over all samples, compared in fp32 like the
    reference.  mode "device": K27 (hip.truncate_select; the scatter is train_ops.TruncScatterFn); "torch": the same fp32
    expressions as torch operators, a boolean index (any device)."""
    if mode == "device":
        from .. import hip
        from . import train_ops
        mask, sel, n = hip.truncate_select(pts_s, centres, sigma)
        return _Truncation(sel.long(), n, lambda rows, P: train_ops.TruncScatterFn.apply(rows.contiguous(), mask, sel))
    keep = []
    for p in pts_s.split(32768):
        d = p[:, None, :] - centres[None]
        d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
        keep.append((d2 + d[..., 2] * d[..., 2]).min(1)[0].sqrt() < torch.tensor(sigma, dtype=p.dtype, device=p.device))
    keep = torch.cat(keep)

    def scatter(rows, P):
        full = rows.new_zeros((P, rows.shape[1]))
        full[keep] = rows                                          # raw[:, mask_preserve, :] = raw_preserved, :256-257
        return full
    return _Truncation(keep, int(keep.sum()), scatter)


# ---- the entry -------------------------------------------------------------------------------------------------------------
def render(renderer, batch, chunk=32768):
    """Renderer.render -> _render (if_clight_renderer.py:486-605) with pts_mask = None: every sample of every ray through
    the network, RGB everywhere.  Differentiable with respect to every parameter of ``renderer.net``."""
    cfg = get_cfg()
    net = renderer.net
    assert cfg.time_steps == 1
    ray_o, ray_d = batch["ray_o"][0], batch["ray_d"][0]

    def read(key, on_device=ray_o.is_cuda):
        return _switch(key, getattr(cfg, key, TRAIN_SWITCHES[key][0]), on_device)

    mode, attention, dense = read("train_kernels"), read("train_attention"), read("train_vit_dense")
    # train_gather_bwd: read with "latents" only, no CPU refusal of its own, its value checked before train_maps' refusal
    maps = read("train_maps", True)
    gather_bwd = read("train_gather_bwd", True) if maps == "latents" else "atomic"
    _switch("train_maps", maps, ray_o.is_cuda)
    point_net, encoder = read("train_point_net"), read("train_encoder")
    near, far = batch["near"][0], batch["far"][0]
    dev = ray_o.device
    S = int(cfg.N_samples)
    z = sample_depths(near, far, S, float(getattr(cfg, "perturb", 0.0)) > 0.0 and net.training)
    xyz = (ray_o[:, None] + ray_d[:, None] * z[..., None]).reshape(-1, 3)
    pts_s = torch.matmul(xyz - batch["Th"][0].reshape(1, 3), batch["Rh"][0])                    # world2smpl :289-295
    viewdir = embed_view(ray_d, int(getattr(cfg, "view_res", 4)))[:, None, :].expand(-1, S, -1).reshape(-1, 27)

    images = batch["input_imgs"][0].reshape(-1, *batch["input_imgs"][0].shape[2:])
    V = images.shape[0]
    R_in, T_in, K_in = (batch[k][0].reshape(V, *sh) for k, sh in (("input_R", (3, 3)), ("input_T", (3, 1)), ("input_K", (3, 3))))
    image_shape = batch["input_imgs"][0].shape[-2:]
    verts_in = batch["input_smpl_vertice"][0][0]
    nv = verts_in.shape[0]
    M = pooling_matrix_cached(renderer, nv, dev, torch.float32)
    centres = M @ batch["tar_smpl_vertice_smplcoord"][0]
    # cfg.use_truncation (cross_transformer.py:175-180, :247-264): the mask over all P samples once; K4, the pixel rows and the
    # per-point network then see the kept rows only, raw is scattered back in front of the noise and the compositor
    P_all, trunc = xyz.shape[0], None
    sigma = sigma_in_force(cfg)
    if sigma > 0.0:
        trunc = truncation_lists(pts_s, centres, sigma, mode)
        xyz, pts_s, viewdir = xyz[trunc.index], pts_s[trunc.index], viewdir[trunc.index]
    if maps == "latents":
        from .. import hip
        # a 1 x 1 convolution commutes with bilinear sampling: reduction_layer on the gathered rows (k_encoder.hip does the same)
        gather = latent_features(net.encoder, images, hip.pack_cams(R_in, T_in, K_in),
                                 hip.feat_scale(net.encoder.feat_scale(*images.shape[2:]), image_shape, dev), encoder=encoder,
                                 gather_bwd=gather_bwd)
        painted = _lin(net.encoder.reduction_layer, gather(verts_in)).permute(1, 0, 2)
        f_lat = gather(xyz) if xyz.shape[0] > 0 else None  # once over all (kept) samples, split per chunk below
    else:
        hol, pix = encode(net.encoder, images, encoder=encoder)
        painted = sample_map(hol, project(verts_in, R_in, T_in, K_in), net.encoder, image_shape).permute(0, 2, 1)
    if cfg.rasterize:
        painted = painted * batch["input_vizmaps"][0][0][..., None].to(painted.dtype)              # :181-182
    tokens = vit_forward(net.ViT, torch.einsum("cn,vnd->vcd", M, painted), renderer._pe_norm(V, dev),
                         attention=attention, dense=dense)
    blend = batch["blend_mtx"][0]
    M64 = pooling_matrix_cached(renderer, nv, dev, blend.dtype)        # (float64 mean, :544)
    rot = (M64 @ blend.reshape(nv, 16)).reshape(-1, 4, 4)[:, :3, :3].to(torch.float32)             # cross_transformer.py:185

    # chosen once: the per-chunk providers of the pixel rows f and the token rows h, the point network, the compositor
    chunks = [slice(s0, s0 + chunk) for s0 in range(0, xyz.shape[0], chunk)]       # batchify_rays :607-656 without a mask
    shade = point_network_device if point_net == "device" else point_network
    dparf = params_in_force(net, cfg)                              # (cfg.KNN, the network's octave count, cfg.KNN_DIST_ALPHA), read per call
    check_centres(dparf[0], centres.shape[0])
    if mode == "device":
        from .. import hip
        from . import train_ops
        hip.set_dparf(*dparf, dev)                                 # cfg.KNN / KNN_FREQ / KNN_DIST_ALPHA in force: K4 and K17 follow the context
        # K5 and K4 once over all (kept) samples: one map-sized gradient per step, nothing of the blends kept for backward
        fs = hs = ()
        if chunks:                                                 # (none: cfg.use_truncation dropped every sample)
            if maps != "latents":
                scale = hip.feat_scale(net.encoder.feat_scale(*pix.shape[2:]), image_shape, dev)
                f_lat = train_ops.PixelGatherFn.apply(pix.permute(0, 2, 3, 1).contiguous(), xyz, hip.pack_cams(R_in, T_in, K_in),
                                                      scale)
            fs = f_lat.split(chunk)
            hs = train_ops.HumanRepresentationFn.apply(tokens.contiguous(), pts_s, centres, rot).split(chunk)
            if point_net != "device":
                hs = (h[..., :195 + 6 * dparf[1]] for h in hs)     # (K4's rows are zero padded to 256 columns, point_network_device takes them)
        compose = lambda raw: train_ops.CompositeFn.apply(raw.contiguous(), z, ray_d, bool(cfg.white_bkgd))
    else:
        if maps == "latents":
            fs = (f_lat[c] for c in chunks)
        else:
            fs = (sample_map(pix, project(xyz[c], R_in, T_in, K_in), net.encoder, image_shape).permute(2, 0, 1) for c in chunks)
        hs = (human_representation(net, pts_s[c], centres, rot, tokens, dparf[0], dparf[2]) for c in chunks)
        compose = lambda raw: composite(raw, z, ray_d, 0.0, bool(cfg.white_bkgd))

    raws = [shade(net, h, f, viewdir[c]) for f, h, c in zip(fs, hs, chunks)]       # (the generators run chunk by chunk)
    raw = torch.cat(raws, 0) if raws else xyz.new_zeros((0, 4))    # (no kept sample: the reference's else branch, :258-260)
    if trunc is not None:
        raw = trunc.scatter(raw, P_all)
    raw = raw.view(-1, S, 4)
    noise_std = float(getattr(cfg, "raw_noise_std", 0.0))
    if noise_std > 0.0:                                            # nerf_net_utils.py:39-44, drawn by torch
        noise = torch.randn(raw[..., 3].shape).to(raw) * noise_std
        raw = torch.cat([raw[..., :3], (raw[..., 3] + noise)[..., None]], -1)
    rgb, acc, depth = compose(raw)
    return {"rgb_map": rgb[None], "acc_map": acc[None], "depth_map": depth[None]}
