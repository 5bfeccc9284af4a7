"""The three non-GEMM stages around the per-point network, and TransHE's attention, as autograd Functions on the device (K17).

``cfg.train_kernels = "device"`` makes ``autograd_path.render`` run the token blend (K4), the pixel-aligned gather (K5) and
the compositing (K7) through the HIP forwards that the inference paths use, with their adjoints as HIP kernels
(k_dparf_bwd.hip, k_pixfeat_bwd.hip, k_composite.hip) instead of torch's index_add / grid_sample / cumprod backwards:

    HumanRepresentationFn   tokens [V,N_c,192]   -> rows [P,V,256]     gradient: tokens
    PixelGatherFn           map    [V,H,W,C]     -> rows [P,V,C]       gradient: map
    CompositeFn             raw    [R,S,4]       -> rgb, acc, depth    gradient: raw

``cfg.train_maps = "latents"`` replaces the encoder's tail -- upsample, concatenate, 1 x 1 reduction, sample -- by one gather
that reads the three latents and the images at the projected points (K19, k_latgather.hip): a bilinear sample of a bilinearly
upsampled latent is a linear combination of at most 3 x 3 of its texels, so neither full-size map nor its gradient exists:

    LatentGatherFn          lat0..2 [V,h,w,C], lift -> rows [P,V,384]  gradient: the latents, the lift    keeps rgb_s [P,V,4]

``cfg.train_gather_bwd = "ordered"`` gives that Function's backward without float atomics (k_latgather_ord.hip): a sort of the
(sample, view) pairs by map pixel, then every latent texel sums what reaches it in a fixed order; "atomic" is the default.

``cfg.train_attention = "device"`` does the same for the attention of every TransHE block:

    AttentionFn             qkv    [V,N,3 C]     -> [V,N,C]            gradient: qkv         (k_vit.hip / k_vit_bwd.hip)

``cfg.train_vit_dense = "device"`` does it for everything else inside TransHE: the dense layers, LayerNorm and GELU
(k_vit_dense_bwd.hip).  Each Function keeps only what cannot be recomputed -- LN(x) and gelu(u) are rebuilt inside the
weight-gradient kernel -- and returns the gradients of the Parameters themselves:

    NormLinearFn            x, ln_w, ln_b, W, b  -> Linear(LN(x))      keeps x          qkv, fc1
    GeluLinearFn            u, W, b              -> Linear(gelu(u))    keeps u          fc2
    LinearFn                a, W, b              -> Linear(a)          keeps a          proj (a is AttentionFn's saved output)
    LayerNormFn             x, w, b              -> LN(x)              keeps x          the final norm

``cfg.train_point_net = "device"`` does it for the per-point network (MLP_forward_ori), layer by layer like th_mlp_forward
(k_vit_dense_bwd.hip / k_pointnet_bwd.hip; composed by ``autograd_path.point_network_device`` from these two and
``LinearFn``):

    ReluLinearFn            a, W, b              -> relu(Linear(a))    keeps a, y       s, p, fc_1, fc_2, fc_3, view_fc, fc_4
    CrossViewAttentionFn    kvp, kvs [P,V,384]   -> n [P,V,256]        keeps kvp, kvs   gradient: both; A is recomputed

The loss the trainer back-propagates through (lib/train/trainers/if_nerf_clight.py:68-72; k_lpips.hip):

    LpipsFn                 in0, in1 [N,3,H,W]   -> LPIPS_vgg [N] float64  keeps in0 and the forward's state   gradient: in0

``cfg.train_encoder = "device"`` does it for the encoder trunk (SpatialEncoder.trunk, encoder.py:114-126): the forward of every
site is the stock torch operator, called without recording a graph, so the latents and the BatchNorm statistics are those of
the "torch" mode bit for bit; the backward is k_encoder_bwd.hip (composed by ``autograd_path.trunk_device``).
``cfg.train_encoder_fwd = "device"`` (read only then) makes the forwards HIP as well: th_conv2d_fwd32 (k_encoder_fwd.hip, K29),
th_bn_act and th_maxpool3x3s2; a SyncBatchNorm site keeps the module call for its BatchNorm:

    ConvFn                  x, W, stride         -> conv2d(x, W)       keeps x, W       gradient: x (not conv1's images), W
    BnActFn                 y, bn, residual, relu, gamma, beta -> relu(bn(y) + residual)   keeps y, the output (with a ReLU), gamma
    MaxPoolFn               x                    -> max_pool2d(x, 3, 2, 1)   keeps x
    SyncBnActFn             as BnActFn, `bn` a train-mode nn.SyncBatchNorm (cfg.train_sync_bn = "device"): the backward is split
                            around one all_gather of the ranks' [C, 6] float64 records (th_bn_act_bwd_sums / _apply)

K4 and K5 are linear in the tensor that gets the gradient, so nothing of the forward is kept for the backward but the
geometry (points, centres, cameras): the [P,7,255] blend operands and the per-chunk map-sized gradients of the torch
formulation do not exist here.  Points, centres, rotations, cameras, depths and ray directions come from the batch and get
no gradient; an input of that kind that asks for one raises.

Beside every kernel its float64 numpy restatement (``*_oracle``), tied to torch autograd through ``autograd_path`` by
tests/test_train_ops_host.py.
"""
import numpy as np
import torch

from .. import hip


def _no_grad_inputs(fn, **tensors):
    for name, t in tensors.items():
        if isinstance(t, torch.Tensor) and t.requires_grad:
            raise ValueError(f"{fn}: '{name}' comes from the batch and has no gradient path (requires_grad=True)")


def _on_device(fn, t):
    if not t.is_cuda:
        raise hip.HipError(f"{fn} needs its tensors on an MI355X (there is no CPU path)")


class HumanRepresentationFn(torch.autograd.Function):
    """get_human_representation (cross_transformer.py:158-205) -> [P,V,256] (195 + 6 KNN_FREQ features, zeros behind them).
    The gradient reaches the tokens only: columns 192.. (positional encoding of the point, pad) do not depend on them.
    cfg.KNN / KNN_FREQ / KNN_DIST_ALPHA are those of the device's context (hip.set_dparf); the backward runs under the
    forward's, whatever was set in between."""

    @staticmethod
    def forward(ctx, tokens, pts_smpl, centres, rot):
        _no_grad_inputs("HumanRepresentationFn", pts_smpl=pts_smpl, centres=centres, rot=rot)
        _on_device("HumanRepresentationFn", tokens)
        ctx.save_for_backward(pts_smpl, centres, rot)
        ctx.dparf = hip.dparf_in_force(tokens.device)
        return hip.dparf_encode(pts_smpl, centres, rot, tokens)

    @staticmethod
    def backward(ctx, grad_out):
        pts_smpl, centres, rot = ctx.saved_tensors
        hip.set_dparf(*ctx.dparf, grad_out.device)
        return hip.dparf_encode_bwd(pts_smpl, centres, rot, grad_out), None, None, None


class PixelGatherFn(torch.autograd.Function):
    """get_pixel_aligned_feature (if_clight_renderer.py:210-269) on the channels-last map -> [P,V,C]"""

    @staticmethod
    def forward(ctx, map_nhwc, pts_world, cams, scale_xy):
        _no_grad_inputs("PixelGatherFn", pts_world=pts_world, cams=cams, scale_xy=scale_xy)
        _on_device("PixelGatherFn", map_nhwc)
        if map_nhwc.dtype is not torch.float32 or not map_nhwc.is_contiguous():
            raise ValueError("PixelGatherFn: the map must be a contiguous float32 [V,H,W,C] tensor")
        ctx.save_for_backward(pts_world, cams, scale_xy)
        ctx.map_shape = tuple(map_nhwc.shape)
        return hip.pixel_gather(map_nhwc.detach(), pts_world, cams, scale_xy)

    @staticmethod
    def backward(ctx, grad_out):
        pts_world, cams, scale_xy = ctx.saved_tensors
        return hip.pixel_gather_bwd(ctx.map_shape, pts_world, cams, scale_xy, grad_out), None, None, None


class LatentGatherFn(torch.autograd.Function):
    """SpatialEncoder.forward's tail (encoder.py:133-146) + get_pixel_aligned_feature (if_clight_renderer.py:210-269) without the
    map between them: the channels-last latents lat0 [V,h0,w0,64], lat1 [V,h1,w1,64], lat2 [V,h2,w2,128] and the colour lift
    (upsample_color's weight [128,3(,1,1)] and bias) -> rows [P,V,384].  Kept for the backward: the geometry and the blended
    raw colours rgb_s [P,V,4] (the lift's weight gradient).  ``gather_bwd`` (cfg.train_gather_bwd): "atomic" (the default) adds
    onto the latent gradients with float atomics and reduces the lift's through torch; "ordered" computes all five with
    fixed-order sums (hip.latent_gather_bwd_ordered): bit-identical from run to run."""

    @staticmethod
    def forward(ctx, lat0, lat1, lat2, lift_w, lift_b, images, pts_world, cams, scale_xy, gather_bwd="atomic"):
        if gather_bwd not in ("atomic", "ordered"):
            raise ValueError(f"LatentGatherFn: gather_bwd must be 'atomic' or 'ordered', not {gather_bwd!r}")
        ctx.gather_bwd = gather_bwd
        _no_grad_inputs("LatentGatherFn", images=images, pts_world=pts_world, cams=cams, scale_xy=scale_xy)
        _on_device("LatentGatherFn", lat0)
        rows, rgb_s = hip.latent_gather(lat0.detach(), lat1.detach(), lat2.detach(), lift_w.detach(), lift_b.detach(), images,
                                        pts_world, cams, scale_xy)
        ctx.save_for_backward(pts_world, cams, scale_xy, rgb_s)
        ctx.shapes = (tuple(lat0.shape), tuple(lat1.shape), tuple(lat2.shape))
        ctx.image_hw = tuple(images.shape[2:])
        ctx.lift_w_shape = tuple(lift_w.shape)
        return rows

    @staticmethod
    def backward(ctx, grad_out):
        pts_world, cams, scale_xy, rgb_s = ctx.saved_tensors
        g = grad_out.contiguous()
        if ctx.gather_bwd == "ordered":
            g0, g1, g2, g_w, g_b = hip.latent_gather_bwd_ordered(ctx.shapes, ctx.image_hw, pts_world, cams, scale_xy, g,
                                                                 rgb_s=rgb_s)
            return g0, g1, g2, g_w.reshape(ctx.lift_w_shape), g_b, None, None, None, None, None
        g0, g1, g2 = hip.latent_gather_bwd(ctx.shapes, ctx.image_hw, pts_world, cams, scale_xy, g)
        # the lift: 128 x 3 + 128 numbers, one small reduction over the rows (not the hot path)
        gl = g[..., 256:384].reshape(-1, 128)
        g_w = (gl.t() @ rgb_s.reshape(-1, 4)[:, :3]).reshape(ctx.lift_w_shape)
        return g0, g1, g2, g_w, gl.sum(0), None, None, None, None, None


class CompositeFn(torch.autograd.Function):
    """raw2outputs (nerf_net_utils.py:14-59) -> rgb [R,3], acc [R], depth [R].  The density noise of training is added to
    raw[..., 3] by the caller (a torch op), not here."""

    @staticmethod
    def forward(ctx, raw, z, ray_d, white_bkgd):
        _no_grad_inputs("CompositeFn", z=z, ray_d=ray_d)
        _on_device("CompositeFn", raw)
        ctx.save_for_backward(raw, z, ray_d)
        ctx.white = bool(white_bkgd)
        return hip.composite(raw, z, ray_d, white_bkgd=ctx.white)

    @staticmethod
    def backward(ctx, g_rgb, g_acc, g_depth):
        raw, z, ray_d = ctx.saved_tensors
        zero = lambda g, shape: g if g is not None else torch.zeros(shape, dtype=torch.float32, device=raw.device)
        R = z.shape[0]
        return hip.composite_bwd(raw, z, ray_d, zero(g_rgb, (R, 3)), zero(g_acc, (R,)), zero(g_depth, (R,)), ctx.white), \
            None, None, None


class TruncScatterFn(torch.autograd.Function):
    """cfg.use_truncation (cross_transformer.py:256-257): the raw rows of the kept samples [P',4] back into all P samples, exact
    zeros elsewhere (K27); ``mask`` uint8 [P] and ``sel`` int32 [P'] from hip.truncate_select.  The adjoint is the gather g[sel]."""

    @staticmethod
    def forward(ctx, rows_kept, mask, sel):
        _on_device("TruncScatterFn", rows_kept)
        ctx.save_for_backward(sel)
        return hip.truncate_scatter(rows_kept, mask, sel)

    @staticmethod
    def backward(ctx, grad_rows):
        (sel,) = ctx.saved_tensors
        return hip.truncate_scatter_bwd(grad_rows.contiguous(), sel), None, None


class AttentionFn(torch.autograd.Function):
    """Attention.forward (vision_transformer.py:271-278) on the fused qkv layer's output: qkv [V,N,3 C] -> [V,N,C], through the
    attention kernels of the inference path (K3) with the backward of k_vit_bwd.hip.  Kept for the backward: qkv, the output
    and the rows' log-sum-exp [V,heads,N] -- nothing N x N, where torch autograd keeps the [V,heads,N,N] probabilities."""

    @staticmethod
    def forward(ctx, qkv, heads):
        _on_device("AttentionFn", qkv)
        if qkv.dtype is not torch.float32 or not qkv.is_contiguous():
            raise ValueError("AttentionFn: qkv must be a contiguous float32 [V,N,3 C] tensor")
        out, lse = hip.attention_train(qkv.detach(), int(heads))
        ctx.save_for_backward(qkv, out, lse)
        ctx.heads = int(heads)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        qkv, out, lse = ctx.saved_tensors
        return hip.attention_bwd(qkv, out, lse, grad_out.contiguous(), ctx.heads), None


def _dense_inputs(fn, **tensors):
    for name, t in tensors.items():
        _on_device(fn, t)
        if t.dtype is not torch.float32 or not t.is_contiguous():
            raise ValueError(f"{fn}: '{name}' must be a contiguous float32 tensor")


class _DenseFn(torch.autograd.Function):
    """act(Linear(op(a))) of one dense layer: th_linear_train_forward / th_linear_bwd with the operand form of the subclass, or,
    for a subclass with RELU, th_linear_relu_forward / th_linear_relu_bwd (which also keep the output y)"""
    FORM = 0
    RELU = False

    @classmethod
    def _fwd(cls, ctx, a, W, b, ln_w=None, ln_b=None, eps=1e-6):
        name = cls.__name__
        _dense_inputs(name, a=a, W=W, b=b, **({"ln_w": ln_w, "ln_b": ln_b} if ln_w is not None else {}))
        ctx.eps = float(eps)
        if cls.RELU:
            y = hip.linear_relu_forward(a.detach(), W.detach(), b.detach())
            ctx.save_for_backward(a, W, y)
            return y
        ctx.save_for_backward(a, W, *((ln_w, ln_b) if ln_w is not None else ()))
        return hip.linear_train_forward(a.detach(), W.detach(), b.detach(), cls.FORM, ln_w, ln_b, ctx.eps)

    @classmethod
    def _bwd(cls, ctx, grad_out):
        a, W, *rest = ctx.saved_tensors
        if cls.RELU:
            return hip.linear_relu_bwd(a, rest[0], W, grad_out.contiguous(), need_input=ctx.needs_input_grad[0])
        ln_w, ln_b = rest if rest else (None, None)
        return hip.linear_bwd(a, W, grad_out.contiguous(), cls.FORM, ln_w, ln_b, ctx.eps)


class LinearFn(_DenseFn):
    """nn.Linear on rows: a [..., in] -> [..., out].  Kept: a (for TransHE's proj the tensor AttentionFn keeps anyway)."""
    FORM = hip.OPERAND_PLAIN

    @staticmethod
    def forward(ctx, a, W, b):
        return LinearFn._fwd(ctx, a, W, b)

    @staticmethod
    def backward(ctx, grad_out):
        g_a, g_w, g_b, _, _ = LinearFn._bwd(ctx, grad_out)
        return g_a, g_w, g_b


class NormLinearFn(_DenseFn):
    """Linear(LayerNorm(x)) (Block.norm1 -> attn.qkv, Block.norm2 -> mlp.fc1; vision_transformer.py:296-306).  Kept: x -- the
    normalised rows are rebuilt, with the forward's statistics bit for bit, on their way into the weight-gradient kernel."""
    FORM = hip.OPERAND_LN

    @staticmethod
    def forward(ctx, x, ln_w, ln_b, W, b, eps=1e-6):
        return NormLinearFn._fwd(ctx, x, W, b, ln_w, ln_b, eps)

    @staticmethod
    def backward(ctx, grad_out):
        g_x, g_w, g_b, g_lw, g_lb = NormLinearFn._bwd(ctx, grad_out)
        return g_x, g_lw, g_lb, g_w, g_b, None


class GeluLinearFn(_DenseFn):
    """Linear(gelu(u)), exact erf (Mlp.act -> fc2).  Kept: u."""
    FORM = hip.OPERAND_GELU

    @staticmethod
    def forward(ctx, u, W, b):
        return GeluLinearFn._fwd(ctx, u, W, b)

    @staticmethod
    def backward(ctx, grad_out):
        g_u, g_w, g_b, _, _ = GeluLinearFn._bwd(ctx, grad_out)
        return g_u, g_w, g_b


class ReluLinearFn(_DenseFn):
    """relu(nn.Linear(a)) on rows: the ReLU is the GEMM's epilogue; the backward gates g_out by [y > 0] on its way into the
    weight-gradient kernel (th_linear_relu_forward / th_linear_relu_bwd).  Kept: a and the output y, which autograd keeps anyway."""
    FORM = hip.OPERAND_PLAIN
    RELU = True

    @staticmethod
    def forward(ctx, a, W, b):
        return ReluLinearFn._fwd(ctx, a, W, b)

    @staticmethod
    def backward(ctx, grad_out):
        return ReluLinearFn._bwd(ctx, grad_out)


class CrossViewAttentionFn(torch.autograd.Function):
    """cross_attention (cross_transformer.py:128-149) on the fused [key(128) | value(256)] rows of the pixel branch (kvp) and the
    token branch (kvs), [P,V,384] each -> n [P,V,256].  Kept: kvp and kvs; the V x V probabilities are recomputed."""

    @staticmethod
    def forward(ctx, kvp, kvs):
        _dense_inputs("CrossViewAttentionFn", kvp=kvp, kvs=kvs)
        ctx.save_for_backward(kvp, kvs)
        return hip.xview_attention(kvp.detach(), kvs.detach())

    @staticmethod
    def backward(ctx, grad_out):
        kvp, kvs = ctx.saved_tensors
        return hip.xview_attention_bwd(kvp, kvs, grad_out.contiguous())


def _encoder_fwd():
    """cfg.train_encoder_fwd through its checked reader: "torch" (the stock operators) or "device" (HIP forwards)"""
    from .autograd_path import encoder_fwd_mode
    return encoder_fwd_mode()


def _trunk_input(fn, name, t):
    _on_device(fn, t)
    if t.dtype is not torch.float32 or t.dim() != 4:
        raise ValueError(f"{fn}: '{name}' must be a float32 [N,C,H,W] tensor")


class ConvFn(torch.autograd.Function):
    """nn.Conv2d(cin, cout, ks, stride, ks // 2, bias=False) of the encoder trunk.  Forward: torch's own convolution (the call the
    module makes), or th_conv2d_fwd32 (K29) under cfg.train_encoder_fwd = "device".  Backward: th_conv2d_dgrad / th_conv2d_wgrad (fp32-input MFMA, fixed-order sums).  conv1 (7x7/2 on the images)
    has no input gradient: images that require one raise."""

    @staticmethod
    def forward(ctx, x, weight, stride):
        _trunk_input("ConvFn", "x", x)
        cout, cin, ks = int(weight.shape[0]), int(weight.shape[1]), int(weight.shape[2])
        have = hip.conv2d_bwd_supported(cin, cout, ks, stride)
        if not have & 1:
            raise hip.HipError(f"ConvFn: no HIP backward is built for a {ks}x{ks}/{stride} convolution {cin}->{cout}")
        if x.requires_grad and not have & 2:
            raise ValueError(f"ConvFn: 'x' requires a gradient, and a {ks}x{ks}/{stride} convolution {cin}->{cout} has no input "
                             "gradient here (the images come from the batch)")
        ctx.stride = int(stride)
        ctx.save_for_backward(x, weight)
        if _encoder_fwd() == "device":
            return hip.conv2d_fwd32(x.detach().contiguous(), weight.detach().contiguous(), int(stride))
        return torch.nn.functional.conv2d(x.detach(), weight.detach(), None, int(stride), ks // 2)

    @staticmethod
    def backward(ctx, grad_out):
        x, weight = ctx.saved_tensors
        g = grad_out.contiguous()
        xc = x.contiguous()
        ks = int(weight.shape[2])
        g_x = None
        if ctx.needs_input_grad[0]:
            g_x = hip.conv2d_dgrad(g, weight.shape, ctx.stride, xc.shape[2:], hip.conv2d_dgrad_image(weight, ctx.stride))
        g_w = hip.conv2d_wgrad(xc, g, ks, ctx.stride) if ctx.needs_input_grad[1] else None
        return g_x, g_w, None


class BnActFn(torch.autograd.Function):
    """The tail of a ``conv -> bn [-> += identity] [-> relu]`` site: relu(bn(y) + residual) with `bn` a train-mode
    nn.BatchNorm2d.  Forward: the stock module call (it updates the running statistics and num_batches_tracked as always), torch's
    add and ReLU; under cfg.train_encoder_fwd = "device" th_bn_act (K11: float64 statistics, the running statistics updated with the
    module's momentum) and num_batches_tracked incremented here.  Backward: th_bn_act_bwd from y, the output (the gate) and gamma.  ``gamma`` / ``beta`` are bn.weight / bn.bias
    (None without affine), passed so that autograd sees them."""

    @staticmethod
    def forward(ctx, y, bn, residual, relu, gamma, beta):
        _trunk_input("BnActFn", "y", y)
        if not (isinstance(bn, torch.nn.BatchNorm2d) and bn.training and bn.momentum is not None):
            raise ValueError("BnActFn: the backward is defined for a train-mode nn.BatchNorm2d with a momentum (batch statistics)")
        if _encoder_fwd() == "device":
            # th_bn_act writes a buffer of its own (y is kept for the backward) and updates running_mean / running_var
            out = hip.bn_act(y.detach().contiguous(), bn, None if residual is None else residual.detach(), bool(relu))
            if bn.track_running_stats and bn.num_batches_tracked is not None:
                bn.num_batches_tracked.add_(1)
        else:
            out = bn(y.detach())
            if residual is not None:
                out = out + residual.detach()
            if relu:
                out = torch.relu_(out)
        ctx.relu, ctx.eps, ctx.has_res = bool(relu), float(bn.eps), residual is not None
        ctx.save_for_backward(y, out if relu else None, gamma)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        y, out, gamma = ctx.saved_tensors
        g = grad_out.contiguous()
        need_res = ctx.has_res and ctx.needs_input_grad[2]
        g_y, g_res, g_gamma, g_beta = hip.bn_act_bwd(y.contiguous(), out, g, gamma, ctx.eps, need_residual=need_res and ctx.relu,
                                                     need_affine=gamma is not None)
        if need_res and not ctx.relu:
            g_res = g                                          # (no gate: the residual's gradient is the arriving one)
        return g_y, None, g_res, None, g_gamma, g_beta


def _bn_group(bn):
    """(torch.distributed or None, the group, world, rank) of a SyncBatchNorm: its process_group, the default one without"""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return None, None, 1, 0
    group = bn.process_group if bn.process_group is not None else dist.group.WORLD
    return dist, group, dist.get_world_size(group), dist.get_rank(group)


class SyncBnActFn(torch.autograd.Function):
    """BnActFn for a site whose ``bn`` is a train-mode nn.SyncBatchNorm.  Forward: the stock module call, made without a graph (it
    runs the module's own collective and updates the running statistics as always), torch's add and ReLU.  Backward:
    th_bn_act_bwd_sums over this rank's batch, ONE all_gather of the [C, 6] float64 record on bn.process_group (the list form on
    gloo, as torch's own SyncBatchNorm; skipped with one rank), th_bn_act_bwd_apply, which adds the ranks' sums in rank order.
    g_gamma / g_beta are the rank's local sums, as torch's SyncBatchNorm returns them: the gradient exchange averages them.
    ``calls`` counts the backward runs of the process."""

    calls = 0

    @staticmethod
    def forward(ctx, y, bn, residual, relu, gamma, beta):
        _trunk_input("SyncBnActFn", "y", y)
        if not (isinstance(bn, torch.nn.SyncBatchNorm) and bn.training and bn.momentum is not None):
            raise ValueError("SyncBnActFn: the backward is defined for a train-mode nn.SyncBatchNorm with a momentum (batch statistics)")
        out = bn(y.detach())
        if residual is not None:
            out = out + residual.detach()
        if relu:
            out = torch.relu_(out)
        ctx.relu, ctx.eps, ctx.has_res = bool(relu), float(bn.eps), residual is not None
        ctx.dist, ctx.group, ctx.world, ctx.rank = _bn_group(bn)
        ctx.save_for_backward(y, out if relu else None, gamma)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        y, out, gamma = ctx.saved_tensors
        g, yc = grad_out.contiguous(), y.contiguous()
        record = hip.bn_act_bwd_sums(yc, out, g)
        if ctx.world == 1:
            records = record[None]
        elif ctx.dist.get_backend(ctx.group) == "gloo":
            parts = [torch.empty_like(record) for _ in range(ctx.world)]
            ctx.dist.all_gather(parts, record, group=ctx.group)
            records = torch.stack(parts)
        else:
            records = record.new_empty((ctx.world, *record.shape))
            ctx.dist.all_gather_into_tensor(records, record, group=ctx.group)
        need_res = ctx.has_res and ctx.needs_input_grad[2]
        g_y, g_res, g_gamma, g_beta = hip.bn_act_bwd_apply(yc, out, g, gamma, ctx.eps, records, ctx.rank,
                                                           need_residual=need_res and ctx.relu, need_affine=gamma is not None)
        if need_res and not ctx.relu:
            g_res = g                                          # (no gate: the residual's gradient is the arriving one)
        SyncBnActFn.calls += 1
        return g_y, None, g_res, None, g_gamma, g_beta


def sync_bn_act_bwd_oracle(ys, outs, gs, gamma, eps):
    """th_bn_act_bwd_sums / _apply in float64 numpy.  ys, outs, gs: per rank, y [N_r,C,H,W], the site's output (None: no ReLU) and
    the arriving gradient; gamma [C] or None -> per rank (g_y, g', g_gamma, g_beta), g' the gated gradient (the residual's) and
    g_gamma / g_beta the rank's LOCAL sums.  The sums are taken against each rank's own pivot and moved to rank 0's in rank order,
    as the kernels do."""
    recs, gates = [], []
    for y, out, g in zip(ys, outs, gs):
        y, g = _np64(y), _np64(g)
        gp = g if out is None else g * (_np64(out) > 0)
        p = y[0, :, 0, 0]
        d = y - p[None, :, None, None]
        recs.append((d.sum((0, 2, 3)), (d * d).sum((0, 2, 3)), gp.sum((0, 2, 3)), (gp * d).sum((0, 2, 3)), p,
                     float(y.shape[0] * y.shape[2] * y.shape[3])))
        gates.append(gp)
    p0 = recs[0][4]
    A0, A1, A2, A3, L = recs[0][0].copy(), recs[0][1].copy(), recs[0][2].copy(), recs[0][3].copy(), recs[0][5]
    for a0, a1, a2, a3, p, Lr in recs[1:]:
        d = p - p0
        A0 += a0 + Lr * d
        A1 += (a1 + (2.0 * d) * a0) + (Lr * d) * d
        A2 += a2
        A3 += a3 + d * a2
        L += Lr
    m = A0 / L
    invstd = 1.0 / np.sqrt(np.maximum(A1 / L - m * m, 0.0) + eps)
    mg, mx = A2 / L, (A3 - m * A2) * invstd / L
    k = (1.0 if gamma is None else _np64(gamma)) * invstd
    res = []
    for (a0, a1, a2, a3, p, Lr), y, gp in zip(recs, ys, gates):
        ml = m - (p - p0)
        sh = (None, slice(None), None, None)
        xhat = ((_np64(y) - p[sh]) - ml[sh]) * invstd[sh]
        res.append((k[sh] * ((gp - mg[sh]) - xhat * mx[sh]), gp, (a3 - ml * a2) * invstd, a2))
    return res


class MaxPoolFn(torch.autograd.Function):
    """nn.MaxPool2d(3, 2, 1).  Forward: torch's, or th_maxpool3x3s2 under cfg.train_encoder_fwd = "device".  Backward: th_maxpool3x3s2_bwd, which finds the element torch recorded again from
    the input (nothing but the input is kept)."""

    @staticmethod
    def forward(ctx, x):
        _trunk_input("MaxPoolFn", "x", x)
        ctx.save_for_backward(x)
        if _encoder_fwd() == "device":
            return hip.maxpool3x3s2(x.detach().contiguous())
        return torch.nn.functional.max_pool2d(x.detach(), 3, 2, 1)

    @staticmethod
    def backward(ctx, grad_out):
        (x,) = ctx.saved_tensors
        return hip.maxpool3x3s2_bwd(x.contiguous(), grad_out.contiguous())


class LayerNormFn(torch.autograd.Function):
    """nn.LayerNorm over the last dimension (VisionTransformer.norm).  Kept: x."""

    @staticmethod
    def forward(ctx, x, w, b, eps=1e-6):
        _dense_inputs("LayerNormFn", x=x, w=w, b=b)
        ctx.eps = float(eps)
        ctx.save_for_backward(x, w)
        return hip.layernorm_train_forward(x.detach(), w.detach(), b.detach(), ctx.eps)

    @staticmethod
    def backward(ctx, grad_out):
        x, w = ctx.saved_tensors
        return (*hip.layernorm_bwd(x, w, grad_out.contiguous(), ctx.eps), None)


class LpipsFn(torch.autograd.Function):
    """LPIPS (VGG16, v0.1) of in0 against in1, [N,3,H,W] in [-1, 1] -> float64 [N], through th_lpips_train with the backward of
    th_lpips_bwd.  ``packed`` / ``packed_bwd``: the images of hip.lpips_pack / hip.lpips_pack_bwd.  Kept for the backward: in0 and
    the forward's state (every layer's output).  in1 is the target and the weights are frozen: only in0 gets a gradient, in its
    own dtype; an in1 that asks for one raises."""

    @staticmethod
    def forward(ctx, in0, in1, packed, packed_bwd):
        if in1.requires_grad:
            raise NotImplementedError("LpipsFn: only in0 has a gradient path (in1 is the target; it requires grad)")
        _on_device("LpipsFn", in0)
        out, state = hip.lpips_train(in0.detach(), in1, packed)
        ctx.save_for_backward(in0, state, packed, packed_bwd)
        return out[:, 5].contiguous()

    @staticmethod
    def backward(ctx, grad_out):
        in0, state, packed, packed_bwd = ctx.saved_tensors
        return hip.lpips_bwd(grad_out, in0, state, packed, packed_bwd).to(in0.dtype), None, None, None


# ---- float64 restatements ---------------------------------------------------------------------------------------------------
def _np64(x):
    return np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x, dtype=np.float64)


def dparf_neighbours_oracle(pts_smpl, centres, K=7, alpha=0.5):
    """get_dist_weight (cross_transformer.py:151-156, :170): the K nearest centres by squared distance (ties: lower index)
    and softmax(-d / alpha) -> idx [P,K] int64, w [P,K] float64"""
    p, c = _np64(pts_smpl), _np64(centres)
    d2 = ((p[:, None, :] - c[None]) ** 2).sum(-1)
    idx = np.argsort(d2, axis=1, kind="stable")[:, :K]
    d = np.sqrt(np.take_along_axis(d2, idx, axis=1))
    e = np.exp(-(d - d.min(1, keepdims=True)) / alpha)
    return idx, e / e.sum(1, keepdims=True)


def dparf_token_grad_oracle(pts_smpl, centres, n_views, grad_out, K=7, alpha=0.5):
    """adjoint of the token blend: grad_out [P,V,>=192] -> grad_tokens [V,N_c,192] (float64)"""
    g = _np64(grad_out)[..., :192]
    idx, w = dparf_neighbours_oracle(pts_smpl, centres, K, alpha)
    out = np.zeros((n_views, _np64(centres).shape[0], 192))
    for v in range(n_views):
        for k in range(idx.shape[1]):
            np.add.at(out[v], idx[:, k], w[:, k, None] * g[:, v])
    return out


def pixel_map_grad_oracle(uv, scale_xy, H, W, grad_out):
    """adjoint of sample_from_feature_map (if_clight_renderer.py:186-208: grid_sample, bilinear, align_corners, border) with
    respect to the map: uv [V,N,2] pixel coordinates, scale_xy [2], grad_out [N,V,C] -> grad_map [V,H,W,C] (float64)"""
    uv, s, g = _np64(uv), _np64(scale_xy), _np64(grad_out)
    V, N = uv.shape[:2]
    out = np.zeros((V, H, W, g.shape[-1]))
    gx, gy = uv[..., 0] * s[0] - 1.0, uv[..., 1] * s[1] - 1.0
    ix = np.clip(((gx + 1.0) / 2.0) * (W - 1), 0.0, W - 1.0)
    iy = np.clip(((gy + 1.0) / 2.0) * (H - 1), 0.0, H - 1.0)
    x0, y0 = np.floor(ix), np.floor(iy)
    x1, y1 = x0 + 1.0, y0 + 1.0
    for xs, ys, wt in ((x0, y0, (x1 - ix) * (y1 - iy)), (x1, y0, (ix - x0) * (y1 - iy)),
                       (x0, y1, (x1 - ix) * (iy - y0)), (x1, y1, (ix - x0) * (iy - y0))):
        ok = (xs <= W - 1) & (ys <= H - 1)                                   # (a corner outside the map adds nothing)
        xi, yi = np.minimum(xs, W - 1).astype(np.int64), np.minimum(ys, H - 1).astype(np.int64)
        for v in range(V):
            np.add.at(out[v], (yi[v], xi[v]), (wt[v] * ok[v])[:, None] * g[:, v])
    return out


def _upsample_taps64(n_out, n_in):
    """upsample_bilinear2d(align_corners=True) along one axis: src = dst (in - 1) / (out - 1) -> i0, i1 [out] int64 and
    l0, l1 [out] float64 (ups_coord of th_internal.h in float64)"""
    scale = (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
    src = scale * np.arange(n_out, dtype=np.float64)
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    l1 = src - i0
    return i0, i1, 1.0 - l1, l1


def _grid_corners64(uv, scale_xy, H, W):
    """grid_sample (bilinear, align_corners, border) of an H x W map at pixel coordinates uv [V,N,2]: the four corners as
    (y [V,N] int64, x [V,N] int64, weight [V,N] float64); a corner outside the map carries weight 0"""
    uv, s = _np64(uv), _np64(scale_xy)
    gx, gy = uv[..., 0] * s[0] - 1.0, uv[..., 1] * s[1] - 1.0
    ix = np.clip(((gx + 1.0) / 2.0) * (W - 1), 0.0, W - 1.0)
    iy = np.clip(((gy + 1.0) / 2.0) * (H - 1), 0.0, H - 1.0)
    x0, y0 = np.floor(ix), np.floor(iy)
    x1, y1 = x0 + 1.0, y0 + 1.0
    out = []
    for xs, ys, wt in ((x0, y0, (x1 - ix) * (y1 - iy)), (x1, y0, (ix - x0) * (y1 - iy)),
                       (x0, y1, (x1 - ix) * (iy - y0)), (x1, y1, (ix - x0) * (iy - y0))):
        ok = (xs <= W - 1) & (ys <= H - 1)
        out.append((np.minimum(ys, H - 1).astype(np.int64), np.minimum(xs, W - 1).astype(np.int64), wt * ok))
    return out


def _latent_taps64(uv, scale_xy, H, W, h, w):
    """the 16 composite taps of one latent level: (row [V,N], column [V,N], coefficient [V,N]) each"""
    ry0, ry1, ly0, ly1 = _upsample_taps64(H, h)
    rx0, rx1, lx0, lx1 = _upsample_taps64(W, w)
    taps = []
    for yi, xi, wt in _grid_corners64(uv, scale_xy, H, W):
        for ry, ly in ((ry0, ly0), (ry1, ly1)):
            for rx, lx in ((rx0, lx0), (rx1, lx1)):
                taps.append((ry[yi], rx[xi], wt * ly[yi] * lx[xi]))
    return taps


def latent_gather_oracle(lat0, lat1, lat2, lift_w, lift_b, images, uv, scale_xy):
    """LatentGatherFn's forward in float64: channels-last latents [V,h,w,C], the lift (weight [128,3], bias [128]), images
    [V,3,H,W], uv [V,N,2] pixel coordinates (autograd_path.project), scale_xy [2] -> (rows [N,V,384], rgb_s [N,V,4])"""
    lats = [_np64(l) for l in (lat0, lat1, lat2)]
    img, wl, bl = _np64(images), _np64(lift_w).reshape(128, 3), _np64(lift_b).reshape(128)
    V, _, H, W = img.shape
    N = _np64(uv).shape[1]
    rows, rgb_s = np.zeros((N, V, 384)), np.zeros((N, V, 4))
    c0 = 0
    for lat in lats:
        Cl = lat.shape[-1]
        for ry, rx, cf in _latent_taps64(uv, scale_xy, H, W, lat.shape[1], lat.shape[2]):
            for v in range(V):
                rows[:, v, c0:c0 + Cl] += cf[v][:, None] * lat[v][ry[v], rx[v]]
        c0 += Cl
    for yi, xi, wt in _grid_corners64(uv, scale_xy, H, W):
        for v in range(V):
            rgb = img[v][:, yi[v], xi[v]].T                                   # [N,3]
            rows[:, v, 256:] += wt[v][:, None] * (rgb @ wl.T + bl)
            rgb_s[:, v, :3] += wt[v][:, None] * rgb
    return rows, rgb_s


def latent_grad_oracle(uv, scale_xy, image_hw, latent_shapes, rgb_s, grad_out):
    """LatentGatherFn's backward in float64: grad_out [N,V,>=384] -> (g_lat0, g_lat1, g_lat2 in the channels-last latent_shapes,
    g_lift_w [128,3], g_lift_b [128]); rgb_s [N,V,4] as the forward returned it"""
    g = _np64(grad_out)
    H, W = (int(x) for x in image_hw)
    outs = []
    c0 = 0
    for sh in latent_shapes:
        V, h, w, Cl = (int(x) for x in sh)
        out = np.zeros((V, h, w, Cl))
        for ry, rx, cf in _latent_taps64(uv, scale_xy, H, W, h, w):
            for v in range(V):
                np.add.at(out[v], (ry[v], rx[v]), cf[v][:, None] * g[:, v, c0:c0 + Cl])
        outs.append(out)
        c0 += Cl
    gl = g[..., 256:384].reshape(-1, 128)
    return (*outs, gl.T @ _np64(rgb_s).reshape(-1, 4)[:, :3], gl.sum(0))


def composite_grad_oracle(raw, z, ray_d, white_bkgd, g_rgb, g_acc, g_depth):
    """adjoint of raw2outputs (nerf_net_utils.py:14-59) with respect to raw [R,S,4] (float64); see k_composite.hip"""
    raw, z, d = _np64(raw), _np64(z), _np64(ray_d)
    g_rgb, g_acc, g_depth = _np64(g_rgb), _np64(g_acc), _np64(g_depth)
    delta = np.concatenate([z[:, 1:] - z[:, :-1], np.full_like(z[:, :1], 1e10)], -1) * np.linalg.norm(d, axis=-1)[:, None]
    sig = np.maximum(raw[..., 3], 0.0)
    e = np.exp(-sig * delta)
    a = 1.0 - e
    t = 1.0 - a + 1e-10
    T = np.concatenate([np.ones_like(t[:, :1]), np.cumprod(t, -1)[:, :-1]], -1)
    w = a * T
    c = 1.0 / (1.0 + np.exp(-raw[..., :3]))
    ga = g_acc - g_rgb.sum(-1) if white_bkgd else g_acc
    G = (c * g_rgb[:, None, :]).sum(-1) + ga[:, None] + g_depth[:, None] * z
    x = G * w
    after = np.concatenate([np.cumsum(x[:, ::-1], -1)[:, ::-1][:, 1:], np.zeros_like(x[:, :1])], -1)   # sum_{j>i} G_j w_j
    g_a = G * T - after / t
    out = np.empty_like(raw)
    out[..., :3] = w[..., None] * g_rgb[:, None, :] * c * (1.0 - c)
    out[..., 3] = np.where(raw[..., 3] > 0.0, g_a * e * delta, 0.0)
    return out


def attention_grad_oracle(qkv, g_out, heads):
    """adjoint of Attention.forward (vision_transformer.py:271-278; head_dim 64, s = 1/8) with respect to the fused qkv rows:
    qkv [V,N,3 C], g_out [V,N,C] -> (g_qkv [V,N,3 C], lse [V,heads,N]) in float64; the formulas of k_vit_bwd.hip"""
    x, g = _np64(qkv), _np64(g_out)
    V, N, C3 = x.shape
    C = C3 // 3
    hd = C // heads
    s = hd ** -0.5
    q, k, v = (x.reshape(V, N, 3, heads, hd).transpose(2, 0, 3, 1, 4)[i] for i in range(3))      # [V,heads,N,hd]
    go = g.reshape(V, N, heads, hd).transpose(0, 2, 1, 3)
    S = s * np.einsum("vhid,vhjd->vhij", q, k)
    m = S.max(-1, keepdims=True)
    lse = (m + np.log(np.exp(S - m).sum(-1, keepdims=True)))[..., 0]
    P = np.exp(S - lse[..., None])
    out = np.einsum("vhij,vhjd->vhid", P, v)
    D = (go * out).sum(-1)
    dV = np.einsum("vhij,vhid->vhjd", P, go)
    dS = P * (np.einsum("vhid,vhjd->vhij", go, v) - D[..., None])
    dQ = s * np.einsum("vhij,vhjd->vhid", dS, k)
    dK = s * np.einsum("vhij,vhid->vhjd", dS, q)
    g_qkv = np.stack([dQ, dK, dV], 0).transpose(1, 3, 0, 2, 4).reshape(V, N, C3)
    return g_qkv, lse


def _gelu64(u):
    from math import erf
    return u * 0.5 * (1.0 + np.vectorize(erf)(u / np.sqrt(2.0)))


def _gelu_grad64(u):
    from math import erf
    return 0.5 * (1.0 + np.vectorize(erf)(u / np.sqrt(2.0))) + u * np.exp(-0.5 * u * u) / np.sqrt(2.0 * np.pi)


def linear_grad_oracle(a, W, g_out):
    """adjoint of y = a W^T + b on rows: a [M,in], W [out,in], g_out [M,out] -> (g_a, g_W, g_b) in float64"""
    a, W, g = _np64(a), _np64(W), _np64(g_out)
    a, g = a.reshape(-1, a.shape[-1]), g.reshape(-1, g.shape[-1])
    return g @ W, g.T @ a, g.sum(0)


def layernorm_grad_oracle(x, w, g_out, eps=1e-6):
    """adjoint of nn.LayerNorm over the last dimension -> (g_x, g_w, g_b) in float64; the formulas of k_vit_dense_bwd.hip"""
    x, w, g = _np64(x), _np64(w), _np64(g_out)
    x, g = x.reshape(-1, x.shape[-1]), g.reshape(-1, g.shape[-1])
    mean = x.mean(1, keepdims=True)
    rstd = 1.0 / np.sqrt(((x - mean) ** 2).mean(1, keepdims=True) + eps)
    xh = (x - mean) * rstd
    gw = g * w
    g_x = rstd * (gw - gw.mean(1, keepdims=True) - xh * (gw * xh).mean(1, keepdims=True))
    return g_x, (g * xh).sum(0), g.sum(0)


def norm_linear_grad_oracle(x, ln_w, ln_b, W, g_out, eps=1e-6):
    """adjoint of Linear(LayerNorm(x)) -> (g_x, g_ln_w, g_ln_b, g_W, g_b) in float64"""
    x2 = _np64(x).reshape(-1, _np64(x).shape[-1])
    mean = x2.mean(1, keepdims=True)
    y = (x2 - mean) / np.sqrt(((x2 - mean) ** 2).mean(1, keepdims=True) + eps) * _np64(ln_w) + _np64(ln_b)
    g_y, g_W, g_b = linear_grad_oracle(y, W, g_out)
    g_x, g_lw, g_lb = layernorm_grad_oracle(x2, ln_w, g_y, eps)
    return g_x, g_lw, g_lb, g_W, g_b


def gelu_linear_grad_oracle(u, W, g_out):
    """adjoint of Linear(gelu(u)), exact erf -> (g_u, g_W, g_b) in float64"""
    u2 = _np64(u).reshape(-1, _np64(u).shape[-1])
    g_a, g_W, g_b = linear_grad_oracle(_gelu64(u2), W, g_out)
    return g_a * _gelu_grad64(u2), g_W, g_b


def relu_linear_grad_oracle(a, W, b, g_out):
    """y = relu(a W^T + b) and its adjoint, torch's rule (gradient 0 where y == 0) -> (y, g_a, g_W, g_b) in float64"""
    a2 = _np64(a).reshape(-1, _np64(a).shape[-1])
    y = np.maximum(a2 @ _np64(W).T + _np64(b), 0.0)
    g = _np64(g_out).reshape(y.shape) * (y > 0.0)
    return (y, *linear_grad_oracle(a2, W, g))


def _xview_probs64(kvp, kvs):
    p, s = _np64(kvp), _np64(kvs)
    S = np.einsum("pjc,pic->pji", p[..., :128], s[..., :128]) / np.sqrt(128.0)
    e = np.exp(S - S.max(1, keepdims=True))
    return p, s, e / e.sum(1, keepdims=True)


def xview_attention_oracle(kvp, kvs):
    """cross_attention (cross_transformer.py:128-149) on [key(128) | value(256)] rows [P,V,384] -> n [P,V,256] in float64"""
    p, s, A = _xview_probs64(kvp, kvs)
    return s[..., 128:] + np.einsum("pjc,pji->pic", p[..., 128:], A)


def xview_attention_grad_oracle(kvp, kvs, g_n):
    """adjoint of xview_attention_oracle: g_n [P,V,256] -> (g_kvp, g_kvs) [P,V,384] in float64; the formulas of
    k_pointnet_bwd.hip"""
    p, s, A = _xview_probs64(kvp, kvs)
    g = _np64(g_n)
    dA = np.einsum("pjc,pic->pji", p[..., 128:], g)
    dS = A * (dA - (A * dA).sum(1, keepdims=True))
    g_kvp, g_kvs = np.empty_like(p), np.empty_like(s)
    g_kvs[..., 128:] = g
    g_kvp[..., 128:] = np.einsum("pji,pic->pjc", A, g)
    g_kvp[..., :128] = np.einsum("pji,pic->pjc", dS, s[..., :128]) / np.sqrt(128.0)
    g_kvs[..., :128] = np.einsum("pji,pjc->pic", dS, p[..., :128]) / np.sqrt(128.0)
    return g_kvp, g_kvs


def bn_act_grad_oracle(y, out, g, gamma, eps):
    """adjoint of out = [relu](bn(y) [+ residual]) with train-mode BatchNorm (batch statistics, biased variance), NCHW.
    ``out``: the site's output, read for the gate [out > 0] (None: no ReLU); gamma [C] or None (1) ->
    (g_y, g_residual, g_gamma, g_beta) in float64; the formulas of k_encoder_bwd.hip"""
    y, g = _np64(y), _np64(g)
    gp = g if out is None else g * (_np64(out) > 0.0)
    ax = (0, 2, 3)
    mean = y.mean(ax, keepdims=True)
    invstd = 1.0 / np.sqrt(((y - mean) ** 2).mean(ax, keepdims=True) + eps)
    xh = (y - mean) * invstd
    gam = np.ones(y.shape[1]) if gamma is None else _np64(gamma)
    g_y = gam.reshape(1, -1, 1, 1) * invstd * (gp - gp.mean(ax, keepdims=True) - xh * (gp * xh).mean(ax, keepdims=True))
    return g_y, gp, (gp * xh).sum(ax), gp.sum(ax)


def maxpool3x3s2_grad_oracle(x, g):
    """adjoint of nn.MaxPool2d(3, 2, 1) on x [N,C,H,W] with torch's routing rule: a window's gradient goes to the last element,
    scanning kh outer / kw inner, for which val > max || isnan(val), starting from -inf -- the FIRST maximum of the window; the
    padding never wins (a window of nothing but -inf is not handled here) -> g_x in float64"""
    x, g = _np64(x), _np64(g)
    N, C, H, W = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = np.full((N, C, 2 * Ho + 1, 2 * Wo + 1), -np.inf)
    xp[:, :, 1:H + 1, 1:W + 1] = x
    best = np.full((N, C, Ho, Wo), -np.inf)
    bi = np.zeros((N, C, Ho, Wo), dtype=np.int64)
    bj = np.zeros((N, C, Ho, Wo), dtype=np.int64)
    oy, ox = np.meshgrid(np.arange(Ho), np.arange(Wo), indexing="ij")
    for kh in range(3):
        for kw in range(3):
            v = xp[:, :, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2]
            take = (v > best) | np.isnan(v)
            best = np.where(take, v, best)
            bi = np.where(take, 2 * oy - 1 + kh, bi)
            bj = np.where(take, 2 * ox - 1 + kw, bj)
    g_x = np.zeros_like(x)
    n, c = np.meshgrid(np.arange(N), np.arange(C), indexing="ij")
    np.add.at(g_x, (n[:, :, None, None], c[:, :, None, None], bi, bj), g)
    return g_x
