"""The training form of the per-point network on the host: the float64 restatements of its two new adjoints
(train_ops.relu_linear_grad_oracle, xview_attention_oracle / xview_attention_grad_oracle, the formulas of
k_vit_dense_bwd.hip's ReLU layers and of k_pointnet_bwd.hip)
against torch's float64 autograd, the switch cfg.train_point_net ("torch" by default, "device" refuses a CPU batch, anything else
is a ValueError), and the re-association of autograd_path.point_network_device -- padded layers, fused key | value layers, one
attention operator -- which is exact algebra: the same composition code, run on plain-torch operators in float64, gives
point_network's result and all of its parameter gradients."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from transhuman_amd.config import get_cfg, override
from transhuman_amd.networks import autograd_path, train_ops
from util import make_net

TOL = 1e-12
KEY0_BIAS = "spatial_key_value_0.key_embed.bias"
POINT_NET = ("fc_0", "fc_1", "fc_2", "fc_3", "fc_4", "alpha_fc", "feature_fc", "view_fc", "rgb_fc", "alpha_res_0", "rgb_res_0",
             "rgb_res_1", "spatial_key_value_0.key_embed", "spatial_key_value_0.value_embed", "spatial_key_value_1.key_embed",
             "spatial_key_value_1.value_embed")


def _close(got, ref, what):
    ref = ref.detach().numpy()
    got = np.asarray(got).reshape(ref.shape)
    assert got.dtype == np.float64, what
    scale = float(np.abs(ref).max())
    assert scale > 0, what
    assert float(np.abs(got - ref).max()) <= TOL * scale, what


@pytest.mark.parametrize("M", (1, 17, 65))
@pytest.mark.parametrize("in_f,out_f", ((256, 256), (384, 256), (288, 128), (128, 128), (256, 16)))
def test_relu_linear_adjoint_equals_autograd(in_f, out_f, M):
    rs = np.random.RandomState(M + in_f + 3 * out_f)
    t = lambda *shape, scale=1.0: torch.from_numpy(rs.normal(scale=scale, size=shape)).requires_grad_(True)
    a, W, b, g = t(M, in_f, scale=2.0), t(out_f, in_f, scale=0.1), t(out_f), torch.from_numpy(rs.normal(size=(M, out_f)))
    y = F.relu(F.linear(a, W, b))
    y.backward(g)
    assert 0.2 < float((y == 0).double().mean()) < 0.8
    for got, ref, what in zip(train_ops.relu_linear_grad_oracle(a, W, b, g), (y, a.grad, W.grad, b.grad),
                              ("y", "g_a", "g_W", "g_b")):
        _close(got, ref, what)


def test_relu_gradient_is_zero_where_the_output_is_zero():
    """torch's rule at the kink: pre-activation exactly 0 -> gradient 0"""
    a, W, b, g = np.array([[1.0, -1.0]] * 2), np.array([[1.0, 1.0]] * 16), np.zeros(16), np.ones((2, 16))
    y, g_a, g_W, g_b = train_ops.relu_linear_grad_oracle(np.tile(a, (1, 8)), np.tile(W, (1, 8)), b, g)
    assert not y.any() and not g_a.any() and not g_W.any() and not g_b.any()


@pytest.mark.parametrize("V", (1, 2, 3, 4))
@pytest.mark.parametrize("P", (1, 5))
def test_xview_attention_oracles_equal_autograd(P, V):
    rs = np.random.RandomState(10 * P + V)
    kvp, kvs = (torch.from_numpy(rs.normal(size=(P, V, 384))).requires_grad_(True) for _ in range(2))
    g = torch.from_numpy(rs.normal(size=(P, V, 256)))
    kp, vp, ks, vs = kvp[..., :128], kvp[..., 128:], kvs[..., :128], kvs[..., 128:]
    A = F.softmax(torch.einsum("pjc,pic->pji", kp, ks) / math.sqrt(128), dim=1)                # point_network's statements
    n = vs + torch.einsum("pjc,pji->pic", vp, A)
    n.backward(g)
    _close(train_ops.xview_attention_oracle(kvp, kvs), n, "n")
    g_kvp, g_kvs = train_ops.xview_attention_grad_oracle(kvp, kvs, g)
    if V == 1:                                             # a softmax over one logit is constant: the key gradients are exactly 0
        assert not g_kvp[..., :128].any() and not g_kvs[..., :128].any()
        assert not kvp.grad[..., :128].any() and not kvs.grad[..., :128].any()
        assert np.array_equal(g_kvp[..., 128:], g.numpy()) and np.array_equal(g_kvs[..., 128:], g.numpy())
    else:
        _close(g_kvp, kvp.grad, "g_kvp")
        _close(g_kvs, kvs.grad, "g_kvs")
        _close(autograd_path.point_network_torch_ops()["xattn"](kvp.detach(), kvs.detach()), n, "xattn of the torch table")


def test_switch_defaults_to_torch():
    from transhuman_amd.config import _defaults
    assert _defaults().train_point_net == "torch" and get_cfg().train_point_net == "torch"


def test_device_refuses_a_cpu_batch_and_a_bad_value_is_an_error():
    from transhuman_amd import hip
    batch = {"ray_o": torch.zeros(1, 4, 3), "ray_d": torch.ones(1, 4, 3)}
    renderer = SimpleNamespace(net=None)
    with override(train_point_net="device"), pytest.raises(hip.HipError, match="MI355X"):
        autograd_path.render(renderer, batch)
    with override(train_point_net="hip"), pytest.raises(ValueError, match="train_point_net"):
        autograd_path.render(renderer, batch)
    w, b = torch.zeros(256, 256, requires_grad=True), torch.zeros(256, requires_grad=True)
    row = torch.zeros(2, 3, 256, requires_grad=True)
    kv = torch.zeros(2, 3, 384, requires_grad=True)
    for call in (lambda: train_ops.ReluLinearFn.apply(row, w, b), lambda: train_ops.CrossViewAttentionFn.apply(kv, kv)):
        with pytest.raises(hip.HipError):
            call()


def _net64():
    with override(vit_depth=2):                            # (make_net sets the key and leaves it set)
        return make_net(2).double()


def _grads(fn, net, h, f, vd, g):
    for p in net.parameters():
        p.grad = None
    h, f = h.clone().requires_grad_(True), f.clone().requires_grad_(True)
    raw = fn(net, h, f, vd)
    raw.backward(g)
    out = {"raw": raw.detach(), "g_h": h.grad, "g_f": f.grad}
    out.update({k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None})
    return out


@pytest.mark.parametrize("V", (1, 3))
def test_device_composition_is_exact_algebra(V):
    """point_network_device on plain-torch operators in float64 against point_network, P = 37: raw, the input gradients and the
    gradient of every parameter of the per-point network (16 layers, weight and bias) to 1e-12 of the tensor's maximum.  The
    exact gradient of spatial_key_value_0.key_embed.bias is 0 (a bias on kp_j adds b . ks_i to every logit of column i: the
    softmax over j cancels it), so it is held to 1e-12 of its layer's weight gradient instead.  At V = 1 the softmax is the
    constant 1 and all four key tensors get exact zeros from both."""
    P = 37
    net = _net64()
    rs = np.random.RandomState(V)
    h, f, vd = (torch.from_numpy(rs.normal(size=s)) for s in ((P, V, 255), (P, V, 384), (P, 27)))
    g = torch.from_numpy(rs.normal(size=(P, 4)))
    ref = _grads(autograd_path.point_network, net, h, f, vd, g)
    ops = autograd_path.point_network_torch_ops()
    got = _grads(lambda *a: autograd_path.point_network_device(*a, ops=ops), net, h, f, vd, g)
    want = {"raw", "g_h", "g_f"} | {f"{layer}.{p}" for layer in POINT_NET for p in ("weight", "bias")}
    assert set(ref) == set(got) == want and len(want) == 3 + 32
    for k, t in ref.items():
        assert got[k].dtype == torch.float64 and got[k].shape == t.shape, k
        if V == 1 and "key_embed" in k:                    # one view: the softmax is the constant 1, the keys get exact zeros
            assert not bool(t.any()) and not bool(got[k].any()), k
            continue
        if k == KEY0_BIAS:
            scale = float(ref["spatial_key_value_0.key_embed.weight"].abs().max())
            assert scale > 0 and float(got[k].abs().max()) <= TOL * scale and float(t.abs().max()) <= TOL * scale
            continue
        scale = float(t.abs().max())
        assert scale > 0, k
        assert float((got[k] - t).abs().max()) <= TOL * scale, (k, float((got[k] - t).abs().max()) / scale)
    # K4's rows, with their zero pad column, are taken as they come
    padded = _grads(lambda *a: autograd_path.point_network_device(*a, ops=ops), net, F.pad(h, (0, 1)), f, vd, g)
    assert torch.equal(padded["raw"], got["raw"]) and torch.equal(padded["g_h"][..., :255], got["g_h"])
