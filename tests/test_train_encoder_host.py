"""The backward of the encoder trunk (K23) on the host: the switch cfg.train_encoder ("torch" by default, "device" refuses a CPU
batch, anything else is a ValueError), the additions to the C ABI (declared, exported, bound; the size queries are pure host calls;
null or unsupported arguments are refused with the function's name in th_last_error), and the float64 restatements of the two
formulas the device tests cite -- train_ops.bn_act_grad_oracle and train_ops.maxpool3x3s2_grad_oracle -- against torch's CPU
float64 autograd: 1e-12 of the tensor's maximum on random inputs, exact on integer-valued inputs with ties."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from transhuman_amd.config import get_cfg, override
from transhuman_amd.networks import autograd_path, train_ops

TOL = 1e-12
ENTRIES = ("th_conv2d_bwd_supported", "th_conv2d_wgrad_chunk_pixels", "th_conv2d_dgrad_tile_rows", "th_conv2d_dgrad_tile_cols",
           "th_bn_act_bwd_slice_elems", "th_bn_act_bwd_workspace_bytes", "th_bn_act_bwd", "th_maxpool3x3s2_bwd",
           "th_conv2d_dgrad_pack_bytes", "th_conv2d_dgrad_pack", "th_conv2d_dgrad", "th_conv2d_wgrad_workspace_bytes",
           "th_conv2d_wgrad")
SHAPES = ((3, 64, 7, 2, 1), (64, 64, 3, 1, 3), (128, 128, 3, 1, 3), (64, 128, 3, 2, 3), (64, 128, 1, 2, 3))   # cin cout ks s bits


@pytest.fixture(scope="module")
def lib():
    from transhuman_amd import build, hip
    build.build(force=False, verbose=False)
    return hip.load_library()


def test_switch_defaults_to_torch():
    from transhuman_amd.config import _defaults
    assert _defaults().train_encoder == "torch" and get_cfg().train_encoder == "torch"


def test_device_refuses_a_cpu_batch_and_a_bad_value_is_an_error():
    from transhuman_amd import hip
    from transhuman_amd.networks.encoder import SpatialEncoder
    batch = {"ray_o": torch.zeros(1, 4, 3), "ray_d": torch.ones(1, 4, 3)}
    renderer = SimpleNamespace(net=None)
    with override(train_encoder="device"), pytest.raises(hip.HipError, match="MI355X"):
        autograd_path.render(renderer, batch)
    with override(train_encoder="hip"), pytest.raises(ValueError, match="train_encoder"):
        autograd_path.render(renderer, batch)
    with pytest.raises(ValueError, match="cfg.train_encoder must be 'torch' or 'device', not 'cuda'"):
        autograd_path._switch("train_encoder", "cuda", True)
    enc = SpatialEncoder().train()
    img = torch.zeros(1, 3, 16, 16)
    for call in (lambda: autograd_path.trunk_device(enc, img), lambda: autograd_path.encode(enc, img, encoder="device"),
                 lambda: autograd_path.latent_features(enc, img, None, None, encoder="device")):
        with pytest.raises(hip.HipError, match="MI355X"):
            call()
    with pytest.raises(ValueError, match="train_encoder"):
        autograd_path.encode(enc, img, encoder="fast")
    x = torch.zeros(1, 64, 4, 4, requires_grad=True)
    w = torch.zeros(64, 64, 3, 3, requires_grad=True)
    bn = torch.nn.BatchNorm2d(64).train()
    for call in (lambda: train_ops.ConvFn.apply(x, w, 1), lambda: train_ops.MaxPoolFn.apply(x),
                 lambda: train_ops.BnActFn.apply(x, bn, None, True, bn.weight, bn.bias)):
        with pytest.raises(hip.HipError):
            call()


def test_batch_statistics_rule():
    """the device backward is defined for train-mode nn.BatchNorm2d sites with a momentum; anything else is torch autograd's"""
    from transhuman_amd.networks.encoder import SpatialEncoder
    enc = SpatialEncoder().train()
    ok = autograd_path._trunk_sites_have_batch_statistics
    assert ok(enc)
    enc.model.layer2[0].downsample[1].eval()
    assert not ok(enc)
    enc.train()
    enc.model.layer1[1].bn2.momentum = None
    assert not ok(enc)
    enc.model.layer1[1].bn2.momentum = 0.1
    assert ok(enc) and not ok(torch.nn.SyncBatchNorm.convert_sync_batchnorm(SpatialEncoder().train()))


def test_entry_points_declared_exported_bound(lib):
    from transhuman_amd import hip
    for name in ENTRIES:
        assert name in hip.SYMBOLS and hasattr(lib, name), name
    assert lib.th_abi_version() == 12


def test_host_queries_need_no_device(lib):
    from transhuman_amd import hip
    for cin, cout, ks, s, bits in SHAPES:
        assert hip.conv2d_bwd_supported(cin, cout, ks, s) == bits
        assert (lib.th_conv2d_dgrad_pack_bytes(cin, cout, ks, s) >= cin * cout * ks * ks * 4) == bool(bits & 2)
        chunks = -(-3 * 17 * 9 // hip.conv2d_wgrad_chunk_pixels()) if s == 2 else -(-3 * 33 * 17 // hip.conv2d_wgrad_chunk_pixels())
        assert lib.th_conv2d_wgrad_workspace_bytes(3, cin, cout, ks, s, 33, 17) >= chunks * cout * cin * ks * ks * 4
    for bad in ((64, 64, 3, 2), (3, 64, 3, 1), (128, 256, 3, 2), (64, 64, 5, 1), (0, 0, 0, 0)):
        assert hip.conv2d_bwd_supported(*bad) == 0
        assert lib.th_conv2d_dgrad_pack_bytes(*bad) == 0 and lib.th_conv2d_wgrad_workspace_bytes(1, *bad, 8, 8) == 0
    assert lib.th_conv2d_dgrad_pack_bytes(3, 64, 7, 2) == 0                  # conv1: no input gradient
    assert lib.th_conv2d_wgrad_workspace_bytes(0, 64, 64, 3, 1, 8, 8) == 0 and lib.th_conv2d_wgrad_workspace_bytes(1, 64, 64, 3, 1, 0, 8) == 0
    assert hip.conv2d_wgrad_chunk_pixels() == 256 and hip.conv2d_dgrad_tile() == (8, 16) and hip.bn_act_bwd_slice_elems() == 8192
    assert lib.th_bn_act_bwd_workspace_bytes(3, 64, 256 * 256) >= 64 * 4 * 8
    assert lib.th_bn_act_bwd_workspace_bytes(0, 64, 4) == 0 and lib.th_bn_act_bwd_workspace_bytes(1, 64, 0) == 0


def test_null_and_bad_arguments_are_refused_by_name(lib):
    """every refusal below happens before anything touches a device: the pointers are never read"""
    p = C.c_void_p(4096)
    z = C.c_void_p(0)
    cases = (
        (b"th_bn_act_bwd", lambda: lib.th_bn_act_bwd(z, p, p, p, 1, 64, 4, p, 1e-5, p, p, p, p, p, 1 << 20, z)),
        (b"th_bn_act_bwd", lambda: lib.th_bn_act_bwd(p, z, p, p, 1, 64, 4, p, 1e-5, p, p, p, p, p, 1 << 20, z)),
        (b"th_bn_act_bwd", lambda: lib.th_bn_act_bwd(p, p, p, p, 0, 64, 4, p, 1e-5, p, p, p, p, p, 1 << 20, z)),
        (b"th_bn_act_bwd", lambda: lib.th_bn_act_bwd(p, p, p, p, 1, 64, 4, p, 1e-5, p, p, p, p, p, 8, z)),
        (b"th_bn_act_bwd", lambda: lib.th_bn_act_bwd(p, p, p, p, 1, 64, 4, p, 0.0, p, p, p, p, p, 1 << 20, z)),
        (b"th_maxpool3x3s2_bwd", lambda: lib.th_maxpool3x3s2_bwd(p, p, z, 1, 4, 4, p, z)),
        (b"th_maxpool3x3s2_bwd", lambda: lib.th_maxpool3x3s2_bwd(p, p, p, 1, 0, 4, p, z)),
        (b"th_conv2d_dgrad_pack", lambda: lib.th_conv2d_dgrad_pack(p, z, 64, 64, 3, 1, p, 1 << 20, z)),
        (b"th_conv2d_dgrad_pack", lambda: lib.th_conv2d_dgrad_pack(p, p, 3, 64, 7, 2, p, 1 << 20, z)),
        (b"th_conv2d_dgrad_pack", lambda: lib.th_conv2d_dgrad_pack(p, p, 64, 64, 3, 1, p, 16, z)),
        (b"th_conv2d_dgrad", lambda: lib.th_conv2d_dgrad(p, p, 1, 64, 64, 3, 1, 8, 8, z, 1 << 20, p, z)),
        (b"th_conv2d_dgrad", lambda: lib.th_conv2d_dgrad(p, p, 1, 64, 64, 3, 2, 8, 8, p, 1 << 20, p, z)),
        (b"th_conv2d_dgrad", lambda: lib.th_conv2d_dgrad(p, p, 1, 64, 64, 3, 1, 8, 8, p, 16, p, z)),
        (b"th_conv2d_dgrad", lambda: lib.th_conv2d_dgrad(p, p, 0, 64, 64, 3, 1, 8, 8, p, 1 << 20, p, z)),
        (b"th_conv2d_wgrad", lambda: lib.th_conv2d_wgrad(p, p, z, 1, 64, 64, 3, 1, 8, 8, p, p, 1 << 20, z)),
        (b"th_conv2d_wgrad", lambda: lib.th_conv2d_wgrad(p, p, p, 1, 64, 32, 3, 1, 8, 8, p, p, 1 << 20, z)),
        (b"th_conv2d_wgrad", lambda: lib.th_conv2d_wgrad(p, p, p, 1, 64, 64, 3, 1, 8, 8, p, p, 16, z)),
    )
    for name, call in cases:
        assert call() != 0
        assert name in lib.th_last_error(), (name, lib.th_last_error())


# ---- the BatchNorm backward formula ------------------------------------------------------------------------------------------
def _bn_autograd(y, res, g, gamma, beta, relu, eps=1e-5):
    y = y.clone().requires_grad_(True)
    res = None if res is None else res.clone().requires_grad_(True)
    gamma = None if gamma is None else gamma.clone().requires_grad_(True)
    beta = None if beta is None else beta.clone().requires_grad_(True)
    out = torch.batch_norm(y, gamma, beta, None, None, True, 0.1, eps, False)
    if res is not None:
        out = out + res
    if relu:
        out = F.relu(out)
    out.backward(g)
    grad = lambda t: None if t is None else t.grad
    return out.detach(), y.grad, grad(res), grad(gamma), grad(beta)


def _close(got, ref, what):
    got, ref = np.asarray(got), ref.numpy()
    assert got.dtype == np.float64 and got.shape == ref.shape, what
    scale = float(np.abs(ref).max())
    assert float(np.abs(got - ref).max()) <= TOL * max(scale, 1e-300), (what, float(np.abs(got - ref).max()), scale)


@pytest.mark.parametrize("relu", (False, True))
@pytest.mark.parametrize("residual", (False, True))
@pytest.mark.parametrize("affine", (False, True))
@pytest.mark.parametrize("shape", ((1, 4, 1, 1), (3, 5, 2, 3), (2, 64, 9, 17)))
def test_bn_backward_formula_equals_autograd(shape, affine, residual, relu):
    rs = np.random.RandomState(sum(shape) + 2 * affine + 4 * residual + 8 * relu)
    t = lambda *s: torch.from_numpy(rs.normal(size=s))
    y, g = t(*shape) * 2.0 + 0.5, t(*shape)
    res = t(*shape) if residual else None
    gamma, beta = (t(shape[1]) + 1.0, t(shape[1])) if affine else (None, None)
    out, g_y, g_res, g_gamma, g_beta = _bn_autograd(y, res, g, gamma, beta, relu)
    got = train_ops.bn_act_grad_oracle(y, out if relu else None, g, gamma, 1e-5)
    _close(got[0], g_y, "g_y")
    if residual:
        _close(got[1], g_res, "g_residual")
    if affine:
        _close(got[2], g_gamma, "g_gamma")
        _close(got[3], g_beta, "g_beta")


def test_bn_backward_formula_gate_is_exact_on_integers():
    """integer inputs with a tenth of the pre-activations exactly 0: the gate [out > 0] and the residual's gradient are exact"""
    rs = np.random.RandomState(5)
    shape = (3, 8, 6, 7)
    y = torch.from_numpy(rs.randint(-3, 4, size=shape).astype(np.float64))
    g = torch.from_numpy(rs.randint(-4, 5, size=shape).astype(np.float64))
    with torch.no_grad():
        bn = torch.batch_norm(y, None, None, None, None, True, 0.1, 1e-5, False)
    res = torch.from_numpy(rs.randint(-2, 3, size=shape).astype(np.float64))
    zero = torch.from_numpy(rs.uniform(size=shape) < 0.1)
    res = torch.where(zero, -bn, res)                       # bn + res == 0 exactly there
    out, g_y, g_res, _, _ = _bn_autograd(y, res, g, None, None, True)
    assert float(((bn + res) == 0).double().mean()) >= 0.08
    got = train_ops.bn_act_grad_oracle(y, out, g, None, 1e-5)
    assert np.array_equal(got[1], g_res.numpy()) and not got[1][zero.numpy()].any()
    _close(got[0], g_y, "g_y")


# ---- the max pool's routing rule ------------------------------------------------------------------------------------------------
def _pool_autograd(x, g):
    x = x.clone().requires_grad_(True)
    F.max_pool2d(x, 3, 2, 1).backward(g)
    return x.grad


@pytest.mark.parametrize("shape", ((1, 1, 1, 1), (2, 3, 2, 3), (1, 4, 8, 16), (3, 2, 9, 17), (1, 2, 33, 47)))
def test_pool_routing_equals_autograd(shape):
    rs = np.random.RandomState(sum(shape))
    N, Cc, H, W = shape
    g = torch.from_numpy(rs.normal(size=(N, Cc, (H - 1) // 2 + 1, (W - 1) // 2 + 1)))
    x = torch.from_numpy(rs.normal(size=shape))
    _close(train_ops.maxpool3x3s2_grad_oracle(x, g), _pool_autograd(x, g), "random")
    # post-ReLU-like integers: all-zero windows and ties are the common case; equality is exact
    xi = torch.from_numpy(np.maximum(rs.randint(-6, 3, size=shape), 0).astype(np.float64))
    gi = torch.from_numpy(rs.randint(-4, 5, size=tuple(g.shape)).astype(np.float64))
    assert np.array_equal(train_ops.maxpool3x3s2_grad_oracle(xi, gi), _pool_autograd(xi, gi).numpy())
    assert np.array_equal(train_ops.maxpool3x3s2_grad_oracle(torch.zeros(shape, dtype=torch.float64), gi),
                          _pool_autograd(torch.zeros(shape, dtype=torch.float64), gi).numpy())
