"""The training form of TransHE's dense layers, LayerNorm and GELU on the host: the float64 restatements of their adjoints
(train_ops.*_grad_oracle, the formulas of k_vit_dense_bwd.hip) against torch's float64 autograd, the switch
cfg.train_vit_dense ("torch" by default, "device" refuses a CPU batch, anything else is a ValueError, vit_forward at the
defaults is the function it was), and the additions to the C ABI (declared, exported, bound; workspace queries)."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from transhuman_amd.config import get_cfg, override
from transhuman_amd.networks import autograd_path, train_ops
from util import make_net

TOL = 1e-10
ROWS = (1, 17, 65)
SHAPES = ((192, 576), (192, 192), (192, 768), (768, 192))            # (in, out) of qkv, proj, fc1, fc2
EPS = 1e-6


def _close(got, ref, what):
    ref = ref.detach().numpy()
    got = np.asarray(got).reshape(ref.shape)
    assert got.dtype == np.float64, what
    scale = float(np.abs(ref).max())
    assert scale > 0, what
    assert float(np.abs(got - ref).max()) <= TOL * scale, what


def _draw(M, in_f, out_f, seed):
    rs = np.random.RandomState(seed)
    t = lambda *shape, scale=1.0: torch.from_numpy(rs.normal(scale=scale, size=shape)).requires_grad_(True)
    return t(M, in_f, scale=2.0), t(out_f, in_f, scale=0.1), t(out_f), torch.from_numpy(rs.normal(size=(M, out_f))), rs


@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("in_f,out_f", SHAPES)
def test_linear_adjoint_equals_autograd(in_f, out_f, M):
    a, W, b, g, _ = _draw(M, in_f, out_f, M + in_f)
    F.linear(a, W, b).backward(g)
    for got, ref, what in zip(train_ops.linear_grad_oracle(a, W, g), (a.grad, W.grad, b.grad), ("g_a", "g_W", "g_b")):
        _close(got, ref, what)


@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("in_f,out_f", ((192, 576), (192, 768)))
def test_norm_linear_adjoint_equals_autograd(in_f, out_f, M):
    x, W, b, g, rs = _draw(M, in_f, out_f, 3 * M + out_f)
    lw = torch.from_numpy(rs.uniform(0.5, 1.5, size=in_f)).requires_grad_(True)
    lb = torch.from_numpy(rs.normal(scale=0.2, size=in_f)).requires_grad_(True)
    F.linear(F.layer_norm(x, (in_f,), lw, lb, EPS), W, b).backward(g)
    got = train_ops.norm_linear_grad_oracle(x, lw, lb, W, g, EPS)
    for v, ref, what in zip(got, (x.grad, lw.grad, lb.grad, W.grad, b.grad), ("g_x", "g_ln_w", "g_ln_b", "g_W", "g_b")):
        _close(v, ref, what)


@pytest.mark.parametrize("M", ROWS)
def test_gelu_linear_adjoint_equals_autograd(M):
    u, W, b, g, _ = _draw(M, 768, 192, 5 * M)
    F.linear(F.gelu(u), W, b).backward(g)
    for got, ref, what in zip(train_ops.gelu_linear_grad_oracle(u, W, g), (u.grad, W.grad, b.grad), ("g_u", "g_W", "g_b")):
        _close(got, ref, what)


@pytest.mark.parametrize("M", ROWS)
def test_layernorm_adjoint_equals_autograd(M):
    rs = np.random.RandomState(7 * M)
    x = torch.from_numpy(rs.normal(loc=0.5, scale=2.0, size=(M, 192))).requires_grad_(True)
    w = torch.from_numpy(rs.uniform(0.5, 1.5, size=192)).requires_grad_(True)
    b = torch.from_numpy(rs.normal(size=192)).requires_grad_(True)
    g = torch.from_numpy(rs.normal(size=(M, 192)))
    F.layer_norm(x, (192,), w, b, EPS).backward(g)
    for got, ref, what in zip(train_ops.layernorm_grad_oracle(x, w, g, EPS), (x.grad, w.grad, b.grad), ("g_x", "g_w", "g_b")):
        _close(got, ref, what)


def test_switch_defaults_to_torch():
    from transhuman_amd.config import _defaults
    assert _defaults().train_vit_dense == "torch" and get_cfg().train_vit_dense == "torch"


def test_device_refuses_a_cpu_batch_and_a_bad_value_is_an_error():
    from transhuman_amd import hip
    batch = {"ray_o": torch.zeros(1, 4, 3), "ray_d": torch.ones(1, 4, 3)}
    renderer = SimpleNamespace(net=None)
    vit = make_net(2).ViT
    x, pe = torch.zeros(1, 5, 192), torch.zeros(1, 5, 3)
    with override(train_vit_dense="device"), pytest.raises(hip.HipError, match="MI355X"):
        autograd_path.render(renderer, batch)
    with override(train_vit_dense="hip"), pytest.raises(ValueError, match="train_vit_dense"):
        autograd_path.render(renderer, batch)
    with pytest.raises(hip.HipError, match="MI355X"):
        autograd_path.vit_forward(vit, x, pe, dense="device")
    with pytest.raises(ValueError, match="train_vit_dense"):
        autograd_path.vit_forward(vit, x, pe, dense="hip")
    w, b = torch.zeros(192, 192, requires_grad=True), torch.zeros(192, requires_grad=True)
    ones = torch.ones(192, requires_grad=True)
    row = torch.zeros(1, 5, 192, requires_grad=True)
    for call in (lambda: train_ops.LinearFn.apply(row, w, b), lambda: train_ops.GeluLinearFn.apply(row, w, b),
                 lambda: train_ops.NormLinearFn.apply(row, ones, b, w, b), lambda: train_ops.LayerNormFn.apply(row, ones, b)):
        with pytest.raises(hip.HipError):
            call()


def test_vit_forward_at_the_defaults_is_unchanged():
    vit = make_net(2).ViT
    rs = np.random.RandomState(3)
    x = torch.from_numpy(rs.normal(size=(2, 17, 192)).astype(np.float32))
    pe = torch.from_numpy(rs.uniform(-1, 1, size=(2, 17, 3)).astype(np.float32))
    with torch.no_grad():
        got = autograd_path.vit_forward(vit, x, pe)
        same = autograd_path.vit_forward(vit, x, pe, attention="torch", dense="torch")
        # the function, written out (vision_transformer.py:257-307)
        t = x + vit.get_PE(pe).to(x.dtype)
        V, N, C = t.shape
        h = vit.num_heads
        for blk in vit.blocks:
            qkv = blk.attn.qkv(blk.norm1(t)).reshape(V, N, 3, h, C // h).permute(2, 0, 3, 1, 4)
            a = (qkv[0] @ qkv[1].transpose(-2, -1)) * blk.attn.scale
            y = (a.softmax(dim=-1) @ qkv[2]).transpose(1, 2).reshape(V, N, C)
            t = t + blk.attn.proj(y)
            t = t + blk.mlp.fc2(F.gelu(blk.mlp.fc1(blk.norm2(t))))
        want = vit.norm(t)
    assert torch.equal(got, want) and torch.equal(same, want)


NEW = ("th_wgrad_chunk_rows", "th_layernorm_bwd_chunk_rows", "th_linear_train_workspace_bytes", "th_linear_train_forward",
       "th_linear_bwd_workspace_bytes", "th_linear_bwd", "th_layernorm_forward", "th_layernorm_bwd_workspace_bytes",
       "th_layernorm_bwd")


def test_header_exports_and_binding_table_carry_the_new_entries():
    import ctypes
    from transhuman_amd import build, hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "transhuman_hip.h")).read()
    build.build(force=False, verbose=False)
    raw = ctypes.CDLL(os.path.join(root, "transhuman_amd", "libtranshuman_hip.so"))
    for name in NEW:
        assert name in hip.SYMBOLS and name + "(" in header and hasattr(raw, name), name
    assert hip.load_library().th_abi_version() == 12


def test_workspace_queries():
    from transhuman_amd import hip
    lib = hip.load_library()
    chunk, ln_rows = lib.th_wgrad_chunk_rows(), lib.th_layernorm_bwd_chunk_rows()
    assert chunk == hip.wgrad_chunk_rows() > 0 and chunk % 16 == 0 and ln_rows > 0
    rows = sorted((1, chunk - 1, chunk, chunk + 1, 900, 1500, 3 * chunk + 5, 4500))
    for in_f, out_f in SHAPES:
        for form in (hip.OPERAND_PLAIN, hip.OPERAND_LN, hip.OPERAND_GELU):
            if form == hip.OPERAND_LN and in_f > 256:
                assert lib.th_linear_bwd_workspace_bytes(900, out_f, in_f, form) == 0
                assert lib.th_linear_train_workspace_bytes(900, out_f, in_f, form) == 0
                continue
            sizes = [lib.th_linear_bwd_workspace_bytes(M, out_f, in_f, form) for M in rows]
            assert sizes == sorted(sizes) and sizes[0] > 0, (in_f, out_f, form, sizes)
            for M, n in zip(rows, sizes):
                chunks = -(-M // chunk)
                # one partial tile set (weights + bias) per chunk, and the W^T image of the input gradient
                assert n >= chunks * (out_f * in_f + out_f) * 4 + out_f * in_f * 4, (M, n)
            fwd = [lib.th_linear_train_workspace_bytes(M, out_f, in_f, form) for M in rows]
            assert fwd == sorted(fwd) and fwd[0] >= lib.th_linear_workspace_bytes(out_f, in_f)
            if form == hip.OPERAND_GELU:
                assert fwd[-1] >= lib.th_linear_workspace_bytes(out_f, in_f) + rows[-1] * in_f * 4
    sizes = [lib.th_layernorm_bwd_workspace_bytes(M, 192) for M in rows]
    assert sizes == sorted(sizes)
    for M, n in zip(rows, sizes):
        assert n >= -(-M // ln_rows) * 2 * 192 * 4
    # refused shapes: a size of 0
    for q in (lib.th_linear_bwd_workspace_bytes, lib.th_linear_train_workspace_bytes):
        assert q(0, 192, 192, 0) == 0 and q(64, 200, 192, 0) == 0 and q(64, 192, 200, 0) == 0 and q(64, 192, 192, 3) == 0
    assert lib.th_layernorm_bwd_workspace_bytes(0, 192) == 0 and lib.th_layernorm_bwd_workspace_bytes(64, 200) == 0
    assert lib.th_layernorm_bwd_workspace_bytes(64, 272) == 0
