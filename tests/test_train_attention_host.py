"""The training form of TransHE's attention on the host: the float64 restatement of its adjoint
(train_ops.attention_grad_oracle, the formulas of k_vit_bwd.hip) against torch's float64 autograd of oracle.attention, and
the switch cfg.train_attention: "torch" by default, "device" refuses a CPU batch, anything else is a ValueError, and
vit_forward at the default is the function it was."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import th_oracle as O
from transhuman_amd.config import get_cfg, override
from transhuman_amd.networks import autograd_path, train_ops
from util import make_net

HEADS = 3
TOL = 1e-10


@pytest.mark.parametrize("V,N", ((1, 1), (2, 17), (3, 65)))
def test_attention_adjoint_equals_autograd(V, N):
    rs = np.random.RandomState(10 * V + N)
    qkv = torch.from_numpy(rs.normal(scale=3.0, size=(V, N, 3 * HEADS * 64))).requires_grad_(True)
    g = torch.from_numpy(rs.normal(size=(V, N, HEADS * 64)))
    O.attention(qkv, HEADS).backward(g)
    ref = qkv.grad.numpy()
    got, lse = train_ops.attention_grad_oracle(qkv, g, HEADS)
    assert got.dtype == np.float64 and got.shape == ref.shape
    scale = float(np.abs(ref).max())
    assert scale > 0
    assert float(np.abs(got - ref).max()) <= TOL * scale
    q, k = (qkv.detach().reshape(V, N, 3, HEADS, 64).permute(2, 0, 3, 1, 4)[i] for i in range(2))
    want = torch.logsumexp((q @ k.transpose(-2, -1)) * 0.125, dim=-1).numpy()
    assert lse.shape == (V, HEADS, N)
    assert float(np.abs(lse - want).max()) <= TOL * float(np.abs(want).max())


def test_switch_defaults_to_torch():
    from transhuman_amd.config import _defaults
    assert _defaults().train_attention == "torch" and get_cfg().train_attention == "torch"


def test_device_refuses_a_cpu_batch_and_a_bad_value_is_an_error():
    from transhuman_amd import hip
    batch = {"ray_o": torch.zeros(1, 4, 3), "ray_d": torch.ones(1, 4, 3)}
    renderer = SimpleNamespace(net=None)
    vit = make_net(2).ViT
    x, pe = torch.zeros(1, 5, 192), torch.zeros(1, 5, 3)
    with override(train_attention="device"), pytest.raises(hip.HipError, match="MI355X"):
        autograd_path.render(renderer, batch)
    with override(train_attention="hip"), pytest.raises(ValueError, match="train_attention"):
        autograd_path.render(renderer, batch)
    with pytest.raises(hip.HipError, match="MI355X"):
        autograd_path.vit_forward(vit, x, pe, attention="device")
    with pytest.raises(ValueError, match="train_attention"):
        autograd_path.vit_forward(vit, x, pe, attention="hip")
    with pytest.raises(hip.HipError):
        train_ops.AttentionFn.apply(torch.zeros(1, 5, 576, requires_grad=True), HEADS)


def test_vit_forward_at_the_default_is_unchanged():
    vit = make_net(2).ViT
    rs = np.random.RandomState(3)
    x = torch.from_numpy(rs.normal(size=(2, 17, 192)).astype(np.float32))
    pe = torch.from_numpy(rs.uniform(-1, 1, size=(2, 17, 3)).astype(np.float32))
    with torch.no_grad():
        a = autograd_path.vit_forward(vit, x, pe)
        b = autograd_path.vit_forward(vit, x, pe, attention="torch")
    assert torch.equal(a, b)


def test_header_exports_and_binding_table_carry_the_new_entries():
    """(tests/test_cabi.py holds the three to each other; this names the additions)"""
    from transhuman_amd import hip
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "transhuman_hip.h")).read()
    for name in ("th_attention_train_workspace_bytes", "th_attention_train", "th_attention_bwd_workspace_bytes",
                 "th_attention_bwd"):
        assert name in hip.SYMBOLS and name + "(" in header
    lib = hip.load_library()
    assert lib.th_abi_version() == 12
    assert lib.th_attention_train_workspace_bytes(3, 500, 3) == lib.th_attention_workspace_bytes(3, 500, 3) > 0
    assert lib.th_attention_bwd_workspace_bytes(3, 500, 3) >= 3 * 3 * 500 * 4
    for fn in (lib.th_attention_train_workspace_bytes, lib.th_attention_bwd_workspace_bytes):
        assert fn(3, 0, 3) == 0 and fn(3, 500, 0) == 0 and fn(0, 500, 3) == 0
