"""K17 on the host: the float64 restatements of the three adjoints (transhuman_amd/networks/train_ops.py) against torch
autograd in float64 through the training entry's own stages -- autograd_path.human_representation / sample_map / composite,
which tests/test_train_path.py pins to the real reference (g18_train_step).  Both sides are float64 evaluations of one
formula, so the tolerance (1e-12 of the largest reference value) covers the order of operations only.  Plus the switch:
cfg.train_kernels defaults to "torch", and "device" refuses a CPU batch."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from transhuman_amd.config import get_cfg, override
from transhuman_amd.networks import autograd_path, train_ops
from transhuman_amd.networks.encoder import SpatialEncoder

TOL = 1e-12


def _close(got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape
    scale = float(np.abs(ref).max())
    assert scale > 0
    err = float(np.abs(got - ref).max())
    assert err <= TOL * scale, (err, scale)


def test_token_blend_adjoint_equals_autograd():
    rs = np.random.RandomState(0)
    P, nc, V = 257, 40, 2
    pts = torch.from_numpy(rs.normal(0, 0.4, (P, 3)))
    cen = torch.from_numpy(rs.normal(0, 0.4, (nc, 3)))
    rot = torch.from_numpy(rs.normal(size=(nc, 3, 3)))
    tok = torch.from_numpy(rs.normal(size=(V, nc, 192))).requires_grad_(True)
    g = torch.from_numpy(rs.normal(size=(P, V, 255)))
    net = SimpleNamespace(PE_relative=lambda x: torch.cat([x] * 21, -1))         # (63 columns that do not touch the tokens)
    h = autograd_path.human_representation(net, pts, cen, rot, tok, 7, 0.5)
    assert h.shape == (P, V, 255)
    ref, = torch.autograd.grad((h * g).sum(), tok)
    got = train_ops.dparf_token_grad_oracle(pts, cen, V, g)
    _close(got, ref.numpy())
    assert (got.reshape(V, nc, -1) != 0).any(-1).any(0).sum() > 7               # many destinations, each hit many times


def test_pixel_gather_adjoint_equals_autograd():
    from transhuman_amd import hip
    rs = np.random.RandomState(1)
    V, C, H, W, N = 2, 8, 12, 16, 301
    feat = torch.from_numpy(rs.normal(size=(V, C, H, W))).requires_grad_(True)
    uv = torch.from_numpy(rs.uniform(-3.0, 19.0, (V, N, 2)))                      # image 16 x 12: some land outside (border)
    uv[0, :5] = torch.tensor([[0.0, 0.0], [15.0, 11.0], [7.0, 3.0], [15.0, 0.5], [2.5, 11.0]], dtype=torch.float64)
    g = torch.from_numpy(rs.normal(size=(N, V, C)))
    out = autograd_path.sample_map(feat, uv, SpatialEncoder, (H, W))              # [V,C,N]
    ref, = torch.autograd.grad((out.permute(2, 0, 1) * g).sum(), feat)
    scale = hip.feat_scale(SpatialEncoder.feat_scale(H, W), (H, W), "cpu")
    got = train_ops.pixel_map_grad_oracle(uv, scale, H, W, g)
    _close(got, ref.permute(0, 2, 3, 1).numpy())


@pytest.mark.parametrize("white", [False, True])
@pytest.mark.parametrize("S", [64, 96, 7, 1])
def test_composite_adjoint_equals_autograd(S, white):
    rs = np.random.RandomState(10 + S)
    R = 24
    raw = rs.normal(0, 2, (R, S, 4))
    raw[R // 2:, :, 3] *= 10.0
    raw[0, :, 3] = -np.abs(raw[0, :, 3])                                          # a ray without density
    z = np.sort(rs.uniform(2, 4, (R, S)), axis=1)
    d = rs.normal(size=(R, 3))
    g_rgb, g_acc, g_dep = rs.normal(size=(R, 3)), rs.normal(size=R), rs.normal(size=R)
    rt = torch.from_numpy(raw).requires_grad_(True)
    rgb, acc, dep = autograd_path.composite(rt, torch.from_numpy(z), torch.from_numpy(d), 0.0, white)
    loss = (rgb * torch.from_numpy(g_rgb)).sum() + (acc * torch.from_numpy(g_acc)).sum() + (dep * torch.from_numpy(g_dep)).sum()
    ref, = torch.autograd.grad(loss, rt)
    got = train_ops.composite_grad_oracle(raw, z, d, white, g_rgb, g_acc, g_dep)
    _close(got, ref.numpy())
    assert (got[0, :, 3] == 0).all()


def test_inputs_without_a_gradient_path_are_refused():
    t = torch.zeros(2, 7, 192, requires_grad=True)
    p = torch.zeros(3, 3, requires_grad=True)
    with pytest.raises(ValueError, match="pts_smpl"):
        train_ops.HumanRepresentationFn.apply(t, p, torch.zeros(7, 3), torch.zeros(7, 9))
    with pytest.raises(ValueError, match="pts_world"):
        train_ops.PixelGatherFn.apply(torch.zeros(2, 4, 4, 8, requires_grad=True), p, torch.zeros(2, 21), torch.zeros(2))
    with pytest.raises(ValueError, match="z"):
        train_ops.CompositeFn.apply(torch.zeros(3, 4, 4, requires_grad=True), torch.zeros(3, 4, requires_grad=True),
                                    torch.zeros(3, 3), False)


def test_switch_defaults_to_torch_and_device_refuses_a_cpu_batch():
    from transhuman_amd import hip
    from transhuman_amd.config import _defaults
    assert _defaults().train_kernels == "torch" and get_cfg().train_kernels == "torch"
    batch = {"ray_o": torch.zeros(1, 4, 3), "ray_d": torch.ones(1, 4, 3)}
    renderer = SimpleNamespace(net=None)
    with override(train_kernels="device"), pytest.raises(hip.HipError, match="MI355X"):
        autograd_path.render(renderer, batch)
    with override(train_kernels="hip"), pytest.raises(ValueError, match="train_kernels"):
        autograd_path.render(renderer, batch)


# ---- all seven switches: the table, the one reader, and the override the tests set them with ---------------------------------
def test_override_restores_a_changed_key_deletes_an_absent_one_also_after_an_exception():
    cfg = get_cfg()
    before = cfg.N_samples
    assert before != 7 and not hasattr(cfg, "no_such_key")
    with override(N_samples=7, no_such_key=1) as live:
        assert live is cfg and cfg.N_samples == 7 and cfg.no_such_key == 1
    assert cfg.N_samples == before and not hasattr(cfg, "no_such_key")
    with pytest.raises(RuntimeError, match="inside"):
        with override(N_samples=7, no_such_key=1):
            cfg.N_samples = 9                                      # (what the block itself assigns is put back too)
            raise RuntimeError("inside")
    assert cfg.N_samples == before and not hasattr(cfg, "no_such_key")


def test_defaults_are_the_first_values_of_the_table():
    from transhuman_amd.config import TRAIN_SWITCHES, _defaults
    assert list(TRAIN_SWITCHES) == ["train_kernels", "train_attention", "train_vit_dense", "train_maps", "train_gather_bwd",
                                    "train_point_net", "train_encoder"]
    for key, values in TRAIN_SWITCHES.items():
        assert len(values) == 2 and getattr(_defaults(), key) == getattr(get_cfg(), key) == values[0], key


def test_the_one_reader_of_every_switch():
    from transhuman_amd import hip
    from transhuman_amd.config import TRAIN_SWITCHES
    for key, values in TRAIN_SWITCHES.items():
        for v in values:
            assert autograd_path._switch(key, v, True) == v
        assert autograd_path._switch(key, values[0], False) == values[0]
        with pytest.raises(ValueError, match=f"cfg.{key} must be '{values[0]}' or '{values[1]}', not 'hip'"):
            autograd_path._switch(key, "hip", True)
        with pytest.raises(hip.HipError, match=f"cfg.{key} = '{values[1]}' needs the tokens on an MI355X .* use '{values[0]}' for"):
            autograd_path._switch(key, values[1], False, "tokens")
