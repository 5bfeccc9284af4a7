"""K19 on the host: the float64 restatements of the latent gather and its adjoint (train_ops.latent_gather_oracle /
latent_grad_oracle) against the torch composition they replace, in float64: F.interpolate(bilinear, align_corners=True) of
every latent -> cat with the colour lift -> grid_sample(bilinear, align_corners=True, border), and that composition's
autograd.  Both sides are float64 evaluations of one formula, so the bar (1e-12 of the largest reference value) covers the
order of operations only.  Plus the switch (cfg.train_maps defaults to "full", "latents" refuses a CPU batch, a bad value
raises) and the C ABI entries."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from transhuman_amd.config import get_cfg, override
from transhuman_amd.networks import autograd_path, train_ops
from transhuman_amd.networks.encoder import SpatialEncoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12

# (H, W), the three latent sizes
SHAPES = [((20, 28), ((10, 14), (5, 7), (3, 4))),
          ((33, 17), ((17, 9), (9, 5), (5, 3))),
          ((12, 16), ((6, 8), (3, 4), (1, 1)))]          # a 1 x 1 level: upsample scale 0


def _close(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape
    scale = float(np.abs(ref).max())
    assert scale > 0
    err = float(np.abs(got - ref).max())
    assert err <= TOL * scale, (err, scale)


def _points(rs, V, H, W):
    """pixel coordinates uv [V,N,2]: inside, beyond each of the four borders, exactly on texel centres, on the last row / column"""
    uv = rs.uniform(0.0, 1.0, (V, 200, 2)) * np.array([W - 1.0, H - 1.0])
    special = np.array([[-2.5, 0.4 * H], [W + 1.7, 0.6 * H], [0.3 * W, -3.0], [0.7 * W, H + 2.2],        # beyond the four borders
                        [-4.0, -4.0], [W + 3.0, H + 3.0],
                        [0.0, 0.0], [3.0, 5.0], [W - 2.0, H - 2.0], [2.0, 0.0], [0.0, 7.0],               # on texel centres
                        [W - 1.0, 4.3], [5.6, H - 1.0], [W - 1.0, H - 1.0], [W - 1.0, 0.0], [0.0, H - 1.0],  # last row / column
                        [W - 1.0, 3.0], [4.0, H - 1.0], [W - 1.25, H - 1.5]])
    uv[:, :len(special)] = special
    return torch.from_numpy(uv)


def _case(shape_id, V=2, seed=0):
    (H, W), dims = SHAPES[shape_id]
    rs = np.random.RandomState(seed + shape_id)
    lats = [torch.from_numpy(rs.normal(size=(V, h, w, C))).requires_grad_(True) for (h, w), C in zip(dims, (64, 64, 128))]
    lift_w = torch.from_numpy(rs.normal(size=(128, 3))).requires_grad_(True)
    lift_b = torch.from_numpy(rs.normal(size=(128,))).requires_grad_(True)
    img = torch.from_numpy(rs.uniform(0, 1, (V, 3, H, W)))
    uv = _points(rs, V, H, W)
    g = torch.from_numpy(rs.normal(size=(uv.shape[1], V, 384)))
    return (H, W), lats, lift_w, lift_b, img, uv, g


def _torch_composition(H, W, lats, lift_w, lift_b, img, uv):
    """autograd_path.encode's tail and sample_map on channels-last latents, float64 -> rows [N,V,384]"""
    up = [F.interpolate(l.permute(0, 3, 1, 2), (H, W), mode="bilinear", align_corners=True) for l in lats]
    pix = torch.cat(up + [F.conv2d(img, lift_w.reshape(128, 3, 1, 1), lift_b)], dim=1)
    return autograd_path.sample_map(pix, uv, SpatialEncoder, (H, W)).permute(2, 0, 1)


def _scale(H, W):
    from transhuman_amd import hip
    return hip.feat_scale(SpatialEncoder.feat_scale(H, W), (H, W), "cpu").double()


@pytest.mark.parametrize("shape_id", range(len(SHAPES)))
def test_latent_gather_oracle_equals_the_torch_composition(shape_id):
    (H, W), lats, lift_w, lift_b, img, uv, _ = _case(shape_id)
    ref = _torch_composition(H, W, lats, lift_w, lift_b, img, uv).detach()
    rows, rgb_s = train_ops.latent_gather_oracle(*lats, lift_w, lift_b, img, uv, _scale(H, W))
    _close(rows, ref.numpy())
    for k in range(4):                                   # the four column blocks, each on its own scale
        lo, hi = (0, 64, 128, 256)[k], (64, 128, 256, 384)[k]
        _close(rows[..., lo:hi], ref[..., lo:hi].numpy())
    raw = autograd_path.sample_map(img, uv, SpatialEncoder, (H, W)).permute(2, 0, 1)
    _close(rgb_s[..., :3], raw.numpy())
    assert (rgb_s[..., 3] == 0).all()


@pytest.mark.parametrize("shape_id", range(len(SHAPES)))
def test_latent_grad_oracle_equals_autograd_of_the_composition(shape_id):
    (H, W), lats, lift_w, lift_b, img, uv, g = _case(shape_id)
    out = _torch_composition(H, W, lats, lift_w, lift_b, img, uv)
    ref = torch.autograd.grad((out * g).sum(), [*lats, lift_w, lift_b])
    _, rgb_s = train_ops.latent_gather_oracle(*lats, lift_w, lift_b, img, uv, _scale(H, W))
    got = train_ops.latent_grad_oracle(uv, _scale(H, W), (H, W), [tuple(l.shape) for l in lats], rgb_s, g)
    assert len(got) == 5
    for a, b in zip(got, ref):
        _close(a, b.numpy())


def test_every_non_zero_tap_lies_in_three_rows_and_three_columns():
    """the tap bound of K19: per level the 16 composite taps with a non-zero coefficient fall on at most 3 x 3 texels whose
    first row / column is the first tap's"""
    for (H, W), dims in SHAPES:
        uv = _points(np.random.RandomState(9), 1, H, W)
        for h, w in dims:
            taps = train_ops._latent_taps64(uv, _scale(H, W), H, W, h, w)
            a, b = taps[0][0], taps[0][1]
            for ry, rx, cf in taps:
                nz = cf != 0
                assert ((ry - a)[nz] >= 0).all() and ((ry - a)[nz] <= 2).all()
                assert ((rx - b)[nz] >= 0).all() and ((rx - b)[nz] <= 2).all()
            assert np.abs(sum(t[2] for t in taps) - 1.0).max() < 1e-12


def test_switch_defaults_to_full_refuses_a_cpu_batch_and_a_bad_value():
    from transhuman_amd import hip
    assert get_cfg().train_maps == "full"
    batch = {"ray_o": torch.zeros(1, 4, 3), "ray_d": torch.ones(1, 4, 3)}
    with override(train_maps="latents"), pytest.raises(hip.HipError, match="MI355X"):
        autograd_path.render(SimpleNamespace(net=None), batch)
    with override(train_maps="half"), pytest.raises(ValueError, match="train_maps"):
        autograd_path.render(SimpleNamespace(net=None), batch)


def test_function_refuses_host_tensors_and_batch_gradients():
    from transhuman_amd import hip
    (H, W), lats, lift_w, lift_b, img, uv, _ = _case(0)
    f32 = lambda t: t.detach().float()
    args = [f32(l) for l in lats] + [f32(lift_w), f32(lift_b), f32(img), torch.zeros(5, 3), torch.zeros(2, 21), torch.ones(2)]
    with pytest.raises(hip.HipError, match="MI355X"):
        train_ops.LatentGatherFn.apply(*args)
    args[6] = args[6].requires_grad_(True)
    with pytest.raises(ValueError, match="pts_world"):
        train_ops.LatentGatherFn.apply(*args)


@pytest.fixture(scope="module")
def lib():
    from transhuman_amd import build, hip
    build.build(force=False, verbose=False)
    return hip.load_library()


def test_latent_gather_entry_points_declared_exported_bound(lib):
    from transhuman_amd import hip
    C = ctypes
    header = open(os.path.join(ROOT, "include", "transhuman_hip.h")).read()
    raw = ctypes.CDLL(os.path.join(ROOT, "transhuman_amd", "libtranshuman_hip.so"))
    for name in ("th_latent_gather", "th_latent_gather_bwd"):
        assert f"{name}(" in header
        assert hasattr(raw, name)
        assert name in hip.SYMBOLS
        res, args = hip.SYMBOLS[name]
        decl = header[header.index(f"int {name}("):]
        decl = decl[:decl.index(";")]
        assert res is C.c_int and decl.count(",") + 1 == len(args)
    assert callable(hip.latent_gather) and callable(hip.latent_gather_bwd)
    assert lib.th_abi_version() == 12


def test_latent_gather_entry_points_refuse_null_arguments_without_a_device(lib):
    dims = (ctypes.c_int32 * 6)(2, 2, 2, 2, 2, 2)
    assert lib.th_latent_gather(None, None, None, None, dims, None, None, None, 1, 4, 4, None, 0, None, None, None, 384, None,
                                None) < 0
    assert b"null" in lib.th_last_error()
    assert lib.th_latent_gather_bwd(None, dims, 1, 4, 4, None, 0, None, None, None, 384, None, None, None, None) < 0
    assert b"null" in lib.th_last_error()
