"""K17 on the device: the HIP adjoints of the token blend (K4), the pixel-aligned gather (K5) and the compositing (K7), and
the training entry with cfg.train_kernels = "device".

K4 and K5 are linear in the tensor that gets the gradient, so their backward is held to the EXACT adjoint of the forward
that tests/test_gpu_parity.py pins: the forward's own weight matrix W is read out of it with one-hot inputs (a blend of
one-hot rows returns the weights themselves, bit for bit), the reference is sum_p W[p,d] g[p,...] in float64, and the
tolerance per element is derived, not chosen:  (n + 2) 2^-24 sum_p |W[p,d] g[p,...]|  with n the number of non-zero terms
-- fp32 summation of n terms in any order plus the rounding of each product.  An element without terms must be exactly 0.

K7 is non-linear: the reference is composite_grad_oracle (float64), the bar 4 x the error of torch's own fp32 backward of
autograd_path.composite on the same inputs (at least 2^-22 of the largest reference value)."""
import numpy as np
import pytest
import torch

from transhuman_amd import config, synth
from transhuman_amd.networks import autograd_path, train_ops
from dparf_cases import dparf_forward_weights
from train_step_case import STEP_CFG, check_step, golden, setup

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def hip(gpu):
    from transhuman_amd import hip as H
    H.load_library()
    return H


def _check_adjoint(got, Wm, g, spec):
    """got = device result, Wm = forward weights (float64), g = upstream gradient (float64); einsum `spec` maps (Wm, g) to
    got's layout.  The derived bound, and exact zeros where nothing contributes."""
    Wm, g = torch.from_numpy(np.ascontiguousarray(Wm)), torch.from_numpy(np.ascontiguousarray(g))
    ref = torch.einsum(spec, Wm, g).numpy()
    mag = torch.einsum(spec, Wm.abs(), g.abs()).numpy()
    n = np.rint(torch.einsum(spec, (Wm != 0).double(), torch.ones_like(g)).numpy())
    got = got.double().cpu().numpy()
    assert got.shape == ref.shape and np.isfinite(got).all()
    assert (got[n == 0] == 0).all()
    tol = (n + 2) * EPS * mag
    err = np.abs(got - ref)
    worst = float((err / np.maximum(tol, 1e-300))[n > 0].max()) if (n > 0).any() else 0.0
    print(f"adjoint {spec}: n up to {int(n.max())}, worst error / bound = {worst:.3f}")
    assert (err <= tol).all(), worst


# ---- K4 ---------------------------------------------------------------------------------------------------------------------
def _dparf_case(P, nc, V, seed, near_one=False):
    rs = np.random.RandomState(seed)
    cen = rs.normal(0, 0.3, (nc, 3)).astype(np.float32)
    if near_one:
        # every point within 1 cm of centre 0, which sits with six companions away from all the others
        cen[0] = 5.0
        cen[1:7] = cen[0] + rs.normal(0, 0.03, (6, 3)).astype(np.float32)
        pts = cen[0] + (rs.uniform(-0.01, 0.01, (P, 3)) / np.sqrt(3.0)).astype(np.float32)
    else:
        pts = cen[rs.randint(0, nc, P)] + rs.normal(0, 0.05, (P, 3)).astype(np.float32)
    rot = rs.normal(size=(nc, 9)).astype(np.float32)
    g = rs.normal(size=(P, V, 256)).astype(np.float32)
    return [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)) for a in (pts, cen, rot, g)]


@pytest.mark.parametrize("P,nc,V,near_one", [(1, 7, 1, False), (129, 7, 3, False), (3000, 300, 3, False), (3000, 300, 3, True)])
def test_dparf_backward_is_the_adjoint_of_the_forward(hip, gpu, P, nc, V, near_one):
    pts, cen, rot, g = (t.to(gpu) for t in _dparf_case(P, nc, V, seed=P + nc, near_one=near_one))
    Wm = dparf_forward_weights(hip, pts, cen, rot)
    if near_one:
        assert ((Wm != 0).sum(0) == P).sum() == 7                  # seven lists of length P: the chunk split
    out = torch.full((V, nc, 192), float("nan"), device=gpu)       # the kernel writes every element
    got = hip.dparf_encode_bwd(pts, cen, rot, g, out=out)
    assert got is out
    _check_adjoint(got, Wm, g[..., :192].double().cpu().numpy(), "pc,pvj->vcj")
    again = hip.dparf_encode_bwd(pts, cen, rot, g)
    assert torch.equal(got, again)                                 # no float atomics: bit-identical from run to run
    # columns 192..255 (positional encoding, pad) do not reach the tokens
    g2 = g.clone()
    g2[..., 192:] = float("nan")
    assert torch.equal(hip.dparf_encode_bwd(pts, cen, rot, g2), got)


def test_dparf_backward_without_samples_writes_zeros(hip, gpu):
    _, cen, rot, _ = (t.to(gpu) for t in _dparf_case(1, 9, 2, seed=0))
    out = torch.full((2, 9, 192), float("nan"), device=gpu)
    hip.dparf_encode_bwd(torch.zeros((0, 3), device=gpu), cen, rot, torch.zeros((0, 2, 256), device=gpu), out=out)
    assert (out == 0).all()


def test_backward_entry_points_refuse_bad_arguments(hip, gpu):
    lib, ctx = hip._lib, hip.ctx(gpu)
    pts, cen, rot, g = (t.to(gpu) for t in _dparf_case(5, 9, 1, seed=0))
    out = torch.zeros((1, 9, 192), device=gpu)
    nb = int(lib.th_dparf_encode_bwd_workspace_bytes(5, 1, 9))
    ws = torch.zeros(nb, dtype=torch.uint8, device=gpu)
    p = hip._p
    assert lib.th_dparf_encode_bwd(ctx, p(pts), 5, p(cen), p(rot), 1, 9, p(g), p(out), p(ws), nb - 1, None) < 0
    assert b"workspace" in lib.th_last_error()
    assert lib.th_dparf_encode_bwd(ctx, p(pts), 5, p(cen), p(rot), 1, 6, p(g), p(out), p(ws), nb, None) < 0
    assert b"7 token centres" in lib.th_last_error()
    assert lib.th_dparf_encode_bwd(ctx, None, 5, p(cen), p(rot), 1, 9, p(g), p(out), p(ws), nb, None) < 0
    assert b"null" in lib.th_last_error()
    m = torch.zeros((1, 4, 4, 8), device=gpu)
    cams, sc = torch.zeros((1, 21), device=gpu), torch.ones(2, device=gpu)
    assert lib.th_pixel_gather_bwd(ctx, 1, 6, 4, 4, p(pts), 5, p(cams), p(sc), p(g), 256, p(m), None) < 0
    assert b"multiples of 4" in lib.th_last_error()
    assert lib.th_pixel_gather_bwd(ctx, 1, 8, 4, 4, p(pts), 5, p(cams), p(sc), None, 256, p(m), None) < 0
    assert b"null" in lib.th_last_error()
    with pytest.raises(hip.HipError, match="S <= 256"):
        hip.composite_bwd(torch.zeros((2, 300, 4), device=gpu), torch.zeros((2, 300), device=gpu), torch.ones((2, 3), device=gpu),
                          torch.zeros((2, 3), device=gpu), torch.zeros(2, device=gpu), torch.zeros(2, device=gpu))


# ---- K5 ---------------------------------------------------------------------------------------------------------------------
PH, PW, PV = 12, 16, 3


def _pix_geometry(gpu):
    from transhuman_amd import hip as H
    b = synth.make_batch(PH, PW, PV, seed=1)
    R, T, K = b["input_R"][0][0], b["input_T"][0][0], b["input_K"][0][0]
    scale = torch.tensor([2.0 / PW, 2.0 / PH])
    return (R, T, K), H.pack_cams(R.to(gpu), T.to(gpu), K.to(gpu)), scale


def _pix_forward_weights(hip, pts, cams, scale):
    """Wt[p,v,texel]: the forward's bilinear weights, read with the identity map (channel = texel)"""
    eye = torch.eye(PH * PW, device=pts.device).reshape(1, PH, PW, PH * PW).repeat(PV, 1, 1, 1).contiguous()
    Wt = hip.pixel_gather(eye, pts, cams, scale).double().cpu()
    if pts.shape[0]:
        assert float((Wt.sum(-1) - 1).abs().max()) < 1e-5 and int((Wt != 0).sum(-1).max()) <= 4
    return Wt.numpy()


def _pix_check(hip, gpu, pts, ldo):
    _, cams, scale = _pix_geometry(gpu)
    pts, scale = pts.to(gpu), scale.to(gpu)
    Wt = _pix_forward_weights(hip, pts, cams, scale)
    torch.manual_seed(5)
    g = torch.randn((pts.shape[0], PV, ldo), device=gpu)
    out = torch.full((PV, PH, PW, 384), float("nan"), device=gpu)   # the call clears the map itself
    got = hip.pixel_gather_bwd((PV, PH, PW, 384), pts, cams, scale, g, out=out)
    _check_adjoint(got.reshape(PV, PH * PW, 384), Wt, g[..., :384].double().cpu().numpy(), "pvt,pvc->vtc")
    return Wt


@pytest.mark.parametrize("ldo", [384, 400])
def test_pixel_gather_backward_is_the_adjoint_of_the_forward(hip, gpu, ldo):
    torch.manual_seed(3)
    pts = torch.randn(777, 3) * 0.6 + torch.tensor([0.0, 0.0, 3.0])
    (R, T, K), _, scale = _pix_geometry(gpu)
    grid = autograd_path.project(pts, R, T, K) * scale - 1.0
    outside = (grid.abs() > 1).any(-1)
    assert outside.any() and not outside.all()                      # border clamp and interior both present
    _pix_check(hip, gpu, pts, ldo)


def test_pixel_gather_backward_many_samples_on_one_texel(hip, gpu):
    Wt = _pix_check(hip, gpu, torch.tensor([[0.02, -0.03, 3.0]]).repeat(500, 1), 384)
    assert int((Wt[:, 0] != 0).all(0).sum()) >= 1                   # one texel takes all 500 samples


def test_pixel_gather_backward_without_samples_writes_zeros(hip, gpu):
    _, cams, scale = _pix_geometry(gpu)
    out = torch.full((PV, PH, PW, 384), float("nan"), device=gpu)
    hip.pixel_gather_bwd((PV, PH, PW, 384), torch.zeros((0, 3), device=gpu), cams, scale.to(gpu),
                         torch.zeros((0, PV, 384), device=gpu), out=out)
    assert (out == 0).all()


# ---- K7 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("white", [False, True])
@pytest.mark.parametrize("S", [64, 96, 7, 1])
def test_composite_backward_vs_float64(hip, gpu, S, white):
    rs = np.random.RandomState(3 + S)
    R = 50
    for dense in (1.0, 10.0):
        raw = rs.normal(0, 2, (R, S, 4)).astype(np.float32)
        raw[..., 3] *= dense
        raw[0, :, 3] = -np.abs(raw[0, :, 3])                         # a ray whose densities are all <= 0
        raw[0, 0, 3] = 0.0
        raw, z = torch.from_numpy(raw), torch.sort(torch.from_numpy(rs.uniform(2, 4, (R, S)).astype(np.float32)), dim=1)[0]
        d = torch.from_numpy(rs.normal(size=(R, 3)).astype(np.float32))
        g_rgb, g_acc, g_dep = (torch.from_numpy(rs.normal(size=s).astype(np.float32)) for s in ((R, 3), (R,), (R,)))
        ref = train_ops.composite_grad_oracle(raw, z, d, white, g_rgb, g_acc, g_dep)
        scale = float(np.abs(ref).max())
        # the yardstick: torch's own fp32 backward of the training entry's composite, on the CPU
        rt = raw.clone().requires_grad_(True)
        rgb, acc, dep = autograd_path.composite(rt, z, d, 0.0, white)
        ((rgb * g_rgb).sum() + (acc * g_acc).sum() + (dep * g_dep).sum()).backward()
        parent = float(np.abs(rt.grad.double().numpy() - ref).max())
        bound = 4.0 * max(parent, 2.0 ** -22 * scale)
        args = [t.to(gpu) for t in (raw, z, d, g_rgb, g_acc, g_dep)]
        got = hip.composite_bwd(*args, white_bkgd=white)
        assert torch.isfinite(got).all()
        err = float(np.abs(got.double().cpu().numpy() - ref).max())
        print(f"S={S} white={white} dense={dense}: device {err / scale:.3e}, torch fp32 {parent / scale:.3e} of max|ref| = {scale:.3e}")
        assert err <= bound, (err, bound)
        assert (got[0, :, 3] == 0).all()
        assert torch.equal(got, hip.composite_bwd(*args, white_bkgd=white))
        # and through the autograd Function
        rg = args[0].clone().requires_grad_(True)
        o = train_ops.CompositeFn.apply(rg, args[1], args[2], white)
        ((o[0] * args[3]).sum() + (o[1] * args[4]).sum() + (o[2] * args[5]).sum()).backward()
        assert torch.equal(rg.grad, got)


# ---- the training entry -----------------------------------------------------------------------------------------------------
def test_training_step_on_the_device_kernels_matches_the_reference(hip, gpu):
    """tests/test_train_path.py::test_training_step_matches_the_reference with cfg.train_kernels = "device": the same golden
    step of the real reference, the same bars"""
    with config.override(**STEP_CFG, train_kernels="device"):
        check_step(golden(), *setup(gpu))


def test_switch_defaults_to_torch_and_device_refuses_a_cpu_batch(hip, gpu):
    from types import SimpleNamespace
    assert config.get_cfg().train_kernels == "torch"
    batch = {"ray_o": torch.zeros(1, 4, 3), "ray_d": torch.ones(1, 4, 3)}
    with config.override(train_kernels="device"):
        with pytest.raises(hip.HipError, match="MI355X"):
            autograd_path.render(SimpleNamespace(net=None), batch)
