"""The backward of the encoder trunk on the device (K23): th_bn_act_bwd, th_conv2d_dgrad / th_conv2d_wgrad, th_maxpool3x3s2_bwd
(k_encoder_bwd.hip), train_ops.ConvFn / BnActFn / MaxPoolFn, autograd_path.trunk_device and cfg.train_encoder = "device".

The reference everywhere is torch's CPU float64 autograd of the same stock operators on the fp32 inputs widened to float64.  With
t64 that reference and d32 torch's fp32 autograd ON THE DEVICE (MIOpen and torch's own kernels: what cfg.train_encoder = "torch"
runs), per gradient tensor

    parent = max|d32 - t64|,  scale = max|t64|,    bar = 4 max(parent, 2^-24 scale)

and every case prints err / bar of every tensor.  Both errors are taken here, in the test.

A ReLU gate is a discontinuous function of the pre-activation.  The per-kernel BatchNorm cases hand the kernel the site's output
itself, so the float64 reference and the kernel gate alike; torch's fp32 forward, which makes its own output, could gate an element
within rounding of 0 differently, so the arriving gradient is 0 at the elements whose float64 pre-activation lies within 1e-3 of 0
(asserted to be a small share).  What happens AT 0 is held exactly by the integer cases.  In the composed cases the device mode's
forward is torch's bit for bit, so both fp32 runs gate and route alike.

Convolution reference data are computed once per (shape, N, H, W) and shared by the dgrad and wgrad tests."""
import contextlib
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from transhuman_amd import config
from transhuman_amd.networks import autograd_path, train_ops
from train_step_case import STEP_CFG, check_step, golden, setup
from util import maxdiff

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -24
CONVS = {"3x3s1_64": (64, 64, 3, 1), "3x3s1_128": (128, 128, 3, 1), "3x3s2": (64, 128, 3, 2), "1x1s2": (64, 128, 1, 2),
         "conv1": (3, 64, 7, 2)}
SIZES = ((1, 1), (2, 3), (8, 16), (9, 17), (33, 47))
CONV1_SIZES = ((5, 6), (32, 32), (45, 37))


@pytest.fixture(scope="module")
def hip(gpu):
    from transhuman_amd import hip as H
    H.load_library()
    return H


@functools.lru_cache(maxsize=None)
def _consts():
    from transhuman_amd import build, hip as H
    build.build(force=False, verbose=False)
    return H.conv2d_wgrad_chunk_pixels(), H.conv2d_dgrad_tile(), H.bn_act_bwd_slice_elems()


def _conv_sizes(name):
    """the issue's sizes, + one input size just below, at and just above the dgrad tile (rows x columns of one parity class) and
    the wgrad chunk (output pixels; at N = 3 the counts 3 * 85 = chunk - 1 and 3 * 86 = chunk + 2 sit on the edge too)"""
    chunk, (tr, tc), _ = _consts()
    assert (chunk, tr, tc) == (256, 8, 16), "the edge sizes below are written for these constants"
    s = CONVS[name][3]
    sizes = list(SIZES) + (list(CONV1_SIZES) if name == "conv1" else [])
    sizes += [(s * tr - 1, s * tc - 1), (s * tr, s * tc), (s * tr + 1, s * tc + 1)]
    out = lambda ho, wo: (s * (ho - 1) + 1, s * (wo - 1) + 1)                   # an input size with ho x wo output pixels
    sizes += [out(15, 17), out(16, 16), out(1, 257), out(5, 17), out(2, 43)]
    return sorted(set(sizes))


def pytest_generate_tests(metafunc):
    if "conv_case" in metafunc.fixturenames:
        cases = [(name, N, hw) for name in CONVS for N in (1, 3) for hw in _conv_sizes(name)]
        metafunc.parametrize("conv_case", cases, ids=[f"{n}-N{N}-{h}x{w}" for n, N, (h, w) in cases])
    if "bn_size" in metafunc.fixturenames:
        sl = _consts()[2]
        assert sl == 8192
        metafunc.parametrize("bn_size", SIZES + ((1, sl - 1), (64, sl // 64), (3, (sl + 1) // 3)), ids=lambda s: f"{s[0]}x{s[1]}")


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def _hold(tag, got, t64, parents):
    failed, worst = [], 0.0
    for k, t in t64.items():
        v = got[k].detach().cpu().double()
        assert v.shape == t.shape and torch.isfinite(v).all(), (tag, k)
        scale, err = float(t.abs().max()), maxdiff(v, t)
        bar = 4.0 * max(parents[k], FLOOR * scale)
        ratio = err / bar if bar > 0 else (0.0 if err == 0 else float("inf"))
        worst = max(worst, ratio)
        print(f"{tag} {k}: device {err:.3e}, torch fp32 {parents[k]:.3e}, max|ref| = {scale:.3e}; err / bar = {ratio:.2f}")
        if not err <= bar:
            failed.append((k, err, bar))
    print(f"{tag}: worst err / bar = {worst:.2f}")
    assert not failed, (tag, failed)


# ---------------------------------------------------------------------------
# 1: the convolutions
# ---------------------------------------------------------------------------
def _conv_autograd(x, w, g, stride, need_x):
    x = x.clone().requires_grad_(need_x)
    w = w.clone().requires_grad_(True)
    F.conv2d(x, w, None, stride, w.shape[2] // 2).backward(g)
    return {"g_x": x.grad, "g_W": w.grad} if need_x else {"g_W": w.grad}


@functools.lru_cache(maxsize=None)
def _conv_case(name, N, hw, integers=False):
    cin, cout, ks, s = CONVS[name]
    H, W = hw
    Ho, Wo = (H + 2 * (ks // 2) - ks) // s + 1, (W + 2 * (ks // 2) - ks) // s + 1
    rs = np.random.RandomState(cin + 3 * cout + 7 * ks + 11 * N + 13 * H + 17 * W)
    if integers:                                           # |g_x| <= 128 * 9 * 3 * 2, |g_W| <= N Ho Wo * 9: exact in fp32
        x, w, g = (_f32(rs.randint(-a, a + 1, size=sh)) for a, sh in ((3, (N, cin, H, W)), (2, (cout, cin, ks, ks)),
                                                                         (3, (N, cout, Ho, Wo))))
        assert N * Ho * Wo * 9 < 2 ** 24
    else:
        x, g = _f32(rs.normal(size=(N, cin, H, W))), _f32(rs.normal(size=(N, cout, Ho, Wo)))
        w = _f32(rs.normal(scale=(cin * ks * ks) ** -0.5, size=(cout, cin, ks, ks)))
    t64 = _conv_autograd(x.double(), w.double(), g.double(), s, name != "conv1")
    return (x, w, g), t64


def _conv_parents(gpu, t, t64, stride):
    d32 = _conv_autograd(*(v.to(gpu) for v in t), stride, "g_x" in t64)
    return {k: maxdiff(d32[k].cpu().double(), t64[k]) for k in t64}


def _conv_run(hip, gpu, name, t):
    cin, cout, ks, s = CONVS[name]
    x, w, g = (v.to(gpu) for v in t)
    got = {"g_W": hip.conv2d_wgrad(x, g, ks, s)}
    assert torch.equal(got["g_W"], hip.conv2d_wgrad(x, g, ks, s)), "g_W: not bit-identical on two runs"
    if name != "conv1":
        packed = hip.conv2d_dgrad_pack(w, s)
        got["g_x"] = hip.conv2d_dgrad(g, w.shape, s, x.shape[2:], packed)
        assert torch.equal(got["g_x"], hip.conv2d_dgrad(g, w.shape, s, x.shape[2:], packed)), "g_x: not bit-identical on two runs"
    assert torch.equal(g.cpu(), t[2]) and torch.equal(x.cpu(), t[0]), "an input was modified"
    return got


def test_conv_gradients_vs_float64(hip, gpu, conv_case):
    name, N, hw = conv_case
    t, t64 = _conv_case(name, N, hw)
    got = _conv_run(hip, gpu, name, t)
    _hold(f"conv {name} N={N} {hw[0]}x{hw[1]}", got, t64, _conv_parents(gpu, t, t64, CONVS[name][3]))


@pytest.mark.parametrize("N,hw", ((3, (9, 17)), (1, (33, 47)), (1, (2, 3)), (3, (17, 33))))
@pytest.mark.parametrize("name", tuple(CONVS))
def test_conv_gradients_are_exact_on_integers(hip, gpu, name, N, hw):
    """integer-valued inputs, weights and gradients, every partial sum exact in fp32: reproduced exactly"""
    t, t64 = _conv_case(name, N, hw, integers=True)
    got = _conv_run(hip, gpu, name, t)
    for k, v in t64.items():
        assert torch.equal(got[k].cpu().double(), v), k
    assert float(t64["g_W"].abs().max()) > 0


def test_conv1_has_no_input_gradient(hip, gpu):
    with pytest.raises(hip.HipError, match="no input gradient"):
        hip.conv2d_dgrad_pack(torch.zeros(64, 3, 7, 7, device=gpu), 2)
    img = torch.zeros(1, 3, 8, 8, device=gpu, requires_grad=True)
    with pytest.raises(ValueError, match="requires a gradient"):
        train_ops.ConvFn.apply(img, torch.zeros(64, 3, 7, 7, device=gpu, requires_grad=True), 2)
    with pytest.raises(hip.HipError, match="no HIP backward"):
        train_ops.ConvFn.apply(img.detach(), torch.zeros(64, 3, 3, 3, device=gpu, requires_grad=True), 1)


def test_a_refusal_leaves_the_context_usable(hip, gpu):
    """an unsupported shape, a short workspace and a short packed image are refused; the same correct calls afterwards give the bits
    they gave before"""
    name = "3x3s2"
    t, _ = _conv_case(name, 3, (9, 17))
    before = _conv_run(hip, gpu, name, t)
    x, w, g = (v.to(gpu) for v in t)
    lib, c, p, st = hip.load_library(), hip.ctx(gpu), hip._p, hip._stream()
    out = torch.empty_like(x)
    gw = torch.empty_like(w)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=gpu)
    packed = hip.conv2d_dgrad_pack(w, 2)
    assert lib.th_conv2d_wgrad(c, p(x), p(g), 3, 64, 128, 3, 2, 9, 17, p(gw), p(ws), 64, st) != 0
    assert b"th_conv2d_wgrad" in lib.th_last_error() and b"workspace too small" in lib.th_last_error()
    assert lib.th_conv2d_wgrad(c, p(x), p(g), 3, 64, 128, 5, 2, 9, 17, p(gw), p(ws), ws.numel(), st) != 0
    assert b"unsupported shape" in lib.th_last_error()
    assert lib.th_conv2d_dgrad(c, p(g), 3, 64, 128, 3, 2, 9, 17, p(packed), 64, p(out), st) != 0
    assert b"th_conv2d_dgrad" in lib.th_last_error() and b"packed buffer too small" in lib.th_last_error()
    assert lib.th_conv2d_dgrad(c, p(g), 3, 64, 128, 3, 1, 9, 17, p(packed), packed.numel(), p(out), st) != 0
    assert lib.th_bn_act_bwd(c, p(x), None, p(x), 3, 64, 9 * 17, None, 1e-5, p(out), None, None, None, p(ws), 8, st) != 0
    assert b"th_bn_act_bwd" in lib.th_last_error() and b"workspace too small" in lib.th_last_error()
    after = _conv_run(hip, gpu, name, t)
    for k in before:
        assert torch.equal(before[k], after[k]), k


# ---------------------------------------------------------------------------
# 2: BatchNorm (+ residual) (+ ReLU)
# ---------------------------------------------------------------------------
C_BN = 64
NAMES = ("g_y", "g_res", "g_gamma", "g_beta")


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
    grads = {"g_y": y.grad}
    if res is not None:
        grads["g_res"] = res.grad
    if gamma is not None:
        grads["g_gamma"], grads["g_beta"] = gamma.grad, beta.grad
    return out.detach(), grads


@functools.lru_cache(maxsize=None)
def _bn_case(N, hw, kind, residual, relu, affine):
    H, W = hw
    shape = (N, C_BN, H, W)
    rs = np.random.RandomState(N + 3 * H + 5 * W + 7 * residual + 11 * relu + 13 * affine + (17 if kind == "offset" else 0))
    y = rs.normal(size=shape)
    if kind == "offset":                                   # per-channel mean 100, standard deviation 1; channel 5 is constant
        y = y + 100.0
        y[:, 5] = 100.0
    y, g = _f32(y), _f32(rs.normal(size=shape))
    res = _f32(rs.normal(size=shape)) if residual else None
    gamma, beta = (_f32(rs.normal(size=C_BN) + 1.0), _f32(rs.normal(size=C_BN))) if affine else (None, None)
    d = lambda v: None if v is None else v.double()
    if relu:                                               # no gradient arrives where the float64 pre-activation is within 1e-3 of 0
        with torch.no_grad():
            pre = torch.batch_norm(d(y), d(gamma), d(beta), None, None, True, 0.1, 1e-5, False) + (0 if res is None else d(res))
        near = pre.abs() < 1e-3
        assert float(near.double().mean()) < 0.05 or N * H * W < 64
        g = torch.where(near, torch.zeros_like(g), g)
    out, t64 = _bn_autograd(d(y), d(res), d(g), d(gamma), d(beta), relu)
    return (y, res, g, gamma, beta, out.float() if relu else None), t64


def _bn_parents(gpu, t, t64, relu):
    y, res, g, gamma, beta, _ = (None if v is None else v.to(gpu) for v in t)
    _, d32 = _bn_autograd(y, res, g, gamma, beta, relu)
    return {k: maxdiff(d32[k].cpu().double(), t64[k]) for k in t64}


def _bn_run(hip, gpu, t, residual, affine):
    y, _, g, gamma, _, out = (None if v is None else v.to(gpu) for v in t)
    call = lambda: hip.bn_act_bwd(y, out, g, gamma, 1e-5, need_residual=residual, need_affine=affine)
    got = {k: v for k, v in zip(NAMES, call()) if v is not None}
    for k, v in zip(NAMES, call()):
        assert (v is None and k not in got) or torch.equal(got[k], v), f"{k}: not bit-identical on two runs"
    assert torch.equal(g.cpu(), t[2]) and torch.equal(y.cpu(), t[0]), "an input was modified"
    return got


@pytest.mark.parametrize("N", (1, 3))
@pytest.mark.parametrize("residual,relu,affine", ((0, 0, 0), (0, 1, 1), (1, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 1)))
@pytest.mark.parametrize("kind", ("normal", "offset"))
def test_bn_backward_vs_float64(hip, gpu, N, bn_size, kind, residual, relu, affine):
    t, t64 = _bn_case(N, bn_size, kind, bool(residual), bool(relu), bool(affine))
    got = _bn_run(hip, gpu, t, bool(residual), bool(affine))
    assert set(got) == set(t64)
    if kind == "offset" and N * bn_size[0] * bn_size[1] > 1 and not relu:
        # the constant channel: variance 0, invstd = eps^-1/2, g_y = gamma invstd (g - mean g)   (a ReLU may gate the whole channel)
        assert float(t64["g_y"][:, 5].abs().max()) > 0
    _hold(f"bn {kind} N={N} {bn_size[0]}x{bn_size[1]} res={residual} relu={relu} affine={affine}", got, t64,
          _bn_parents(gpu, t, t64, bool(relu)))


@pytest.mark.parametrize("N,hw", ((3, (9, 17)), (1, (33, 47)), (1, (1, 1))))
def test_bn_gate_and_residual_gradient_are_exact(hip, gpu, N, hw):
    """integer inputs, a tenth of the site's outputs exactly 0 (and the ReLU's zeros on top): the gate [out > 0] and the residual's
    gradient are exact, g_beta -- an integer sum -- as well; g_y, g_gamma are held to the float64 formula at 4 * 2^-24 (the kernel
    rounds once from fp64)"""
    rs = np.random.RandomState(N + hw[0])
    shape = (N, C_BN, *hw)
    y, g = _f32(rs.randint(-3, 4, size=shape)), _f32(rs.randint(-4, 5, size=shape))
    out = np.maximum(rs.randint(-2, 6, size=shape), 0)
    out[rs.uniform(size=shape) < 0.1] = 0
    out = _f32(out)
    assert float((out == 0).double().mean()) >= 0.1
    gamma = _f32(rs.randint(1, 4, size=C_BN))
    g_y, g_res, g_gamma, g_beta = hip.bn_act_bwd(y.to(gpu), out.to(gpu), g.to(gpu), gamma.to(gpu), 1e-5, need_residual=True)
    want = train_ops.bn_act_grad_oracle(y, out, g, gamma, 1e-5)
    assert torch.equal(g_res.cpu(), torch.where(out > 0, g, torch.zeros_like(g)))
    assert np.array_equal(g_res.cpu().double().numpy(), want[1])
    assert np.array_equal(g_beta.cpu().double().numpy(), want[3])
    for v, ref, k in ((g_y, want[0], "g_y"), (g_gamma, want[2], "g_gamma")):
        err, scale = float(np.abs(v.cpu().double().numpy() - ref).max()), float(np.abs(ref).max())
        print(k, err, scale)
        assert err <= 4 * FLOOR * scale, (k, err, scale)


# ---------------------------------------------------------------------------
# 3: the max pool
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N", (1, 3))
@pytest.mark.parametrize("hw", SIZES + ((16, 16), (15, 18)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_pool_backward_is_torchs_exactly(hip, gpu, N, hw):
    """integer-valued post-ReLU-like inputs: at least a third of the windows are all-zero or tied at their maximum (asserted), and
    the result equals torch's CPU backward exactly -- on integer gradients, and on random ones too (one window's gradient per
    addition, windows in torch's order).  Odd and even sizes."""
    H, W = hw
    rs = np.random.RandomState(N + 3 * H + W)
    x = _f32(np.maximum(rs.randint(-5, 3, size=(N, 8, H, W)), 0))
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    # the windows as torch sees them, the padding as -1 (below every post-ReLU value): [planes, 9, Ho * Wo]
    win = F.unfold(F.pad(x.reshape(N * 8, 1, H, W), (1, 2 * Wo - W, 1, 2 * Ho - H), value=-1.0), 3, stride=2)
    assert win.shape[2] == Ho * Wo
    top = win.max(dim=1, keepdim=True).values
    tied = ((win == top).sum(dim=1) > 1) | (top[:, 0] == 0)
    assert float(tied.double().mean()) >= 1 / 3 or H * W < 6, float(tied.double().mean())
    for integers in (True, False):
        g = _f32(rs.randint(-4, 5, size=(N, 8, Ho, Wo)) if integers else rs.normal(size=(N, 8, Ho, Wo)))
        xr = x.clone().requires_grad_(True)
        F.max_pool2d(xr, 3, 2, 1).backward(g)
        got = hip.maxpool3x3s2_bwd(x.to(gpu), g.to(gpu))
        assert torch.equal(got.cpu(), xr.grad)
        assert torch.equal(got, hip.maxpool3x3s2_bwd(x.to(gpu), g.to(gpu)))
        if integers:                                       # the restatement the host test ties to float64 autograd
            assert np.array_equal(got.cpu().double().numpy(), train_ops.maxpool3x3s2_grad_oracle(x, g))
    zero = torch.zeros_like(x)                             # nothing but ties: the first element of every window
    xr = zero.clone().requires_grad_(True)
    F.max_pool2d(xr, 3, 2, 1).backward(g)
    assert torch.equal(hip.maxpool3x3s2_bwd(zero.to(gpu), g.to(gpu)).cpu(), xr.grad)


# ---------------------------------------------------------------------------
# 4: the Functions composed
# ---------------------------------------------------------------------------
@contextlib.contextmanager
def _reproducible_torch():
    """torch's own forward is not reproducible from call to call on this stack by default: the stock trunk called twice on one
    3 x 3 x 64 x 64 input gave third latents 2.9e-6 apart (MIOpen's choice for layer2's convolutions; layer1 and conv1 did
    reproduce).  "The same calls give the same bits" can only be checked where torch repeats itself, so the equality tests ask
    MIOpen for its deterministic kernels, in both modes alike, and first assert that the stock trunk then does repeat itself."""
    keep = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        yield
    finally:
        torch.backends.cudnn.deterministic = keep


def _encoder(dtype=torch.float32):
    from transhuman_amd.networks.encoder import SpatialEncoder
    torch.manual_seed(3)
    enc = SpatialEncoder()
    rs = np.random.RandomState(9)
    with torch.no_grad():
        for b in enc._bn_sites():                          # (fresh BatchNorms have gamma 1, beta 0: make them parameters that matter)
            b.weight.copy_(_f32(rs.uniform(0.5, 1.5, size=b.weight.shape)))
            b.bias.copy_(_f32(rs.normal(scale=0.2, size=b.bias.shape)))
    return enc.to(dtype).train()


def _trunk_names(enc):
    used = ("model.conv1.", "model.bn1.", "model.layer1.", "model.layer2.")
    return [k for k, _ in enc.named_parameters() if k.startswith(used)]


def _trunk_grads(fn, enc, images, seeds):
    for p in enc.parameters():
        p.grad = None
    lat = fn(enc, images)
    torch.autograd.backward(lat, [s.to(l) for s, l in zip(seeds, lat)])
    grads = {k: p.grad.detach().cpu().clone() for k, p in enc.named_parameters() if p.grad is not None}
    return [l.detach() for l in lat], grads


def _stats(enc):
    return {k: v.detach().cpu().clone() for k, v in enc.state_dict().items() if "running_" in k or "num_batches" in k}


@functools.lru_cache(maxsize=None)
def _trunk_case(shape):
    rs = np.random.RandomState(sum(shape))
    images = _f32(rs.uniform(size=shape))
    enc64 = _encoder(torch.float64)
    with torch.no_grad():
        sizes = [tuple(l.shape) for l in enc64.trunk(images.double(), fused_bn=False)]
    seeds = [_f32(rs.normal(size=s)) for s in sizes]
    enc64 = _encoder(torch.float64)
    _, t64 = _trunk_grads(lambda e, x: e.trunk(x, fused_bn=False), enc64, images.double(), seeds)
    return images, seeds, t64


@pytest.mark.parametrize("shape", ((3, 3, 64, 64), (1, 3, 37, 45)), ids=("3x3x64x64", "1x3x37x45"))
def test_trunk_on_the_functions(hip, gpu, shape):
    """trunk_device against the stock trunk: the three latents are torch.equal, the running statistics and num_batches_tracked equal
    the torch mode's after one and after two calls, all 30 parameter gradients are within the bar of the float64 run for seeded
    gradients on the three latents, and two backward passes are bit-identical"""
    images, seeds, t64 = _trunk_case(shape)
    x = images.to(gpu)
    stock, ours = _encoder().to(gpu), _encoder().to(gpu)
    names = _trunk_names(ours)
    assert len(names) == 30 and set(t64) == set(names)
    torch_fn = lambda e, t: e.trunk(t, fused_bn=False)
    with _reproducible_torch():
        with torch.no_grad():
            twice = [_encoder().to(gpu).trunk(x, fused_bn=False) for _ in range(2)]
        for i, (a, b) in enumerate(zip(*twice)):
            assert torch.equal(a, b), f"torch's own trunk does not repeat latent {i}: max|diff| = {maxdiff(a, b):.3e}"
        for call in (1, 2):
            lat_t, d32 = _trunk_grads(torch_fn, stock, x, seeds)
            lat_d, got = _trunk_grads(autograd_path.trunk_device, ours, x, seeds)
            assert len(lat_t) == len(lat_d) == 3
            for i, (a, b) in enumerate(zip(lat_t, lat_d)):
                assert torch.equal(a, b), f"latent {i} differs (call {call}): max|diff| = {maxdiff(a, b):.3e}"
            st_t, st_d = _stats(stock), _stats(ours)
            assert len(st_t) >= 30 and set(st_t) >= {"model.bn1.num_batches_tracked"}
            for k in st_t:
                assert torch.equal(st_t[k], st_d[k]), (k, call)
            assert int(st_d["model.bn1.num_batches_tracked"]) == call and int(st_d["model.layer3.0.bn1.num_batches_tracked"]) == 0
        assert type(autograd_path.trunk_device(ours, x)[0].grad_fn).__name__ == "BnActFnBackward"
        _, again = _trunk_grads(autograd_path.trunk_device, ours, x, seeds)
    assert set(got) == set(names)
    for k in names:
        assert torch.equal(got[k], again[k]), f"{k}: not bit-identical on two runs"
    parents = {k: maxdiff(d32[k].double(), t64[k]) for k in names}
    _hold(f"trunk {shape}", got, t64, parents)


def test_trunk_without_batch_statistics_is_torch_autograds(hip, gpu):
    """an eval-mode site, or SyncBatchNorm after the reference trainer's conversion: the whole trunk is the stock call"""
    x = _f32(np.random.RandomState(0).uniform(size=(2, 3, 32, 32))).to(gpu)
    for kind in ("eval", "sync"):
        a, b = _encoder().to(gpu), _encoder().to(gpu)
        if kind == "eval":
            a.eval(), b.eval()
        else:
            a, b = (torch.nn.SyncBatchNorm.convert_sync_batchnorm(e) for e in (a, b))
        with _reproducible_torch():
            lat_t = a.trunk(x, fused_bn=False)
            lat_d = autograd_path.trunk_device(b, x)
        for u, v in zip(lat_t, lat_d):
            assert torch.equal(u, v) and type(v.grad_fn).__name__ == type(u.grad_fn).__name__ != "BnActFnBackward", kind


# ---------------------------------------------------------------------------
# 5: the golden training step
# ---------------------------------------------------------------------------
ALL_DEVICE = {"train_kernels": "device", "train_attention": "device", "train_vit_dense": "device", "train_maps": "latents",
              "target_prep": "device", "train_point_net": "device"}


@pytest.mark.parametrize("others", ({"train_kernels": "torch"}, {"train_kernels": "device"}, {"train_maps": "latents"}, ALL_DEVICE),
                         ids=("kernels-torch", "kernels-device", "maps-latents", "all-six-device"))
def test_training_step_with_the_encoder_on_the_device_matches_the_reference(hip, gpu, others):
    """tests/test_gpu_train_ops.py::test_training_step_on_the_device_kernels_matches_the_reference with cfg.train_encoder = "device":
    the same golden step of the real reference, the same bars, under both values of cfg.train_kernels, under cfg.train_maps =
    "latents" (the default "full" is in the first two) and with all six training switches on their device values"""
    with config.override(**STEP_CFG, train_encoder="device", **others):
        check_step(golden(), *setup(gpu))


@pytest.mark.parametrize("maps", ("full", "latents"))
def test_only_the_encoder_switch_changed_gives_the_same_outputs(hip, gpu, maps):
    """the forward is the same torch calls: rgb, acc and depth are torch.equal to the "torch" mode's, and every trunk parameter gets a
    gradient close to torch autograd's"""
    outs, grads = {}, {}
    for mode in ("torch", "device"):
        with config.override(**STEP_CFG, train_encoder=mode, train_maps=maps):
            net, r, b = setup(gpu)
            with _reproducible_torch():
                ret = autograd_path.render(r, b)
            (ret["rgb_map"].mean() + 0.1 * ret["acc_map"].mean() + 0.01 * ret["depth_map"].mean()).backward()
            outs[mode] = {k: ret[k].detach().clone() for k in ("rgb_map", "acc_map", "depth_map")}
            grads[mode] = {k: p.grad.clone() for k, p in net.encoder.named_parameters() if p.grad is not None}
            stats = _stats(net.encoder)
        outs[mode]["stats"] = stats
    for k in ("rgb_map", "acc_map", "depth_map"):
        assert torch.equal(outs["torch"][k], outs["device"][k]), k
    for k, v in outs["torch"]["stats"].items():
        assert torch.equal(v, outs["device"]["stats"][k]), k
    assert set(grads["torch"]) == set(grads["device"]) and len(grads["device"]) >= 30
    for k, v in grads["torch"].items():
        err, scale = maxdiff(grads["device"][k], v), float(v.abs().max())
        print(k, err, scale)
        assert err <= 1e-3 * scale + 1e-12, (k, err, scale)


def test_a_trunk_without_batch_statistics_trains_as_in_the_torch_mode(hip, gpu):
    """cfg.train_encoder = "device" on an eval-mode encoder: the call is the torch mode's (no Function of train_ops in the graph of
    the trunk), the step's outputs are torch.equal"""
    outs = {}
    for mode in ("torch", "device"):
        with config.override(**STEP_CFG, train_encoder=mode):
            net, r, b = setup(gpu)
            net.encoder.eval()
            with _reproducible_torch():
                ret = autograd_path.render(r, b)
            outs[mode] = {k: ret[k].detach().clone() for k in ("rgb_map", "acc_map", "depth_map")}
            ret["rgb_map"].mean().backward()
            assert net.encoder.model.conv1.weight.grad is not None
    for k, v in outs["torch"].items():
        assert torch.equal(v, outs["device"][k]), k
