"""The forward of the encoder trunk on the device (K29): th_conv2d_fwd32 (k_encoder_fwd.hip), and cfg.train_encoder_fwd = "device",
which makes train_ops.ConvFn / BnActFn / MaxPoolFn run it, th_bn_act and th_maxpool3x3s2 in their forward.

The reference everywhere is torch's CPU float64 operator on the fp32 inputs widened to float64.  With y64 that reference and d32
torch's fp32 operator ON THE DEVICE (MIOpen / torch's own kernels: what the key's "torch" value runs), per tensor

    parent = max|d32 - y64|,  scale = max|y64|,    bar = 4 max(parent, 2^-24 scale)           (K23's bar)

elementwise against that scalar, and every case prints err / bar.  Both errors are taken here, in the test.

Sizes: output heights and widths 1, tile - 1, tile, tile + 1, 2 tile + 1 from the tile queries, paired so that every value of either
axis occurs; at stride 2 each pair through two inputs, (2 ho - 1, 2 wo) and (2 ho, 2 wo - 1), so both parities of H and of W occur
at every edge; the inputs 1 x 1, 2 x 3 and 33 x 47; one 64 x 64 case per shape.  "Larger" is counted in input pixels: nothing but
the 64 x 64 case has more than 33 * 47 of them (the widest, 18 x 66 at stride 2, has 1188)."""
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
CONVS = {"conv1": (3, 64, 7, 2), "3x3s1_64": (64, 64, 3, 1), "3x3s2": (64, 128, 3, 2), "1x1s2": (64, 128, 1, 2),
         "3x3s1_128": (128, 128, 3, 1)}
FIXED = ((1, 1), (2, 3), (33, 47))
BIG = (64, 64)
ALL_SEVEN = {k: v[1] for k, v in config.TRAIN_SWITCHES.items()}


@pytest.fixture(scope="module")
def hip(gpu):
    from transhuman_amd import hip as H
    H.load_library()
    return H


@functools.lru_cache(maxsize=None)
def _tile():
    from transhuman_amd import build, hip as H
    build.build(force=False, verbose=False)
    return H.conv2d_fwd32_tile()


def _edge_outputs():
    tr, tc = _tile()
    hs, ws = (1, tr - 1, tr, tr + 1, 2 * tr + 1), (1, tc - 1, tc, tc + 1, 2 * tc + 1)
    pairs = list(zip(hs[:4], ws[:4])) + [(hs[4], ws[3]), (hs[3], ws[4]), (hs[0], ws[4]), (hs[4], ws[0])]
    assert {p[0] for p in pairs} == set(hs) and {p[1] for p in pairs} == set(ws)
    return pairs


def _inputs_for(stride):
    if stride == 1:
        return list(_edge_outputs())
    out = []
    for ho, wo in _edge_outputs():
        out += [(2 * ho - 1, 2 * wo), (2 * ho, 2 * wo - 1)]
    return out


def _sizes(name, big=True):
    sizes = sorted(set(_inputs_for(CONVS[name][3])) | set(FIXED))
    assert all(h * w <= 33 * 47 for h, w in sizes)
    return sizes + ([BIG] if big else [])


def _edge_sizes(name):
    """the tile-edge sizes alone: outputs tile - 1, tile, tile + 1 and 2 tile + 1 (both parities at stride 2), and 1 x 1"""
    return [s for s in _sizes(name, big=False) if s not in ((2, 3), (33, 47))]


def pytest_generate_tests(metafunc):
    if "conv_case" in metafunc.fixturenames:
        cases = [(name, N, hw) for name in CONVS for hw in _sizes(name) for N in ((3,) if hw == BIG else (1, 3))]
        metafunc.parametrize("conv_case", cases, ids=[f"{n}-N{N}-{h}x{w}" for n, N, (h, w) in cases])


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def _out(n, ks, s):
    return (n + 2 * (ks // 2) - ks) // s + 1


@functools.lru_cache(maxsize=None)
def _conv_case(name, N, hw, integers=False):
    cin, cout, ks, s = CONVS[name]
    H, W = hw
    rs = np.random.RandomState(cin + 3 * cout + 7 * ks + 11 * N + 13 * H + 17 * W + 1)
    if integers:                                           # |y| <= 128 * 9 * 9 (conv1: 147 * 9): every partial sum exact in fp32
        x, w = _f32(rs.randint(-3, 4, size=(N, cin, H, W))), _f32(rs.randint(-3, 4, size=(cout, cin, ks, ks)))
    else:
        x, w = _f32(rs.normal(size=(N, cin, H, W))), _f32(rs.normal(size=(cout, cin, ks, ks)))
    y64 = F.conv2d(x.double(), w.double(), None, s, ks // 2)
    assert tuple(y64.shape) == (N, cout, _out(H, ks, s), _out(W, ks, s))
    return x, w, y64


def _hold(tag, got, y64, d32, floor=True):
    v = got.detach().cpu().double()
    assert v.shape == y64.shape and torch.isfinite(v).all(), tag
    scale, err, parent = float(y64.abs().max()), maxdiff(v, y64), maxdiff(d32.detach().cpu().double(), y64)
    bar = 4.0 * (max(parent, FLOOR * scale) if floor else parent)
    ratio = err / bar if bar > 0 else (0.0 if err == 0 else float("inf"))
    print(f"{tag}: device {err:.3e}, torch fp32 {parent:.3e}, max|ref| = {scale:.3e}; err / bar = {ratio:.2f}")
    assert err <= bar, (tag, err, bar)
    return ratio


# ---------------------------------------------------------------------------
# 1 - 4: th_conv2d_fwd32
# ---------------------------------------------------------------------------
def test_conv_forward_vs_float64(hip, gpu, conv_case):
    name, N, hw = conv_case
    s = CONVS[name][3]
    x, w, y64 = _conv_case(name, N, hw)
    xd, wd = x.to(gpu), w.to(gpu)
    got = hip.conv2d_fwd32(xd, wd, s)
    d32 = F.conv2d(xd, wd, None, s, w.shape[2] // 2)
    assert torch.equal(xd.cpu(), x) and torch.equal(wd.cpu(), w), "an input was modified"
    _hold(f"conv {name} N={N} {hw[0]}x{hw[1]}", got, y64, d32)


def _integer_cases():
    return [(name, N, hw) for name in CONVS for hw in _edge_sizes(name) for N in (1, 3)]


@pytest.mark.parametrize("name,N,hw", _integer_cases(), ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_conv_forward_is_exact_on_integers(hip, gpu, name, N, hw):
    """x and w integers in [-3, 3]: every partial sum is an integer below 2^24 in any order, so the result is the float64 one"""
    x, w, y64 = _conv_case(name, N, hw, integers=True)
    assert float(y64.abs().max()) < 2 ** 24
    got = hip.conv2d_fwd32(x.to(gpu), w.to(gpu), CONVS[name][3])
    assert torch.equal(got.cpu().double(), y64)
    assert float(y64.abs().max()) > 0


def _raw_call(hip, gpu, x, w, s, y):
    lib = hip.load_library()
    N, cin, H, W = x.shape
    return lib.th_conv2d_fwd32(hip.ctx(gpu), hip._p(x), N, cin, H, W, hip._p(w), w.shape[0], w.shape[2], s, hip._p(y), hip._stream())


@pytest.mark.parametrize("name", tuple(CONVS))
def test_every_element_is_stored_once_whatever_the_buffer_held(hip, gpu, name):
    """one call into a buffer of NaNs, one into random bytes: torch.equal (so no NaN survives, in the rows and columns whose windows
    reach into the padding either), finite, and equal to the binding's own result"""
    s = CONVS[name][3]
    for hw in _edge_sizes(name) + [(33, 47)]:
        x, w, y64 = _conv_case(name, 3, hw)
        xd, wd = x.to(gpu), w.to(gpu)
        a = torch.full(y64.shape, float("nan"), dtype=torch.float32, device=gpu)
        b = torch.randint(0, 256, (y64.numel() * 4,), dtype=torch.uint8, device=gpu).view(torch.float32).reshape(y64.shape)
        assert _raw_call(hip, gpu, xd, wd, s, a) == 0 and _raw_call(hip, gpu, xd, wd, s, b) == 0
        assert torch.isfinite(a).all() and torch.equal(a, b), hw
        assert torch.equal(a, hip.conv2d_fwd32(xd, wd, s)), hw


def test_refusals_leave_the_context_usable(hip, gpu):
    x, w, _ = _conv_case("3x3s2", 3, (9, 17))
    xd, wd = x.to(gpu), w.to(gpu)
    before = hip.conv2d_fwd32(xd, wd, 2)
    lib = hip.load_library()
    with pytest.raises(hip.HipError, match="no HIP forward"):
        hip.conv2d_fwd32(torch.zeros(1, 3, 8, 8, device=gpu), torch.zeros(64, 3, 3, 3, device=gpu), 1)
    with pytest.raises(hip.HipError, match="no HIP forward"):
        hip.conv2d_fwd32(torch.zeros(1, 64, 8, 8, device=gpu), torch.zeros(64, 64, 5, 5, device=gpu), 1)
    with pytest.raises(hip.HipError, match="no HIP forward"):
        hip.conv2d_fwd32(xd, wd, 1)                                         # 3x3/1 64->128
    with pytest.raises(ValueError, match="contiguous float32"):
        hip.conv2d_fwd32(xd.transpose(2, 3), wd, 2)
    with pytest.raises(ValueError, match="contiguous float32"):
        hip.conv2d_fwd32(xd.half(), wd, 2)
    with pytest.raises(ValueError, match="contiguous float32"):
        hip.conv2d_fwd32(xd, wd.half(), 2)
    with pytest.raises(ValueError, match="channels"):
        hip.conv2d_fwd32(xd[:, :32].contiguous(), wd, 2)
    y = torch.empty_like(before)
    c, p, st = hip.ctx(gpu), hip._p, hip._stream()
    assert lib.th_conv2d_fwd32(c, p(xd), 3, 64, 9, 17, p(wd), 128, 5, 2, p(y), st) < 0
    assert b"th_conv2d_fwd32" in lib.th_last_error() and b"unsupported shape" in lib.th_last_error()
    assert lib.th_conv2d_fwd32(c, p(xd), 3, 64, 9, 17, p(wd), 128, 3, 2, None, st) < 0 and b"null" in lib.th_last_error()
    assert lib.th_conv2d_fwd32(c, p(xd), 0, 64, 9, 17, p(wd), 128, 3, 2, p(y), st) < 0
    assert lib.th_conv2d_fwd32(c, p(xd), 3, 64, 0, 17, p(wd), 128, 3, 2, p(y), st) < 0
    assert torch.equal(before, hip.conv2d_fwd32(xd, wd, 2))


# ---------------------------------------------------------------------------
# 5: the Functions under cfg.train_encoder_fwd = "device"
# ---------------------------------------------------------------------------
def _fwd(value):
    return config.override(train_encoder_fwd=value)


@pytest.mark.parametrize("name", tuple(CONVS))
def test_conv_function(hip, gpu, name):
    cin, cout, ks, s = CONVS[name]
    x, w, y64 = _conv_case(name, 3, (33, 47))
    g = _f32(np.random.RandomState(5).normal(size=tuple(y64.shape))).to(gpu)
    res = {}
    for mode in ("device", "torch"):
        xd, wd = x.to(gpu).requires_grad_(name != "conv1"), w.to(gpu).requires_grad_(True)
        with _fwd(mode):
            y = train_ops.ConvFn.apply(xd, wd, s)
        y.backward(g)
        res[mode] = (y.detach(), xd.grad, wd.grad)
    _hold(f"ConvFn {name}", res["device"][0], y64, res["torch"][0])
    assert torch.equal(res["device"][0], hip.conv2d_fwd32(x.to(gpu), w.to(gpu), s))
    assert torch.equal(res["device"][2], res["torch"][2]) and float(res["torch"][2].abs().max()) > 0
    if name != "conv1":
        assert torch.equal(res["device"][1], res["torch"][1]) and float(res["torch"][1].abs().max()) > 0


def _bn_module(C, affine, track, dtype, seed=0):
    rs = np.random.RandomState(seed)
    bn = torch.nn.BatchNorm2d(C, affine=affine, track_running_stats=track, momentum=0.3).train()
    with torch.no_grad():
        if affine:
            bn.weight.copy_(_f32(rs.uniform(0.5, 1.5, size=C)))
            bn.bias.copy_(_f32(rs.normal(scale=0.2, size=C)))
        if track:
            bn.running_mean.copy_(_f32(rs.normal(size=C)))
            bn.running_var.copy_(_f32(rs.uniform(0.5, 2.0, size=C)))
            bn.num_batches_tracked.fill_(7)
    return bn.to(dtype)


def _site(bn, y, res, relu):
    out = bn(y)
    if res is not None:
        out = out + res
    return torch.relu(out) if relu else out


@pytest.mark.parametrize("track", (True, False), ids=("track", "notrack"))
@pytest.mark.parametrize("affine,residual,relu", ((1, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 0), (0, 1, 1), (1, 0, 0)))
@pytest.mark.parametrize("N,hw", ((3, (9, 17)), (1, (33, 47))))
def test_bn_act_function(hip, gpu, N, hw, affine, residual, relu, track):
    C = 64
    rs = np.random.RandomState(N + hw[0] + 2 * affine + 4 * residual + 8 * relu)
    shape = (N, C, *hw)
    y = _f32(rs.normal(size=shape) * rs.uniform(0.5, 2.0, size=(1, C, 1, 1)) + rs.normal(size=(1, C, 1, 1)))
    res = _f32(rs.normal(size=shape)) if residual else None
    g = _f32(rs.normal(size=shape))
    bn64 = _bn_module(C, affine, track, torch.float64)
    with torch.no_grad():
        out64 = _site(bn64, y.double(), None if res is None else res.double(), relu)
        if relu:                                           # no gradient arrives where the float64 pre-activation is within 1e-3 of 0:
            pre = _site(_bn_module(C, affine, track, torch.float64), y.double(), None if res is None else res.double(), False)
            near = pre.abs() < 1e-3                        # two fp32 forwards may gate such an element differently
            assert float(near.double().mean()) < 0.05
            g = torch.where(near, torch.zeros_like(g), g)
    got = {}
    for mode in ("device", "torch"):
        bn = _bn_module(C, affine, track, torch.float32).to(gpu)
        yd = y.to(gpu).requires_grad_(True)
        rd = None if res is None else res.to(gpu).requires_grad_(True)
        with _fwd(mode):
            out = train_ops.BnActFn.apply(yd, bn, rd, bool(relu), bn.weight, bn.bias)
        assert out.data_ptr() != yd.data_ptr() and (rd is None or out.data_ptr() != rd.data_ptr())
        out.backward(g.to(gpu))
        grads = [yd.grad] + ([rd.grad] if residual else []) + ([bn.weight.grad, bn.bias.grad] if affine else [])
        assert all(v is not None for v in grads)
        got[mode] = (out.detach(), bn, grads)
        assert torch.equal(yd.detach().cpu(), y), "the BatchNorm's input was modified"
    tag = f"BnActFn N={N} {hw[0]}x{hw[1]} affine={affine} res={residual} relu={relu} track={track}"
    _hold(tag + " out", got["device"][0], out64, got["torch"][0])
    dev, tor = got["device"][1], got["torch"][1]
    if track:
        _hold(tag + " running_mean", dev.running_mean, bn64.running_mean, tor.running_mean)
        _hold(tag + " running_var", dev.running_var, bn64.running_var, tor.running_var)
        assert int(dev.num_batches_tracked) == int(tor.num_batches_tracked) == int(bn64.num_batches_tracked) == 8
    else:
        assert dev.running_mean is None and dev.num_batches_tracked is None
    for i, (a, b) in enumerate(zip(got["device"][2], got["torch"][2])):
        assert torch.equal(a, b), f"{tag}: gradient {i} is not the torch-forward mode's bit for bit"
    # and the backward fed the device forward's own y / out directly
    direct = hip.bn_act_bwd(y.to(gpu), got["device"][0] if relu else None, g.to(gpu), dev.weight, float(dev.eps),
                            need_residual=bool(residual and relu), need_affine=bool(affine))
    assert torch.equal(direct[0], got["device"][2][0])


@pytest.mark.parametrize("N,hw", ((1, (1, 1)), (3, (2, 3)), (3, (16, 16)), (3, (15, 18)), (1, (33, 47))))
def test_pool_function(hip, gpu, N, hw):
    rs = np.random.RandomState(N + hw[0])
    x = _f32(np.maximum(rs.normal(size=(N, 64, *hw)), 0))
    g = None
    res = {}
    for mode in ("device", "torch"):
        xd = x.to(gpu).requires_grad_(True)
        with _fwd(mode):
            y = train_ops.MaxPoolFn.apply(xd)
        if g is None:
            g = _f32(rs.normal(size=tuple(y.shape))).to(gpu)
        y.backward(g)
        res[mode] = (y.detach(), xd.grad)
    want = F.max_pool2d(x.to(gpu), 3, 2, 1)
    assert torch.equal(res["device"][0], want) and torch.equal(res["torch"][0], want)
    assert torch.equal(res["device"][0].cpu(), F.max_pool2d(x, 3, 2, 1))
    assert torch.equal(res["device"][1], res["torch"][1]) and float(res["torch"][1].abs().max()) > 0


def test_a_bad_value_of_the_key_raises_on_the_device(hip, gpu):
    x = torch.zeros(1, 64, 4, 4, device=gpu)
    with _fwd("miopen"), pytest.raises(ValueError, match="cfg.train_encoder_fwd must be 'torch' or 'device'"):
        train_ops.MaxPoolFn.apply(x)


# ---------------------------------------------------------------------------
# 6: the composed trunk
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ((3, 3, 33, 47), (3, 3, 64, 64)), ids=("3x3x33x47", "3x3x64x64"))
def test_trunk_on_the_device_forward(hip, gpu, shape):
    """trunk_device with the key on "device" against the float64 trunk: the three latents within 4 x the error of the "torch" mode's
    latents, the 30 parameter gradients at K23's bar, the running statistics at the bar and num_batches_tracked equal; two runs
    are bit-identical in latents, gradients and statistics without asking MIOpen for anything"""
    from test_gpu_train_encoder import _encoder, _hold as hold_grads, _stats, _trunk_case, _trunk_grads, _trunk_names
    images, seeds, t64 = _trunk_case(shape)
    enc64 = _encoder(torch.float64)
    with torch.no_grad():
        lat64 = enc64.trunk(images.double(), fused_bn=False)
    st64 = _stats(enc64)
    x = images.to(gpu)
    runs = {}
    for mode in ("torch", "device", "device-again"):
        enc = _encoder().to(gpu)
        with config.override(train_encoder="device", train_encoder_fwd=mode.split("-")[0]):
            lat, grads = _trunk_grads(autograd_path.trunk_device, enc, x, seeds)
        runs[mode] = (lat, grads, _stats(enc))
    names = _trunk_names(_encoder())
    assert len(names) == 30 and set(runs["device"][1]) == set(names) == set(t64)
    for i in range(3):
        _hold(f"trunk {shape} latent {i}", runs["device"][0][i], lat64[i], runs["torch"][0][i], floor=False)
    parents = {k: maxdiff(runs["torch"][1][k].double(), t64[k]) for k in names}
    hold_grads(f"trunk {shape} fwd=device", runs["device"][1], t64, parents)
    stats = [k for k in st64 if k.startswith(("model.bn1.", "model.layer1.", "model.layer2."))]
    assert len(stats) == 30
    for k in stats:
        if "num_batches" in k:
            assert int(runs["device"][2][k]) == int(runs["torch"][2][k]) == int(st64[k]) == 1, k
        else:
            _hold(f"trunk {shape} {k}", runs["device"][2][k], st64[k], runs["torch"][2][k])
    a, b = runs["device"], runs["device-again"]
    assert all(torch.equal(u, v) for u, v in zip(a[0], b[0]))
    assert all(torch.equal(a[1][k], b[1][k]) for k in names) and all(torch.equal(a[2][k], b[2][k]) for k in stats)


def test_trunk_with_an_eval_site_is_torch_autograds(hip, gpu):
    from test_gpu_train_encoder import _encoder, _reproducible_torch
    x = _f32(np.random.RandomState(0).uniform(size=(2, 3, 32, 32))).to(gpu)
    a, b = _encoder().to(gpu).eval(), _encoder().to(gpu).eval()
    with _reproducible_torch(), config.override(train_encoder="device", train_encoder_fwd="device"):
        lat_t = a.trunk(x, fused_bn=False)
        lat_d = autograd_path.trunk_device(b, x)
    for u, v in zip(lat_t, lat_d):
        assert torch.equal(u, v) and type(v.grad_fn).__name__ == type(u.grad_fn).__name__ != "BnActFnBackward"


# ---------------------------------------------------------------------------
# 7: the golden training step of the real reference
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("others", ({"train_maps": "full"}, {"train_maps": "latents"}, ALL_SEVEN),
                         ids=("maps-full", "maps-latents", "all-seven-device"))
def test_training_step_with_the_device_forward_matches_the_reference(hip, gpu, others):
    assert len(ALL_SEVEN) == 7 and ALL_SEVEN["train_maps"] == "latents" and ALL_SEVEN["train_gather_bwd"] == "ordered"
    with config.override(**STEP_CFG, **{"train_encoder": "device", **others}, train_encoder_fwd="device"):
        check_step(golden(), *setup(gpu))


# ---------------------------------------------------------------------------
# 8: no vendor convolution, no torch batch norm in the step
# ---------------------------------------------------------------------------
def _spied_step(gpu, monkeypatch, fwd):
    seen = {"conv2d": [], "batch_norm": 0}
    conv2d, batch_norm = F.conv2d, F.batch_norm

    def spy_conv2d(input, weight, bias=None, stride=1, *a, **k):
        st = tuple(stride) if isinstance(stride, (tuple, list)) else (int(stride), int(stride))
        seen["conv2d"].append((tuple(weight.shape[2:]), st))
        return conv2d(input, weight, bias, stride, *a, **k)

    def spy_batch_norm(*a, **k):
        seen["batch_norm"] += 1
        return batch_norm(*a, **k)

    with config.override(**STEP_CFG, **ALL_SEVEN, train_encoder_fwd=fwd):
        net, r, b = setup(gpu)
        monkeypatch.setattr(torch.nn.functional, "conv2d", spy_conv2d)
        monkeypatch.setattr(torch.nn.functional, "batch_norm", spy_batch_norm)
        try:
            ret = r.render(b)
            (ret["rgb_map"].mean() + 0.1 * ret["acc_map"].mean() + 0.01 * ret["depth_map"].mean()).backward()
        finally:
            monkeypatch.undo()
    assert net.encoder.model.conv1.weight.grad is not None
    return seen


def test_no_vendor_convolution_in_the_step(hip, gpu, monkeypatch):
    big = lambda seen: [c for c in seen["conv2d"] if c[0] != (1, 1) or c[1] != (1, 1)]
    seen = _spied_step(gpu, monkeypatch, "torch")
    assert seen["batch_norm"] == 10 and len(big(seen)) == 10, seen                  # the spy works: the trunk's sites
    seen = _spied_step(gpu, monkeypatch, "device")
    print("conv2d calls left:", seen["conv2d"])
    assert seen["batch_norm"] == 0 and not big(seen), seen


# ---------------------------------------------------------------------------
# 9: reproducible without asking MIOpen for its deterministic kernels
# ---------------------------------------------------------------------------
def test_the_whole_step_twice_gives_the_same_bits_without_the_flag(hip, gpu):
    """tests/test_gpu_latgather_ordered.py::test_the_whole_step_twice_gives_the_same_bits with the key on "device" and
    torch.backends.cudnn.deterministic = False, benchmark = False set explicitly: outputs, the gradient of every parameter that
    gets one and the BatchNorm running statistics are torch.equal between two runs from equal seeds"""
    from test_gpu_train_encoder import _stats
    keep = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = False, False
    runs = []
    try:
        for _ in range(2):
            with config.override(**STEP_CFG, **ALL_SEVEN, train_encoder_fwd="device"):
                net, r, b = setup(gpu)
                ret = autograd_path.render(r, b)
                (ret["rgb_map"].mean() + 0.1 * ret["acc_map"].mean() + 0.01 * ret["depth_map"].mean()).backward()
                out = {k: ret[k].detach().clone() for k in ("rgb_map", "acc_map", "depth_map")}
                out.update({"grad:" + k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None})
                out.update({"stat:" + k: v for k, v in _stats(net.encoder).items()})
                runs.append(out)
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = keep
    a, b2 = runs
    assert set(a) == set(b2)
    trunk = [k for k in a if k.startswith(("grad:encoder.model.conv1.", "grad:encoder.model.bn1.", "grad:encoder.model.layer1.",
                                           "grad:encoder.model.layer2."))]
    assert len(trunk) == 30 and sum(k.startswith("stat:") for k in a) >= 30
    assert int(a["stat:model.bn1.num_batches_tracked"]) == 1
    differ = [k for k in a if not torch.equal(a[k], b2[k])]
    print(f"{len(a)} tensors compared ({len(trunk)} trunk gradients); differing: {differ}")
    assert not differ, differ
