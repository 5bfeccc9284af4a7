"""The training form of the per-point network on the device (K20): th_linear_relu_forward / th_linear_relu_bwd
(k_vit_dense_bwd.hip), th_xview_attention / th_xview_attention_bwd (k_pointnet_bwd.hip), train_ops.ReluLinearFn / CrossViewAttentionFn,
autograd_path.point_network_device and cfg.train_point_net = "device".

The bars are those of tests/test_gpu_train_vit_dense.py: inputs are fp32 values widened to float64 for the truth; with t64 torch's
float64 autograd and o32 its fp32 autograd on the CPU, per tensor

    parent = max|o32 - t64|,  scale = max|t64|,    bar = 4 max(parent, 2^-22 scale)

and every case prints err / bar of every tensor.

A ReLU makes the gradient a discontinuous function of the inputs: where a pre-activation is within fp32 rounding of 0, the fp32
gate and the float64 gate may differ and the gradients then differ by a whole term, whatever computed them.  The random cases are
therefore BUILT, from the float64 reference alone, so that no pre-activation lies within 2^-14 of its layer's rms (2^10 ulps of a
typical value; fp32 rounding of a 128..384-term chain is a few ulps of that): rows (samples) that do are drawn again, which is
asserted when the case is built.  What happens AT 0 is held exactly by the integer cases (test_relu_gate_is_exact): there every
sum is exact in fp32 and a tenth or more of the pre-activations are exactly 0.

The forward of th_xview_attention is xattn_kernel of k_mlp.hip itself, the kernel th_mlp_forward launches (one launcher serves
both), so "the bits of the inference path" holds by construction; here it is held to the bar against float64.
The stress inputs are kept only where torch's own fp32 stays finite (asserted when the case is built)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from transhuman_amd import config
from transhuman_amd.networks import autograd_path, train_ops
from train_step_case import STEP_CFG, check_step, golden, setup
from util import make_net, maxdiff

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -22
MARGIN = 2.0 ** -14
LAYERS = ((256, 256), (384, 256), (288, 128), (128, 128), (256, 16))               # (in, out)
EDGES = (1, 15, 16, 17, 63, 64, 65)
KEY0_BIAS = "spatial_key_value_0.key_embed.bias"
KEY0_WEIGHT = "spatial_key_value_0.key_embed.weight"


@pytest.fixture(scope="module")
def hip(gpu):
    from transhuman_amd import hip as H
    H.load_library()
    return H


@functools.lru_cache(maxsize=None)
def _chunk():
    from transhuman_amd import build, hip as H
    build.build(force=False, verbose=False)
    return H.wgrad_chunk_rows()


def pytest_generate_tests(metafunc):
    c = _chunk() if {"M_edge", "M_big"} & set(metafunc.fixturenames) else 0
    if "M_edge" in metafunc.fixturenames:
        metafunc.parametrize("M_edge", EDGES + (c - 1, c, c + 1, 2 * c + 37))
    if "M_big" in metafunc.fixturenames:
        metafunc.parametrize("M_big", (65, 2 * c + 37))


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def _hold(tag, got, t64, parents, bars_from=None):
    """every tensor of t64 within its bar; bars_from: {tensor: tensor whose parent and scale make its bar}"""
    failed, worst = [], 0.0
    for k, t in t64.items():
        v = got[k].detach().cpu()
        assert v.shape == t.shape and torch.isfinite(v).all(), (tag, k)
        src = (bars_from or {}).get(k, k)
        scale, err = float(t64[src].abs().max()), maxdiff(v, t)
        bar = 4.0 * max(parents[src], FLOOR * scale)
        if bar > 0:
            worst = max(worst, err / bar)
            print(f"{tag} {k}: device {err:.3e}, torch fp32 {parents[k]:.3e}, max|ref| = {float(t.abs().max()):.3e}; "
                  f"err / bar = {err / bar:.2f}")
        if not err <= bar:
            failed.append((k, err, bar))
    print(f"{tag}: worst err / bar = {worst:.2f}")
    assert not failed, (tag, failed)


# ---------------------------------------------------------------------------
# 1: the ReLU layer
# ---------------------------------------------------------------------------
def _relu_autograd(t, dtype):
    a, W, b = (t[k].to(dtype).clone().requires_grad_(True) for k in ("a", "W", "b"))
    y = F.relu(F.linear(a, W, b))
    y.backward(t["g"].to(dtype))
    return {"y": y.detach(), "g_a": a.grad, "g_W": W.grad, "g_b": b.grad}


@functools.lru_cache(maxsize=None)
def _relu_case(in_f, out_f, M):
    rs = np.random.RandomState(in_f + 7 * out_f + 31 * M)
    W, b = _f32(rs.normal(scale=0.1, size=(out_f, in_f))), _f32(rs.normal(scale=0.1, size=out_f))
    pool = _f32(rs.normal(scale=2.0, size=(2 * M + 16, in_f)))
    pre = F.linear(pool.double(), W.double(), b.double())
    clear = (pre.abs() > MARGIN * float(pre.pow(2).mean().sqrt())).all(dim=1)
    assert int(clear.sum()) >= M, "the case needs M rows whose pre-activations keep clear of 0"
    a = pool[clear][:M].contiguous()
    t = {"a": a, "W": W, "b": b, "g": _f32(rs.normal(size=(M, out_f)))}
    t64, o32 = _relu_autograd(t, torch.float64), _relu_autograd(t, torch.float32)
    assert M * out_f < 1024 or 0.2 < float((t64["y"] == 0).double().mean()) < 0.8
    return t, t64, {k: maxdiff(o32[k], t64[k]) for k in t64}


def _relu_run(hip, gpu, t):
    d = {k: v.to(gpu) for k, v in t.items()}
    y = hip.linear_relu_forward(d["a"], d["W"], d["b"])
    names = ("g_a", "g_W", "g_b")
    got = dict(zip(names, hip.linear_relu_bwd(d["a"], y, d["W"], d["g"])))
    for k, v in zip(names, hip.linear_relu_bwd(d["a"], y, d["W"], d["g"])):
        assert torch.equal(got[k], v), f"{k}: not bit-identical on two runs"
    assert torch.equal(d["g"].cpu(), t["g"]), "g_Y was modified"
    got["y"] = y
    return got, d


@pytest.mark.parametrize("in_f,out_f", LAYERS)
def test_relu_layer_vs_float64_at_the_edges(hip, gpu, in_f, out_f, M_edge):
    t, t64, parents = _relu_case(in_f, out_f, M_edge)
    got, d = _relu_run(hip, gpu, t)
    assert torch.equal(got["y"], torch.relu(hip.linear_train_forward(d["a"], d["W"], d["b"], 0))), "the epilogue's ReLU"
    _hold(f"relu-linear {in_f}->{out_f} M={M_edge}", got, t64, parents)


@functools.lru_cache(maxsize=None)
def _gate_case(in_f, out_f, M):
    """integers: every product and every sum below is exact in fp32 (|pre| <= 2 in_f + 2, |g_W| <= 6 M, |g_a| <= 3 out_f)"""
    rs = np.random.RandomState(3 * in_f + out_f + M)
    a = rs.randint(-2, 3, size=(M, in_f))
    W = rs.randint(-1, 2, size=(out_f, in_f)) * (rs.uniform(size=(out_f, in_f)) < 4.0 / in_f)      # ~4 taps per output
    b = rs.randint(-1, 2, size=out_f)
    g = rs.randint(-3, 4, size=(M, out_f))
    pre = a @ W.T + b
    assert float((pre == 0).mean()) >= 0.1 and float((pre > 0).mean()) >= 0.1
    return {k: _f32(v) for k, v in dict(a=a, W=W, b=b, g=g).items()}


@pytest.mark.parametrize("in_f,out_f", LAYERS)
def test_relu_gate_is_exact(hip, gpu, in_f, out_f, M_big):
    """the gate at pre-activation == 0 (gradient 0, torch's rule), held exactly: Y and the three gradients EQUAL the float64 oracle"""
    t = _gate_case(in_f, out_f, M_big)
    got, _ = _relu_run(hip, gpu, t)
    want = dict(zip(("y", "g_a", "g_W", "g_b"), train_ops.relu_linear_grad_oracle(t["a"], t["W"], t["b"], t["g"])))
    for k, w in want.items():
        assert np.array_equal(got[k].cpu().double().numpy().reshape(w.shape), w), k
    # ... which is torch's own rule
    ref = _relu_autograd(t, torch.float64)
    for k, w in want.items():
        assert np.array_equal(ref[k].numpy().reshape(w.shape), w), k


def _filled(nbytes, byte, gpu):
    return torch.full((max(int(nbytes), 256),), byte, dtype=torch.uint8, device=gpu)


def _raw_relu(hip, gpu, d, M, in_f, out_f, byte):
    """forward and backward through the C ABI itself, on workspaces filled with `byte` and outputs filled with NaN"""
    lib = hip.load_library()
    h, s, p = hip.ctx(gpu), hip._stream(), hip._p
    nan = lambda *shape: torch.full(shape, float("nan"), device=gpu)
    lin = hip.ThLinear(p(d["W"]), p(d["b"]), out_f, in_f)
    y, g_a, g_w, g_b = nan(M, out_f), nan(M, in_f), nan(out_f, in_f), nan(out_f)
    ws = _filled(lib.th_linear_relu_workspace_bytes(M, out_f, in_f), byte, gpu)
    hip._check(lib.th_linear_relu_forward(h, p(d["a"]), in_f, M, C.byref(lin), p(y), out_f, p(ws), ws.numel(), s))
    ws = _filled(lib.th_linear_relu_bwd_workspace_bytes(M, out_f, in_f), byte, gpu)
    hip._check(lib.th_linear_relu_bwd(h, p(d["a"]), in_f, p(y), out_f, M, C.byref(lin), p(d["g"]), out_f, p(g_a), in_f, p(g_w),
                                      p(g_b), p(ws), ws.numel(), s))
    return [v.cpu() for v in (y, g_a, g_w, g_b)]


@pytest.mark.parametrize("in_f,out_f", LAYERS)
def test_relu_layer_ignores_workspace_contents(hip, gpu, in_f, out_f, M_big):
    t = _relu_case(in_f, out_f, M_big)[0]
    got, d = _relu_run(hip, gpu, t)                                        # (two runs bit-identical: asserted inside)
    res = [_raw_relu(hip, gpu, d, M_big, in_f, out_f, byte) for byte in (0x00, 0xFF)]       # 0xFF..: NaN as fp32
    for a, b, k in zip(*res, ("y", "g_a", "g_W", "g_b")):
        assert torch.isfinite(a).all() and torch.equal(a, b) and torch.equal(a, got[k].cpu()), k


def test_relu_layer_refusals(hip, gpu):
    """an argument error comes back as a code < 0 and a message; nothing is launched: the outputs keep their contents"""
    lib = hip.load_library()
    M, in_f, out_f = 65, 288, 128
    d = {k: v.to(gpu) for k, v in _relu_case(in_f, out_f, M)[0].items()}
    wide = torch.zeros(M, in_f + 4, device=gpu)
    h, s, p = hip.ctx(gpu), hip._stream(), hip._p
    seven = lambda *shape: torch.full(shape, 7.0, device=gpu)
    y, g_a, g_w, g_b = seven(M, out_f), seven(M, in_f), seven(out_f, in_f), seven(out_f)
    nf, nb = int(lib.th_linear_relu_workspace_bytes(M, out_f, in_f)), int(lib.th_linear_relu_bwd_workspace_bytes(M, out_f, in_f))
    assert nf > 0 and nb > 0
    assert lib.th_linear_relu_workspace_bytes(M, 3, in_f) == 0 and lib.th_linear_relu_bwd_workspace_bytes(M, 3, in_f) == 0
    assert lib.th_linear_relu_bwd_workspace_bytes(0, out_f, in_f) == 0
    wf, wb = _filled(nf, 0, gpu), _filled(nb, 0, gpu)

    def refused(rc, word):
        assert rc < 0
        msg = lib.th_last_error()
        assert msg and word in msg, msg

    def fwd(a=p(d["a"]), lda=in_f, o=out_f, nbytes=nf):
        lin = hip.ThLinear(p(d["W"]), p(d["b"]), o, in_f)
        return lib.th_linear_relu_forward(h, a, lda, M, C.byref(lin), p(y), out_f, p(wf), nbytes, s)

    def bwd(a=p(d["a"]), lda=in_f, o=out_f, g=p(d["g"]), nbytes=nb):
        lin = hip.ThLinear(p(d["W"]), None, o, in_f)
        return lib.th_linear_relu_bwd(h, a, lda, p(y), out_f, M, C.byref(lin), g, out_f, p(g_a), in_f, p(g_w), p(g_b), p(wb),
                                      nbytes, s)

    for call in (fwd, bwd):
        refused(call(o=3), b"multiples of 16")
        refused(call(lda=in_f - 4), b"lda")
        refused(call(a=C.c_void_p(d["a"].data_ptr() + 4)), b"aligned")
        refused(call(nbytes=nb // 2 if call is bwd else nf - 1), b"workspace")
        refused(call(a=C.c_void_p(0)), b"null")
    refused(bwd(g=C.c_void_p(d["g"].data_ptr() + 4)), b"aligned")
    torch.cuda.synchronize()
    for v in (y, g_a, g_w, g_b):
        assert bool((v == 7.0).all())
    hip._check(fwd())
    hip._check(bwd())
    for v in (y, g_a, g_w, g_b):
        assert torch.isfinite(v).all() and not bool((v == 7.0).all())
    assert wide.shape[1] == in_f + 4                     # a wider leading dimension is fine
    wide[:, :in_f] = d["a"]
    y2 = seven(M, out_f)
    lin = hip.ThLinear(p(d["W"]), p(d["b"]), out_f, in_f)
    hip._check(lib.th_linear_relu_forward(h, p(wide), in_f + 4, M, C.byref(lin), p(y2), out_f, p(wf), nf, s))
    assert torch.equal(y2, y)


def test_relu_linear_fn_gradients_are_the_kernels(hip, gpu):
    in_f, out_f = 384, 256
    M = 3 * ((_chunk() + 3) // 3)
    t = _relu_case(in_f, out_f, M)[0]
    want, _ = _relu_run(hip, gpu, t)
    a3 = t["a"].to(gpu).reshape(M // 3, 3, in_f).requires_grad_(True)
    W, b = t["W"].to(gpu).requires_grad_(True), t["b"].to(gpu).requires_grad_(True)
    y = train_ops.ReluLinearFn.apply(a3, W, b)
    assert torch.equal(y.reshape(M, out_f), want["y"])
    y.backward(t["g"].to(gpu).reshape(y.shape))
    for k, v in (("g_a", a3.grad.reshape(M, in_f)), ("g_W", W.grad), ("g_b", b.grad)):
        assert torch.equal(v, want[k]), k
    with pytest.raises(ValueError, match="contiguous float32"):
        train_ops.ReluLinearFn.apply(a3.double(), W, b)
    with pytest.raises(hip.HipError):
        train_ops.ReluLinearFn.apply(a3.cpu(), W, b)


# ---------------------------------------------------------------------------
# 2: the cross-view attention
# ---------------------------------------------------------------------------
XV, XP = (1, 2, 3, 4), (1, 3, 4, 5, 255, 256, 257)
XNAMES = ("n", "g_kp", "g_vp", "g_ks", "g_vs")


def _xview_autograd(t, dtype):
    kvp, kvs = (t[k].to(dtype).clone().requires_grad_(True) for k in ("kvp", "kvs"))
    kp, vp, ks, vs = kvp[..., :128], kvp[..., 128:], kvs[..., :128], kvs[..., 128:]
    A = F.softmax(torch.einsum("pjc,pic->pji", kp, ks) / math.sqrt(128), dim=1)               # point_network's statements
    n = vs + torch.einsum("pjc,pji->pic", vp, A)
    n.backward(t["g"].to(dtype))
    return {"n": n.detach(), "g_kp": kvp.grad[..., :128], "g_vp": kvp.grad[..., 128:], "g_ks": kvs.grad[..., :128],
            "g_vs": kvs.grad[..., 128:]}


@functools.lru_cache(maxsize=None)
def _xview_case(P, V, kind="gauss"):
    rs = np.random.RandomState(100 * P + V)
    kvp, kvs, g = rs.normal(size=(P, V, 384)), rs.normal(size=(P, V, 384)), rs.normal(size=(P, V, 256))
    if kind == "one_hot":                      # logits of standard deviation 20: they reach +-60, the softmax is one-hot
        kvp[..., :128] *= math.sqrt(20.0)
        kvs[..., :128] *= math.sqrt(20.0)
        logits = np.einsum("pjc,pic->pji", kvp[..., :128], kvs[..., :128]) / math.sqrt(128)
        assert logits.max() > 60 and logits.min() < -60
    elif kind == "equal_keys":                 # A is uniform; the sums behind g_kp cancel
        kvp[..., :128] = kvs[..., :128] = rs.normal(size=(P, 1, 128))
    elif kind == "zero_view":
        kvp[:, 1], kvs[:, 1] = 0.0, 0.0
    elif kind == "g_zero":
        g[:] = 0.0
    else:
        assert kind == "gauss", kind
    t = {"kvp": _f32(kvp), "kvs": _f32(kvs), "g": _f32(g)}
    t64, o32 = _xview_autograd(t, torch.float64), _xview_autograd(t, torch.float32)
    for k, v in o32.items():
        assert torch.isfinite(v).all(), (kind, k)                       # (torch's own fp32 must survive the case)
    return t, t64, {k: maxdiff(o32[k], t64[k]) for k in t64}


def _xview_run(hip, gpu, t):
    kvp, kvs, g = (t[k].to(gpu) for k in ("kvp", "kvs", "g"))
    n = hip.xview_attention(kvp, kvs)
    assert torch.equal(n, hip.xview_attention(kvp, kvs)), "forward: not bit-identical on two runs"
    g_kvp, g_kvs = hip.xview_attention_bwd(kvp, kvs, g)
    for a, b in zip((g_kvp, g_kvs), hip.xview_attention_bwd(kvp, kvs, g)):
        assert torch.equal(a, b), "backward: not bit-identical on two runs"
    return {"n": n, "g_kp": g_kvp[..., :128], "g_vp": g_kvp[..., 128:], "g_ks": g_kvs[..., :128], "g_vs": g_kvs[..., 128:]}


@pytest.mark.parametrize("P", XP)
@pytest.mark.parametrize("V", XV)
def test_xview_attention_vs_float64_at_the_block_edges(hip, gpu, V, P):
    t, t64, parents = _xview_case(P, V)
    got = _xview_run(hip, gpu, t)
    _hold(f"xview V={V} P={P}", got, t64, parents)
    assert torch.equal(got["g_vs"].cpu(), t["g"])
    if V == 1:                                 # exact zeros and copies
        assert not bool(got["g_kp"].any()) and not bool(got["g_ks"].any())
        assert torch.equal(got["g_vp"].cpu(), t["g"])
        assert torch.equal(got["n"].cpu(), t["kvp"][..., 128:] + t["kvs"][..., 128:])


@pytest.mark.parametrize("kind", ("one_hot", "equal_keys", "zero_view", "g_zero"))
def test_xview_attention_stress(hip, gpu, kind):
    t, t64, parents = _xview_case(257, 3, kind)
    got = _xview_run(hip, gpu, t)
    _hold(f"xview {kind} V=3 P=257", got, t64, parents)
    if kind == "g_zero":
        for k in XNAMES[1:]:
            assert not bool(got[k].any()), k


def test_cross_view_attention_fn_gradient_is_the_kernels(hip, gpu):
    t = _xview_case(257, 3)[0]
    want = _xview_run(hip, gpu, t)
    kvp, kvs = (t[k].to(gpu).requires_grad_(True) for k in ("kvp", "kvs"))
    n = train_ops.CrossViewAttentionFn.apply(kvp, kvs)
    assert torch.equal(n, want["n"])
    n.backward(t["g"].to(gpu))
    assert torch.equal(kvp.grad[..., :128], want["g_kp"]) and torch.equal(kvp.grad[..., 128:], want["g_vp"])
    assert torch.equal(kvs.grad[..., :128], want["g_ks"]) and torch.equal(kvs.grad[..., 128:], want["g_vs"])
    with pytest.raises(ValueError):
        train_ops.CrossViewAttentionFn.apply(kvp[:, :, :256].contiguous(), kvs)
    with pytest.raises(ValueError):
        hip.xview_attention(torch.zeros(2, 5, 384, device=gpu), torch.zeros(2, 5, 384, device=gpu))      # V = 5
    lib = hip.load_library()
    z = torch.zeros(1, 5, 384, device=gpu)
    assert lib.th_xview_attention_bwd(hip.ctx(gpu), hip._p(z), hip._p(z), hip._p(z), 1, 5, hip._p(z), hip._p(z), hip._stream()) < 0
    assert b"V in 1..4" in lib.th_last_error()


# ---------------------------------------------------------------------------
# 3: the whole network
# ---------------------------------------------------------------------------
def _net():
    with config.override(vit_depth=2):                     # (make_net sets the key and leaves it set)
        return make_net(2).train()


def _net_grads(fn, net, h, f, vd, g):
    for p in net.parameters():
        p.grad = None
    h, f = h.clone().requires_grad_(True), f.clone().requires_grad_(True)
    raw = fn(net, h, f, vd)
    raw.backward(g)
    out = {"raw": raw.detach(), "g_h": h.grad, "g_f": f.grad}
    out.update({k: p.grad for k, p in net.named_parameters() if p.grad is not None})
    return {k: v.detach().cpu().clone() for k, v in out.items()}


def _clear_samples(net64, h, f, vd, margin=MARGIN):
    """the samples none of whose ReLU pre-activations (float64) lies within `margin` of its layer's rms of 0"""
    ops = autograd_path.point_network_torch_ops()
    ok = torch.ones(h.shape[0], dtype=torch.bool)

    def relu_linear(a, W, b):
        nonlocal ok
        pre = F.linear(a, W, b)
        far = pre.abs() > margin * float(pre.pow(2).mean().sqrt())
        ok = ok & far.reshape(h.shape[0], -1).all(dim=1)
        return F.relu(pre)

    with torch.no_grad():
        autograd_path.point_network_device(net64, h, f, vd, ops=dict(ops, relu_linear=relu_linear))
    return ok


@functools.lru_cache(maxsize=None)
def _net_case(P, V):
    rs = np.random.RandomState(1000 * V + P)
    n = 2 * P + 16
    h, f, vd = (_f32(rs.normal(size=s)) for s in ((n, V, 255), (n, V, 384), (n, 27)))
    g = _f32(rs.normal(size=(P, 4)))
    net64 = _net().double()
    ok = _clear_samples(net64, h.double(), f.double(), vd.double(), 2 * MARGIN)    # (the rms of the kept samples differs a little)
    assert int(ok.sum()) >= P, "the case needs P samples whose pre-activations keep clear of 0"
    h, f, vd = (x[ok][:P].contiguous() for x in (h, f, vd))
    assert bool(_clear_samples(net64, h.double(), f.double(), vd.double()).all())
    t64 = _net_grads(autograd_path.point_network, net64, h.double(), f.double(), vd.double(), g.double())
    o32 = _net_grads(autograd_path.point_network, _net(), h, f, vd, g)
    assert len(t64) == 3 + 32
    return (h, f, vd, g), t64, {k: maxdiff(o32[k], t64[k]) for k in t64}


@pytest.mark.parametrize("P", (1, 300))
@pytest.mark.parametrize("V", (1, 3))
def test_point_network_on_the_device_vs_float64(hip, gpu, V, P):
    """point_network_device on the HIP Functions against the float64 run of point_network: raw, g_h, g_f and the gradient of every
    parameter of the per-point network (16 layers, weight and bias: 32 tensors) within the bar.  The exact gradient of
    spatial_key_value_0.key_embed.bias is 0 (a bias on kp_j shifts every logit of a softmax column alike), so what any fp32 run
    leaves there is rounding of its layer's sums: it is held to the bar computed from the layer's WEIGHT gradient (parent and scale
    of that tensor).  Two runs give bit-identical gradients."""
    (h, f, vd, g), t64, parents = _net_case(P, V)
    net = _net().to(gpu)
    args = [x.to(gpu) for x in (h, f, vd, g)]
    got = _net_grads(autograd_path.point_network_device, net, *args)
    again = _net_grads(autograd_path.point_network_device, net, *args)
    assert set(got) == set(t64)
    for k in got:
        assert torch.equal(got[k], again[k]), f"{k}: not bit-identical on two runs"
    _hold(f"point network V={V} P={P}", got, t64, parents, bars_from={KEY0_BIAS: KEY0_WEIGHT})
    # K4's rows with their zero pad column give the same bits
    padded = _net_grads(autograd_path.point_network_device, net, F.pad(args[0], (0, 1)), *args[1:])
    assert torch.equal(padded["raw"], got["raw"]) and torch.equal(padded["g_h"][..., :255], got["g_h"])


# ---------------------------------------------------------------------------
# 4: the golden training step
# ---------------------------------------------------------------------------
ALL_DEVICE = {"train_kernels": "device", "train_attention": "device", "train_vit_dense": "device", "train_maps": "latents",
              "target_prep": "device"}


@pytest.mark.parametrize("others", ({"train_kernels": "torch"}, {"train_kernels": "device"}, ALL_DEVICE),
                         ids=("kernels-torch", "kernels-device", "all-five-device"))
def test_training_step_with_the_point_network_on_the_device_matches_the_reference(hip, gpu, others):
    """tests/test_gpu_train_ops.py::test_training_step_on_the_device_kernels_matches_the_reference with cfg.train_point_net =
    "device": the same golden step of the real reference, the same bars, under both values of cfg.train_kernels and with all five
    other training switches on their device values (the batch carries its rays, so cfg.target_prep = "device" takes them from it)"""
    with config.override(**STEP_CFG, train_point_net="device", **others):
        check_step(golden(), *setup(gpu))
