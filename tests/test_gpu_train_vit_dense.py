"""The training form of TransHE's dense layers, LayerNorm and GELU on the device: th_linear_train_forward / th_linear_bwd /
th_layernorm_forward / th_layernorm_bwd (k_vit_dense_bwd.hip), train_ops.NormLinearFn / GeluLinearFn / LinearFn /
LayerNormFn and cfg.train_vit_dense = "device".

Inputs are fp32 values widened to float64 for the truth, so input rounding is not counted as error.  The yardstick of every
case is measured, never assumed (the bar of tests/test_gpu_train_attention.py): with t64 torch's float64 autograd and o32 its
fp32 autograd on the CPU, per tensor

    parent = max|o32 - t64|,  scale = max|t64|,    bar = 4 max(parent, 2^-22 scale)

Every case prints err / bar of every tensor.  The bar is held by every gradient.  The forward output `y` of the Linear entries is
printed beside it and not asserted: it is th_gemm / th_gemm_ln of the inference path (one fp32 fmaf chain over K, up to 768
terms), whose own parity tests are tests/test_gpu_vit.py; what this file holds of it is that form 0 gives th_linear_forward's
bits.  LayerNorm's forward is new here and is held to the bar.  The stress inputs are kept only where torch's own fp32 stays finite (asserted
when the case is built).  Figures measured on an MI355X are in DESIGN.md section 4."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from transhuman_amd import config, synth
from transhuman_amd.networks import autograd_path, train_ops
from train_step_case import STEP_CFG, check_step, golden, setup
from util import make_net, maxdiff

pytestmark = pytest.mark.gpu

PLAIN, LN, GELU = 0, 1, 2
FLOOR = 2.0 ** -22
EPS = 1e-6
DIM = 192
LAYERS = ((PLAIN, 192, 576), (PLAIN, 192, 192), (PLAIN, 192, 768), (PLAIN, 768, 192),      # (form, in, out)
          (LN, 192, 576), (LN, 192, 768), (GELU, 768, 192))
EDGES = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129)


@pytest.fixture(scope="module")
def hip(gpu):
    from transhuman_amd import hip as H
    H.load_library()
    return H


@functools.lru_cache(maxsize=None)
def _chunk():
    """the rows per partial tile of the weight-gradient kernel, asked of the library (a host call)"""
    from transhuman_amd import build, hip as H
    build.build(force=False, verbose=False)
    return H.wgrad_chunk_rows()


def _rows():
    c = _chunk()
    return EDGES + (c - 1, c, c + 1, 2 * c + 37)


def pytest_generate_tests(metafunc):
    if "M_edge" in metafunc.fixturenames:
        metafunc.parametrize("M_edge", _rows())
    if "M_stress" in metafunc.fixturenames:
        metafunc.parametrize("M_stress", (65, 2 * _chunk() + 37))


# ---------------------------------------------------------------------------
# inputs and references, built once per case
# ---------------------------------------------------------------------------
def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def _inputs(form, in_f, out_f, M, kind):
    rs = np.random.RandomState(1000 * form + in_f + 7 * out_f + 31 * M)
    a = rs.normal(loc=0.3 if form == LN else 0.0, scale=2.0, size=(M, in_f))
    g = rs.normal(size=(M, out_f))
    if kind == "mean100":                      # LayerNorm rows with mean = 100 x std
        a = 100.0 + rs.normal(size=(M, in_f))
    elif kind == "const_row":                  # variance exactly 0: rstd = 1 / sqrt(eps)
        a[::5] = 0.5
    elif kind == "outlier":                    # a single 1e4 in a row
        a[np.arange(0, M, 3), rs.randint(0, in_f, size=len(range(0, M, 3)))] = 1e4
    elif kind == "tiny":                       # variance 4e-8 < eps
        a = a * 1e-4
    elif kind == "grid":                       # u over [-8, 8] with +-0 and the saturated tails
        grid = np.concatenate([np.linspace(-8.0, 8.0, 4093), [0.0, -0.0, -8.0]])
        a = np.resize(grid, M * in_f).reshape(M, in_f).copy()
    elif kind == "zero_row":
        a[M // 2] = 0.0
    elif kind == "g_zero_cols":
        g[:, ::3] = 0.0
    elif kind == "g_range":                    # 2^20 between the smallest and the largest column scale
        g = g * np.exp2(-rs.randint(0, 21, size=out_f))[None]
    else:
        assert kind == "gauss", kind
    W = rs.normal(scale=0.1, size=(out_f, in_f))
    b = rs.normal(scale=0.1, size=out_f)
    lw = rs.uniform(0.5, 1.5, size=in_f) if form == LN else None
    lb = rs.normal(scale=0.2, size=in_f) if form == LN else None
    return {k: (None if v is None else _f32(v)) for k, v in dict(a=a, W=W, b=b, lw=lw, lb=lb, g=g).items()}


def _autograd(form, t, dtype):
    leaf = lambda x: None if x is None else x.to(dtype).clone().requires_grad_(True)
    a, W, b, lw, lb = (leaf(t[k]) for k in ("a", "W", "b", "lw", "lb"))
    op = F.layer_norm(a, (a.shape[-1],), lw, lb, EPS) if form == LN else F.gelu(a) if form == GELU else a
    y = F.linear(op, W, b)
    y.backward(t["g"].to(dtype))
    out = {"y": y.detach(), "g_a": a.grad, "g_W": W.grad, "g_b": b.grad}
    if form == LN:
        out.update(g_ln_w=lw.grad, g_ln_b=lb.grad)
    return out


@functools.lru_cache(maxsize=None)
def _case(form, in_f, out_f, M, kind="gauss"):
    t = _inputs(form, in_f, out_f, M, kind)
    t64, o32 = _autograd(form, t, torch.float64), _autograd(form, t, torch.float32)
    for k, v in o32.items():
        assert v.dtype == torch.float32 and torch.isfinite(v).all(), (kind, k)       # (torch's own fp32 must survive the case)
    return t, t64, {k: maxdiff(o32[k], t64[k]) for k in t64}


def _hold(tag, got, t64, parents, report=()):
    failed = []
    for k, t in t64.items():
        v = got[k].cpu()
        assert v.shape == t.shape and torch.isfinite(v).all(), (tag, k)
        scale, err = float(t.abs().max()), maxdiff(v, t)
        bar = 4.0 * max(parents[k], FLOOR * scale)
        if scale > 0:
            print(f"{tag} {k}: device {err / scale:.3e}, torch fp32 {parents[k] / scale:.3e} of max|ref| = {scale:.3e}; "
                  f"err / bar = {err / bar:.2f}")
        if not err <= bar and k not in report:
            failed.append((k, err, bar))
    assert not failed, (tag, failed)


def _run(hip, gpu, form, t):
    d = {k: (None if v is None else v.to(gpu)) for k, v in t.items()}
    y = hip.linear_train_forward(d["a"], d["W"], d["b"], form, d["lw"], d["lb"], EPS)
    names = ("g_a", "g_W", "g_b", "g_ln_w", "g_ln_b")
    got = dict(zip(names, hip.linear_bwd(d["a"], d["W"], d["g"], form, d["lw"], d["lb"], EPS)))
    again = dict(zip(names, hip.linear_bwd(d["a"], d["W"], d["g"], form, d["lw"], d["lb"], EPS)))
    for k in names:
        assert (got[k] is None) == (form != LN and k.startswith("g_ln")), k
        if got[k] is not None:
            assert torch.equal(got[k], again[k]), f"{k}: not bit-identical on two runs"
    if form == PLAIN:
        assert torch.equal(y, hip.linear(d["a"], d["W"], d["b"])), "form 0 is th_linear_forward"
    got["y"] = y
    return got


# ---------------------------------------------------------------------------
# 1: operator level, every layer shape and operand form, at the tile and chunk edges
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("form,in_f,out_f", LAYERS)
def test_linear_backward_vs_float64_at_the_edges(hip, gpu, form, in_f, out_f, M_edge):
    t, t64, parents = _case(form, in_f, out_f, M_edge)
    _hold(f"dense form={form} {in_f}->{out_f} M={M_edge}", _run(hip, gpu, form, t), t64, parents, report=("y",))


@functools.lru_cache(maxsize=None)
def _ln_case(M, kind="gauss"):
    t = _inputs(LN, DIM, DIM, M, kind)
    out = {}
    for dtype in (torch.float64, torch.float32):
        x, w, b = (t[k].to(dtype).clone().requires_grad_(True) for k in ("a", "lw", "lb"))
        y = F.layer_norm(x, (DIM,), w, b, EPS)
        y.backward(t["g"].to(dtype))
        out[dtype] = {"y": y.detach(), "g_x": x.grad, "g_w": w.grad, "g_b": b.grad}
    for k, v in out[torch.float32].items():
        assert torch.isfinite(v).all(), (kind, k)
    return t, out[torch.float64], {k: maxdiff(out[torch.float32][k], v) for k, v in out[torch.float64].items()}


def _run_ln(hip, gpu, t):
    x, w, b, g = (t[k].to(gpu) for k in ("a", "lw", "lb", "g"))
    got = dict(zip(("g_x", "g_w", "g_b"), hip.layernorm_bwd(x, w, g, EPS)))
    for k, v in zip(("g_x", "g_w", "g_b"), hip.layernorm_bwd(x, w, g, EPS)):
        assert torch.equal(got[k], v), f"{k}: not bit-identical on two runs"
    got["y"] = hip.layernorm_train_forward(x, w, b, EPS)
    return got


def test_layernorm_backward_vs_float64_at_the_edges(hip, gpu, M_edge):
    t, t64, parents = _ln_case(M_edge)
    _hold(f"layernorm M={M_edge}", _run_ln(hip, gpu, t), t64, parents)


# ---------------------------------------------------------------------------
# 2: stress inputs
# ---------------------------------------------------------------------------
LN_STRESS = ("mean100", "const_row", "outlier", "tiny")


@pytest.mark.parametrize("kind", LN_STRESS + ("g_zero_cols", "g_range"))
def test_norm_linear_stress(hip, gpu, kind, M_stress):
    t, t64, parents = _case(LN, 192, 576, M_stress, kind)
    _hold(f"norm-linear {kind} M={M_stress}", _run(hip, gpu, LN, t), t64, parents, report=("y",))


@pytest.mark.parametrize("kind", LN_STRESS + ("g_range",))
def test_layernorm_stress(hip, gpu, kind, M_stress):
    t, t64, parents = _ln_case(M_stress, kind)
    _hold(f"layernorm {kind} M={M_stress}", _run_ln(hip, gpu, t), t64, parents)


@pytest.mark.parametrize("kind", ("grid", "g_zero_cols", "g_range"))
def test_gelu_linear_stress(hip, gpu, kind, M_stress):
    t, t64, parents = _case(GELU, 768, 192, M_stress, kind)
    _hold(f"gelu-linear {kind} M={M_stress}", _run(hip, gpu, GELU, t), t64, parents, report=("y",))


@pytest.mark.parametrize("kind", ("zero_row", "g_zero_cols", "g_range"))
def test_linear_stress(hip, gpu, kind, M_stress):
    t, t64, parents = _case(PLAIN, 192, 192, M_stress, kind)
    _hold(f"linear {kind} M={M_stress}", _run(hip, gpu, PLAIN, t), t64, parents, report=("y",))


# ---------------------------------------------------------------------------
# 3: hygiene
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("form,in_f,out_f", ((PLAIN, 192, 192), (LN, 192, 576), (GELU, 768, 192)))
def test_zero_upstream_gradient_gives_zero(hip, gpu, form, in_f, out_f, M_stress):
    t = dict(_case(form, in_f, out_f, M_stress)[0])
    t["g"] = torch.zeros_like(t["g"])
    got = _run(hip, gpu, form, t)
    for k in ("g_a", "g_W", "g_b") + (("g_ln_w", "g_ln_b") if form == LN else ()):
        assert bool((got[k] == 0).all()), k
    if form == LN:
        x, w = t["a"].to(gpu), t["lw"].to(gpu)
        for v in hip.layernorm_bwd(x, w, torch.zeros_like(x), EPS):
            assert bool((v == 0).all())


def _filled(nbytes, byte, gpu):
    return torch.full((max(int(nbytes), 256),), byte, dtype=torch.uint8, device=gpu)


def _raw_linear(hip, gpu, form, d, M, in_f, out_f, byte):
    """forward and backward through the C ABI itself, on workspaces filled with `byte` and outputs filled with NaN"""
    lib = hip.load_library()
    h, s, p = hip.ctx(gpu), hip._stream(), hip._p
    nan = lambda *shape: torch.full(shape, float("nan"), device=gpu)
    lin = hip.ThLinear(p(d["W"]), p(d["b"]), out_f, in_f)
    y, g_a, g_w, g_b, g_lw, g_lb = nan(M, out_f), nan(M, in_f), nan(out_f, in_f), nan(out_f), nan(in_f), nan(in_f)
    ws = _filled(lib.th_linear_train_workspace_bytes(M, out_f, in_f, form), byte, gpu)
    hip._check(lib.th_linear_train_forward(h, p(d["a"]), in_f, M, form, p(d["lw"]), p(d["lb"]), EPS, C.byref(lin), p(y), out_f,
                                           p(ws), ws.numel(), s))
    ws = _filled(lib.th_linear_bwd_workspace_bytes(M, out_f, in_f, form), byte, gpu)
    hip._check(lib.th_linear_bwd(h, p(d["a"]), in_f, M, form, p(d["lw"]), p(d["lb"]), EPS, C.byref(lin), p(d["g"]), out_f, p(g_a),
                                 in_f, p(g_w), p(g_b), p(g_lw), p(g_lb), p(ws), ws.numel(), s))
    out = [y, g_a, g_w, g_b] + ([g_lw, g_lb] if form == LN else [])
    return [v.cpu() for v in out]


@pytest.mark.parametrize("form,in_f,out_f", ((PLAIN, 192, 192), (LN, 192, 768), (GELU, 768, 192)))
def test_results_ignore_workspace_contents(hip, gpu, form, in_f, out_f, M_stress):
    t = _case(form, in_f, out_f, M_stress)[0]
    d = {k: (None if v is None else v.to(gpu)) for k, v in t.items()}
    res = [_raw_linear(hip, gpu, form, d, M_stress, in_f, out_f, byte) for byte in (0x00, 0xFF)]      # 0xFF..: NaN as fp32
    for a, b in zip(*res):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    # ... and they are what the binding returns
    via = _run(hip, gpu, form, t)
    for a, k in zip(res[0], ("y", "g_a", "g_W", "g_b", "g_ln_w", "g_ln_b")):
        assert torch.equal(a, via[k].cpu()), k
    if form == LN:
        lib = hip.load_library()
        x, w, g = d["a"], d["lw"], d["g"][:, :in_f].contiguous()
        outs = []
        for byte in (0x00, 0xFF):
            ws = _filled(lib.th_layernorm_bwd_workspace_bytes(M_stress, in_f), byte, gpu)
            g_x, g_w, g_b = (torch.full(sh, float("nan"), device=gpu) for sh in ((M_stress, in_f), (in_f,), (in_f,)))
            hip._check(lib.th_layernorm_bwd(hip.ctx(gpu), hip._p(x), in_f, M_stress, in_f, hip._p(w), EPS, hip._p(g), in_f,
                                            hip._p(g_x), in_f, hip._p(g_w), hip._p(g_b), hip._p(ws), ws.numel(), hip._stream()))
            outs.append((g_x.cpu(), g_w.cpu(), g_b.cpu()))
        for a, b in zip(*outs):
            assert torch.isfinite(a).all() and torch.equal(a, b)


def test_refusals(hip, gpu):
    """an argument error comes back as a code and a message; nothing is launched: the outputs keep their contents; the next
    valid call works"""
    lib = hip.load_library()
    M, in_f, out_f = 65, 192, 576
    t = _case(LN, in_f, out_f, M)[0]
    d = {k: v.to(gpu) for k, v in t.items()}
    h, s, p = hip.ctx(gpu), hip._stream(), hip._p
    null = C.c_void_p(0)
    seven = lambda *shape: torch.full(shape, 7.0, device=gpu)
    y, g_a, g_w, g_b, g_lw, g_lb, g_x = (seven(M, out_f), seven(M, in_f), seven(out_f, in_f), seven(out_f), seven(in_f),
                                         seven(in_f), seven(M, in_f))
    nf, nb = (int(q(M, out_f, in_f, LN)) for q in (lib.th_linear_train_workspace_bytes, lib.th_linear_bwd_workspace_bytes))
    nl = int(lib.th_layernorm_bwd_workspace_bytes(M, in_f))
    assert nf > 0 and nb > 0 and nl > 0
    wf, wb, wl = _filled(nf, 0, gpu), _filled(nb, 0, gpu), _filled(nl, 0, gpu)

    def layer(o=out_f, i=in_f, w=p(d["W"])):
        return hip.ThLinear(w, p(d["b"]), o, i)

    def refused(rc, word):
        assert rc != 0
        msg = lib.th_last_error()
        assert msg and word in msg, msg

    def fwd(ctx=h, a=p(d["a"]), m=M, form=LN, lw=p(d["lw"]), lb=p(d["lb"]), lin=None, c=p(y), w=p(wf), nbytes=nf):
        lin = lin or layer()
        return lib.th_linear_train_forward(ctx, a, in_f, m, form, lw, lb, EPS, C.byref(lin), c, out_f, w, nbytes, s)

    def bwd(ctx=h, a=p(d["a"]), m=M, form=LN, lw=p(d["lw"]), lb=p(d["lb"]), lin=None, g=p(d["g"]), ga=p(g_a), gw=p(g_w),
            gb=p(g_b), glw=p(g_lw), glb=p(g_lb), w=p(wb), nbytes=nb):
        lin = lin or layer()
        return lib.th_linear_bwd(ctx, a, in_f, m, form, lw, lb, EPS, C.byref(lin), g, out_f, ga, in_f, gw, gb, glw, glb, w,
                                 nbytes, s)

    def lnb(ctx=h, x=p(d["a"]), m=M, dim=in_f, w=p(d["lw"]), g=p(d["a"]), gx=p(g_x), gw=p(g_lw), gb=p(g_lb), ws=p(wl), nbytes=nl):
        return lib.th_layernorm_bwd(ctx, x, in_f, m, dim, w, EPS, g, in_f, gx, in_f, gw, gb, ws, nbytes, s)

    for name in ("ctx", "a", "lw", "lb", "c", "w"):
        refused(fwd(**{name: null}), b"null")
    refused(fwd(lin=layer(w=null)), b"null")
    refused(fwd(lin=layer(i=184)), b"multiples of 16")              # in_f = 184 is no multiple of 16 (lda = 192 covers it)
    refused(fwd(lin=layer(o=568)), b"multiples of 16")
    refused(fwd(nbytes=nf - 1), b"workspace")
    refused(fwd(m=0), b"M >= 1")
    refused(fwd(form=3), b"form")
    refused(fwd(a=C.c_void_p(d["a"].data_ptr() + 4)), b"aligned")
    for name in ("ctx", "a", "lw", "lb", "g", "gw", "glw", "glb", "w"):
        refused(bwd(**{name: null}), b"null")
    refused(bwd(lin=layer(w=null)), b"null")
    refused(bwd(lin=layer(i=184)), b"multiples of 16")
    refused(bwd(lin=layer(o=568)), b"multiples of 16")
    refused(bwd(nbytes=nb - 1), b"workspace")
    refused(bwd(m=0), b"M >= 1")
    refused(bwd(form=-1), b"form")
    refused(bwd(g=C.c_void_p(d["g"].data_ptr() + 4)), b"aligned")
    for name in ("ctx", "x", "w", "g", "gx", "gw", "gb", "ws"):
        refused(lnb(**{name: null}), b"null")
    refused(lnb(dim=184), b"multiple of 16")
    refused(lnb(nbytes=nl - 1), b"workspace")
    refused(lnb(m=0), b"M >= 1")
    refused(lib.th_layernorm_forward(h, p(d["a"]), in_f, M, 184, p(d["lw"]), p(d["lb"]), EPS, p(g_x), in_f, s), b"multiple of 16")
    refused(lib.th_layernorm_forward(h, null, in_f, M, in_f, p(d["lw"]), p(d["lb"]), EPS, p(g_x), in_f, s), b"null")
    torch.cuda.synchronize()
    for v in (y, g_a, g_w, g_b, g_lw, g_lb, g_x):
        assert bool((v == 7.0).all())
    # ... and the same calls with nothing wrong go through (g_b and g_A are optional)
    hip._check(fwd())
    hip._check(bwd())
    hip._check(lnb())
    for v in (y, g_a, g_w, g_b, g_lw, g_lb, g_x):
        assert torch.isfinite(v).all() and not bool((v == 7.0).any())
    want_w = g_w.clone()
    g_w.fill_(7.0)
    hip._check(bwd(ga=null, gb=null, glw=null, glb=null))
    assert torch.equal(g_w, want_w)


# ---------------------------------------------------------------------------
# 4: through autograd
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("form,in_f,out_f", ((PLAIN, 192, 192), (LN, 192, 576), (GELU, 768, 192)))
def test_function_gradients_are_the_kernels(hip, gpu, form, in_f, out_f):
    M = 3 * ((_chunk() + 3) // 3)                        # more than one chunk, and three "views"
    t = _case(form, in_f, out_f, M)[0]
    want = _run(hip, gpu, form, t)
    leaf = lambda k: None if t[k] is None else t[k].to(gpu).requires_grad_(True)
    a, W, b, lw, lb = (leaf(k) for k in ("a", "W", "b", "lw", "lb"))
    a3 = a.detach().reshape(3, M // 3, in_f).requires_grad_(True)                             # (any leading shape)
    if form == LN:
        y = train_ops.NormLinearFn.apply(a3, lw, lb, W, b, EPS)
    elif form == GELU:
        y = train_ops.GeluLinearFn.apply(a3, W, b)
    else:
        y = train_ops.LinearFn.apply(a3, W, b)
    assert torch.equal(y.reshape(M, out_f), want["y"])
    y.backward(t["g"].to(gpu).reshape(y.shape))
    got = {"g_a": a3.grad.reshape(M, in_f), "g_W": W.grad, "g_b": b.grad}
    if form == LN:
        got.update(g_ln_w=lw.grad, g_ln_b=lb.grad)
    for k, v in got.items():
        assert torch.equal(v, want[k]), k


def test_layernorm_fn_gradient_is_the_kernels(hip, gpu):
    M = 129
    t = _ln_case(M)[0]
    want = _run_ln(hip, gpu, t)
    x, w, b = (t[k].to(gpu).requires_grad_(True) for k in ("a", "lw", "lb"))
    y = train_ops.LayerNormFn.apply(x, w, b, EPS)
    assert torch.equal(y, want["y"])
    y.backward(t["g"].to(gpu))
    for k, v in (("g_x", x.grad), ("g_w", w.grad), ("g_b", b.grad)):
        assert torch.equal(v, want[k]), k


def test_functions_refuse_what_they_cannot_take(hip, gpu):
    w, b = torch.zeros(192, 192, device=gpu, requires_grad=True), torch.zeros(192, device=gpu, requires_grad=True)
    x = torch.zeros(2, 5, 192, device=gpu)
    with pytest.raises(ValueError, match="contiguous float32"):
        train_ops.LinearFn.apply(x.double(), w, b)
    with pytest.raises(ValueError, match="contiguous float32"):
        train_ops.LinearFn.apply(x.transpose(0, 1), w, b)
    with pytest.raises(ValueError, match="contiguous float32"):
        train_ops.LayerNormFn.apply(x, b.double(), b)
    with pytest.raises(hip.HipError):
        train_ops.GeluLinearFn.apply(x.cpu(), w, b)


# ---------------------------------------------------------------------------
# 5, 6: the ViT with both switches on the device
# ---------------------------------------------------------------------------
def _vit(depth):
    with config.override(vit_depth=depth):                 # (make_net sets the key and leaves it set)
        return make_net(depth).ViT


def _vit_grads(vit, x, pe, w, attention, dense):
    """gradients of sum(w * vit_forward) with respect to x and EVERY parameter of every block and of the final norm"""
    for p in vit.parameters():
        p.grad = None
    x = x.clone().requires_grad_(True)
    (autograd_path.vit_forward(vit, x, pe, attention=attention, dense=dense) * w).sum().backward()
    out = {"x": x.grad}
    for k, p in vit.named_parameters():
        if k.startswith(("blocks.", "norm.")):
            assert p.grad is not None, k
            out[k] = p.grad
    return {k: v.detach().cpu().clone() for k, v in out.items()}


def _vit_inputs(V, N):
    x = torch.from_numpy(synth.smooth_noise((V, N, DIM), 31 + N, passes=0))
    pe = torch.rand(V, N, 3, generator=torch.Generator().manual_seed(N)) * 2 - 1
    w = torch.randn(V, N, DIM, generator=torch.Generator().manual_seed(N + 1))
    return x, pe, w


@pytest.mark.parametrize("V,N", ((2, 17), (3, 300)))
def test_vit_forward_on_the_device_vs_float64(hip, gpu, V, N):
    x, pe, w = _vit_inputs(V, N)
    vit = _vit(2).train()
    o32 = _vit_grads(vit, x, pe, w, "torch", "torch")
    # the float64 network takes the SAME positional table, widened (see tests/test_gpu_train_attention.py)
    tab = vit.get_PE(pe).clone()
    vit64 = _vit(2).double().train()
    vit64.get_PE = lambda _pe: tab.double()
    t64 = _vit_grads(vit64, x.double(), pe, w.double(), "torch", "torch")
    got = _vit_grads(_vit(2).to(gpu).train(), x.to(gpu), pe.to(gpu), w.to(gpu), "device", "device")
    assert len(got) == len(t64) == 1 + 2 * 12 + 2
    failed = []
    for k, t in t64.items():
        assert t.dtype == torch.float64 and got[k].shape == t.shape and torch.isfinite(got[k]).all(), k
        scale, parent, err = float(t.abs().max()), maxdiff(o32[k], t), maxdiff(got[k], t)
        bar = 4.0 * max(parent, FLOOR * scale)
        print(f"TransHE on the device V={V} N={N} {k}: device {err / scale:.3e}, torch fp32 {parent / scale:.3e}; "
              f"err / bar = {err / bar:.2f}")
        if not err <= bar:
            failed.append((k, err, bar))
    assert not failed, failed


def test_vit_gradient_is_bit_identical_from_run_to_run(hip, gpu):
    x, pe, w = (t.to(gpu) for t in _vit_inputs(3, 300))
    vit = _vit(2).to(gpu).train()
    a = _vit_grads(vit, x, pe, w, "device", "device")
    b = _vit_grads(vit, x, pe, w, "device", "device")
    assert len(a) == 27
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ---------------------------------------------------------------------------
# 7: the golden training step
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kernels", ("torch", "device"))
def test_training_step_with_transhe_on_the_device_matches_the_reference(hip, gpu, kernels):
    """tests/test_train_path.py::test_training_step_matches_the_reference with cfg.train_vit_dense = cfg.train_attention =
    "device": the same golden step of the real reference, the same bars, under both values of cfg.train_kernels"""
    with config.override(**STEP_CFG, train_kernels=kernels, train_attention="device", train_vit_dense="device"):
        check_step(golden(), *setup(gpu))


# ---------------------------------------------------------------------------
# 8: memory
# ---------------------------------------------------------------------------
def test_device_dense_layers_keep_fewer_activations(hip, gpu):
    """per layer and row torch autograd keeps 3072 floats, the device form 1920 (LN1(x), LN2(x1) and gelu(u) are recomputed):
    1152 M 4 B = 20.7 MB per layer at M = V N = 4500.  Against that the device form spends, once, one layer's transients (the
    gelu(u) operand of fc2's forward, 768 floats per row, or the gradients in flight) and the weight-gradient partials.  From
    depth 4 on the saving (83 MB) dominates: the peak must be strictly lower"""
    V, N, depth = 3, 1500, 4
    vit = _vit(depth).to(gpu).train()
    assert len(vit.blocks) == depth
    x = torch.from_numpy(synth.smooth_noise((V, N, DIM), 5, passes=0)).to(gpu)
    pe = (torch.rand(V, N, 3, generator=torch.Generator().manual_seed(5)) * 2 - 1).to(gpu)
    peak = {}
    for dense in ("device", "torch"):
        _vit_grads(vit, x, pe, 1.0, "device", dense)           # (warm-up: library handles and workspaces of the first call)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        _vit_grads(vit, x, pe, 1.0, "device", dense)
        torch.cuda.synchronize()
        peak[dense] = torch.cuda.max_memory_allocated()
    print(f"peak allocated, depth {depth}, V = {V}, N = {N}, attention on the device: dense torch {peak['torch'] / 2 ** 20:.1f} MiB, "
          f"dense device {peak['device'] / 2 ** 20:.1f} MiB")
    assert peak["device"] < peak["torch"], peak
