"""The training form of TransHE's attention on the device: th_attention_train (the inference kernels, which also write each
row's log-sum-exp), th_attention_bwd (k_vit_bwd.hip), train_ops.AttentionFn and cfg.train_attention = "device".

Inputs are fp32 values widened to float64 for the truth, so input rounding is not counted as error.  The yardstick of every
case is measured, never assumed: with t64 torch's float64 autograd of oracle.attention and o32 its fp32 autograd on the CPU,

    parent = max|o32 - t64|,  scale = max|t64|,    bar = 4 max(parent, 2^-22 scale)

taken per block (dQ, dK, dV) with the block's own parent and scale -- the project's bar for a non-linear backward
(test_composite_backward_vs_float64).  Every case prints err / scale beside torch's ("K3 training form", records
the worst ratios).

Figures measured on an MI355X are in DESIGN.md section 4."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import th_oracle as O
from transhuman_amd import config, synth
from transhuman_amd.networks import autograd_path, train_ops
from train_step_case import STEP_CFG, check_step, golden, setup
from util import make_net, maxdiff

pytestmark = pytest.mark.gpu

HEADS, HD = 3, 64
DIM = HEADS * HD
EDGES = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 700, 701)
FLOOR = 2.0 ** -22


@pytest.fixture(scope="module")
def hip(gpu):
    from transhuman_amd import hip as H
    H.load_library()
    return H


# ---------------------------------------------------------------------------
# inputs (the case generators of tests/test_gpu_vit.py) and references, built once per case
# ---------------------------------------------------------------------------
def _pack(q, k, v):
    """q, k, v [V, heads, N, 64] -> qkv [V, N, 3 dim] in the layout the qkv layer writes (column = which dim + head 64 + d)"""
    V, H, N, _ = q.shape
    return torch.stack([q, k, v], 0).permute(1, 3, 0, 2, 4).reshape(V, N, 3 * H * HD).contiguous().float()


def _planes(fn, V, N, seed):
    """fn(rs, N) -> (q, k, v) float arrays [N, 64]; every (view, head) plane draws from a seed of its own"""
    qkv = np.empty((3, V, HEADS, N, HD), np.float32)
    for view in range(V):
        for head in range(HEADS):
            qkv[:, view, head] = np.stack(fn(np.random.RandomState(seed + 97 * view + 13 * head), N))
    return _pack(*torch.from_numpy(qkv))


def _gauss(rs, N, sigma=3.0):
    return tuple(rs.normal(scale=sigma, size=(N, HD)) for _ in range(3))


def _along_u(coeff):
    """q = 8 u + 0.1 noise, key j = coeff(N, rs)[j] u: the logit of key j is about coeff[j] for every query"""
    def fn(rs, N):
        u = rs.normal(size=HD)
        u /= np.linalg.norm(u)
        q = 8.0 * u[None] + 0.1 * rs.normal(size=(N, HD))
        k = coeff(N, rs)[:, None] * u[None]
        return q, k, rs.normal(scale=3.0, size=(N, HD))
    return fn


def _dominant(pos):
    def coeff(N, rs):
        c = rs.uniform(0.0, 4.0, size=N)
        c[pos if pos >= 0 else N + pos] = 12.0
        return c
    return coeff


def _scaled(sq, sk, sv):
    def fn(rs, N):
        q, k, v = _gauss(rs, N)
        return q * sq, k * sk, v * sv
    return fn


STRESS = {
    "rising": _along_u(lambda N, rs: np.arange(N) / 4.0),                 # every tile raises the running maximum
    "falling": _along_u(lambda N, rs: np.arange(N)[::-1] / 4.0),          # the first key wins
    "negative": _along_u(lambda N, rs: -44.0 - 60.0 * rs.uniform(size=N)),    # every logit <= -40
    "dominant_last": _along_u(_dominant(-1)),
    "dominant_63": _along_u(_dominant(63)),
    "dominant_64": _along_u(_dominant(64)),
    "v_small": _scaled(1.0, 1.0, 2.0 ** -10),
    "v_large": _scaled(1.0, 1.0, 2.0 ** 10),
    "q_small_k_large": _scaled(2.0 ** -4, 2.0 ** 4, 1.0),
}


def _blocks(g_qkv):
    """[V, N, 3 dim] -> (dQ, dK, dV), each [V, N, dim]"""
    V, N, _ = g_qkv.shape
    r = g_qkv.reshape(V, N, 3, DIM)
    return r[:, :, 0], r[:, :, 1], r[:, :, 2]


def _logits(qkv):
    V, N, _ = qkv.shape
    r = qkv.reshape(V, N, 3, HEADS, HD).permute(2, 0, 3, 1, 4)
    return (r[0] @ r[1].transpose(-2, -1)) * 0.125


@functools.lru_cache(maxsize=None)
def _case(name, V, N):
    """qkv, g_out (fp32, CPU); float64 gradient and log-sum-exp; the fp32 CPU evaluation's error of each (the yardstick)"""
    qkv = _planes(_gauss if name == "gauss" else STRESS[name], V, N, seed=1000 + N)
    g_out = torch.from_numpy(np.random.RandomState(5000 + N + V).normal(size=(V, N, DIM)).astype(np.float32))
    x64 = qkv.double().requires_grad_(True)
    O.attention(x64, HEADS).backward(g_out.double())
    x32 = qkv.clone().requires_grad_(True)
    O.attention(x32, HEADS).backward(g_out)
    t64, o32 = x64.grad, x32.grad
    assert t64.dtype == torch.float64 and o32.dtype == torch.float32 and torch.isfinite(o32).all()
    lse64 = torch.logsumexp(_logits(qkv.double()), dim=-1)
    lse32 = torch.logsumexp(_logits(qkv), dim=-1)
    assert float(_logits(qkv.double()).abs().max()) <= 250.0
    parents = [maxdiff(a, b) for a, b in zip(_blocks(o32), _blocks(t64))]
    return qkv, g_out, t64, parents, lse64, maxdiff(lse32, lse64)


def _hold_backward(hip, gpu, name, V, N):
    qkv, g_out, t64, parents, _, _ = _case(name, V, N)
    qd, gd = qkv.to(gpu), g_out.to(gpu)
    out, lse = hip.attention_train(qd, HEADS)
    got = hip.attention_bwd(qd, out, lse, gd, HEADS)
    again = hip.attention_bwd(qd, out, lse, gd, HEADS)
    assert torch.equal(got, again), "not bit-identical on two runs"
    got = got.cpu()
    assert torch.isfinite(got).all()
    failed = []
    for blk, g, t, parent in zip(("dQ", "dK", "dV"), _blocks(got), _blocks(t64), parents):
        scale = float(t.abs().max())
        err = maxdiff(g, t)
        bar = 4.0 * max(parent, FLOOR * scale)
        if scale > 0:
            print(f"K3 backward {name} V={V} N={N} {blk}: device {err / scale:.3e}, torch fp32 {parent / scale:.3e} of "
                  f"max|ref| = {scale:.3e}; err / bar = {err / bar:.2f}")
        if not err <= bar:
            failed.append((blk, err, bar))
    assert not failed, (name, V, N, failed)
    return got


# ---------------------------------------------------------------------------
# 1: the forward is th_attention's, and its log-sum-exp
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("V", (1, 3))
@pytest.mark.parametrize("N", EDGES)
def test_forward_equals_attention_and_lse_vs_float64(hip, gpu, N, V):
    qkv, _, _, _, lse64, parent = _case("gauss", V, N)
    qd = qkv.to(gpu)
    bar = 4.0 * max(parent, FLOOR * float(lse64.abs().max()))
    for form in (0, 2, 3):
        out, lse = hip.attention_train(qd, HEADS, form)
        assert torch.equal(out, hip.attention(qd, HEADS, form)), form
        assert tuple(lse.shape) == (V, HEADS, N) and torch.isfinite(lse).all()
        err = maxdiff(lse.cpu(), lse64)
        print(f"K3 lse V={V} N={N} form={form}: device {err:.3e}, torch fp32 {parent:.3e}, bar {bar:.3e}")
        assert err <= bar, (form, err, bar)


# ---------------------------------------------------------------------------
# 2: the backward at the tile edges
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("V", (1, 3))
@pytest.mark.parametrize("N", EDGES)
def test_backward_vs_float64_at_tile_edges(hip, gpu, N, V):
    _hold_backward(hip, gpu, "gauss", V, N)


# ---------------------------------------------------------------------------
# 3: the softmax where it carries weight
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N", (65, 705))
@pytest.mark.parametrize("name", sorted(STRESS))
def test_backward_softmax_stress(hip, gpu, name, N):
    _hold_backward(hip, gpu, name, 2, N)


# ---------------------------------------------------------------------------
# 4: exact small cases
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("V", (1, 3))
def test_single_token_is_exact(hip, gpu, V):
    qkv, g_out = _case("gauss", V, 1)[:2]
    qd, gd = qkv.to(gpu), g_out.to(gpu)
    out, lse = hip.attention_train(qd, HEADS)
    dq, dk, dv = _blocks(hip.attention_bwd(qd, out, lse, gd, HEADS))
    assert bool((dq == 0).all()) and bool((dk == 0).all())
    assert torch.equal(dv, gd)


@pytest.mark.parametrize("V,N", ((2, 65), (1, 700)))
def test_zero_upstream_gradient_gives_zero(hip, gpu, V, N):
    qd = _case("gauss", 3, N)[0][:V].contiguous().to(gpu)
    out, lse = hip.attention_train(qd, HEADS)
    got = hip.attention_bwd(qd, out, lse, torch.zeros((V, N, DIM), device=gpu), HEADS)
    assert bool((got == 0).all())


def _filled(nbytes, byte, gpu):
    return torch.full((max(int(nbytes), 256),), byte, dtype=torch.uint8, device=gpu)


@pytest.mark.parametrize("V,N", ((3, 300), (1, 64), (2, 705)))
def test_results_ignore_workspace_contents(hip, gpu, V, N):
    lib = hip.load_library()
    qkv = _planes(_gauss, V, N, seed=7 + N).to(gpu)
    g_out = torch.randn((V, N, DIM), generator=torch.Generator().manual_seed(N)).to(gpu)
    h, s = hip.ctx(gpu), hip._stream()
    nf, nb = lib.th_attention_train_workspace_bytes(V, N, HEADS), lib.th_attention_bwd_workspace_bytes(V, N, HEADS)
    res = []
    for byte in (0x00, 0xFF):                            # 0xFF..: NaN as fp32 and as fp16
        ws = _filled(nf, byte, gpu)
        out = torch.full((V, N, DIM), float("nan"), device=gpu)
        lse = torch.full((V, HEADS, N), float("nan"), device=gpu)
        hip._check(lib.th_attention_train(h, hip._p(qkv), V, N, HEADS, 0, hip._p(out), hip._p(lse), hip._p(ws), ws.numel(), s))
        ws = _filled(nb, byte, gpu)
        g = torch.full((V, N, 3 * DIM), float("nan"), device=gpu)
        hip._check(lib.th_attention_bwd(h, hip._p(qkv), hip._p(out), hip._p(lse), hip._p(g_out), V, N, HEADS, hip._p(g),
                                        hip._p(ws), ws.numel(), s))
        res.append((out.cpu(), lse.cpu(), g.cpu()))
    for a, b in zip(*res):
        assert torch.isfinite(a).all() and torch.equal(a, b)


# ---------------------------------------------------------------------------
# 5: refusals
# ---------------------------------------------------------------------------
def test_refusals(hip, gpu):
    """an argument error comes back as a code and a message; nothing is launched: the outputs keep their contents"""
    lib = hip.load_library()
    V, N = 2, 65
    qkv = _planes(_gauss, V, N, seed=3).to(gpu)
    g_out = torch.ones((V, N, DIM), device=gpu)
    nf, nb = int(lib.th_attention_train_workspace_bytes(V, N, HEADS)), int(lib.th_attention_bwd_workspace_bytes(V, N, HEADS))
    assert nf >= 2 * V * HEADS * 2 * 128 * 64 * 2 and nb >= V * HEADS * N * 4
    wf, wb = _filled(nf, 0, gpu), _filled(nb, 0, gpu)
    out = torch.full((V, N, DIM), 7.0, device=gpu)
    lse = torch.full((V, HEADS, N), 7.0, device=gpu)
    g = torch.full((V, N, 3 * DIM), 7.0, device=gpu)
    h, s = hip.ctx(gpu), hip._stream()
    null = C.c_void_p(0)
    p = hip._p

    def off4(t):
        return C.c_void_p(t.data_ptr() + 4)

    def refused(rc, word):
        assert rc != 0
        msg = lib.th_last_error()
        assert msg and word in msg, msg

    def fwd(ctx=h, q=p(qkv), v=V, n=N, heads=HEADS, form=2, o=p(out), l=p(lse), w=p(wf), nbytes=nf):
        return lib.th_attention_train(ctx, q, v, n, heads, form, o, l, w, nbytes, s)

    def bwd(ctx=h, q=p(qkv), o=p(out), l=p(lse), go=p(g_out), v=V, n=N, heads=HEADS, gq=p(g), w=p(wb), nbytes=nb):
        return lib.th_attention_bwd(ctx, q, o, l, go, v, n, heads, gq, w, nbytes, s)

    for name in ("ctx", "q", "o", "l", "w"):
        refused(fwd(**{name: null}), b"null")
    for name in ("q", "o", "l", "w"):
        refused(fwd(**{name: off4({"q": qkv, "o": out, "l": lse, "w": wf}[name])}), b"aligned")
    refused(fwd(nbytes=nf - 1), b"workspace")
    refused(fwd(form=1), b"form")
    refused(fwd(heads=0), b"heads")
    refused(fwd(n=0), b"N")
    for name in ("ctx", "q", "o", "l", "go", "gq", "w"):
        refused(bwd(**{name: null}), b"null")
    for name in ("q", "o", "l", "go", "gq", "w"):
        refused(bwd(**{name: off4({"q": qkv, "o": out, "l": lse, "go": g_out, "gq": g, "w": wb}[name])}), b"aligned")
    refused(bwd(nbytes=nb - 1), b"workspace")
    refused(bwd(heads=0), b"heads")
    refused(bwd(n=0), b"N")
    for fn in (lib.th_attention_train_workspace_bytes, lib.th_attention_bwd_workspace_bytes):
        assert fn(V, 0, HEADS) == 0 and fn(V, N, 0) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((lse == 7.0).all()) and bool((g == 7.0).all())
    # ... and the same calls with nothing wrong go through
    hip._check(fwd())
    hip._check(bwd())
    for t in (out, lse, g):
        assert torch.isfinite(t).all() and not bool((t == 7.0).any())


# ---------------------------------------------------------------------------
# 6: through autograd
# ---------------------------------------------------------------------------
def test_attention_fn_gradient_is_the_kernels(hip, gpu):
    qkv, g_out = _case("gauss", 3, 129)[:2]
    qd, gd = qkv.to(gpu), g_out.to(gpu)
    out, lse = hip.attention_train(qd, HEADS)
    want = hip.attention_bwd(qd, out, lse, gd, HEADS)
    x = qd.clone().requires_grad_(True)
    y = train_ops.AttentionFn.apply(x, HEADS)
    assert torch.equal(y, out)
    y.backward(gd)
    assert torch.equal(x.grad, want)


def _vit_grads(vit, x, pe, w, attention):
    """gradients of sum(w * vit_forward) with respect to x and each block's attn.qkv.weight / bias and attn.proj.weight"""
    for p in vit.parameters():
        p.grad = None
    x = x.clone().requires_grad_(True)
    (autograd_path.vit_forward(vit, x, pe, attention=attention) * w).sum().backward()
    out = {"x": x.grad}
    for i, blk in enumerate(vit.blocks):
        out[f"blocks.{i}.attn.qkv.weight"] = blk.attn.qkv.weight.grad
        out[f"blocks.{i}.attn.qkv.bias"] = blk.attn.qkv.bias.grad
        out[f"blocks.{i}.attn.proj.weight"] = blk.attn.proj.weight.grad
    return {k: v.detach().cpu().clone() for k, v in out.items()}


@pytest.mark.parametrize("V,N", ((2, 17), (3, 300)))
def test_vit_forward_with_device_attention_vs_float64(hip, gpu, V, N):
    x = torch.from_numpy(synth.smooth_noise((V, N, DIM), 31 + N, passes=0))
    pe = torch.rand(V, N, 3, generator=torch.Generator().manual_seed(N)) * 2 - 1
    w = torch.randn(V, N, DIM, generator=torch.Generator().manual_seed(N + 1))
    vit = make_net(2).ViT
    vit.train()
    o32 = _vit_grads(vit, x, pe, w, "torch")
    # the float64 network takes the SAME positional table, widened (get_PE evaluates 32 octaves of sin / cos in the dtype of
    # the module: in float64 it is another table, not a more exact one)
    tab = vit.get_PE(pe).clone()
    vit64 = make_net(2).ViT.double().train()
    vit64.get_PE = lambda _pe: tab.double()
    t64 = _vit_grads(vit64, x.double(), pe, w.double(), "torch")
    got = _vit_grads(make_net(2).ViT.to(gpu).train(), x.to(gpu), pe.to(gpu), w.to(gpu), "device")
    assert len(got) == 1 + 3 * 2
    failed = []
    for k, t in t64.items():
        assert t.dtype == torch.float64 and got[k].shape == t.shape and torch.isfinite(got[k]).all(), k
        scale, parent, err = float(t.abs().max()), maxdiff(o32[k], t), maxdiff(got[k], t)
        bar = 4.0 * max(parent, FLOOR * scale)
        print(f"K3 training form V={V} N={N} {k}: device {err / scale:.3e}, torch fp32 {parent / scale:.3e}; err / bar = {err / bar:.2f}")
        if not err <= bar:
            failed.append((k, err, bar))
    assert not failed, failed


# ---------------------------------------------------------------------------
# 7: the golden training step
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kernels", ("torch", "device"))
def test_training_step_with_device_attention_matches_the_reference(hip, gpu, kernels):
    """tests/test_train_path.py::test_training_step_matches_the_reference with cfg.train_attention = "device": the same golden
    step of the real reference, the same bars, under both values of cfg.train_kernels"""
    with config.override(**STEP_CFG, train_kernels=kernels, train_attention="device"):
        check_step(golden(), *setup(gpu))


# ---------------------------------------------------------------------------
# 8: memory
# ---------------------------------------------------------------------------
def test_device_attention_keeps_no_probability_tensor(hip, gpu):
    """torch autograd must keep at least one [V, heads, N, N] fp32 probability tensor of the layer for its backward; the device
    form keeps none: the peaks differ by at least that tensor"""
    V, N = 3, 1500
    vit = make_net(2).ViT
    del vit.blocks[1:]
    vit = vit.to(gpu).train()
    assert len(vit.blocks) == 1
    x = torch.from_numpy(synth.smooth_noise((V, N, DIM), 5, passes=0)).to(gpu)
    pe = (torch.rand(V, N, 3, generator=torch.Generator().manual_seed(5)) * 2 - 1).to(gpu)
    peak = {}
    for mode in ("device", "torch"):
        _vit_grads(vit, x, pe, 1.0, mode)                # (warm-up: library handles and workspaces of the first call)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        _vit_grads(vit, x, pe, 1.0, mode)
        torch.cuda.synchronize()
        peak[mode] = torch.cuda.max_memory_allocated()
    need = V * HEADS * N * N * 4
    print(f"peak allocated: torch {peak['torch'] / 2 ** 20:.1f} MiB, device {peak['device'] / 2 ** 20:.1f} MiB; "
          f"one probability tensor {need / 2 ** 20:.1f} MiB")
    assert peak["torch"] - peak["device"] >= need, (peak, need)
