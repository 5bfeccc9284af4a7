"""K3 (TransHE) at the edges of its tiles: the two attention kernels, kv_split_kernel, the dense layers on both sides of the
8192-token switch and the whole forward against float64 restatements on the CPU (oracle/th_oracle.py).

Attention bar (B1, B2), measured per case and never assumed: with t64 the oracle in float64 and o32 the same oracle in float32,

    |gpu - t64|.max()  <=  4 * |o32 - t64|.max() + 1e-6 * max|v|

4 separates the scheme's operand precision (x = hi + lo to 2^-22) from fp32's 2^-24; the floor covers cases where fp32 happens to
be exact.  Every case keeps max |logit| <= 250 (above that the softmax is one-hot and the fp32 error collapses), checks that o32 is
finite and that the case is not degenerate (max|t64| > 0.05 max|v|), and prints its ratio |gpu - t64| / |o32 - t64|
("K3 parity", records the worst ones).  Whole forwards are held to the project's bar for ViT outputs, 1e-4."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import th_oracle as O
from transhuman_amd import synth
from util import make_sd, make_net, maxdiff

pytestmark = pytest.mark.gpu

HEADS, HD = 3, 64
DIM = HEADS * HD


@pytest.fixture(scope="module")
def hip(gpu):
    from transhuman_amd import hip as H
    H.load_library()
    return H


@pytest.fixture(scope="module")
def net(gpu, hip):
    return make_net(12).to(gpu)


@pytest.fixture(scope="module")
def net2(gpu, hip):
    return make_net(2).to(gpu)


# ---------------------------------------------------------------------------
# inputs and references of the attention cases (built once per case, shared by the forms)
# ---------------------------------------------------------------------------
def _pack(q, k, v):
    """q, k, v [V, heads, N, 64] -> qkv [V, N, 3 dim] in the layout the qkv layer writes (column = which dim + head 64 + d)"""
    V, H, N, _ = q.shape
    return torch.stack([q, k, v], 0).permute(1, 3, 0, 2, 4).reshape(V, N, 3 * H * HD).contiguous().float()


def _planes(fn, V, N, seed):
    """fn(rs, N) -> (q, k, v) float arrays [N, 64]; every (view, head) plane draws from a seed of its own, so a slip in the plane
    indexing of the kernels cannot go unnoticed"""
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
    "falling": _along_u(lambda N, rs: np.arange(N)[::-1] / 4.0),          # the first key wins: corr == 1 from the second tile on
    # every real logit <= -40: a padding key scoring 0 would take all the mass (spread over 60, so that a handful of keys carry
    # the row and the output is not an average of hundreds of v)
    "negative": _along_u(lambda N, rs: -44.0 - 60.0 * rs.uniform(size=N)),
    "dominant_last": _along_u(_dominant(-1)),
    "dominant_63": _along_u(_dominant(63)),
    "dominant_64": _along_u(_dominant(64)),
    "v_small": _scaled(1.0, 1.0, 2.0 ** -10),
    "v_large": _scaled(1.0, 1.0, 2.0 ** 10),
    "q_small_k_large": _scaled(2.0 ** -4, 2.0 ** 4, 1.0),
}


@functools.lru_cache(maxsize=None)
def _case(name, V, N):
    """qkv (fp32, CPU), t64, the fp32 oracle's error, max|v|, max|logit|, max logit"""
    qkv = _planes(_gauss if name == "gauss" else STRESS[name], V, N, seed=1000 + N)
    q64 = qkv.double()
    t64 = O.attention(q64, HEADS)
    o32 = O.attention(qkv, HEADS)
    assert t64.dtype == torch.float64 and o32.dtype == torch.float32
    assert torch.isfinite(o32).all()
    r = q64.reshape(V, N, 3, HEADS, HD).permute(2, 0, 3, 1, 4)
    logit = (r[0] @ r[1].transpose(-2, -1)) * 0.125
    vmax = float(r[2].abs().max())
    assert float(logit.abs().max()) <= 250.0
    assert float(t64.abs().max()) > 0.05 * vmax, "degenerate case"
    return qkv, t64, maxdiff(o32, t64), vmax, float(logit.max())


def _hold(hip, gpu, name, V, N, form):
    qkv, t64, e32, vmax, _ = _case(name, V, N)
    out = hip.attention(qkv.to(gpu), HEADS, form)
    again = hip.attention(qkv.to(gpu), HEADS, form)
    assert torch.equal(out, again), "not bit-identical on two runs"
    out = out.cpu()
    assert torch.isfinite(out).all()
    err = maxdiff(out, t64)
    bar = 4.0 * e32 + 1e-6 * vmax
    print(f"K3 parity {name} V={V} N={N} form={form}: gpu {err:.3e} fp32 {e32:.3e} ratio {err / e32 if e32 > 0 else float('inf'):.2f} "
          f"bar {bar:.3e}")
    assert err <= bar, (name, V, N, form, err, e32, bar)
    return out


# ---------------------------------------------------------------------------
# B1: both kernels against float64 at the tile edges
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", (2, 3))
@pytest.mark.parametrize("V", (1, 3))
@pytest.mark.parametrize("N", (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 700, 701))
def test_attention_vs_float64_at_tile_edges(hip, gpu, N, V, form):
    """one partial query block, 16 k +- 1, 64 k (no padding keys), 64 k + 1 (a last tile with one live key), both sides of the
    700 / 701 switch; Gaussian q, k, v of sigma 3 (the magnitude of the product's own qkv rows)"""
    out = _hold(hip, gpu, "gauss", V, N, form)
    if N in (700, 701):
        # form 0 is the forward's own rule: attn2_kernel up to 700, attn3_kernel above
        if form == (2 if N == 700 else 3):
            own = hip.attention(_case("gauss", V, N)[0].to(gpu), HEADS, 0).cpu()
            assert torch.equal(own, out)


# ---------------------------------------------------------------------------
# B2: the online softmax where it carries weight
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", (2, 3))
@pytest.mark.parametrize("N", (65, 705))
@pytest.mark.parametrize("name", sorted(STRESS))
def test_attention_softmax_stress(hip, gpu, name, N, form):
    V = 2
    out = _hold(hip, gpu, name, V, N, form)
    if name == "negative":
        qkv, _, _, vmax, top = _case(name, V, N)
        assert top <= -40.0, top
        v = qkv.reshape(V, N, 3, HEADS, HD)[:, :, 2]                     # [V, N, heads, 64]
        lo, hi = v.min(1, keepdim=True).values, v.max(1, keepdim=True).values
        o = out.reshape(V, N, HEADS, HD)
        # a convex combination of the real keys' v, up to the rounding of its evaluation (the bar's floor)
        eps = 1e-6 * vmax
        assert bool((o >= lo - eps).all()) and bool((o <= hi + eps).all())


# ---------------------------------------------------------------------------
# B3 / B4: the whole forward
# ---------------------------------------------------------------------------
def _vit_inputs(V, N):
    x = torch.from_numpy(synth.smooth_noise((V, N, DIM), 31 + N, passes=0))
    pe = torch.rand(V, N, 3, generator=torch.Generator().manual_seed(N)) * 2 - 1
    return x, pe


@functools.lru_cache(maxsize=None)
def _sd64(depth):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in make_sd(depth).items()}


@functools.lru_cache(maxsize=None)
def _vit_ref(V, N, depth):
    x, pe = _vit_inputs(V, N)
    with torch.no_grad():
        ref = O.vit_forward(x.double(), pe, _sd64(depth), depth)
    assert ref.dtype == torch.float64
    return ref


def _forward_in_mode(hip, gpu, vit, x, pe, mode):
    lib = hip.load_library()
    hip._sync_weights(vit, "vit")                       # (a weight upload never changes the mode; done first all the same)
    try:
        hip._check(lib.th_set_vit_mode(hip.ctx(gpu), mode))
        return vit(x.to(gpu), pe.to(gpu), mask=None).cpu()
    finally:
        hip._check(lib.th_set_vit_mode(hip.ctx(gpu), 1))


@pytest.mark.parametrize("mode", (1, 0))
@pytest.mark.parametrize("V,N", ((1, 1), (2, 17), (5, 65), (1, 64), (2, 700), (2, 705), (3, 1500)))
def test_vit_forward_vs_float64_at_the_edges(hip, gpu, net, V, N, mode):
    x, pe = _vit_inputs(V, N)
    out = _forward_in_mode(hip, gpu, net.ViT, x, pe, mode)
    assert torch.isfinite(out).all()
    err = maxdiff(out, _vit_ref(V, N, 12))
    print(f"K3 forward V={V} N={N} mode={mode}: {err:.3e}")
    assert err < 1e-4, (V, N, mode, err)


@pytest.mark.parametrize("V,N,depth", ((16, 513, 12), (4, 2049, 2)))
def test_vit_forward_above_8192_tokens(hip, gpu, net, net2, V, N, depth):
    """T = V N > 8192: layernorm_kernel, the large-M form of the fp32 MFMA GEMM and kv_split_kernel, in both modes"""
    assert V * N > 8192
    vit = (net if depth == 12 else net2).ViT
    x, pe = _vit_inputs(V, N)
    outs = [_forward_in_mode(hip, gpu, vit, x, pe, mode) for mode in (1, 0)]
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1]), "both modes land on the same kernels above 8192 tokens"
    err = maxdiff(outs[0], _vit_ref(V, N, depth))
    print(f"K3 forward V={V} N={N} depth={depth}: {err:.3e}")
    assert err < 1e-4, (V, N, depth, err)


# ---------------------------------------------------------------------------
# B5: the result does not depend on what the workspace held
# ---------------------------------------------------------------------------
def _filled(nbytes, byte, gpu):
    return torch.full((max(int(nbytes), 256),), byte, dtype=torch.uint8, device=gpu)


@pytest.mark.parametrize("mode", (1, 0))
@pytest.mark.parametrize("V,N", ((3, 300), (1, 64), (2, 705)))
def test_vit_forward_ignores_workspace_contents(hip, gpu, net, V, N, mode):
    lib = hip.load_library()
    x, pe = _vit_inputs(V, N)
    vit = net.ViT
    hip._sync_weights(vit, "vit")
    xd, tab = x.to(gpu), vit.get_PE(pe.to(gpu))
    assert tab.dtype == torch.float32 and tab.is_contiguous() and tuple(tab.shape) == (V, N, DIM)
    nbytes = lib.th_vit_workspace_bytes(V, N, DIM, HEADS)
    outs = []
    try:
        hip._check(lib.th_set_vit_mode(hip.ctx(gpu), mode))
        for byte in (0x00, 0xFF):                        # 0xFF..: NaN as fp32 and as fp16
            ws = _filled(nbytes, byte, gpu)
            out = torch.full((V, N, DIM), float("nan"), device=gpu)
            hip._check(lib.th_vit_forward(hip.ctx(gpu), hip._p(xd), hip._p(tab), V, N, hip._p(out), hip._p(ws), ws.numel(),
                                          hip._stream()))
            outs.append(out.cpu())
    finally:
        hip._check(lib.th_set_vit_mode(hip.ctx(gpu), 1))
    assert torch.isfinite(outs[0]).all() and torch.isfinite(outs[1]).all()
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("form", (2, 3))
@pytest.mark.parametrize("V,N", ((3, 300), (1, 64), (2, 705)))
def test_attention_ignores_workspace_contents(hip, gpu, V, N, form):
    lib = hip.load_library()
    qkv = _planes(_gauss, V, N, seed=7 + N).to(gpu)
    nbytes = lib.th_attention_workspace_bytes(V, N, HEADS)
    outs = []
    for byte in (0x00, 0xFF):
        ws = _filled(nbytes, byte, gpu)
        out = torch.full((V, N, DIM), float("nan"), device=gpu)
        hip._check(lib.th_attention(hip.ctx(gpu), hip._p(qkv), V, N, HEADS, form, hip._p(out), hip._p(ws), ws.numel(),
                                    hip._stream()))
        outs.append(out.cpu())
    assert torch.isfinite(outs[0]).all() and torch.isfinite(outs[1]).all()
    assert torch.equal(outs[0], outs[1])


# ---------------------------------------------------------------------------
# B6: refusals
# ---------------------------------------------------------------------------
def test_attention_refusals(hip, gpu):
    """an argument error comes back as a code and a message; nothing is launched: `out` keeps its contents"""
    lib = hip.load_library()
    V, N = 2, 65
    qkv = _planes(_gauss, V, N, seed=3).to(gpu)
    nbytes = int(lib.th_attention_workspace_bytes(V, N, HEADS))
    assert nbytes >= 2 * V * HEADS * 2 * 128 * 64 * 2
    ws = _filled(nbytes, 0, gpu)
    out = torch.full((V, N, DIM), 7.0, device=gpu)
    h, s = hip.ctx(gpu), hip._stream()
    null = C.c_void_p(0)

    def refused(rc, word):
        assert rc != 0
        msg = lib.th_last_error()
        assert msg and word in msg, msg

    refused(lib.th_attention(h, hip._p(qkv), V, N, HEADS, 2, hip._p(out), hip._p(ws), nbytes - 1, s), b"workspace")
    refused(lib.th_attention(h, hip._p(qkv), V, N, HEADS, 1, hip._p(out), hip._p(ws), nbytes, s), b"form")
    refused(lib.th_attention(h, hip._p(qkv), V, N, 0, 2, hip._p(out), hip._p(ws), nbytes, s), b"heads")
    refused(lib.th_attention(h, hip._p(qkv), V, 0, HEADS, 2, hip._p(out), hip._p(ws), nbytes, s), b"N")
    refused(lib.th_attention(null, hip._p(qkv), V, N, HEADS, 2, hip._p(out), hip._p(ws), nbytes, s), b"null")
    refused(lib.th_attention(h, null, V, N, HEADS, 2, hip._p(out), hip._p(ws), nbytes, s), b"null")
    refused(lib.th_attention(h, hip._p(qkv), V, N, HEADS, 2, null, hip._p(ws), nbytes, s), b"null")
    refused(lib.th_attention(h, hip._p(qkv), V, N, HEADS, 2, hip._p(out), null, nbytes, s), b"null")
    assert lib.th_attention_workspace_bytes(V, 0, HEADS) == 0 and lib.th_attention_workspace_bytes(V, N, 0) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    # ... and the same call with nothing wrong goes through
    hip._check(lib.th_attention(h, hip._p(qkv), V, N, HEADS, 2, hip._p(out), hip._p(ws), nbytes, s))
    assert torch.isfinite(out).all() and not bool((out == 7.0).all())
