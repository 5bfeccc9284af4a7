"""GPU: th_rank_sum (K28, csrc/k_optim.hip) -- the sum of the rank-ordered exchange's reduce-scatter -- against the numpy sum in rank
order, bit for bit: the 32-bit patterns of every element that is not a NaN in the numpy result (signed zeros, subnormals and
infinities included), a NaN exactly where numpy has one, and at world = 1, where the kernel copies, NaN payloads as well
(as tests/test_gpu_train_dist.py compares).

Every case plants triples whose sum depends on the order: (1e8, -1e8, 1) on ranks (0, 1, 2) gives 1 in rank order and 0 when rank 0
comes last; (1, 1e8, -1e8) gives 0 in rank order and 1 otherwise.  A kernel that added in any other order fails on one of them."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = 1234.5
WORLDS = (1, 2, 3, 5, 8)
SLICES = (4, 8, 252, 256, 260, 4100, 1, 7, 4101)     # (the last three: no whole float4 groups, the 32-bit path)
SPECIAL = np.array([np.inf, -np.inf, np.nan, 0.0, -0.0, 1e-40, -1e-39, 1.4e-45, -1.4e-45, 3.4e38, -3.4e38, 1.1754944e-38,
                    -1.1754942e-38, 1.0, 3.0, -7.0], np.float32)


@pytest.fixture(scope="module")
def hip(gpu):
    from transhuman_amd import hip as H
    H.load_library()
    return H


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(got, want, what, nan_payload=False):
    ok = np.ones(want.shape, bool) if nan_payload else ~np.isnan(want)
    bad = np.nonzero(bits(got)[ok] != bits(want)[ok])[0]
    assert bad.size == 0, (what, int(bad.size), got[ok][bad[:4]], want[ok][bad[:4]])
    assert np.isnan(got[~ok]).all(), what


def make_parts(world, n, seed=0):
    rs = np.random.RandomState(100 * world + n + seed)
    parts = (rs.standard_normal((world, n)) * np.exp(rs.uniform(-20, 20, (world, n)))).astype(np.float32)
    for r in range(world):                                            # specials meet ordinary values and each other
        k = min(n, len(SPECIAL))
        parts[r, rs.choice(n, k, replace=False)] = SPECIAL[rs.permutation(len(SPECIAL))[:k]]
    if world >= 3 and n >= 2:                                         # the order decides (module docstring)
        a, b = rs.choice(n, 2, replace=False)
        parts[:, a], parts[:, b] = 0.0, 0.0
        parts[:3, a] = (1e8, -1e8, 1.0)
        parts[:3, b] = (1.0, 1e8, -1e8)
    return parts


def rank_order_sum(parts):
    with np.errstate(all="ignore"):
        acc = parts[0].copy()
        for r in range(1, parts.shape[0]):
            acc = acc + parts[r]
    assert acc.dtype == np.float32
    return acc


def test_the_planted_triples_tell_the_orders_apart():
    parts = make_parts(3, 8)
    want = rank_order_sum(parts)
    others = [(parts[o[0]] + parts[o[1]]) + parts[o[2]] for o in ((0, 2, 1), (1, 2, 0))]
    with np.errstate(all="ignore"):
        assert all((bits(o) != bits(want))[~np.isnan(want)].any() for o in others)


def device_buffers(gpu, parts, out_shift=0, parts_shift=0):
    """parts and out inside sentinel-filled buffers; a shift of 1 moves a tensor 4 bytes off the 16-byte grid"""
    world, n = parts.shape
    pbig = torch.full((world * n + 12,), SENTINEL, dtype=torch.float32, device=gpu)
    obig = torch.full((n + 12,), SENTINEL, dtype=torch.float32, device=gpu)
    assert pbig.data_ptr() % 16 == 0 and obig.data_ptr() % 16 == 0
    p = pbig[4 + parts_shift:4 + parts_shift + world * n]
    o = obig[4 + out_shift:4 + out_shift + n]
    p.copy_(torch.from_numpy(parts.reshape(-1)))
    o.view(torch.int32).fill_(-1)                                      # NaN bytes underneath
    return pbig, p, obig, o


def guards(big, lo, n):
    h = big.cpu().numpy()
    return bool((h[:lo] == SENTINEL).all() and (h[lo + n:] == SENTINEL).all())


@pytest.mark.parametrize("n", SLICES)
@pytest.mark.parametrize("world", WORLDS)
def test_rank_sum_equals_numpy(hip, gpu, world, n):
    parts = make_parts(world, n)
    want = rank_order_sum(parts)
    for out_shift, parts_shift in ((0, 0), (1, 0), (0, 1), (1, 1)):    # the 128-bit path (when n % 4 == 0), then three 32-bit ones
        pbig, p, obig, o = device_buffers(gpu, parts, out_shift, parts_shift)
        assert (o.data_ptr() % 16 != 0) == bool(out_shift) and (p.data_ptr() % 16 != 0) == bool(parts_shift)
        assert hip.rank_sum(p, world, n, o) is o
        torch.cuda.synchronize()
        what = (world, n, out_shift, parts_shift)
        same_bits(o.cpu().numpy(), want, what, nan_payload=world == 1)
        assert guards(obig, 4 + out_shift, n), what                   # nothing outside out[0 : slice_elems)
        same_bits(p.cpu().numpy(), parts.reshape(-1), what, nan_payload=True)     # the parts are read, nothing else
        assert guards(pbig, 4 + parts_shift, world * n), what
        first = o.view(torch.int32).cpu().numpy().copy()
        o.view(torch.int32).fill_(-1)
        hip.rank_sum(p, world, n, o)
        assert np.array_equal(first, o.view(torch.int32).cpu().numpy()), what    # two calls write identical bytes


@pytest.mark.parametrize("n", (4, 260, 4100, 7))
@pytest.mark.parametrize("world", WORLDS)
def test_out_may_be_any_of_the_parts(hip, gpu, world, n):
    parts = make_parts(world, n, seed=1)
    want = rank_order_sum(parts)
    for r in range(world):
        for shift in (0, 1):
            pbig, p, _, _ = device_buffers(gpu, parts, 0, shift)
            hip.rank_sum(p, world, n, p[r * n:(r + 1) * n])
            torch.cuda.synchronize()
            got = p.cpu().numpy().reshape(world, n)
            same_bits(got[r], want, (world, n, r, shift), nan_payload=world == 1)
            keep = [k for k in range(world) if k != r]
            same_bits(got[keep].reshape(-1), parts[keep].reshape(-1), (world, n, r, shift), nan_payload=True)
            assert guards(pbig, 4 + shift, world * n)


def test_refusals(hip, gpu):
    lib, c, p, st = hip.load_library(), hip.ctx(gpu), hip._p, hip._stream()
    parts = torch.zeros(64 * 8, device=gpu)
    out = torch.full((8,), SENTINEL, device=gpu)
    calls = {
        "world 0": lambda: lib.th_rank_sum(c, p(parts), 0, 8, p(out), st),
        "world -1": lambda: lib.th_rank_sum(c, p(parts), -1, 8, p(out), st),
        "world 65": lambda: lib.th_rank_sum(c, p(parts), 65, 4, p(out), st),
        "no elements": lambda: lib.th_rank_sum(c, p(parts), 2, 0, p(out), st),
        "negative elements": lambda: lib.th_rank_sum(c, p(parts), 2, -4, p(out), st),
        "null parts": lambda: lib.th_rank_sum(c, None, 2, 8, p(out), st),
        "null out": lambda: lib.th_rank_sum(c, p(parts), 2, 8, None, st),
        "null context": lambda: lib.th_rank_sum(None, p(parts), 2, 8, p(out), st),
    }
    for what, call in calls.items():
        assert call() != 0, what
        assert b"th_rank_sum" in lib.th_last_error(), (what, lib.th_last_error())
    assert lib.th_rank_sum(c, p(parts), 64, 8, p(out), st) == 0 and not bool(out.any())    # 64 ranks are served
    out.fill_(SENTINEL)
    for bad in (lambda: hip.rank_sum(parts.cpu(), 2, 8, out), lambda: hip.rank_sum(parts, 2, 8, out.cpu()),
                lambda: hip.rank_sum(parts[:15], 2, 8, out), lambda: hip.rank_sum(parts, 2, 8, out[:7]),
                lambda: hip.rank_sum(parts.double(), 2, 8, out), lambda: hip.rank_sum(parts.view(64, 8)[:, :4], 2, 8, out)):
        with pytest.raises(hip.HipError):
            bad()
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())                              # a refused call wrote nothing
