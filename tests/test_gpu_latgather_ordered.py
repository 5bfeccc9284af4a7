"""K19's ordered backward on the device: th_latent_gather_bwd_ordered (k_latgather_ord.hip), LatentGatherFn(..., "ordered") and
the training entry with cfg.train_gather_bwd = "ordered".

The adjoint: tests/test_gpu_train_maps.py's check and bound, unchanged -- the exact adjoint of the coefficients read out of
the forward, sum_p coef[p,t] g[p,c] in float64, within (n + 18) 2^-24 sum |coef g| (any summation order of n fp32 terms plus
the product's rounding plus the merged coefficient's own), exactly 0 where nothing contributes.  Outputs and workspace are
filled with NaN bytes before every call: the kernels clear nothing and must not read what they have not written.
The lift: (rows + 2) 2^-24 sum |terms|, the bound of test_function_gradients_of_the_latents_and_the_lift.
Reproducibility: torch.equal between calls whose outputs and workspace held different garbage; the whole synthetic training step
twice, every output and every parameter gradient torch.equal."""
import numpy as np
import pytest
import torch

from transhuman_amd import config
from transhuman_amd.networks import autograd_path, train_ops
from test_gpu_train_maps import SHAPES, CH, EPS, _check_adjoint, _coefficients, _geometry, _grid_weights, _inputs, _points
from train_step_case import STEP_CFG, check_step, golden, setup

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip(gpu):
    from transhuman_amd import hip as H
    H.load_library()
    return H


def _garbage(n, gpu, kind):
    """n bytes of: 0 all-ones (every float a NaN, every index -1), 1 random bytes, 2 0x7f (large floats, large indices)"""
    if kind == 1:
        return torch.randint(0, 256, (n,), dtype=torch.uint8, device=gpu, generator=torch.Generator(gpu).manual_seed(n))
    return torch.full((n,), 0xFF if kind == 0 else 0x7F, dtype=torch.uint8, device=gpu)


def _shapes(dims, V):
    return [(V, h, w, C) for (h, w), C in zip(dims, CH)]


def _call(hip, gpu, H, W, dims, V, pts, cams, scale, g, rgb_s, kind=0):
    shapes = _shapes(dims, V)
    out = tuple(_garbage(4 * int(np.prod(s)), gpu, kind).view(torch.float32).reshape(s) for s in shapes)
    need = max(int(hip._lib.th_latent_gather_bwd_ordered_ws(V, H, W, pts.shape[0])), 256)
    ws = _garbage(need, gpu, kind)
    got = hip.latent_gather_bwd_ordered(shapes, (H, W), pts, cams, scale, g, rgb_s=rgb_s, out=out, workspace=ws)
    assert all(a is b for a, b in zip(got, out)) and len(got) == (5 if rgb_s is not None else 3)
    return got


def _check_lift(g_w, g_b, g64, rgb_s, what):
    gl, s = g64[..., 256:384].reshape(-1, 128), rgb_s.double().cpu().numpy().reshape(-1, 4)[:, :3]
    rows = gl.shape[0]
    for name, got, ref, mag in (("lift weight", g_w, gl.T @ s, np.abs(gl).T @ np.abs(s)),
                                ("lift bias", g_b, gl.sum(0), np.abs(gl).sum(0))):
        got = got.double().cpu().numpy()
        assert got.shape == ref.shape and np.isfinite(got).all()
        err, tol = np.abs(got - ref), (rows + 2) * EPS * mag
        print(f"{what} {name}: {rows} rows, worst error / bound = {float((err / np.maximum(tol, 1e-300)).max()):.4f}")
        assert (err <= tol).all()


def _ordered_case(hip, gpu, H, W, dims, V, pts, ldo, what):
    """-> (coefficients, the five gradients, the inputs of the call)"""
    (R, T, K), cams, scale = _geometry(hip, gpu, H, W, V)
    pts = pts.to(gpu)
    P = pts.shape[0]
    coef = _coefficients(hip, gpu, H, W, dims, V, pts, cams, scale)
    torch.manual_seed(5)
    g = torch.randn((P, V, ldo), device=gpu)
    rgb_s = torch.rand((P, V, 4), device=gpu)
    got = _call(hip, gpu, H, W, dims, V, pts, cams, scale, g, rgb_s)
    g64 = g.double().cpu().numpy()
    for l, (c0, C) in enumerate(zip((0, 64, 128), CH)):
        _check_adjoint(got[l].reshape(V, -1, C), coef[l], g64[..., c0:c0 + C], f"{what} level {l}")
    _check_lift(got[3], got[4], g64, rgb_s, what)
    # columns 256.. (the lift, the pad) do not reach the latents: the same bits with NaN there
    g2 = g.clone()
    g2[..., 256:] = float("nan")
    again = _call(hip, gpu, H, W, dims, V, pts, cams, scale, g2, None, kind=2)
    assert all(torch.equal(a, b) for a, b in zip(again, got[:3]))
    return coef, got, (pts, cams, scale, g, rgb_s)


# ---- 1: the adjoint -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ldo", [384, 400])
@pytest.mark.parametrize("P", [1, 17, 3000])
@pytest.mark.parametrize("V", [1, 3])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_ordered_backward_is_the_adjoint_of_the_forward(hip, gpu, shape, V, P, ldo):
    (H, W), dims = SHAPES[shape]
    (R, T, K), _, scale = _geometry(hip, gpu, H, W, V)
    _ordered_case(hip, gpu, H, W, dims, V, _points(P, 3 + P, R, T, K, scale), ldo, f"{shape} V={V} P={P} ldo={ldo}")


# ---- 2: where an ordered form can go wrong --------------------------------------------------------------------------------------
def _one_texel_points(P=3000):
    g = torch.Generator().manual_seed(11)
    return torch.tensor([[0.02, -0.03, 3.0]]) + (torch.rand((P, 3), generator=g) - 0.5) * 2e-4


def _one_texel_case(hip, gpu):
    (H, W), dims = SHAPES["20x28"]
    V, P = 3, 3000
    pts = _one_texel_points(P)
    (R, T, K), cams, scale = _geometry(hip, gpu, H, W, V)
    Wt = _grid_weights(hip, gpu, H, W, V, pts.to(gpu), cams, scale)
    for v in range(V):                                              # every sample inside ONE full-resolution texel cell per view
        assert int((Wt[:, v] != 0).any(0).sum()) <= 4 and int((Wt[:, v] != 0).all(0).sum()) >= 1
    return H, W, dims, V, pts


def test_many_samples_inside_one_texel(hip, gpu):
    """one list of 3000 pairs per view: more than two batches of the sum kernel plus one, the 9000 pairs more than two sort
    tiles plus one and more than two lift partials plus one"""
    sz = hip.LATENT_GATHER_ORDERED_SIZES
    H, W, dims, V, pts = _one_texel_case(hip, gpu)
    P = pts.shape[0]
    assert P >= 2 * sz["batch"] + 1 and P * V >= 2 * sz["sort_tile"] + 1 and P * V >= 2 * sz["lift_rows"] + 1
    coef, _, _ = _ordered_case(hip, gpu, H, W, dims, V, pts, 384, "one texel")
    for c in coef:
        assert int((c[:, 0] != 0).all(0).sum()) >= 1               # a latent texel that takes all 3000 samples


def test_exact_duplicate_points(hip, gpu):
    """equal keys throughout: the order inside a list is the sample index alone"""
    (H, W), dims = SHAPES["33x17"]
    V = 3
    (R, T, K), _, scale = _geometry(hip, gpu, H, W, V)
    pts = _points(40, 43, R, T, K, scale).repeat(50, 1)              # sample p and p + 40 k are the same point
    _ordered_case(hip, gpu, H, W, dims, V, pts, 384, "duplicates")
    _ordered_case(hip, gpu, H, W, dims, 1, pts[:1].repeat(700, 1), 400, "one point 700 times")


def test_every_point_outside_the_image(hip, gpu):
    """the border clamp piles every pair onto the map's edge pixels, hence onto the latents' edge texels"""
    (H, W), dims = SHAPES["20x28"]
    V = 3
    (R, T, K), _, scale = _geometry(hip, gpu, H, W, V)
    g = torch.Generator().manual_seed(17)
    cand = torch.randn((20000, 3), generator=g) * 6.0 + torch.tensor([0.0, 0.0, 3.0])
    grid = autograd_path.project(cand, R, T, K) * scale.cpu() - 1.0             # [V,N,2]
    outside = (grid.abs() > 1).any(-1).all(0) & torch.isfinite(grid).all(-1).all(0)
    pts = cand[outside][:1500]
    assert pts.shape[0] == 1500
    _, cams, scale = _geometry(hip, gpu, H, W, V)
    Wt = _grid_weights(hip, gpu, H, W, V, pts.to(gpu), cams, scale).reshape(-1, V, H, W)
    assert (Wt[:, :, 1:-1, 1:-1] == 0).all()                        # every bilinear weight sits on the map's border
    coef, _, _ = _ordered_case(hip, gpu, H, W, dims, V, pts, 384, "all outside")
    assert max(int((c != 0).sum(0).max()) for c in coef) >= 100     # and some latent texel collects a long list


def test_a_one_by_one_level(hip, gpu):
    (H, W), dims, V, P = (12, 16), ((6, 8), (3, 4), (1, 1)), 2, 333
    (R, T, K), _, scale = _geometry(hip, gpu, H, W, V)
    coef, got, (_, _, _, g, _) = _ordered_case(hip, gpu, H, W, dims, V, _points(P, 5, R, T, K, scale), 384, "1 x 1 level")
    assert int((coef[2] != 0).sum(-1).max()) == 1                   # the level's only texel takes every tap of every sample
    assert got[2].shape == (V, 1, 1, 128)


def test_without_samples_writes_zeros(hip, gpu):
    (H, W), dims = SHAPES["33x17"]
    V = 2
    _, cams, scale = _geometry(hip, gpu, H, W, V)
    got = _call(hip, gpu, H, W, dims, V, torch.zeros((0, 3), device=gpu), cams, scale, torch.zeros((0, V, 384), device=gpu),
                torch.zeros((0, V, 4), device=gpu))
    assert all((o == 0).all() for o in got) and got[3].shape == (128, 3) and got[4].shape == (128,)


def _edges():
    from transhuman_amd import hip as H
    sizes = sorted(set(H.LATENT_GATHER_ORDERED_SIZES.values()))
    return [(1, n + d) for n in sizes for d in (-1, 0, 1)] + [(3, P) for n in sizes for P in ((n - 1) // 3, (n + 3) // 3)]


@pytest.mark.parametrize("V,P", _edges(), ids=lambda x: str(x))
def test_pair_counts_around_the_batch_round_tile_and_chunk_sizes(hip, gpu, V, P):
    """P V one below, at and one above the sum kernel's batch (64), the sort's round (256) and tile (2048) and the lift's chunk
    (256) with V = 1; with V = 3 the nearest counts below and above"""
    (H, W), dims = SHAPES["33x17"]
    (R, T, K), _, scale = _geometry(hip, gpu, H, W, V)
    _ordered_case(hip, gpu, H, W, dims, V, _points(P, 100 + P, R, T, K, scale), 384, f"V={V} P={P}")


def test_a_list_around_the_batch_size(hip, gpu):
    """ONE list of n pairs, n around one, two and four batches of the sum kernel: the batch boundary inside a list, and the
    batches dealt to the one, two and four waves that share a texel of the first, second and third level at this shape"""
    (H, W), dims = SHAPES["20x28"]
    for n in (63, 64, 65, 127, 128, 129, 255, 256, 257):
        _ordered_case(hip, gpu, H, W, dims, 1, _one_texel_points(n), 384, f"list of {n}")


# ---- 3: reproducibility ----------------------------------------------------------------------------------------------------------
def test_three_runs_over_different_garbage_are_bit_identical(hip, gpu):
    H, W, dims, V, pts = _one_texel_case(hip, gpu)
    (H2, W2), dims2 = SHAPES["20x28"]
    (R, T, K), _, scale = _geometry(hip, gpu, H2, W2, 3)
    cases = {"one texel": (H, W, dims, V, pts), "P=3000 V=3": (H2, W2, dims2, 3, _points(3000, 3003, R, T, K, scale))}
    for what, (H, W, dims, V, pts) in cases.items():
        _, cams, scale = _geometry(hip, gpu, H, W, V)
        pts = pts.to(gpu)
        torch.manual_seed(5)
        g, rgb_s = torch.randn((pts.shape[0], V, 384), device=gpu), torch.rand((pts.shape[0], V, 4), device=gpu)
        runs = [[t.clone() for t in _call(hip, gpu, H, W, dims, V, pts, cams, scale, g, rgb_s, kind=k)] for k in (0, 1, 2)]
        for r in runs[1:]:
            assert len(r) == 5 and all(torch.equal(a, b) for a, b in zip(r, runs[0])), what
        if what == "one texel":
            shapes = _shapes(dims, V)
            atomic = [[t.clone() for t in hip.latent_gather_bwd(shapes, (H, W), pts, cams, scale, g)] for _ in range(3)]
            same = all(torch.equal(a, b) for r in atomic[1:] for a, b in zip(r, atomic[0]))
            print(f"{what}: the atomic form repeated itself over three runs: {same}")


# ---- 4: the Function -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,V", [(17, 1), (3000, 3)])
def test_function_in_the_ordered_mode(hip, gpu, P, V):
    (H, W), dims = SHAPES["20x28"]
    (R, T, K), cams, scale = _geometry(hip, gpu, H, W, V)
    pts = _points(P, 21, R, T, K, scale).to(gpu)
    lat, img, lift_w, lift_b = _inputs(gpu, H, W, dims, V, seed=9)
    torch.manual_seed(6)
    g = torch.randn((P, V, 384), device=gpu)
    grads = []
    for _ in range(2):
        leaves = [t.clone().requires_grad_(True) for t in (*lat, lift_w.reshape(128, 3, 1, 1), lift_b)]
        rows = train_ops.LatentGatherFn.apply(*leaves, img, pts, cams, scale, "ordered")
        rows.backward(g)
        grads.append([t.grad for t in leaves])
    nine = train_ops.LatentGatherFn.apply(*lat, lift_w.reshape(128, 3, 1, 1), lift_b, img, pts, cams, scale)
    assert torch.equal(rows, nine)
    assert all(torch.equal(a, b) for a, b in zip(*grads))                       # two backward passes: the same bits
    got = grads[0]
    assert got[3].shape == (128, 3, 1, 1) and got[4].shape == (128,)
    coef = _coefficients(hip, gpu, H, W, dims, V, pts, cams, scale)
    g64 = g.double().cpu().numpy()
    for l, (c0, C) in enumerate(zip((0, 64, 128), CH)):
        _check_adjoint(got[l].reshape(V, -1, C), coef[l], g64[..., c0:c0 + C], f"Function level {l}")
    _, rgb_s = hip.latent_gather(*lat, lift_w, lift_b, img, pts, cams, scale)
    _check_lift(got[3].reshape(128, 3), got[4], g64, rgb_s, "Function")


# ---- 5: the golden training step -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernels", ["torch", "device"])
def test_training_step_with_the_ordered_gather_matches_the_reference(hip, gpu, kernels):
    """tests/test_gpu_train_maps.py::test_training_step_on_the_latents_matches_the_reference with cfg.train_gather_bwd =
    "ordered": the same golden step of the real reference, the same bars"""
    with config.override(**STEP_CFG, train_maps="latents", train_kernels=kernels, train_gather_bwd="ordered"):
        check_step(golden(), *setup(gpu))


# ---- 6: the whole step, twice ----------------------------------------------------------------------------------------------------
def test_the_whole_step_twice_gives_the_same_bits(hip, gpu):
    """the synthetic step of tests/test_gpu_train_encoder.py, rebuilt from its seeds for each run, every training switch on its
    device value and the ordered gather backward, MIOpen on its deterministic kernels: the three outputs and every parameter
    gradient are torch.equal between two runs"""
    from test_gpu_train_encoder import ALL_DEVICE, _reproducible_torch
    runs = []
    for _ in range(2):
        with config.override(**STEP_CFG, **ALL_DEVICE, train_encoder="device", train_gather_bwd="ordered"):
            net, r, b = setup(gpu)
            with _reproducible_torch():
                ret = autograd_path.render(r, b)
                (ret["rgb_map"].mean() + 0.1 * ret["acc_map"].mean() + 0.01 * ret["depth_map"].mean()).backward()
            out = {k: ret[k].detach().clone() for k in ("rgb_map", "acc_map", "depth_map")}
            out.update({"grad:" + k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None})
            runs.append(out)
    a, b2 = runs
    assert set(a) == set(b2)
    trunk = [k for k in a if k.startswith(("grad:encoder.model.conv1.", "grad:encoder.model.bn1.", "grad:encoder.model.layer1.",
                                           "grad:encoder.model.layer2."))]
    assert len(trunk) == 30
    differ = [k for k in a if not torch.equal(a[k], b2[k])]
    print(f"{len(a)} tensors compared ({len(trunk)} trunk gradients); differing: {differ}")
    assert not differ, differ
