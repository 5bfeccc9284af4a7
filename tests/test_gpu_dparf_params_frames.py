"""cfg.KNN / cfg.KNN_FREQ / cfg.KNN_DIST_ALPHA on the paths of the product: the hand-over forms of K4 against each other, the
recordings of the real reference (tests/golden/g28_dparf_params*.npz, tools/gen_golden_dparf_params.py; triples A..E of
dparf_params_case.TRIPLES), the life of the parameters in a context, and cfg.use_truncation beside them.

K4 on its own under the same parameters: tests/test_gpu_dparf_params.py (its docstring derives the row bounds used here)."""
import functools

import numpy as np
import pytest
import torch

import dparf_cases as D
import dparf_params_case as C
import train_step_case as step
from oracle import th_oracle as O
from transhuman_amd import config, synth
from transhuman_amd.truncation import truncation_mask_oracle
from util import GOLD, can64, can_centres64, csr, gold, make_net, maxdiff, synth_assign

pytestmark = pytest.mark.gpu
DEFAULT = (7, 10, 0.5)


@pytest.fixture(scope="module")
def hip(gpu):
    from transhuman_amd import hip as H
    H.load_library()
    return H


@pytest.fixture(autouse=True)
def defaults_afterwards(hip, gpu):
    """every test leaves the context at (7, 10, 0.5): the other files' direct hip.* calls assume a new context's values"""
    yield
    hip.set_dparf(*DEFAULT, gpu)


@pytest.fixture(scope="module")
def nets(gpu):
    """the networks of the triples, built once on the device"""
    made = {}

    def get(t):
        if t not in made:
            made[t] = (make_net(12) if t == "default" else C.make_net(t)).to(gpu)
        return made[t]
    yield get
    made.clear()


def _renderer(net, mesh=False):
    from transhuman_amd.networks.renderer import if_clight_renderer, if_mesh_renderer
    return (if_mesh_renderer if mesh else if_clight_renderer).Renderer(net, vertex_can=can64().numpy(), pc2voxel_ind=synth_assign(300))


# ---- 7: the forms agree ----------------------------------------------------------------------------------------------------------
def _case_frame(hip, gpu, name):
    """a hip.Frame around a case of dparf_cases (as tests/test_gpu_dparf_knn.py builds it): the points are the hull's vertices,
    seeded tokens, short rays of two samples through every point"""
    c = D.case(name)
    b = synth.make_batch(32, 32, 3, seed=0)
    Rh, Th = b["Rh"][0].numpy().astype(np.float64), b["Th"][0].numpy().astype(np.float64)
    world = torch.from_numpy((c.pts.astype(np.float64) @ np.linalg.inv(Rh) + Th).astype(np.float32)).to(gpu)
    nc = c.cen.shape[0]
    cams = hip.pack_cams(b["input_R"][0][0].to(gpu), b["input_T"][0][0].to(gpu), b["input_K"][0][0].to(gpu))
    scale = hip.feat_scale(np.array([32, 32]) / (np.array([32, 32]) - 1) * 2.0, (32, 32), gpu)
    pix = torch.from_numpy(synth.smooth_noise((3, 384, 32, 32), 24)).to(gpu)
    tok = torch.from_numpy(np.random.RandomState(6).normal(size=(3, nc, 192)).astype(np.float32)).to(gpu)
    frame = hip.Frame(world, torch.from_numpy(Rh.astype(np.float32)).to(gpu), torch.from_numpy(Th.astype(np.float32)).to(gpu),
                      cams, scale, hip.nchw_to_nhwc(pix), tok, torch.from_numpy(c.cen).to(gpu), torch.from_numpy(c.rot).to(gpu))
    P = world.shape[0]
    d = torch.from_numpy(np.random.RandomState(8).normal(size=(P, 3)).astype(np.float32))
    d = (d / d.norm(dim=1, keepdim=True)).to(gpu)
    near, far = torch.full((P,), -0.01, device=gpu), torch.full((P,), 0.01, device=gpu)
    return frame, world, d, near, far


@pytest.mark.parametrize("name", ["tight", "islands"])
@pytest.mark.parametrize("t", ["B", "D"])
def test_the_forms_of_the_frame_paths_agree(hip, gpu, nets, monkeypatch, t, name):
    """neighbour records (the default), K4's own fp32 blend of T' rows (th_set_tok_gather 0: the generic folded rows) and the
    per-layer path against the zero-padded fp32 rows: 2e-6 between the two hand-overs (tests/test_gpu_parity.py, ray sharding) and
    5e-5 between the fused and the per-layer network (its chunk-invariance test); candidate grid = full scan, bit for bit"""
    net = nets(t)
    frame, world, d, near, far = _case_frame(hip, gpu, name)
    P = world.shape[0]

    def render():
        hip.set_dparf(*C.TRIPLES[t], gpu)
        pts = hip.Points(world, d, near, far, n_samples=2)
        hip.render_prepass(pts, world, 3, n_clusters=frame.c.n_clusters)
        hip.render_pregather(net, frame, pts)
        return hip.render_rays(net, frame, pts)

    nbr = render()
    assert hip.mlp_is_fused(gpu) and nbr[3]["valid_samples"] == 2 * P and float(nbr[1].max()) > 0
    try:
        hip.set_tok_gather(False)
        folded = render()
    finally:
        hip.set_tok_gather(True)
    try:
        hip.set_mlp_mode(0)
        layers = render()
    finally:
        hip.set_mlp_mode(1)
    monkeypatch.setenv("TH_DPARF_NOGRID", "1")
    full_scan = render()
    for a, b in zip(nbr[:3], full_scan[:3]):
        assert torch.equal(a, b)
    d_fold = max(maxdiff(a.cpu(), b.cpu()) for a, b in zip(nbr[:2], folded[:2]))
    d_layers = max(maxdiff(a.cpu(), b.cpu()) for a, b in zip(nbr[:2], layers[:2]))
    print(f"{name} {t}: records vs folded rows {d_fold:.2e}, fused vs per-layer {d_layers:.2e}")
    assert d_fold < 2e-6 and d_layers < 5e-5


# ---- 8: the recordings -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", list(C.TRIPLES))
def test_rows_vs_the_recording(hip, gpu, t):
    K, F_, alpha = C.TRIPLES[t]
    g7 = np.load(GOLD + "/g7_dparf.npz")
    tok = gold("g6_vit")["out"]
    rot = np.ascontiguousarray(g7["blend"][:, :3, :3].astype(np.float32).reshape(-1, 9))
    ref = np.moveaxis(C.golden()[f"rep_{t}"], 2, 0).astype(np.float64)                           # [P,V,195 + 6 F]
    hip.set_dparf(K, F_, alpha, gpu)
    got = hip.dparf_encode(torch.from_numpy(g7["pts_s"]).to(gpu), torch.from_numpy(g7["centres"]).to(gpu),
                           torch.from_numpy(rot).to(gpu), tok.to(gpu)).double().cpu().numpy()
    n = 195 + 6 * F_
    tol_tok, tol_pe = C.row_bounds(g7["pts_s"], g7["centres"], rot, tok, K, F_, alpha)
    assert (got[..., n:] == 0).all()
    e_tok, e_pe = np.abs(got[..., :192] - ref[..., :192]), np.abs(got[..., 192:n] - ref[..., 192:])
    print(f"rep_{t}: tokens worst error / bound {float((e_tok / tol_tok).max()):.3f}, xyz/PE {float((e_pe / tol_pe[:, None, :]).max()):.3f}")
    assert (e_tok <= tol_tok).all() and (e_pe <= tol_pe[:, None, :]).all()


@pytest.mark.parametrize("t", list(C.TRIPLES))
def test_network_forward_vs_the_recording(hip, gpu, nets, t):
    """the bar tests/test_gpu_parity.py holds g8 to: 1e-4"""
    g = C.golden()
    pf, vd, pts, mask, centres, blend, tok = (x.to(gpu) for x in C.forward_inputs())
    dd = lambda: {"pts_smplcoord": pts[None], "obs_smpl_smplcoord": centres[None], "blend_mtx": blend[None]}
    net = nets(t)
    with C.under(t):
        for tag, V, mk in (("none", 3, None), ("rand", 3, mask[None])) + ((("v1_none", 1, None), ("v1_rand", 1, mask[None])) if t == "B" else ()):
            raw = net(pf[:V], vd[None], dd(), holder=tok[:V], face_idx=None, pts_mask=mk)
            d = maxdiff(raw[0].cpu(), torch.from_numpy(g[f"fwd_{t}_{tag}"]))
            print(f"fwd_{t}_{tag}: {d:.2e}")
            assert raw.shape == (1, 1024, 4) and d < 1e-4, (tag, d)
    assert hip.dparf_in_force(gpu) == C.TRIPLES[t]


@pytest.mark.parametrize("t", ["B", "D"])
def test_render_fast_vs_the_recording(hip, gpu, nets, t):
    """the assertions of tests/test_gpu_parity.py::test_render_fast_vs_golden[small]"""
    g, g11 = C.golden(), gold("g11_render_small")
    b = synth.batch_to(synth.make_batch(32, 32, 3, seed=0), gpu)
    with C.under(t, N_samples=32, num_class=300):
        r = _renderer(nets(t))
        out = r.render_fast(b, is_train=False)
        assert r.last_stats["hit_rays"] == int(g11["hit_rays"]) and r.last_stats["unmasked"] == 1
    rgb, acc, depth = (torch.from_numpy(g[f"frame_{t}_{k}"]) for k in ("rgb", "acc", "depth"))
    assert maxdiff(out["rgb_map"][0].cpu(), rgb) < 1e-4
    assert maxdiff(out["acc_map"][0].cpu(), acc) < 1e-4
    assert maxdiff(out["depth_map"][0].cpu(), depth) < 5e-4
    mse = float(((out["rgb_map"][0].cpu().double() - rgb.double()) ** 2).mean())
    assert -10 * np.log10(max(mse, 1e-30)) > 80.0
    assert maxdiff(rgb, g11["rgb"]) > 1e-3, "the recording differs from the frame at the defaults"


ALL_DEVICE = {"train_kernels": "device", "train_attention": "device", "train_vit_dense": "device", "train_maps": "latents",
              "train_gather_bwd": "ordered", "train_point_net": "device", "train_encoder": "device"}
STEP_SWITCHES = {"kernels-torch": {"train_kernels": "torch"}, "kernels-device": {"train_kernels": "device"},
                 "kernels-device-point-net-torch": {"train_kernels": "device", "train_point_net": "torch"},
                 "all-seven-device": ALL_DEVICE}


@pytest.mark.parametrize("name", list(STEP_SWITCHES))
def test_training_step_under_B_matches_the_reference(hip, gpu, name):
    """g18's unchanged bars: outputs 2e-5, loss 1e-6, the 20 gradients 2e-3 of their maximum (train_step_case.check_step)"""
    with config.override(**step.STEP_CFG, **C.build_cfg("B"), **STEP_SWITCHES[name]):
        net, r, b = step.setup(gpu)
        with C.under("B"):                                          # (KNN: per call)
            step.check_step(C.step_recording("B"), net, r, b)


def test_sigma_grid_and_eval_points_under_B_vs_the_oracle(hip, gpu, nets, monkeypatch):
    """the grid of g12_mesh_cube (20^3, padded to 40^3) at its bar, 1e-4 and the same empty voxels; eval_points at the same bar"""
    K, F_, alpha = C.TRIPLES["B"]
    monkeypatch.setattr(O, "network_forward", functools.partial(O.network_forward, K=K, n_freq=F_, alpha=alpha))
    net = nets("B")
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    bc = synth.make_batch(32, 32, 3, seed=0)
    bc["pts"] = synth.make_grid_pts(bc, 20)
    off, mem = csr(synth_assign(300))
    with torch.no_grad():
        hol, pix = O.encoder_forward(sd, bc["input_imgs"][0][0])
        ref = O.render_sigma_grid(sd, bc, bc["pts"], hol, pix, off, mem, can_centres64(synth_assign(300)))
    b = synth.batch_to(bc, gpu)
    with C.under("B", N_samples=32, num_class=300):
        r = _renderer(net, mesh=True)
        out = r.render(b)
        cube = torch.from_numpy(out["cube"][10:-10, 10:-10, 10:-10])
        assert out["cube"].shape == (40, 40, 40) and int((ref != 0).sum()) > 500
        assert maxdiff(cube, ref) < 1e-4 and torch.equal(cube != 0, ref != 0)
        # eval_points: the grid's points again, with the zero view embedding -- the sigma column is the cube
        from transhuman_amd import mesh_color
        frame = r.prepare_frame(b)
        hip.set_dparf(*C.TRIPLES["B"], gpu)
        raw, stats = hip.eval_points(net, frame, b["pts"].reshape(-1, 3)[::7].contiguous())
    assert maxdiff(raw[:, 3].cpu(), ref.reshape(-1)[::7]) < 1e-4 and stats["valid_samples"] > 50


# ---- 9: the life of the parameters ---------------------------------------------------------------------------------------------------
def test_parameters_switch_both_ways_and_networks_of_two_widths_share_a_device(hip, gpu, nets):
    b = synth.batch_to(synth.make_batch(32, 32, 3, seed=0), gpu)
    frames = []
    with config.override(N_samples=32, num_class=300):
        for t in ("default", "B", "default", "D", "B", "default"):
            cfg = {} if t == "default" else C.cfg_of(t)
            with config.override(**cfg):
                out = _renderer(nets(t)).render_fast(b, is_train=False)
            assert hip.dparf_in_force(gpu) == (DEFAULT if t == "default" else C.TRIPLES[t])
            frames.append({k: out[k].clone() for k in ("rgb_map", "acc_map", "depth_map")})
    g11 = gold("g11_render_small")
    assert maxdiff(frames[0]["rgb_map"][0].cpu(), g11["rgb"]) < 1e-4
    for i in (2, 5):                                                  # back at the defaults: the first frame, bit for bit
        assert all(torch.equal(frames[i][k], frames[0][k]) for k in frames[0]), i
    assert all(torch.equal(frames[4][k], frames[1][k]) for k in frames[1])       # B again, after a network of another width
    assert maxdiff(frames[1]["rgb_map"], frames[0]["rgb_map"]) > 1e-3 and maxdiff(frames[3]["rgb_map"], frames[1]["rgb_map"]) > 1e-3


def test_weights_of_the_wrong_width_are_refused_with_both_numbers(hip, gpu, nets):
    lib = hip.load_library()
    net = nets("B")                                                   # fc_0 is 256 x 231
    hip.set_dparf(7, 10, 0.5, gpu)
    W, keep = hip.ThMlpWeights(), []
    lin, k = hip._linear(net.fc_0.weight, net.fc_0.bias)
    keep.append(k)
    W.fc_0 = lin
    assert lib.th_set_mlp_weights(hip.ctx(gpu), hip.C.byref(W), hip._stream()) != 0
    msg = lib.th_last_error().decode()
    assert "256 x 231" in msg and "256 x 255" in msg, msg
    hip._state(gpu).owner.pop("mlp", None)                            # (whatever the context held: the next frame uploads)


# ---- 10: truncation ------------------------------------------------------------------------------------------------------------------
def test_truncation_under_B_drops_what_the_oracle_drops(hip, gpu, nets):
    """K27's distance is K4's first neighbour whatever K: every sample of g8's inputs, at the margin-settled radius of g27"""
    g = C.golden()
    sigma = float(np.load(GOLD + "/g27_truncation.npz")["fwd_sigma"])
    pf, vd, pts, mask, centres, blend, tok = (x.to(gpu) for x in C.forward_inputs())
    keep = truncation_mask_oracle(pts.cpu().numpy(), centres.cpu().numpy(), sigma)
    assert 0.1 < keep.mean() < 0.9
    dd = {"pts_smplcoord": pts[None], "obs_smpl_smplcoord": centres[None], "blend_mtx": blend[None]}
    with C.under("B", use_truncation=True, KNN_SIGMA=sigma):
        raw = nets("B")(pf, vd[None], dd, holder=tok, face_idx=None, pts_mask=None)[0].cpu()
    assert np.array_equal((raw != 0).any(1).numpy(), keep)
    assert maxdiff(raw[torch.from_numpy(keep)], torch.from_numpy(g["fwd_B_none"][keep])) < 1e-4
