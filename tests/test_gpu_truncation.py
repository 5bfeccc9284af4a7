"""K27 (transhuman_amd/csrc/k_truncate.hip) and cfg.use_truncation on the device.

 (a) hip.truncate_select = truncation.truncation_mask_oracle exactly -- mask, sel, count -- across the block and wave edges, with
     1 .. 1500 token centres, everything / nothing / alternating waves kept, over K4's candidate grid and without it
 (b) the threshold: dyadic points at sigma, one ulp below, one ulp above; the reference's recorded mask (fp32 comparison)
 (c) truncate_scatter / truncate_scatter_bwd / train_ops.TruncScatterFn: exact zeros, exact rows, the gather as adjoint
 (d) both kernels twice: bit-identical, and the same after NaN bytes in every output and in the workspace
 (e) the reference's recorded training step under truncation at train_step_case.check_step's bars, across the training switches
 (f) the per-point network sees P' rows, not P
 (g) Network.forward, render_fast and eval_points under truncation against the recordings / the oracle; off = never set
"""
import functools

import numpy as np
import pytest
import torch

import train_step_case as step
import truncation_case as tc
from transhuman_amd import config, synth
from transhuman_amd.truncation import truncation_mask_oracle
from util import can64, gold, make_net, maxdiff, synth_assign

pytestmark = pytest.mark.gpu
F = np.float32
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1025, 70001)


@pytest.fixture(scope="module")
def hip(gpu):
    from transhuman_amd import hip as H
    H.load_library()
    return H


@functools.lru_cache(maxsize=None)
def _case(P, nc):
    pts, cen = tc.body_case(P, nc)
    return pts, cen, truncation_mask_oracle(pts, cen, 0.1)


def _select(hip, gpu, pts, cen, sigma):
    mask, sel, n = hip.truncate_select(torch.from_numpy(pts).to(gpu), torch.from_numpy(cen).to(gpu), sigma)
    return mask.cpu().numpy().astype(bool), sel.cpu().numpy(), n


def _holds(got, keep):
    mask, sel, n = got
    assert mask.shape == keep.shape and sel.dtype == np.int32
    assert np.array_equal(mask, keep)
    assert n == int(keep.sum()) and np.array_equal(sel, np.where(keep)[0])


# ---- (a) ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", (True, False), ids=("grid", "full-scan"))
@pytest.mark.parametrize("nc", (1, 7, 300, 1500))
def test_select_equals_the_oracle(hip, gpu, monkeypatch, nc, grid):
    if not grid:
        monkeypatch.setenv("TH_DPARF_NOGRID", "1")
    for P in SIZES:
        pts, cen, keep = _case(P, nc)
        if P >= 1023 and nc >= 7:
            assert 0.05 < keep.mean() < 0.95, (P, nc, keep.mean())
        _holds(_select(hip, gpu, pts, cen, 0.1), keep)


@pytest.mark.parametrize("grid", (True, False), ids=("grid", "full-scan"))
@pytest.mark.parametrize("P", (257, 1025, 70001))
def test_select_patterns(hip, gpu, monkeypatch, P, grid):
    """everything kept, nothing kept, alternating waves of 64 kept"""
    if not grid:
        monkeypatch.setenv("TH_DPARF_NOGRID", "1")
    pts, cen, _ = _case(P, 300)
    _holds(_select(hip, gpu, pts, cen, 100.0), np.ones(P, bool))
    _holds(_select(hip, gpu, pts, cen, 1e-6), np.zeros(P, bool))
    assert not truncation_mask_oracle(pts, cen, 1e-6).any()
    alt = pts.copy()
    even = (np.arange(P) // 64) % 2 == 0
    alt[even] = cen[np.arange(P)[even] % len(cen)] + F(0.001)
    alt[~even] += F(5.0)
    keep = truncation_mask_oracle(alt, cen, 0.1)
    assert np.array_equal(keep, even)
    _holds(_select(hip, gpu, alt, cen, 0.1), keep)


def test_select_drops_nan_and_inf(hip, gpu):
    pts, cen, _ = _case(257, 300)
    pts = pts.copy()
    pts[3, 1], pts[64, 0], pts[200, 2] = np.nan, np.inf, -np.inf
    keep = truncation_mask_oracle(pts, cen, 10.0)
    assert not keep[[3, 64, 200]].any() and keep.sum() == 254
    _holds(_select(hip, gpu, pts, cen, 10.0), keep)


# ---- (b) ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", (True, False), ids=("grid", "full-scan"))
def test_threshold(hip, gpu, monkeypatch, grid):
    if not grid:
        monkeypatch.setenv("TH_DPARF_NOGRID", "1")
    for sigma in (0.25, 0.5):
        pts, cen, keep = tc.threshold_case(sigma)
        assert np.array_equal(truncation_mask_oracle(pts, cen, sigma), keep)
        _holds(_select(hip, gpu, pts, cen, sigma), keep)
    g = tc.golden()
    for sigma, keep in zip(g["mask_sigmas"], g["mask_keep"]):       # incl. 0.7: fp32(0.7) < 0.7, the point at fp32(0.7) is dropped
        _holds(_select(hip, gpu, g["mask_pts"], g["mask_centres"], float(sigma)), keep)


# ---- (c) ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", (1, 255, 1025, 70001))
def test_scatter_and_its_adjoint(hip, gpu, P):
    from transhuman_amd.networks import train_ops
    pts, cen, keep = _case(P, 300)
    mask, sel, n = hip.truncate_select(torch.from_numpy(pts).to(gpu), torch.from_numpy(cen).to(gpu), 0.1)
    rs = np.random.RandomState(P)
    rows = torch.from_numpy(rs.normal(size=(n, 4)).astype(F)).to(gpu)
    g = torch.from_numpy(rs.normal(size=(P, 4)).astype(F)).to(gpu)
    full = hip.truncate_scatter(rows, mask, sel)
    k = torch.from_numpy(keep).to(gpu)
    assert full.shape == (P, 4) and torch.equal(full[k], rows)
    assert torch.equal(full[~k].view(torch.int32), torch.zeros((P - n, 4), dtype=torch.int32, device=gpu)), "exact +0 rows"
    assert torch.equal(hip.truncate_scatter_bwd(g, sel), g[sel.long()])
    leaf = rows.clone().requires_grad_(True)
    out = train_ops.TruncScatterFn.apply(leaf, mask, sel)
    assert torch.equal(out, full)
    out.backward(g)
    assert torch.equal(leaf.grad, g[sel.long()])


def test_scatter_of_nothing_and_of_everything(hip, gpu):
    pts, cen, _ = _case(257, 300)
    p, c = torch.from_numpy(pts).to(gpu), torch.from_numpy(cen).to(gpu)
    mask, sel, n = hip.truncate_select(p, c, 1e-6)
    assert n == 0 and sel.numel() == 0
    assert not hip.truncate_scatter(torch.zeros((0, 4), device=gpu), mask, sel).any()
    assert hip.truncate_scatter_bwd(torch.ones((257, 4), device=gpu), sel).shape == (0, 4)
    mask, sel, n = hip.truncate_select(p, c, 100.0)
    rows = torch.arange(257 * 4.0, device=gpu).reshape(257, 4)
    assert n == 257 and torch.equal(hip.truncate_scatter(rows, mask, sel), rows)


# ---- (d) ----------------------------------------------------------------------------------------------------------------------
def _raw_select(hip, gpu, p, c, sigma, fill):
    """th_truncate_select into buffers of the test's own, every byte of outputs and workspace set to ``fill`` first"""
    lib = hip.load_library()
    P, nc = p.shape[0], c.shape[0]
    nb = int(lib.th_truncate_select_workspace_bytes(P, nc))
    bufs = [torch.full((n,), fill, dtype=torch.uint8, device=gpu) for n in (P, 4 * P, 4, nb)]
    mask, sel, count, ws = bufs
    hip._check(lib.th_truncate_select(hip.ctx(gpu), hip._p(p), P, hip._p(c), nc, float(sigma), hip._p(mask), hip._p(sel),
                                      hip._p(count), hip._p(ws), nb, hip._stream()))
    torch.cuda.synchronize()
    n = int(count.view(torch.int32)[0])
    return mask.clone(), sel.view(torch.int32)[:n].clone(), n, sel.view(torch.int32)[n:].clone()


@pytest.mark.parametrize("grid", (True, False), ids=("grid", "full-scan"))
def test_select_is_deterministic_and_ignores_old_contents(hip, gpu, monkeypatch, grid):
    if not grid:
        monkeypatch.setenv("TH_DPARF_NOGRID", "1")
    pts, cen, keep = _case(70001, 300)
    p, c = torch.from_numpy(pts).to(gpu), torch.from_numpy(cen).to(gpu)
    a = _raw_select(hip, gpu, p, c, 0.1, 0x00)
    b = _raw_select(hip, gpu, p, c, 0.1, 0x00)
    n = _raw_select(hip, gpu, p, c, 0.1, 0xFF)                      # 0xFF bytes: NaN as floats, -1 as counts
    for other in (b, n):
        assert a[2] == other[2] and torch.equal(a[0], other[0]) and torch.equal(a[1], other[1])
    _holds((a[0].cpu().numpy().astype(bool), a[1].cpu().numpy(), a[2]), keep)
    assert (n[3] == -1).all(), "nothing is stored behind the list"


def test_scatter_is_deterministic_and_ignores_old_contents(hip, gpu):
    lib = hip.load_library()
    pts, cen, _ = _case(70001, 300)
    P = 70001
    mask, sel, n = hip.truncate_select(torch.from_numpy(pts).to(gpu), torch.from_numpy(cen).to(gpu), 0.1)
    rows = torch.randn((n, 4), device=gpu)
    g = torch.randn((P, 4), device=gpu)
    first = hip.truncate_scatter(rows, mask, sel)
    assert torch.equal(hip.truncate_scatter(rows, mask, sel), first)
    out = torch.full((P, 4), float("nan"), device=gpu)
    hip._check(lib.th_truncate_scatter(hip.ctx(gpu), hip._p(rows), hip._p(mask), hip._p(sel), n, P, 4, hip._p(out), hip._stream()))
    assert torch.equal(out, first)
    back = hip.truncate_scatter_bwd(g, sel)
    out = torch.full((n, 4), float("nan"), device=gpu)
    hip._check(lib.th_truncate_scatter_bwd(hip.ctx(gpu), hip._p(g), hip._p(sel), n, P, 4, hip._p(out), hip._stream()))
    assert torch.equal(out, back) and torch.equal(hip.truncate_scatter_bwd(g, sel), back)


def test_entry_refusals(hip, gpu):
    lib = hip.load_library()
    p = torch.zeros((4, 3), device=gpu)
    out = torch.zeros(64, dtype=torch.int32, device=gpu)
    assert lib.th_truncate_scatter(hip.ctx(gpu), hip._p(p), hip._p(out), hip._p(out), 1, 4, 3, hip._p(out), hip._stream()) != 0
    assert lib.th_truncate_scatter(hip.ctx(gpu), hip._p(p), hip._p(out), hip._p(out), 5, 4, 4, hip._p(out), hip._stream()) != 0
    assert lib.th_truncate_select(hip.ctx(gpu), hip._p(p), 4, hip._p(p), 1, 0.1, hip._p(out), hip._p(out), hip._p(out),
                                  hip._p(out), 8, hip._stream()) != 0, "workspace too small"
    assert lib.th_set_truncation(hip.ctx(gpu), float("nan")) != 0


# ---- (e), (f) -----------------------------------------------------------------------------------------------------------------
ALL_DEVICE = {"train_kernels": "device", "train_attention": "device", "train_vit_dense": "device", "train_maps": "latents",
              "train_gather_bwd": "ordered", "train_point_net": "device", "train_encoder": "device"}
# ("kernels-device" runs cfg.train_maps = "full", its default; "maps-latents" the other value)
STEP_SWITCHES = {"kernels-device": {"train_kernels": "device"}, "all-seven-device": ALL_DEVICE,
                 "kernels-device-point-net-torch": {"train_kernels": "device", "train_point_net": "torch"},
                 "maps-latents": {"train_kernels": "device", "train_maps": "latents"},
                 "kernels-torch": {"train_kernels": "torch"}}


@pytest.mark.parametrize("name", list(STEP_SWITCHES))
def test_training_step_under_truncation_matches_the_reference(hip, gpu, name):
    """recording 3: outputs 2e-5, loss 1e-6, the 20 gradients 2e-3 of their maximum (train_step_case.check_step)"""
    with config.override(**step.STEP_CFG, **tc.step_cfg(), **STEP_SWITCHES[name]):
        step.check_step(tc.golden(), *step.setup(gpu))


@pytest.mark.parametrize("point_net", ("device", "torch"))
def test_the_point_network_sees_the_kept_rows_only(hip, gpu, monkeypatch, point_net):
    from transhuman_amd.networks import autograd_path as ap
    g = tc.golden()
    seen = []
    which = "point_network_device" if point_net == "device" else "point_network"
    real = getattr(ap, which)

    def counting(net, h, f, viewdir, *a, **k):
        seen.append((h.shape[0], f.shape[0], viewdir.shape[0]))
        return real(net, h, f, viewdir, *a, **k)
    monkeypatch.setattr(ap, which, counting)
    with config.override(**step.STEP_CFG, **tc.step_cfg(), train_kernels="device", train_point_net=point_net):
        net, r, b = step.setup(gpu)
        ap.render(r, b)
        kept, P = int(g["step_kept"]), int(g["rays"]) * int(config.get_cfg().N_samples)
    assert 0 < kept < P
    assert sum(s[0] for s in seen) == kept and all(s[0] == s[1] == s[2] for s in seen)


def test_nothing_kept_on_the_device(hip, gpu):
    from transhuman_amd.networks import autograd_path as ap
    with config.override(**step.STEP_CFG, use_truncation=True, KNN_SIGMA=1e-9, **ALL_DEVICE):
        net, r, b = step.setup(gpu)
        ret = ap.render(r, b)
    assert all(float(ret[k].abs().max()) == 0.0 for k in ("rgb_map", "acc_map", "depth_map"))


# ---- (g) ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net(gpu, hip):
    return make_net(12).to(gpu)


def test_network_forward_under_truncation_vs_golden(hip, gpu, net):
    """recording 2, Network.forward through the reference's own call signature at the bar of the g8_forward test (1e-4): truncation
    inside pts_mask (progressive branch), the non-progressive branch on the kept rows without one, zeros elsewhere"""
    g, g8 = tc.golden(), gold("g8_forward")
    g7, tok = gold("g7_dparf"), gold("g6_vit")["out"]
    centres, blend = g7["centres"], g7["blend"]
    pf = torch.from_numpy(synth.smooth_noise((3, 384, 1024), 23, passes=0))
    dd = lambda: {"pts_smplcoord": g8["pts_s"][None].to(gpu), "obs_smpl_smplcoord": centres[None].to(gpu),
                  "blend_mtx": blend[None].to(gpu)}
    mask = g8["mask"][None].to(gpu)
    with config.override(use_truncation=True, KNN_SIGMA=float(g["fwd_sigma"])):
        for tag, V, mk in (("none", 3, None), ("rand", 3, mask), ("zero", 3, torch.zeros_like(mask)), ("v1_rand", 1, mask),
                           ("v1_none", 1, None)):
            raw = net(pf[:V].to(gpu), g8["viewdir"][None].to(gpu), dd(), holder=tok[:V].to(gpu), face_idx=None, pts_mask=mk)
            ref = torch.from_numpy(g["fwd_raw_" + tag])
            assert raw.shape == (1, 1024, 4)
            assert maxdiff(raw[0].cpu(), ref) < 1e-4, tag
            assert torch.equal(raw[0].cpu() == 0, ref == 0), tag            # the same rows are dropped
    far = ~truncation_mask_oracle(g8["pts_s"].numpy(), centres.numpy(), float(g["fwd_sigma"]))
    assert 0.1 < far.mean() < 0.9 and (g["fwd_raw_none"][far] == 0).all()


def _renderer(net):
    from transhuman_amd.networks.renderer import if_clight_renderer
    return if_clight_renderer.Renderer(net, vertex_can=can64().numpy(), pc2voxel_ind=synth_assign(300))


def test_render_fast_under_truncation_vs_golden(hip, gpu, net):
    """recording 4 at the assertion of test_gpu_parity.test_render_fast_vs_golden[small]; with the option off the frame is
    torch.equal to one rendered before the setter was ever called with a radius"""
    g, g11 = tc.golden(), gold("g11_render_small")
    b = synth.batch_to(synth.make_batch(32, 32, 3, seed=0), gpu)
    with config.override(N_samples=32, num_class=300):
        r = _renderer(net)
        plain = r.render_fast(b, is_train=False)
        assert maxdiff(plain["rgb_map"][0].cpu(), g11["rgb"]) < 1e-4
        with config.override(use_truncation=True, KNN_SIGMA=float(g["frame_sigma"])):
            out = r.render_fast(b, is_train=False)
        assert r.last_stats["hit_rays"] == int(g11["hit_rays"]) and r.last_stats["unmasked"] == 1
        off = r.render_fast(b, is_train=False)
    assert all(torch.equal(off[k], plain[k]) for k in plain)
    rgb, acc, depth = (torch.from_numpy(g["frame_" + k]) for k in ("rgb", "acc", "depth"))
    assert maxdiff(out["rgb_map"][0].cpu(), rgb) < 1e-4
    assert maxdiff(out["acc_map"][0].cpu(), acc) < 1e-4
    assert maxdiff(out["depth_map"][0].cpu(), depth) < 5e-4
    mse = float(((out["rgb_map"][0].cpu().double() - rgb.double()) ** 2).mean())
    assert -10 * np.log10(max(mse, 1e-30)) > 80.0
    assert maxdiff(rgb, g11["rgb"]) > 1e-2, "the recording differs from the frame without truncation"


def test_eval_points_zero_rows_where_the_oracle_drops(hip, gpu, net):
    b = synth.batch_to(synth.make_batch(32, 32, 3, seed=0), gpu)
    sigma = 0.05
    with config.override(N_samples=32, num_class=300):
        r = _renderer(net)
        frame = r.prepare_frame(b)
    rs = np.random.RandomState(27)
    verts = b["tar_smpl_vertice"][0].cpu().numpy()
    cand = (verts[rs.randint(0, len(verts), size=600)] + rs.normal(0, 0.04, (600, 3))).astype(F)
    Rh, Th = frame.Rh.cpu().numpy().reshape(3, 3).astype(np.float64), frame.Th.cpu().numpy().astype(np.float64)
    cen = frame.centres.cpu().numpy()
    d = np.sqrt(((((cand - Th) @ Rh)[:, None, :] - cen[None].astype(np.float64)) ** 2).sum(-1).min(1))
    pts_np = cand[np.abs(d - sigma) > 1e-5][:300]              # (the device forms world2smpl in fp32: keep clear of the threshold)
    assert len(pts_np) == 300
    drop = torch.from_numpy(d[np.abs(d - sigma) > 1e-5][:300] >= sigma)
    pts = torch.from_numpy(pts_np).to(gpu)
    try:
        hip.set_truncation(0.0, gpu)
        raw_off, _ = hip.eval_points(net, frame, pts)
        sig_off, _ = hip.eval_sigma_grid(net, frame, pts)
        hip.set_truncation(sigma, gpu)
        raw_on, _ = hip.eval_points(net, frame, pts)
        sig_on, _ = hip.eval_sigma_grid(net, frame, pts)
    finally:
        hip.set_truncation(0.0, gpu)
    raw_off, raw_on, sig_off, sig_on = (t.cpu() for t in (raw_off, raw_on, sig_off, sig_on))
    assert 30 < int(drop.sum()) < 270
    assert (raw_off[drop][:, 3] != 0).sum() > 10, "dropped points that the hull keeps"
    assert (raw_on[drop] == 0).all() and (sig_on[drop] == 0).all()
    assert torch.equal(raw_on[~drop], raw_off[~drop]) and torch.equal(sig_on[~drop], sig_off[~drop])
    again, _ = hip.eval_points(net, frame, pts)
    assert torch.equal(again.cpu(), raw_off), "off again: the frame without truncation"
