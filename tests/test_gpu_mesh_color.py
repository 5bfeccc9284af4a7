"""th_eval_points (the radiance field at arbitrary points, with the RGB branch and a direction per point) against the oracle, and
the vertex colours built on it (transhuman_amd/mesh_color.py, cfg.mesh_colors).

The case of test_sigma_grid_32: make_batch(64, 64, V), N_c = 300, the depth-12 net, V = 3 and V = 1.  Points are drawn uniformly
in the body's box and dealt seven inside the hull to one outside (the oracle's mask decides), so that the VALID samples of
P = 1 .. 2048 sit around K6's 32-sample tile: 1, 28, 28, 29, 32, 33, 85 and 1792 of them.  The oracle (th_oracle, fp32 on the host) is
assembled once per V on the first 512 points and shared.

Bars: sigma within 1e-4 (test_mesh_sigma_cube_vs_golden's), sigmoid(rgb) within 1e-4 (the project's RGB bar), the hull mask and
the sigma > 0 pattern equal.  A point whose oracle |sigma| <= 2e-5 may take the other branch ("What's weak" 1(a)) and
is left out of the pattern and RGB comparison, at most 1 % of the compared points.  On this seed the oracle itself has NO such
point and its fp32 and float64 forms agree on every branch (checked on the host before the seed was fixed: V = 3 and V = 1,
512 points each)."""
import numpy as np
import pytest
import torch

from transhuman_amd import synth
from util import make_net, make_sd, synth_assign, can64, csr, can_centres64

pytestmark = pytest.mark.gpu

SEED = 24
N_ORACLE = 512
SIZES = [1, 31, 32, 33, 36, 37, 97, 2048]


def make_points(bc, n=2048, seed=SEED):
    """-> (pts fp32 [n,3], unit dirs fp32 [n,3], oracle hull mask bool [n]): uniform draws in the body's box, reordered 7 inside : 1
    outside (position 7 of every 8 is outside)"""
    from oracle import th_oracle as O
    rs = np.random.RandomState(seed)
    lo, hi = bc["can_bounds"][0].numpy().astype(np.float64)
    cand = torch.from_numpy((lo + rs.rand(4 * n, 3) * (hi - lo)).astype(np.float32))
    d = rs.randn(n, 3)
    dirs = torch.from_numpy((d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32))
    hull = O.hull_mask(cand, bc["tar_smpl_vertice"][0])
    inside, outside = torch.nonzero(hull).reshape(-1), torch.nonzero(~hull).reshape(-1)
    want_out = torch.arange(n) % 8 == 7
    assert len(inside) >= int((~want_out).sum()) and len(outside) >= int(want_out.sum())
    order = torch.empty(n, dtype=torch.long)
    order[~want_out] = inside[:int((~want_out).sum())]
    order[want_out] = outside[:int(want_out.sum())]
    return cand[order].contiguous(), dirs, hull[order]


def oracle_raw(bc, pts, dirs, hull):
    """th_oracle at the points: raw [P,4] with the caller's directions and with the zero embedding (fp32, host)"""
    from oracle import th_oracle as O
    sd = make_sd(12)
    assign = synth_assign(300)
    off, mem = csr(assign)
    with torch.no_grad():
        hol, pix = O.encoder_forward(sd, bc["input_imgs"][0][0])
        fc = O.frame_constants(sd, bc, hol, off, mem, can_centres64(assign), 12)
        ps = O.world2smpl(pts, bc["Rh"][0], bc["Th"][0])
        pf = O.pixel_aligned(pix, pts, bc)
        with_dirs = O.network_forward(sd, pf, O.view_embed(dirs), ps, fc["centres"], fc["blend"], fc["tokens"], hull)
        zero = O.network_forward(sd, pf, torch.zeros(pts.shape[0], 27), ps, fc["centres"], fc["blend"], fc["tokens"], hull)
    return with_dirs, zero


@pytest.fixture(scope="module")
def hip(gpu):
    from transhuman_amd import hip as H
    H.load_library()
    return H


_scenes = {}


def scene(gpu, V):
    """batch, renderer, frame, points and the oracle of one view count, made once"""
    if V not in _scenes:
        from transhuman_amd.config import get_cfg
        from transhuman_amd.networks.renderer import if_mesh_renderer
        cfg = get_cfg()
        cfg.N_samples, cfg.num_class = 32, 300
        bc = synth.make_batch(64, 64, V, seed=0)
        bc["pts"] = synth.make_grid_pts(bc, 32)
        b = synth.batch_to(bc, gpu)
        r = if_mesh_renderer.Renderer(make_net(12).to(gpu), vertex_can=can64().numpy(), pc2voxel_ind=synth_assign(300))
        frame = r.prepare_frame(b)
        pts, dirs, hull = make_points(bc)
        ref, ref_zero = oracle_raw(bc, pts[:N_ORACLE], dirs[:N_ORACLE], hull[:N_ORACLE])
        _scenes[V] = dict(bc=bc, b=b, r=r, frame=frame, pts=pts.to(gpu), dirs=dirs.to(gpu), hull=hull, ref=ref, ref_zero=ref_zero)
    return _scenes[V]


def against_oracle(raw, ref, hull, tag):
    """the four checks of one raw [n,4] against the oracle's rows"""
    n = raw.shape[0]
    raw, ref, hull = raw.cpu(), ref[:n], hull[:n]
    assert torch.equal((raw != 0).any(1) | hull, hull), tag                      # rows outside the hull are exactly 0
    assert float(raw[~hull].abs().max()) == 0.0 if bool((~hull).any()) else True
    d_sigma = float((raw[:, 3] - ref[:, 3]).abs().max())
    near = hull & (ref[:, 3].abs() <= 2e-5)                                      # may take the other branch
    cmp = hull & ~near
    pos_d, pos_r = raw[:, 3] > 0, ref[:, 3] > 0
    d_rgb = float((torch.sigmoid(raw[cmp, :3]) - torch.sigmoid(ref[cmp, :3])).abs().max()) if bool(cmp.any()) else 0.0
    print(f"{tag}: n={n} inside {int(hull.sum())} sigma>0 {int(pos_r.sum())} left out {int(near.sum())}  "
          f"max|sigma - oracle| {d_sigma:.2e}  max|sigmoid(rgb) - oracle| {d_rgb:.2e}")
    assert int(near.sum()) <= 0.01 * n, tag
    assert torch.equal(pos_d[cmp], pos_r[cmp]), tag
    assert float(raw[hull & ~pos_d, :3].abs().max()) == 0.0 if bool((hull & ~pos_d).any()) else True      # no RGB where sigma <= 0
    assert d_sigma < 1e-4, (tag, d_sigma)
    assert d_rgb < 1e-4, (tag, d_rgb)


@pytest.mark.parametrize("V", [3, 1])
@pytest.mark.parametrize("P", SIZES)
def test_eval_points_vs_oracle(hip, gpu, V, P):
    s = scene(gpu, V)
    pts, dirs, hull = s["pts"][:P], s["dirs"][:P], s["hull"][:P]
    raw, stats = hip.eval_points(s["r"].net, s["frame"], pts, dirs)
    assert raw.dtype == torch.float32 and tuple(raw.shape) == (P, 4)
    m, _ = hip.hull_mask(hip.Points(pts=pts), s["b"]["tar_smpl_vertice"][0])
    assert torch.equal(m.view(-1).cpu(), hull) and int(stats["valid_samples"]) == int(hull.sum())      # the hull mask is the oracle's
    n = min(P, N_ORACLE)
    against_oracle(raw[:n], s["ref"], s["hull"], f"V={V} P={P} dirs")
    # dirs=None: the rows of a zero embedding
    raw0, _ = hip.eval_points(s["r"].net, s["frame"], pts)
    against_oracle(raw0[:n], s["ref_zero"], s["hull"], f"V={V} P={P} zero embedding")
    # sigma does not depend on the direction, nor on the RGB branch being on: the sigma grid's kernel form on the same points
    sig, st2 = hip.eval_sigma_grid(s["r"].net, s["frame"], pts)
    d = float((raw[:, 3] - sig).abs().max())
    bar = 2e-5 * max(1.0, float(sig.abs().max()))
    print(f"V={V} P={P}: max |sigma(eval_points) - sigma(eval_sigma_grid)| = {d:.2e} (bar {bar:.2e})")
    assert int(st2["valid_samples"]) == int(stats["valid_samples"])
    assert d <= bar
    # run to run
    again, _ = hip.eval_points(s["r"].net, s["frame"], pts, dirs)
    assert torch.equal(again, raw)


@pytest.mark.parametrize("V", [3, 1])
def test_eval_points_on_the_fp32_per_layer_path(hip, gpu, V):
    s = scene(gpu, V)
    P = 97
    pts, dirs = s["pts"][:P], s["dirs"][:P]
    hip.set_mlp_mode(0)
    try:
        raw, _ = hip.eval_points(s["r"].net, s["frame"], pts, dirs)
        again, _ = hip.eval_points(s["r"].net, s["frame"], pts, dirs)
        raw0, _ = hip.eval_points(s["r"].net, s["frame"], pts)
    finally:
        hip.set_mlp_mode(1)
    against_oracle(raw, s["ref"], s["hull"], f"V={V} P={P} fp32 per-layer")
    against_oracle(raw0, s["ref_zero"], s["hull"], f"V={V} P={P} fp32 per-layer, zero embedding")
    assert torch.equal(again, raw)


def test_empty_point_list(hip, gpu):
    s = scene(gpu, 3)
    raw, stats = hip.eval_points(s["r"].net, s["frame"], s["pts"][:0], s["dirs"][:0])
    assert tuple(raw.shape) == (0, 4) and stats["valid_samples"] == 0


def _true_voxel(bc, n=32):
    lo, hi = bc["can_bounds"][0].numpy().astype(np.float64)
    return [float(x) for x in (hi - lo) / (n - 1)]


@pytest.fixture(scope="module")
def extracted(hip, gpu):
    """the mesh the renderer extracts from the 32^3 grid (iso 0.5: the synthetic weights' sigma_raw is O(1); the voxel size is the
    grid's own spacing, so the vertices lie where the field was sampled)"""
    from transhuman_amd.config import override
    s = scene(gpu, 3)
    with override(mesh_th=0.5, voxel_size=_true_voxel(s["bc"])):
        out = s["r"].render(s["b"], frame=s["frame"])
    assert out["mesh"].faces.shape[0] > 100 and out["mesh"].vertex_colors is None
    return out


def test_vertex_colors_of_the_extracted_mesh(hip, gpu, extracted):
    from transhuman_amd import mesh_color as MCol
    s = scene(gpu, 3)
    mesh = extracted["mesh"]
    nv = mesh.vertices.shape[0]
    col, info = MCol.vertex_colors(s["r"], s["b"], mesh, frame=s["frame"], return_info=True)
    assert col.dtype == torch.uint8 and tuple(col.shape) == (nv, 3) and col.is_cuda
    cf = MCol.vertex_colors(s["r"], s["b"], mesh.vertices, mesh.faces, frame=s["frame"], as_float=True)
    assert cf.dtype == torch.float32 and torch.equal(col, torch.clamp(torch.floor(255.0 * cf + 0.5), 0, 255).to(torch.uint8))
    print(f"extracted mesh: {nv} vertices, {info['valid_samples']} inside the hull, {info['no_rgb']} without RGB (grey)")
    # (a cut edge between two grid points inside the hull puts its vertex where the field is near the iso value 0.5 > 0: some
    # vertices are coloured; one on an edge that leaves the hull may lie outside it and stays grey -- counted, not bounded here)
    assert info["valid_samples"] <= nv and nv - info["valid_samples"] <= info["no_rgb"] < nv
    # a camera centre instead of the normals: another direction, same branch
    cc = MCol.vertex_colors(s["r"], s["b"], mesh, view=(0.0, 0.0, 0.0), frame=s["frame"])
    assert cc.dtype == torch.uint8 and tuple(cc.shape) == (nv, 3)
    # the same through eval_points: rows without RGB are 128 grey
    d = MCol.view_directions(mesh.vertices, mesh.faces)
    raw_u, st_u = hip.eval_points(s["r"].net, s["frame"], mesh.vertices, d)
    cu, n_u = MCol.colors_from_raw(raw_u)
    assert torch.equal(cu, col) and n_u == info["no_rgb"] == int((raw_u[:, 3] <= 0).sum())
    assert bool((col[raw_u[:, 3] <= 0] == 128).all())
    # a coloured vertex moved 1 m away, outside the hull, gets 128 and is counted (the directions are the unmoved mesh's).  Along
    # z: the synthetic body is 0.32 m deep there and 1.6 m wide in x and y, where 1 m can land on an arm
    k = int(torch.nonzero(raw_u[:, 3] > 0)[0])
    moved = mesh.vertices.clone()
    moved[k, 2] += 1.0
    raw_m, st_m = hip.eval_points(s["r"].net, s["frame"], moved, d)
    cm, n_m = MCol.colors_from_raw(raw_m)
    keep = torch.ones(nv, dtype=torch.bool, device=gpu)
    keep[k] = False
    assert cm[k].tolist() == [128, 128, 128] and torch.equal(cm[keep], col[keep])
    assert n_m == n_u + 1 and int(st_m["valid_samples"]) == int(st_u["valid_samples"]) - 1


def test_direction_rule_on_a_marching_cubes_ball(hip, gpu):
    """view="normal": d = -n with the orientation render_mesh_sequence uses for marching-cubes meshes: d . (v - centre) < 0"""
    from transhuman_amd import mesh_color as MCol
    ax = torch.arange(40, dtype=torch.float32)
    g = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1)
    centre = torch.tensor([19.3, 20.1, 19.7])
    cube = 9.0 - (g - centre).norm(dim=-1)
    v, f = hip.marching_cubes(cube.to(gpu), 0.0)
    d = MCol.view_directions(v, f, "normal")
    assert d.dtype == torch.float32 and tuple(d.shape) == tuple(v.shape)
    assert float((d.norm(dim=1) - 1).abs().max()) < 1e-5
    assert bool(((d.double() * (v - centre.to(gpu).double())).sum(1) < 0).all())
    c = torch.tensor([100.0, 20.0, 20.0])
    dc = MCol.view_directions(v, f, c.tolist())
    want = (v - c.to(gpu).double())
    want = want / want.norm(dim=1, keepdim=True)
    assert float((dc.double() - want).abs().max()) < 1e-5


def test_renderer_option_colours_the_mesh(hip, gpu, extracted, tmp_path):
    from transhuman_amd import mesh_color as MCol
    from transhuman_amd.config import override
    from transhuman_amd.mesh import read_ply
    s = scene(gpu, 3)
    with override(mesh_th=0.5, voxel_size=_true_voxel(s["bc"]), mesh_colors="normal"):
        out = s["r"].render(s["b"], frame=s["frame"])
    mesh = out["mesh"]
    assert np.array_equal(out["cube"], extracted["cube"])
    assert torch.equal(mesh.vertices, extracted["mesh"].vertices) and torch.equal(mesh.faces, extracted["mesh"].faces)
    direct = MCol.vertex_colors(s["r"], s["b"], extracted["mesh"], frame=s["frame"])
    assert mesh.vertex_colors is not None and torch.equal(mesh.vertex_colors, direct)
    v, f, c = read_ply(mesh.export(str(tmp_path / "coloured.ply")), colors=True)
    assert np.array_equal(c, direct.cpu().numpy()) and np.array_equal(f, mesh.faces.cpu().numpy())
    # filter first, then colours: the colours of the kept vertices
    with override(mesh_th=0.5, voxel_size=_true_voxel(s["bc"]), mesh_colors="normal", mesh_components="largest"):
        both = s["r"].render(s["b"], frame=s["frame"])["mesh"]
    kept = extracted["mesh"].largest_component()
    assert torch.equal(both.vertices, kept.vertices) and torch.equal(both.faces, kept.faces)
    assert both.vertex_colors.shape[0] == kept.vertices.shape[0]
    assert torch.equal(both.vertex_colors, MCol.vertex_colors(s["r"], s["b"], kept, frame=s["frame"]))
