"""K24 on the device (csrc/k_meshcc.hip through th_mesh_components / th_mesh_filter_count / th_mesh_filter_emit): labels, filtered
vertices, faces and the vertex map EQUAL the numpy definition (transhuman_amd/mesh_clean.py) on every case, twice -- with the
workspace and every output pre-filled with 0xFF bytes and with seeded random bytes -- so nothing depends on what memory held."""
import ctypes as C

import numpy as np
import pytest
import torch

from transhuman_amd import mesh_clean as MC
from test_mesh_clean_host import HAND_CASES, strips

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip(gpu):
    from transhuman_amd import hip as H
    H.load_library()
    return H


def _filled(shape, dtype, gpu, fill, gen):
    t = torch.empty(shape, dtype=dtype, device=gpu)
    nbytes = t.numel() * t.element_size()
    if nbytes:
        b = t.view(-1).view(torch.uint8)
        if fill == "ff":
            b.fill_(0xFF)
        else:
            b.copy_(torch.randint(0, 256, (nbytes,), dtype=torch.uint8, generator=gen).to(gpu))
    return t


def device_run(hip, gpu, faces, verts, keep, fill, seed=0):
    """the three C-ABI calls with every buffer pre-filled -> (labels, verts', faces', vert_map, info, counts)"""
    lib = hip.load_library()
    gen = torch.Generator().manual_seed(seed)
    f = torch.as_tensor(np.asarray(faces).reshape(-1, 3), dtype=torch.int32).to(gpu).contiguous()
    v = torch.as_tensor(verts, dtype=torch.float64).to(gpu).contiguous()
    nv, nf = v.shape[0], f.shape[0]
    ws = _filled((max(int(lib.th_mesh_components_workspace_bytes(nv, nf)), 256),), torch.uint8, gpu, fill, gen)
    labels = _filled((nv,), torch.int32, gpu, fill, gen)
    info, counts = (C.c_int64 * 5)(), (C.c_int64 * 4)()
    p = lambda t: hip._p(t) if t.numel() else None
    hip._check(lib.th_mesh_components(hip.ctx(gpu), p(f), nf, nv, p(labels), hip._p(ws), ws.numel(), info, hip._stream()))
    hip._check(lib.th_mesh_filter_count(hip.ctx(gpu), p(f), nf, nv, p(labels), MC._keep_arg(keep), hip._p(ws), ws.numel(), counts,
                                        hip._stream()))
    v2 = _filled((int(counts[0]), 3), torch.float64, gpu, fill, gen)
    f2 = _filled((int(counts[1]), 3), torch.int32, gpu, fill, gen)
    vm = _filled((nv,), torch.int32, gpu, fill, gen)
    hip._check(lib.th_mesh_filter_emit(hip.ctx(gpu), p(v), p(f), nf, nv, hip._p(ws), ws.numel(), p(v2), p(f2), p(vm), hip._stream()))
    torch.cuda.synchronize()
    return labels, v2, f2, vm, [int(x) for x in info], [int(x) for x in counts]


def check_case(hip, gpu, faces, nv, keeps=("largest", 1)):
    """device == oracle exactly, for both prefills, through the C ABI and through the Python surface"""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    verts = np.random.RandomState(nv).randn(nv, 3)
    ref_labels, ref_info = MC.components_oracle(faces, nv)
    sweeps = None
    for keep in keeps:
        rv, rf, rinfo = MC.filter_components_oracle(verts, faces, keep)
        got = {}
        for fill in ("ff", "rand"):
            labels, v2, f2, vm, info, counts = device_run(hip, gpu, faces, verts, keep, fill)
            assert torch.equal(labels.cpu(), torch.from_numpy(ref_labels)), (keep, fill)
            assert torch.equal(v2.cpu(), torch.from_numpy(rv).reshape(-1, 3)), (keep, fill)
            assert torch.equal(f2.cpu(), torch.from_numpy(rf).reshape(-1, 3)), (keep, fill)
            assert torch.equal(vm.cpu(), torch.from_numpy(rinfo["vert_map"])), (keep, fill)
            assert info[0] == ref_info["n_components"] == counts[2] and info[3] == rinfo["largest_label"] == counts[3]
            assert counts[0] == rinfo["kept_verts"] and counts[1] == rinfo["kept_faces"]
            assert (info[1] >= 1 and info[2] >= 1) if len(faces) else (info[1] == 0 and info[2] == 0)
            assert info[1] <= nv + 2
            got[fill] = (labels, v2, f2, vm)
            sweeps = info[1]
        for a, b in zip(got["ff"], got["rand"]):
            assert torch.equal(a, b)
    # the Python surface
    labels, info = MC.components(torch.from_numpy(faces).to(gpu), nv)
    assert labels.dtype == torch.int32 and torch.equal(labels.cpu(), torch.from_numpy(ref_labels))
    assert info["n_components"] == ref_info["n_components"] and info["sweeps"] <= nv + 2
    col = np.random.RandomState(1).randint(0, 256, size=(nv, 3)).astype(np.uint8)
    v2, f2, dinfo = MC.filter_components(verts, faces, keeps[0], colors=col)
    rv, rf, rinfo = MC.filter_components_oracle(verts, faces, keeps[0], colors=col)
    assert torch.equal(v2.cpu(), torch.from_numpy(rv).reshape(-1, 3)) and torch.equal(f2.cpu(), torch.from_numpy(rf).reshape(-1, 3))
    assert torch.equal(dinfo["vert_map"].cpu(), torch.from_numpy(rinfo["vert_map"]))
    assert torch.equal(dinfo["colors"].cpu(), torch.from_numpy(rinfo["colors"]).reshape(-1, 3))
    for k in ("kept_verts", "removed_verts", "kept_faces", "removed_faces", "n_components", "largest_label"):
        assert dinfo[k] == rinfo[k], k
    return sweeps


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1023, 8191])
def test_strips(hip, gpu, n):
    """one strip of n triangles (i, i+1, i+2): vertices renumbered by the identity, the reversal and a random permutation, faces
    in order and shuffled -- around the wave (64), the block (256), the scan block (1024) and many blocks"""
    base, nv = strips([n], interleave=False)
    rs = np.random.RandomState(n)
    for pname, perm in (("identity", np.arange(nv)), ("reversed", np.arange(nv)[::-1].copy()), ("random", rs.permutation(nv))):
        for order in ("in_order", "shuffled"):
            f = perm[base]
            if order == "shuffled":
                f = f[rs.permutation(len(f))]
            sweeps = check_case(hip, gpu, f, nv, keeps=("largest",))
            print(f"strip n={n} {pname} {order}: {sweeps} sweeps")


def test_eight_strips_ties_at_every_rank(hip, gpu):
    f, nv = strips([5, 5, 64, 64, 65, 1, 300, 300])
    check_case(hip, gpu, f, nv, keeps=("largest", 1, 5, 6, 64, 65, 66, 300, 301))
    rs = np.random.RandomState(8)
    check_case(hip, gpu, rs.permutation(nv)[f][rs.permutation(len(f))], nv, keeps=("largest", 64, 65, 300))


@pytest.mark.parametrize("name", sorted(HAND_CASES))
def test_hand_cases(hip, gpu, name):
    faces, nv, want, ncomp = HAND_CASES[name]
    check_case(hip, gpu, faces, nv, keeps=("largest", 1, 2))
    labels, info = MC.components(np.asarray(faces, np.int64).reshape(-1, 3), nv)
    assert labels.cpu().tolist() == want and info["n_components"] == ncomp


def test_a_face_index_outside_the_mesh_raises(hip, gpu):
    good = [[0, 1, 2], [2, 3, 4]]
    for bad in (5, -1):
        f = torch.tensor(good + [[0, 1, bad]], dtype=torch.int32, device=gpu)
        with pytest.raises(hip.HipError):
            MC.components(f, 5)
        with pytest.raises(hip.HipError):
            MC.filter_components(np.zeros((5, 3)), f, "largest")
    with pytest.raises(hip.HipError):                         # faces of a mesh without vertices
        MC.components(torch.tensor(good, dtype=torch.int32, device=gpu), 0)
    labels, _ = MC.components(torch.tensor(good, dtype=torch.int32, device=gpu), 5)      # (and the context still works)
    assert labels.cpu().tolist() == [0, 0, 0, 0, 0]


def _ball(n, centre, radius):
    ax = torch.arange(n, dtype=torch.float32)
    g = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1)
    return radius - (g - torch.tensor(centre, dtype=torch.float32)).norm(dim=-1)


def test_filter_of_a_marching_cubes_cube_removes_the_floater(hip, gpu):
    """40^3 sigma cubes: A = a ball of radius 9; B = the same ball and a ball of radius 3 in a far corner (no shared cell).
    Order-preserving compaction of a row-major emission: the largest component of B's mesh IS A's mesh."""
    from transhuman_amd.mesh import Mesh
    a = _ball(40, (19.3, 20.1, 19.7), 9.0)
    b = torch.maximum(a, _ball(40, (33.2, 33.4, 32.9), 3.0))
    scale, origin = (0.005, 0.006, 0.007), (-0.4, 0.25, 2.6)
    va, fa = hip.marching_cubes(a.to(gpu), 0.0, scale=scale, origin=origin)
    vb, fb = hip.marching_cubes(b.to(gpu), 0.0, scale=scale, origin=origin)
    assert vb.shape[0] > va.shape[0] > 500 and fb.shape[0] > fa.shape[0]
    labels, info = MC.components(fb, vb.shape[0])
    assert info["n_components"] == 2 and info["largest_faces"] == fa.shape[0]
    v1, f1, i1 = MC.filter_components(vb, fb, "largest")
    assert torch.equal(v1, va) and torch.equal(f1, fa)
    assert i1["removed_verts"] == vb.shape[0] - va.shape[0] and i1["removed_faces"] == fb.shape[0] - fa.shape[0]
    v2, f2, i2 = MC.filter_components(vb, fb, 1)                       # both balls survive
    assert torch.equal(v2, vb) and torch.equal(f2, fb) and i2["removed_verts"] == 0
    m = Mesh(vb, fb.to(torch.int64)).largest_component()
    assert m.is_watertight and m.faces.dtype == torch.int64
    assert torch.equal(m.vertices, va) and torch.equal(m.faces, fa.to(torch.int64))
    rl, _ = MC.components_oracle(fb.cpu().numpy(), vb.shape[0])
    assert torch.equal(labels.cpu(), torch.from_numpy(rl))


def test_renderer_option_keeps_the_largest_component(hip, gpu):
    """the synthetic 32^3 grid of test_sigma_grid_32: cfg.mesh_components = "largest" returns filter_components of the default
    call's mesh; the default call and its cube are what they were"""
    from transhuman_amd import synth
    from transhuman_amd.config import get_cfg, override
    from transhuman_amd.networks.renderer import if_mesh_renderer
    from util import make_net, synth_assign, can64
    cfg = get_cfg()
    cfg.N_samples, cfg.num_class = 32, 300
    bc = synth.make_batch(64, 64, 3, seed=0)
    bc["pts"] = synth.make_grid_pts(bc, 32)
    b = synth.batch_to(bc, gpu)
    r = if_mesh_renderer.Renderer(make_net(12).to(gpu), vertex_can=can64().numpy(), pc2voxel_ind=synth_assign(300))
    with override(mesh_th=0.5):                              # (the synthetic weights' sigma_raw is O(1))
        base = r.render(b)
        with override(mesh_components="largest"):
            big = r.render(b)
        with override(mesh_components=1):
            every = r.render(b)
    assert set(base) == {"cube", "mesh"} and base["mesh"].vertex_colors is None and base["mesh"].faces.shape[0] > 100
    assert np.array_equal(base["cube"], big["cube"]) and np.array_equal(base["cube"], every["cube"])
    v, f, info = MC.filter_components(base["mesh"].vertices, base["mesh"].faces, "largest")
    assert torch.equal(big["mesh"].vertices, v) and torch.equal(big["mesh"].faces, f.to(torch.int64))
    assert torch.equal(every["mesh"].vertices, base["mesh"].vertices) and torch.equal(every["mesh"].faces, base["mesh"].faces)
    print(f"32^3 grid mesh: {info['n_components']} components, {info['kept_faces']} of {base['mesh'].faces.shape[0]} faces kept")
