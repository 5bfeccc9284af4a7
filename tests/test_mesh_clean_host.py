"""CPU: the definition of the mesh components and the component filter (transhuman_amd/mesh_clean.py, the numpy oracles the
device is held to), the coloured PLY layout and the two renderer options' defaults."""
import numpy as np
import pytest

from transhuman_amd import mesh_clean as MC
from transhuman_amd.mesh import Mesh, read_ply

# name -> (faces, n_verts, expected labels, expected n_components)
HAND_CASES = {
    "empty": (np.zeros((0, 3), np.int64), 0, [], 0),
    "no_faces": (np.zeros((0, 3), np.int64), 3, [0, 1, 2], 0),
    "one_triangle": ([[0, 1, 2]], 3, [0, 0, 0], 1),
    "two_disjoint": ([[0, 1, 2], [3, 4, 5]], 6, [0, 0, 0, 3, 3, 3], 2),
    "bow_tie": ([[0, 1, 2], [2, 3, 4]], 5, [0, 0, 0, 0, 0], 1),              # one shared VERTEX connects (trimesh: an edge)
    "degenerate": ([[1, 1, 3]], 4, [0, 1, 2, 1], 1),                         # a face (a, a, b)
    "duplicate": ([[2, 1, 0], [2, 1, 0], [3, 4, 5]], 6, [0, 0, 0, 3, 3, 3], 2),
    "unreferenced": ([[1, 2, 3], [5, 6, 3], [7, 8, 9]], 11, [0, 1, 1, 1, 4, 1, 1, 7, 7, 7, 10], 2),   # 0, 4 and 10 in no face
    "chain_down": ([[9, 8, 7], [7, 6, 5], [5, 4, 3]], 10, [0, 1, 2, 3, 3, 3, 3, 3, 3, 3], 1),
}


def strips(sizes, interleave=True):
    """strips of n triangles (i, i+1, i+2) each, vertex ranges one after the other; faces interleaved round-robin"""
    per, base = [], 0
    for n in sizes:
        i = np.arange(n, dtype=np.int64) + base
        per.append(np.stack([i, i + 1, i + 2], 1))
        base += n + 2
    if not interleave:
        return np.concatenate(per), base
    out, k = [], 0
    while any(k < len(p) for p in per):
        out += [p[k] for p in per if k < len(p)]
        k += 1
    return np.stack(out), base


@pytest.mark.parametrize("name", sorted(HAND_CASES))
def test_components_oracle_hand_cases(name):
    faces, nv, want, ncomp = HAND_CASES[name]
    labels, info = MC.components_oracle(faces, nv)
    assert labels.dtype == np.int32 and labels.shape == (nv,)
    assert labels.tolist() == want
    assert info["n_components"] == ncomp


def test_components_oracle_refuses_a_bad_index():
    for bad in (3, -1):
        with pytest.raises(ValueError):
            MC.components_oracle([[0, 1, bad]], 3)


def test_components_oracle_agrees_with_scipy():
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    rs = np.random.RandomState(0)
    cases = [(np.asarray(f, np.int64).reshape(-1, 3), nv) for f, nv, _, _ in HAND_CASES.values()]
    f8, nv8 = strips([5, 5, 64, 64, 65, 1, 300, 300])
    cases.append((rs.permutation(nv8)[f8], nv8))
    cases.append((rs.randint(0, 400, size=(150, 3)), 400))
    for f, nv in cases:
        labels, info = MC.components_oracle(f, nv)
        e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]]]) if len(f) else np.zeros((0, 2), np.int64)
        g = sp.coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(nv, nv))
        n, lab = connected_components(g, directed=False) if nv else (0, np.zeros(0, np.int64))
        # scipy numbers the components arbitrarily: ours is the smallest member of each
        smallest = np.full(n, nv, np.int64)
        np.minimum.at(smallest, lab, np.arange(nv))
        assert np.array_equal(labels, smallest[lab].astype(np.int32))
        assert info["n_components"] == (len(np.unique(lab[f[:, 0]])) if len(f) else 0)


def _grid_verts(nv):
    return np.arange(3 * nv, dtype=np.float64).reshape(nv, 3) * 0.25


def test_filter_largest_tie_goes_to_the_smaller_label():
    f, nv = strips([5, 7, 7, 3])
    v = _grid_verts(nv)
    v2, f2, info = MC.filter_components_oracle(v, f, "largest")
    assert info["largest_label"] == 7 and info["kept_faces"] == 7 and info["kept_verts"] == 9
    assert np.array_equal(v2, v[7:16])
    assert info["removed_faces"] == 15 and info["removed_verts"] == nv - 9 and info["n_components"] == 4
    # the same tie with the vertex ranges swapped: still the smaller label
    perm = np.arange(nv)
    perm[7:16], perm[16:25] = np.arange(16, 25), np.arange(7, 16)
    _, _, info = MC.filter_components_oracle(v, perm[f], "largest")
    assert info["largest_label"] == 7


@pytest.mark.parametrize("delta,kept", [(-1, 2), (0, 2), (1, 1)])
def test_filter_min_faces_around_a_size(delta, kept):
    f, nv = strips([5, 9, 12])                              # sizes 5, 9, 12: thresholds around 9
    _, f2, info = MC.filter_components_oracle(_grid_verts(nv), f, 9 + delta)
    assert len(np.unique(info["labels"][info["vert_map"] >= 0])) == kept
    assert info["kept_faces"] == (21 if kept == 2 else 12) == len(f2)


def test_filter_preserves_order_and_the_map_is_consistent():
    rs = np.random.RandomState(3)
    f, nv = strips([4, 30, 2, 30, 6])
    perm = rs.permutation(nv + 5)[:nv]                      # five vertices stay unreferenced
    f, nv = perm[f], nv + 5
    v = rs.randn(nv, 3)
    col = rs.randint(0, 256, size=(nv, 3)).astype(np.uint8)
    v2, f2, info = MC.filter_components_oracle(v, f, 6, colors=col, weight=np.arange(nv))
    vm = info["vert_map"]
    kept = np.nonzero(vm >= 0)[0]
    assert vm.dtype == np.int32 and np.array_equal(vm[kept], np.arange(len(kept)))      # original order, dense numbers
    assert np.array_equal(v2, v[kept]) and np.array_equal(v2[vm[kept]], v[kept])
    assert np.array_equal(info["colors"], col[kept]) and np.array_equal(info["weight"], kept)
    size = np.bincount(info["labels"][f[:, 0]], minlength=nv)
    keep_f = size[info["labels"][f[:, 0]]] >= 6
    assert np.array_equal(f2, vm[f[keep_f]]) and (f2 >= 0).all()                         # faces in order, every corner remapped
    assert np.array_equal(v2[f2], v[f[keep_f]])
    assert info["kept_faces"] == 66 and info["kept_verts"] == 32 + 32 + 8
    assert set(np.nonzero(vm < 0)[0]) >= set(np.setdiff1d(np.arange(nv), f.reshape(-1)))   # unreferenced: always dropped


def test_filter_of_a_clean_single_component_returns_it():
    f, nv = strips([17])
    v = _grid_verts(nv)
    for keep in ("largest", 1, 17):
        v2, f2, info = MC.filter_components_oracle(v, f, keep)
        assert np.array_equal(v2, v) and np.array_equal(f2, f) and f2.dtype == np.int32
        assert np.array_equal(info["vert_map"], np.arange(nv)) and info["removed_verts"] == info["removed_faces"] == 0
    v2, f2, info = MC.filter_components_oracle(v, f, 18)
    assert v2.shape == (0, 3) and f2.shape == (0, 3) and (info["vert_map"] == -1).all()


def test_filter_of_the_empty_mesh_and_bad_keep():
    v2, f2, info = MC.filter_components_oracle(np.zeros((0, 3)), np.zeros((0, 3), np.int64), "largest")
    assert v2.shape == (0, 3) and f2.shape == (0, 3) and info["largest_label"] == -1 and info["n_components"] == 0
    for bad in ("all", 2.5, True, None):
        with pytest.raises(ValueError):
            MC.filter_components_oracle(np.zeros((3, 3)), [[0, 1, 2]], bad)


# ---- PLY ----
def _expected_uncoloured(v, f):
    """the file Mesh.export wrote before colours existed, built here byte by byte"""
    header = ("ply\nformat binary_little_endian 1.0\ncomment transhuman_amd marching cubes\n"
              f"element vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n"
              f"element face {len(f)}\nproperty list uchar int vertex_indices\nend_header\n").encode("ascii")
    body = np.asarray(v, "<f4").tobytes()
    for t in f:
        body += b"\x03" + np.asarray(t, "<i4").tobytes()
    return header + body


def test_uncoloured_export_is_byte_identical(tmp_path):
    rs = np.random.RandomState(1)
    v, f = rs.randn(7, 3), rs.randint(0, 7, size=(5, 3))
    p = Mesh(v, f).export(str(tmp_path / "a.ply"))
    assert open(p, "rb").read() == _expected_uncoloured(v, f)
    assert Mesh(v, f).vertex_colors is None
    out = read_ply(p)
    assert len(out) == 2 and np.array_equal(out[1], f)
    v3, f3, c3 = read_ply(p, colors=True)
    assert c3 is None and np.array_equal(v3, v.astype(np.float32))


def test_coloured_export_round_trips(tmp_path):
    rs = np.random.RandomState(2)
    v, f = rs.randn(9, 3), rs.randint(0, 9, size=(4, 3))
    col = rs.randint(0, 256, size=(9, 3)).astype(np.uint8)
    p = Mesh(v, f, vertex_colors=col).export(str(tmp_path / "c.ply"))
    raw = open(p, "rb").read()
    head = raw[:raw.index(b"end_header\n") + 11].decode("ascii")
    assert ("property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\n"
            "element face") in head
    assert len(raw) == len(head) + 9 * 16 + 4 * 13
    rec = np.frombuffer(raw[len(head):len(head) + 9 * 16], dtype=[("xyz", "<f4", (3,)), ("rgba", "u1", (4,))])
    assert (rec["rgba"][:, 3] == 255).all()
    out = read_ply(p)
    assert len(out) == 2 and np.array_equal(out[0], v.astype(np.float32)) and np.array_equal(out[1], f)
    v3, f3, c3 = read_ply(p, colors=True)
    assert c3.dtype == np.uint8 and np.array_equal(c3, col) and np.array_equal(v3, out[0]) and np.array_equal(f3, f)
    with pytest.raises(ValueError):
        Mesh(v, f, vertex_colors=col[:5]).export(str(tmp_path / "bad.ply"))


def test_renderer_options_default_to_the_reference_behaviour():
    from transhuman_amd.config import TRAIN_SWITCHES, _defaults, get_cfg
    d = _defaults()
    assert d.mesh_components == "all" and d.mesh_colors == "none"
    assert get_cfg().mesh_components == "all" and get_cfg().mesh_colors == "none"
    assert "mesh_components" not in TRAIN_SWITCHES and "mesh_colors" not in TRAIN_SWITCHES
