"""CPU: the training targets of a step (transhuman_amd/train_targets.py, K18).  ``sample_patch_rays_oracle`` restates the train split
of the reference's sample_ray_patch (lib/utils/if_nerf/if_nerf_data_utils.py:445-499) on dense per-pixel rays; it is held here
  * to the reference's own outputs (tests/golden/g22_patch_rays.npz, tools/gen_golden_patch_rays.py: the reference's function with
    its two random calls fed from recorded draws), bit for bit, in every output of all four cases, and
  * to an independent formulation (np.argwhere for the centres, a full-image window mask and np.cumsum for the rays, the way the
    reference's helpers are written) on random masks and draws.
Everything is selection and copying, so every comparison is exact.  tests/test_gpu_train_targets.py holds the device to the
restatement.  Also: the C-ABI surface of the new entry points and the new configuration defaults, which need no device."""
import ctypes
import os

import numpy as np
import pytest

from transhuman_amd import train_targets as tt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "g22_patch_rays.npz")
ONE = 1.0 - 2.0 ** -53
CASES = ("axis_p8", "axis_p5", "oblique_p8", "wide_p20")
OUTPUTS = ("rgb", "ray_o", "ray_d", "near", "far", "sub_mask", "patch_masks", "patch_masks_sub", "target_patches", "patch_div_indices")


def golden_case(g, name):
    """(inputs of sample_patch_rays_oracle, the reference's outputs) of one fixture case"""
    f = lambda k: g[f"{name}_{k}"]
    dense = dict(ray_o=f("dense_ray_o"), ray_d=f("dense_ray_d"), near=f("dense_near"), far=f("dense_far"), mask_at_box=f("dense_mask"))
    args = dict(img=f("img"), msk=f("msk"), bound_mask=f("bound_mask"), dense_rays=dense, draws=g["draws"], patch_size=int(f("P")),
                subject_ratio=float(g["subject_ratio"]))
    return args, {k: f(k) for k in OUTPUTS}


def assert_same(got, want, keys=None):
    for k in (want if keys is None else keys):
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape, (k, a.dtype, b.dtype, a.shape, b.shape)
        assert np.array_equal(a, b), k


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def test_fixture_holds_the_cases_it_was_made_for(gold):
    assert tuple(gold["names"]) == CASES
    assert np.array_equal(gold["draws"], [[0.9, 0], [0.9, ONE], [0.1, 0], [0.1, ONE], [0.5, 0.37], [0.5, 0.37]])
    want = {"axis_p8": [16, 25, 48, 40, 48, 48], "axis_p5": [9, 9, 25, 15, 25, 25], "oblique_p8": [32, 64, 56, 64, 64, 64]}
    for name, counts in want.items():
        assert np.diff(gold[f"{name}_patch_div_indices"]).tolist() == counts
    H, W = gold["oblique_p8_HW"]
    assert (H * W) % 256 != 0


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_reference(gold, name):
    args, want = golden_case(gold, name)
    got = tt.sample_patch_rays_oracle(**args)
    assert_same(got, want)
    # what the reference does not return: the windows and the indices into its masked ray list
    P = args["patch_size"]
    assert np.array_equal(got["xy_max"], got["xy_min"] + P)
    compact = {k: args["dense_rays"][k][args["dense_rays"]["mask_at_box"]] for k in ("ray_o", "ray_d", "near", "far")}
    for k, v in compact.items():
        assert np.array_equal(v[got["select_inds"]], want[k]), k                   # :347-353 select_rays
    for i, (x, y) in enumerate(got["xy_min"]):
        assert np.array_equal(want["target_patches"][i], args["img"][y:y + P, x:x + P])


def independent(img, msk, bound, dense, draws, P, ratio):
    """the same targets, written the way the reference's helpers are (:287-443): np.argwhere for the centre, a full-image window
    mask intersected with the masks, np.where for the ray order, np.cumsum for select_inds, the masked ray list indexed by it"""
    H, W = msk.shape
    ray_mask = np.asarray(dense["mask_at_box"]).reshape(-1).astype(bool)
    human = (msk.astype(np.uint8) * bound.astype(np.uint8)) > 0
    bbox_minus = np.bitwise_and(ray_mask.reshape(H, W), np.bitwise_not(human))
    lists = {k: np.asarray(dense[k])[ray_mask] for k in ("ray_o", "ray_d", "near", "far")}
    lists["rgb"], lists["sub_mask"] = img.reshape(-1, 3)[ray_mask], human.reshape(-1, 1)[ray_mask]
    inds, masks, subs, mins, centres, div = [], [], [], [], [], [0]
    for u0, u1 in draws:
        pts = np.argwhere(human if u0 < ratio else bbox_minus)
        cy, cx = pts[min(int(np.floor(u1 * float(len(pts)))), len(pts) - 1)]
        x0, y0 = min(max(cx - P // 2, 0), W - P), min(max(cy - P // 2, 0), H - P)
        sel = np.zeros((H, W), bool)
        sel[y0:y0 + P, x0:x0 + P] = True
        inter = sel.reshape(-1) & ray_mask
        inds.append((np.cumsum(ray_mask) - 1)[np.where(inter)])
        masks.append(inter.reshape(H, W)[y0:y0 + P, x0:x0 + P])
        subs.append((sel & human)[y0:y0 + P, x0:x0 + P])
        mins.append([x0, y0])
        centres.append([cx, cy])
        div.append(div[-1] + len(inds[-1]))
    inds = np.concatenate(inds)
    out = {k: v[inds] for k, v in lists.items()}
    out.update(patch_masks=np.stack(masks), patch_masks_sub=np.stack(subs), select_inds=inds, xy_min=np.asarray(mins, np.int64),
               target_patches=np.stack([img[y:y + P, x:x + P] for x, y in mins]), patch_div_indices=np.asarray(div, np.int64))
    return out, np.asarray(centres)


def random_case(H, W, N, seed, density=0.5):
    rs = np.random.RandomState(seed)
    img = rs.uniform(size=(H, W, 3)).astype(np.float32)
    msk = rs.choice(np.array([0, 1, 100, 7], np.uint8), size=(H, W), p=[1 - density, density * 0.6, density * 0.3, density * 0.1])
    bound = (rs.uniform(size=(H, W)) < 0.8).astype(np.uint8)
    dense = dict(ray_o=rs.normal(size=(H * W, 3)).astype(np.float32), ray_d=rs.normal(size=(H * W, 3)).astype(np.float32),
                 near=rs.uniform(size=H * W).astype(np.float32), far=rs.uniform(size=H * W).astype(np.float32),
                 mask_at_box=rs.uniform(size=H * W) < 0.7)
    draws = rs.uniform(size=(N, 2))
    draws[:4] = np.array([[0.1, 0.0], [0.1, ONE], [0.95, 0.0], [0.95, ONE]])[:N]
    return img, msk, bound, dense, draws


@pytest.mark.parametrize("H,W,P,N,seed", [(37, 29, 8, 64, 0), (16, 16, 16, 8, 1), (23, 41, 5, 64, 2), (64, 48, 1, 16, 3),
                                           (30, 70, 20, 64, 4)])
def test_restatement_equals_an_independent_formulation(H, W, P, N, seed):
    img, msk, bound, dense, draws = random_case(H, W, N, seed)
    want, centres = independent(img, msk, bound, dense, draws, P, 0.8)
    got = tt.sample_patch_rays_oracle(img, msk, bound, dense, draws, patch_size=P, subject_ratio=0.8)
    assert_same(got, want)
    if (H, W, P) == (37, 29, 8):
        # the case exercises what it is here for: H W is no multiple of 256, windows clipped at all four image borders
        assert (H * W) % 256 != 0
        lo, hi = centres - P // 2 < 0, centres - P // 2 > np.array([W - P, H - P])
        assert lo[:, 0].any() and lo[:, 1].any() and hi[:, 0].any() and hi[:, 1].any()
        assert (got["xy_min"] >= 0).all() and (got["xy_max"] <= [W, H]).all()


def test_overlapping_patches_repeat_their_rays():
    img, msk, bound, dense, draws = random_case(20, 20, 2, 5)
    draws[1] = draws[0]
    got = tt.sample_patch_rays_oracle(img, msk, bound, dense, draws, patch_size=6, subject_ratio=0.8)
    a, b, c = got["patch_div_indices"]
    assert b - a == c - b and np.array_equal(got["select_inds"][a:b], got["select_inds"][b:c])


def test_empty_candidate_set_raises_value_error():
    img, msk, bound, dense, draws = random_case(12, 12, 2, 6)
    with pytest.raises(ValueError, match="empty"):
        tt.sample_patch_rays_oracle(img, np.zeros_like(msk), bound, dense, np.array([[0.1, 0.5]]), patch_size=4, subject_ratio=0.8)
    dense["mask_at_box"] = np.zeros(144, bool)
    with pytest.raises(ValueError, match="empty"):
        tt.sample_patch_rays_oracle(img, msk, bound, dense, np.array([[0.9, 0.5]]), patch_size=4, subject_ratio=0.8)
    # counts read back from the device with an empty set: the same error
    with pytest.raises(ValueError, match="empty"):
        tt.assemble({}, np.array([[5, 0], [3, 0]]))


@pytest.mark.parametrize("H,W,N,P", [(12, 12, 2, 0), (12, 12, 2, 13), (80, 70, 2, 65), (12, 12, 0, 4), (12, 12, 65, 4), (4097, 8, 1, 4),
                                      (8, 4097, 1, 4), (12, 7, 1, 8)])
def test_argument_limits_are_refused(H, W, N, P):
    with pytest.raises(ValueError):
        tt.check_limits(H, W, N, P)
    if H * W < 10000:
        img, msk, bound, dense, _ = random_case(H, W, 1, 0)
        with pytest.raises(ValueError):
            tt.sample_patch_rays_oracle(img, msk, bound, dense, np.full((N, 2), 0.5), patch_size=P, subject_ratio=0.8)
        # the device entry refuses them before it asks for a device
        with pytest.raises(ValueError):
            tt.sample_patch_rays(img, msk, np.eye(3), np.eye(3), np.zeros((3, 1)), np.zeros((2, 3)), draws=np.full((N, 2), 0.5),
                                 patch_size=P, subject_ratio=0.8)


def test_limits_themselves_are_accepted():
    tt.check_limits(4096, 4096, 64, 64)
    tt.check_limits(1, 1, 1, 1)


def test_draws_outside_the_unit_interval_are_refused():
    img, msk, bound, dense, _ = random_case(12, 12, 1, 0)
    for bad in ([[1.0, 0.5]], [[0.5, -0.1]], [[0.5, float("nan")]], [[0.5]]):
        with pytest.raises(ValueError):
            tt.sample_patch_rays_oracle(img, msk, bound, dense, np.array(bad), patch_size=4, subject_ratio=0.8)


@pytest.fixture(scope="module")
def lib():
    from transhuman_amd import build, hip
    build.build(force=False, verbose=False)
    return hip.load_library()


def test_patch_entry_points_declared_exported_bound(lib):
    from transhuman_amd import hip
    C = ctypes
    header = open(os.path.join(ROOT, "include", "transhuman_hip.h")).read()
    raw = ctypes.CDLL(os.path.join(ROOT, "transhuman_amd", "libtranshuman_hip.so"))
    for name in ("th_patch_rays", "th_patch_workspace_bytes"):
        assert f"{name}(" in header
        assert hasattr(raw, name)
        assert name in hip.SYMBOLS
    assert hip.SYMBOLS["th_patch_workspace_bytes"] == (C.c_size_t, [C.c_int, C.c_int])
    res, args = hip.SYMBOLS["th_patch_rays"]
    # ctx + 8 inputs, 2 strides, H, W, draws, subject_ratio, N, P, 12 outputs + workspace, its size, the stream
    assert res is C.c_int and args == [C.c_void_p] * 9 + [C.c_longlong] * 2 + [C.c_int] * 2 + [C.c_void_p, C.c_double] + \
        [C.c_int] * 2 + [C.c_void_p] * 13 + [C.c_size_t, C.c_void_p]
    decl = header[header.index("int th_patch_rays("):]
    decl = decl[:decl.index(";")]
    assert decl.count(",") + 1 == len(args)
    assert lib.th_abi_version() == 12


def test_patch_workspace_query_and_refusals_need_no_device(lib):
    # three rows of per-block prefixes and one 64-bit ballot per wave of 64 pixels
    nb = 512 * 512 // 256
    assert lib.th_patch_workspace_bytes(512, 512) >= 3 * (nb + 1) * 4 + nb * 4 * 8
    assert lib.th_patch_workspace_bytes(1, 1) > 0 and lib.th_patch_workspace_bytes(4096, 4096) > 0
    assert lib.th_patch_workspace_bytes(4097, 8) == 0 and lib.th_patch_workspace_bytes(8, 0) == 0
    assert lib.th_patch_rays(*([None] * 9), 3, 1, 8, 8, None, 0.8, 1, 4, *([None] * 13), 0, None) != 0
    assert b"null" in lib.th_last_error()


def test_configuration_defaults():
    from transhuman_amd.config import _defaults
    d = _defaults()
    assert d.target_prep == "batch"
    assert (d.patch.N_patches, d.patch.size, d.patch.sample_subject_ratio, d.patch.use_patch_sampling) == (6, 20, 0.8, True)
