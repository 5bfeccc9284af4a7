"""CPU: the dataset's other targets (transhuman_amd/train_targets.py, K26).  ``sample_rays_h36m_oracle`` restates the reference's
sample_ray_h36m (lib/utils/if_nerf/if_nerf_data_utils.py:516-614), both splits, on dense per-pixel rays; it is held here to the
reference's own outputs (tests/golden/g26_ray_sample.npz, tools/gen_golden_ray_sample.py: the reference's function with
np.random.randint fed from recorded draws), bit for bit, in every key of every case.  ``get_acc_oracle`` restates cv2.dilate with a
25 x 25 kernel of ones read at the coordinates (:635-641); cv2 is absent, it is cross-checked against scipy's maximum filter.
Everything is selection and copying, so every comparison is exact.  tests/test_gpu_ray_sample.py holds the device to the
restatement.  Also: the three ValueErrors of the train loop, how ``add_targets`` routes under cfg.target_sampler, and the new
configuration defaults, which need no device."""
import os

import numpy as np
import pytest
import torch

from transhuman_amd import train_targets as tt
from transhuman_amd.config import get_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "g26_ray_sample.npz")
ONE = 1.0 - 2.0 ** -53
CASES = ("one_iter", "two_iters", "three_iters", "face", "empty_body", "empty_rand", "nrays_1")
VIEWS = ("axis", "oblique", "inside")
RAY_KEYS = ("rgb", "ray_o", "ray_d", "near", "far", "coord", "mask_at_box")
ITERS = dict(one_iter=1, two_iters=2, three_iters=3, face=1, empty_body=2, empty_rand=2, nrays_1=1)


def golden_view(g, view):
    """(img, bound_mask, dense_rays, the reference's test split) of one fixture view"""
    f = lambda k: g[f"view_{view}_{k}"]
    dense = dict(ray_o=f("dense_ray_o"), ray_d=f("dense_ray_d"), near=f("dense_near"), far=f("dense_far"), mask_at_box=f("dense_mask"))
    return f("img"), f("bound_mask"), dense, {k: f(f"test_{k}") for k in RAY_KEYS}


def golden_case(g, name):
    """(inputs of sample_rays_h36m_oracle, the reference's train split) of one fixture case"""
    f = lambda k: g[f"{name}_{k}"]
    img, bound, dense, _ = golden_view(g, str(f("view")))
    args = dict(img=img, msk=f("msk"), bound_mask=bound, dense_rays=dense, split="train", nrays=int(f("nrays")), draws=f("draws"),
                body_ratio=float(f("body_ratio")), face_ratio=float(f("face_ratio")))
    return args, {k: f(k) for k in RAY_KEYS}


def assert_same(got, want, keys=None):
    for k in (want if keys is None else keys):
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape, (k, a.dtype, b.dtype, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), k


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def test_fixture_holds_the_cases_it_was_made_for(gold):
    assert tuple(gold["names"]) == CASES and tuple(gold["views"]) == VIEWS
    assert os.path.getsize(GOLD) < 300 * 1024
    assert all(max(gold[f"view_{v}_HW"][0], gold[f"view_{v}_HW"][1]) <= 96 for v in VIEWS)
    assert {int(gold[f"{n}_iters"]) for n in CASES} >= {1, 2, 3}
    assert int(gold["nrays_1_nrays"]) == 1 and float(gold["face_face_ratio"]) > 0
    for name in ("empty_body", "empty_rand"):                                   # the final count is nrays + 1
        assert gold[f"{name}_rgb"].shape[0] == int(gold[f"{name}_nrays"]) + 1
    # the reference's coord is int64 except where both fallbacks (two uint8 arrays) are all an iteration offers
    assert {n: str(gold[f"{n}_coord_dtype"]) for n in CASES} == {n: "uint8" if n == "empty_rand" else "int64" for n in CASES}
    used = gold["one_iter_draws"][0, :, :int(gold["one_iter_nrays"]) // 2]
    assert (used[[0, 2]] == 0.0).any(1).all() and (used[[0, 2]] == ONE).any(1).all()


@pytest.mark.parametrize("name", CASES)
def test_train_split_equals_the_reference(gold, name):
    args, want = golden_case(gold, name)
    got = tt.sample_rays_h36m_oracle(**args)
    assert_same(got, want)
    assert got["iters"] == int(gold[f"{name}_iters"]) == ITERS[name] <= tt.MAX_ITERS
    assert got["acc"].dtype == np.uint8 and got["acc"].shape == (want["rgb"].shape[0],)
    assert np.array_equal(got["acc"], tt.get_acc_oracle(want["coord"], args["msk"]))
    m = args["msk"] * args["bound_mask"]
    picked = m[want["coord"][:, 0], want["coord"][:, 1]]
    if name == "face":
        assert (picked == 13).sum() == int(args["nrays"] * args["face_ratio"]) > 0
    if name == "empty_body":
        assert not (m == 1).any() and want["coord"][0].tolist() == [1, 1]
    if name == "empty_rand":
        assert not ((args["bound_mask"] == 1) & (m != 100)).any() and want["coord"].tolist() == [[1, 1], [0, 0]] * 2


@pytest.mark.parametrize("view", VIEWS)
def test_test_split_equals_the_reference(gold, view):
    img, bound, dense, want = golden_view(gold, view)
    msk = np.zeros(bound.shape, np.uint8)
    msk[5, 7] = 1
    got = tt.sample_rays_h36m_oracle(img, msk, bound, dense, "test")
    assert_same(got, want)
    n = want["rgb"].shape[0]
    assert 0 < n == int(dense["mask_at_box"].sum()) and want["mask_at_box"].shape == (bound.size,)
    # coord is all zeros, so acc is get_acc at (0, 0) repeated (the reference's behaviour): the window [0, 12] x [0, 12] holds (5, 7)
    assert got["acc"].dtype == np.uint8 and got["acc"].tolist() == [1] * n
    msk[:] = 0
    msk[13, 0] = msk[0, 13] = 255
    assert tt.sample_rays_h36m_oracle(img, msk, bound, dense, "test")["acc"].tolist() == [0] * n


def _filter_acc(coord, msk):
    from scipy.ndimage import maximum_filter
    dil = maximum_filter(msk, size=25, mode="constant", cval=0)
    return (dil[coord[:, 0], coord[:, 1]] != 0).astype(np.uint8)


def border_coords(H, W):
    """every pixel of the four borders, and a grid inside"""
    ys, xs = np.mgrid[0:H, 0:W]
    edge = (ys == 0) | (ys == H - 1) | (xs == 0) | (xs == W - 1) | ((ys % 5 == 2) & (xs % 7 == 3))
    return np.argwhere(edge).astype(np.int64)


@pytest.mark.parametrize("H,W", [(40, 56), (13, 30), (25, 26), (2, 2), (64, 12)])
def test_get_acc_equals_the_maximum_filter(H, W):
    rs = np.random.RandomState(H * 100 + W)
    coord = border_coords(H, W)
    msks = [np.zeros((H, W), np.uint8)]                                         # empty
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):               # the only nonzero pixel in a corner
        m = np.zeros((H, W), np.uint8)
        m[y, x] = rs.randint(1, 256)
        msks.append(m)
    for density in (0.002, 0.02, 0.5):
        msks.append((rs.uniform(size=(H, W)) < density).astype(np.uint8) * rs.randint(1, 256, size=(H, W)).astype(np.uint8))
    for i, m in enumerate(msks):
        got = tt.get_acc_oracle(coord, m)
        assert got.dtype == np.uint8 and got.shape == (coord.shape[0],)
        assert np.array_equal(got, _filter_acc(coord, m)), i
    assert not tt.get_acc_oracle(coord, msks[0]).any()
    if H > 13 and W > 13:
        assert 0 < tt.get_acc_oracle(coord, msks[1]).sum() < coord.shape[0]
    assert tt.get_acc_oracle(np.zeros((0, 2), np.int64), msks[1]).shape == (0,)
    with pytest.raises(ValueError):
        tt.get_acc_oracle(np.array([[H, 0]]), msks[1])


def unfinished_draws(args):
    """draws [MAX_ITERS,3,16] for nrays = 16, body_ratio = 0: half of every iteration's picks land on a rand_set pixel whose ray
    misses the box (16 -> 8 -> 4 -> 2 -> 1 rays missing), so the loop is unfinished after MAX_ITERS = 4"""
    m = args["msk"] * args["bound_mask"]
    rand = np.flatnonzero(((args["bound_mask"] == 1) & (m != 100)).reshape(-1))
    in_box = np.asarray(args["dense_rays"]["mask_at_box"]).reshape(-1)[rand]
    hit, off = np.flatnonzero(in_box)[0], np.flatnonzero(~in_box)[0]
    draws = np.full((tt.MAX_ITERS, 3, 16), (hit + 0.5) / rand.size)
    for i in range(tt.MAX_ITERS):
        draws[i, 2, :8 >> i] = (off + 0.5) / rand.size
    return draws


def test_the_three_value_errors(gold):
    args, _ = golden_case(gold, "two_iters")
    # an iteration that adds nothing: every pick lands on a rand_set pixel whose ray misses the box
    m = args["msk"] * args["bound_mask"]
    rand = np.flatnonzero(((args["bound_mask"] == 1) & (m != 100)).reshape(-1))
    off = np.flatnonzero(~args["dense_rays"]["mask_at_box"][rand])
    assert off.size > 0
    draws = np.full((tt.MAX_ITERS, 3, 8), (off[0] + 0.5) / rand.size)
    with pytest.raises(ValueError, match="added nothing"):
        tt.sample_rays_h36m_oracle(**{**args, "nrays": 8, "draws": draws, "body_ratio": 0.0})
    draws = unfinished_draws(args)
    with pytest.raises(ValueError, match="unfinished after MAX_ITERS"):
        tt.sample_rays_h36m_oracle(**{**args, "nrays": 16, "draws": draws, "body_ratio": 0.0})
    draws[3, 2, 0] = draws[3, 2, 1]                                             # ... and ends in the fourth when that one hits
    assert tt.sample_rays_h36m_oracle(**{**args, "nrays": 16, "draws": draws, "body_ratio": 0.0})["iters"] == 4
    # H < 2 or W < 2
    for H, W in ((1, 8), (8, 1)):
        dense = dict(ray_o=np.zeros((H * W, 3), np.float32), ray_d=np.ones((H * W, 3), np.float32), near=np.zeros(H * W, np.float32),
                     far=np.ones(H * W, np.float32), mask_at_box=np.ones(H * W, bool))
        small = dict(img=np.zeros((H, W, 3), np.float32), msk=np.ones((H, W), np.uint8), bound_mask=np.ones((H, W), np.uint8),
                     dense_rays=dense, nrays=2, draws=np.zeros((tt.MAX_ITERS, 3, 2)))
        with pytest.raises(ValueError, match="H, W >= 2"):
            tt.sample_rays_h36m_oracle(split="train", **small)
        assert tt.sample_rays_h36m_oracle(split="test", **small)["rgb"].shape == (H * W, 3)
    # and the argument checks
    for bad in (dict(nrays=0), dict(nrays=tt.MAX_RAYS + 1), dict(body_ratio=0.7, face_ratio=0.4), dict(body_ratio=-0.1),
                dict(draws=args["draws"][:3]), dict(draws=np.ones_like(args["draws"])), dict(split="val")):
        with pytest.raises(ValueError):
            tt.sample_rays_h36m_oracle(**{**args, **bad})


def test_config_defaults():
    cfg = get_cfg()
    assert cfg.target_sampler == "patch" and cfg.target_prep == "batch"
    assert cfg.N_rand == 1024 and cfg.body_sample_ratio == 0.5 and cfg.face_sample_ratio == 0.0
    assert tt._h36m_cfg(None, None, None) == (1024, 0.5, 0.0)
    assert tt.H36M_KEYS == ("rgb", "ray_o", "ray_d", "near", "far", "acc", "mask_at_box") and tt.MAX_ITERS == 4


def _batch():
    z = torch.zeros
    return dict(target_img=z(1, 8, 8, 3), target_msk=z(1, 8, 8, dtype=torch.uint8), target_K=z(1, 3, 3), target_R=z(1, 3, 3),
                target_T=z(1, 3, 1), can_bounds=z(1, 2, 3))


def test_add_targets_routes_by_sampler_and_split(monkeypatch):
    calls = []
    patch_out = {k: torch.zeros(2) for k in tt.REFERENCE_KEYS}
    ray_out = {k: torch.ones(3) for k in tt.H36M_KEYS + ("coord",)}
    monkeypatch.setattr(tt, "sample_patch_rays", lambda *a, **kw: calls.append(("patch", kw)) or patch_out)
    monkeypatch.setattr(tt, "sample_rays_h36m", lambda *a, **kw: calls.append((a[6], kw)) or ray_out)
    cfg = get_cfg()
    try:
        # "patch" (the default): as before K26, whatever split says
        for split in (None, "train", "test"):
            b = tt.add_targets(_batch(), split) if split else tt.add_targets(_batch())
            assert calls.pop()[0] == "patch" and not calls and all(b[k].shape == (1, 2) for k in tt.REFERENCE_KEYS) and "acc" not in b
        cfg.patch.use_patch_sampling = False
        with pytest.raises(ValueError, match="makes the patch targets only: cfg.patch.use_patch_sampling is false"):
            tt.add_targets(_batch())
        with pytest.raises(ValueError, match="use_patch_sampling"):
            tt.add_targets({**_batch(), "ray_o": torch.zeros(1, 1, 3)}, "test")
        assert not calls
        # "dataset": what the reference's dataset makes for the split
        cfg.target_sampler = "dataset"
        for split in ("train", "test"):
            b = tt.add_targets(_batch(), split)
            assert calls.pop() == (split, dict(draws=None)) and not calls
            assert all(b[k].shape == (1, 3) for k in tt.H36M_KEYS) and "coord" not in b and "patch_masks" not in b
        with torch.no_grad():
            tt.add_targets(_batch())
        assert calls.pop()[0] == "test"
        with torch.enable_grad():
            tt.add_targets({**_batch(), "ray_draws": torch.zeros(1, 4, 3, 1024, dtype=torch.float64)})
        split, kw = calls.pop()
        assert split == "train" and kw["draws"].shape == (4, 3, 1024)
        cfg.patch.use_patch_sampling = True
        tt.add_targets(_batch(), "train")
        assert calls.pop()[0] == "patch"
        tt.add_targets(_batch(), "test")
        assert calls.pop()[0] == "test" and not calls
        # a present key is kept, a batch with ray_o is left alone, a bad value is refused
        kept = torch.full((1, 5), 7.0)
        b = tt.add_targets({**_batch(), "acc": kept}, "test")
        assert b["acc"] is kept and b["rgb"].shape == (1, 3)
        calls.clear()
        own = {**_batch(), "ray_o": torch.zeros(1, 1, 3)}
        before = dict(own)
        assert tt.add_targets(own, "test") is own and own.keys() == before.keys() and not calls
        with pytest.raises(ValueError, match="split"):
            tt.add_targets(_batch(), "val")
        with pytest.raises(ValueError, match="target view"):
            tt.add_targets({"can_bounds": torch.zeros(1, 2, 3)}, "test")
        cfg.target_sampler = "rays"
        with pytest.raises(ValueError, match="target_sampler"):
            tt.add_targets(_batch())
    finally:
        cfg.target_sampler, cfg.patch.use_patch_sampling = "patch", True
