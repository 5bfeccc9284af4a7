"""GPU: the dataset's other targets made on the device (csrc/k_raysample.hip, transhuman_amd/train_targets.py, K26):
sample_ray_h36m's two splits and get_acc.  The stage only selects and copies, so every comparison here is bit for bit: K26 through
the C ABI against the reference's own outputs (tests/golden/g26_ray_sample.npz, fed the fixture's dense rays) and against the
numpy restatement on synthetic dense arrays (image sizes around the 256-pixel block, ray counts around the 1024-lane loop, class
sizes around one block, picks at block edges, both image layouts and a strided image, dirty outputs and workspace),
``sample_rays_h36m`` end to end against the restatement fed the device's own dense rays and bound mask (parity of those with the
reference is what the K9 tests pin), determinism, the error returns, and the renderer under cfg.target_sampler == "dataset"."""
import numpy as np
import pytest
import torch

from transhuman_amd.config import get_cfg
from test_ray_sample_host import CASES, GOLD, ONE, VIEWS, border_coords, golden_case, golden_view, unfinished_draws

pytestmark = pytest.mark.gpu
ROWS = ("rgb", "ray_o", "ray_d", "near", "far", "coord")
ALL_KEYS = ROWS + ("mask_at_box", "acc")
NRAYS = (1, 2, 63, 64, 65, 1023, 1024, 1025)
BLOCK = 256


@pytest.fixture(scope="module")
def tt(gpu):
    from transhuman_amd import hip, train_targets
    hip.load_library()
    return train_targets


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _dev(gpu, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _assert_bits(got, want, keys):
    for k in keys:
        a, b = got[k].cpu().numpy() if torch.is_tensor(got[k]) else np.asarray(got[k]), np.asarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape, (k, a.dtype, b.dtype, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), k


def _layout(gpu, img, layout):
    """the [H,W,3] image as a device tensor in one of the layouts th_ray_sample_* reads through strides"""
    t = _dev(gpu, img)
    if layout == "chw":
        return t.permute(2, 0, 1).contiguous()
    if layout == "strided":                                                     # pixels 5 floats apart inside a wider buffer
        wide = torch.full((*t.shape[:2], 5), float("nan"), device=gpu)
        wide[..., 1:4] = t
        return wide[..., 1:4]
    return t


def _train_on_device(tt, gpu, args, layout="hwc"):
    """hip.ray_sample_train + hip.ray_acc on the arrays of ``args`` (the restatement's arguments) -> (dict cut to its count, info)"""
    from transhuman_amd import hip
    dense = {k: _dev(gpu, v) for k, v in args["dense_rays"].items()}
    msk = _dev(gpu, args["msk"])
    raw = hip.ray_sample_train(dense, msk, _dev(gpu, args["bound_mask"]), _layout(gpu, args["img"], layout),
                               _dev(gpu, args["draws"]), args["nrays"], args["body_ratio"], args["face_ratio"])
    info = raw["info"].cpu().numpy()
    n = int(info[0])
    out = {k: raw[k][:n] for k in ROWS}
    out.update(mask_at_box=torch.ones(n, dtype=torch.bool, device=gpu), acc=hip.ray_acc(out["coord"], msk))
    return out, info


def _check_train(tt, gpu, args, layout="hwc"):
    """the device equals the restatement on ``args``: the same rays, or the same refusal"""
    try:
        want = tt.sample_rays_h36m_oracle(**args)
    except ValueError as e:
        want = str(e)
    got, info = _train_on_device(tt, gpu, args, layout)
    err = tt._loop_error(int(info[2]), int(info[0]), args["nrays"], int(info[1]))
    if isinstance(want, str):
        assert err is not None and str(err) == want, (err, want)
        return None
    assert err is None and int(info[1]) == want["iters"] and int(info[0]) == want["rgb"].shape[0], (info, want["iters"])
    _assert_bits(got, want, ALL_KEYS)
    return want


# ---- against the reference's own outputs --------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["hwc", "chw", "strided"])
@pytest.mark.parametrize("name", CASES)
def test_train_kernel_on_the_reference_rays_equals_the_reference(tt, gpu, gold, name, layout):
    args, want = golden_case(gold, name)
    got, info = _train_on_device(tt, gpu, args, layout)
    assert info.dtype == np.int32 and info[1] == int(gold[f"{name}_iters"]) and info[2] == 0
    _assert_bits(got, want, want.keys())
    _assert_bits(got, dict(acc=tt.get_acc_oracle(want["coord"], args["msk"])), ["acc"])


@pytest.mark.parametrize("layout", ["hwc", "chw", "strided"])
@pytest.mark.parametrize("view", VIEWS)
def test_test_kernel_on_the_reference_rays_equals_the_reference(tt, gpu, gold, view, layout):
    from transhuman_amd import hip
    img, _, dense, want = golden_view(gold, view)
    H, W = gold[f"view_{view}_HW"]
    raw = hip.ray_sample_test({k: _dev(gpu, v) for k, v in dense.items()}, _layout(gpu, img, layout), H, W)
    info = raw["info"].cpu().numpy()
    assert info.tolist() == [want["rgb"].shape[0], 0, 0, 0]
    _assert_bits({k: raw[k][:info[0]] for k in ROWS[:5]}, want, ROWS[:5])


# ---- against the restatement on synthetic dense arrays ------------------------------------------------------------------------
def _synthetic(H, W, seed, in_box=0.9):
    """dense arrays nothing relates to a camera: random rows, a random box mask, a random bound mask and a msk of every value the
    definition tells apart (0, 1, 13, 100, another)"""
    rs = np.random.RandomState(seed)
    n = H * W
    dense = dict(ray_o=rs.uniform(-1, 1, (n, 3)).astype(np.float32), ray_d=rs.uniform(-1, 1, (n, 3)).astype(np.float32),
                 near=rs.uniform(0, 1, n).astype(np.float32), far=rs.uniform(1, 2, n).astype(np.float32),
                 mask_at_box=rs.uniform(size=n) < in_box)
    msk = rs.choice(np.array([0, 1, 13, 100, 7], np.uint8), size=(H, W), p=[0.3, 0.3, 0.1, 0.2, 0.1])
    return dict(img=rs.uniform(size=(H, W, 3)).astype(np.float32), msk=msk, bound_mask=(rs.uniform(size=(H, W)) < 0.7).astype(np.uint8),
                dense_rays=dense)


def _draws(seed, nrays):
    d = np.random.RandomState(seed).uniform(size=(4, 3, nrays))
    d[:, :, 0] = 0.0                                                            # the first and the last member of every class
    d[:, :, -1] = ONE
    return d


@pytest.mark.parametrize("H,W", [(2, 2), (7, 65), (64, 64), (96, 80), (33, 1025), (300, 300)])
def test_train_kernel_equals_the_restatement(tt, gpu, H, W):
    """(300 x 300: 352 pixel blocks, more than one per lane of the scan)"""
    base = _synthetic(H, W, H * 1000 + W, in_box=1.0 if H * W < 64 else 0.9)
    ended = 0
    for i, nrays in enumerate(NRAYS if H < 300 else (65, 1025)):
        args = dict(base, split="train", nrays=nrays, draws=_draws(nrays, nrays), body_ratio=0.5, face_ratio=0.25)
        want = _check_train(tt, gpu, args, ("hwc", "chw", "strided")[i % 3])
        ended += want is not None
        if want is not None and nrays >= 64 and H * W >= 64:
            assert want["iters"] >= 2 and nrays <= want["rgb"].shape[0] <= nrays + 1
    assert ended >= 2


def _class_case(kind):
    """24 x 32 = 768 pixels = 3 pixel blocks, every ray in the box but those of ``miss``; -> (msk, bound, miss, aimed body members)"""
    H, W = 24, 32
    flat = np.zeros(H * W, np.uint8)
    bound = np.ones(H * W, np.uint8)
    miss = np.zeros(H * W, bool)
    if kind == "body_0":
        flat[5::7] = 100
    elif kind == "body_1":
        flat[BLOCK + 255] = 1                                                   # the last pixel of block 1
    elif kind == "body_block":
        flat[BLOCK:2 * BLOCK] = 1                                               # exactly block 1
    elif kind == "body_block_plus_1":
        flat[BLOCK:2 * BLOCK + 1] = 1                                           # ... and the first pixel of block 2
    elif kind == "body_256_spread":
        flat[np.arange(256) * 3] = 1                                            # 256 members over the three blocks
    elif kind == "face_1_rand_257":
        bound[:] = 0
        bound[BLOCK - 1:2 * BLOCK] = 1                                          # rand_set: 257 pixels across a block edge
        flat[2 * BLOCK - 1] = 13
    elif kind == "rand_0":
        flat[:] = 100
    elif kind == "rand_1":
        flat[:] = 100
        flat[767] = 0                                                           # the image's last pixel
    else:
        assert kind == "rand_off_the_box"
        flat[::2] = 1
        miss[1::2] = True                                                       # every rand_set pixel that is no body pixel misses
    return H, W, flat.reshape(H, W), bound.reshape(H, W), miss


@pytest.mark.parametrize("kind", ["body_0", "body_1", "body_block", "body_block_plus_1", "body_256_spread", "face_1_rand_257",
                                  "rand_0", "rand_1", "rand_off_the_box"])
def test_class_sizes_around_a_block_and_picks_at_block_edges(tt, gpu, kind):
    H, W, msk, bound, miss = _class_case(kind)
    base = _synthetic(H, W, 24)
    base.update(msk=msk, bound_mask=bound)
    base["dense_rays"]["mask_at_box"] = ~miss
    m = msk * bound
    sizes = [int(c.sum()) for c in (m == 1, m == 13, (bound == 1) & (m != 100))]
    assert sizes == dict(body_0=[0, 0, 659], body_1=[1, 0, 768], body_block=[256, 0, 768], body_block_plus_1=[257, 0, 768],
                         body_256_spread=[256, 0, 768], face_1_rand_257=[0, 1, 257], rand_0=[0, 0, 0], rand_1=[0, 0, 1],
                         rand_off_the_box=[384, 0, 768])[kind]
    for nrays, body_ratio, face_ratio in ((64, 0.5, 0.25), (7, 1.0, 0.0), (300, 0.0, 0.0), (2, 0.5, 0.5)):
        draws = _draws(nrays + 7, nrays)
        # aim picks at the first and the last member of every pixel block that holds members of the class
        for c, cls in enumerate((m == 1, m == 13, (bound == 1) & (m != 100))):
            members = np.flatnonzero(cls.reshape(-1))
            edges = [k for k in range(members.size) if k == 0 or k == members.size - 1 or
                     members[k] // BLOCK != members[k - 1] // BLOCK or members[k] // BLOCK != members[k + 1] // BLOCK]
            for j, k in enumerate(edges[:max(nrays - 2, 0)]):
                draws[:, c, 1 + j] = (k + 0.5) / members.size
        args = dict(base, split="train", nrays=nrays, draws=draws, body_ratio=body_ratio, face_ratio=face_ratio)
        want = _check_train(tt, gpu, args)
        if kind == "body_1" and body_ratio == 1.0:                              # all picks land on one pixel
            assert want["coord"].tolist() == [[(BLOCK + 255) // W, (BLOCK + 255) % W]] * nrays
        if kind == "rand_0":
            assert (want is None) == (nrays > 8)                                # two rays per iteration: (1,1) and (0,0)
        if kind == "rand_off_the_box" and body_ratio == 0.0:
            assert want is None or want["iters"] > 1


@pytest.mark.parametrize("H,W", [(2, 2), (7, 65), (64, 64), (96, 80), (33, 1025), (300, 300)])
def test_test_kernel_and_acc_equal_the_restatement(tt, gpu, H, W):
    from transhuman_amd import hip
    base = _synthetic(H, W, H * 1000 + W + 1, in_box=0.6)
    want = tt.sample_rays_h36m_oracle(split="test", **base)
    dense = {k: _dev(gpu, v) for k, v in base["dense_rays"].items()}
    for layout in ("hwc", "chw", "strided"):
        raw = hip.ray_sample_test(dense, _layout(gpu, base["img"], layout), H, W)
        n = int(raw["info"][0])
        assert n == want["rgb"].shape[0] and raw["info"].tolist()[1:] == [0, 0, 0]
        _assert_bits({k: raw[k][:n] for k in ROWS[:5]}, want, ROWS[:5])
    for empty in (True, False):                                                 # no ray in the box / every ray
        dense["mask_at_box"] = torch.zeros(H * W, dtype=torch.bool, device=gpu) if empty else ~dense["mask_at_box"].new_zeros(H * W)
        raw = hip.ray_sample_test(dense, _dev(gpu, base["img"]), H, W)
        assert int(raw["info"][0]) == (0 if empty else H * W)
        assert empty or torch.equal(raw["near"], dense["near"]) and torch.equal(raw["ray_d"], dense["ray_d"])
    # get_acc: the four borders and a grid, on a sparse mask, an empty one and one whose only pixel sits in a corner
    coord = border_coords(H, W)
    rs = np.random.RandomState(H + W)
    corner = np.zeros((H, W), np.uint8)
    corner[H - 1, W - 1] = 200
    for msk in ((rs.uniform(size=(H, W)) < 0.003).astype(np.uint8) * 255, np.zeros((H, W), np.uint8), corner):
        got = hip.ray_acc(_dev(gpu, coord), _dev(gpu, msk))
        _assert_bits(dict(acc=got), dict(acc=tt.get_acc_oracle(coord, msk)), ["acc"])
    assert hip.ray_acc(torch.zeros((0, 2), dtype=torch.int64, device=gpu), _dev(gpu, corner)).shape == (0,)


def test_dirty_outputs_and_workspace_change_nothing_and_only_valid_rows_are_written(tt, gpu):
    from transhuman_amd import hip
    H, W, nrays = 33, 65, 200
    base = _synthetic(H, W, 3365)
    args = dict(base, split="train", nrays=nrays, draws=_draws(5, nrays), body_ratio=0.5, face_ratio=0.25)
    want = _check_train(tt, gpu, args)
    n = want["rgb"].shape[0]
    lib, p = hip._lib, hip._p
    dense = {k: _dev(gpu, v) for k, v in base["dense_rays"].items()}
    rm = dense["mask_at_box"].view(torch.uint8)
    msk, bound, img, draws = (_dev(gpu, a) for a in (base["msk"], base["bound_mask"], base["img"], args["draws"]))
    nbytes = int(lib.th_ray_sample_workspace_bytes(H, W, nrays))
    assert nbytes > 0 and lib.th_ray_sample_workspace_bytes(H, W, 0) == nbytes
    rows = nrays + tt.MAX_ITERS
    runs = []
    for seed in (1, 2):
        torch.manual_seed(seed)
        ws = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device=gpu)
        f = lambda *shape: torch.full(shape, float("nan"), device=gpu)
        out = dict(rgb=f(rows, 3), ray_o=f(rows, 3), ray_d=f(rows, 3), near=f(rows), far=f(rows),
                   coord=torch.full((rows, 2), -77, dtype=torch.int64, device=gpu),
                   info=torch.full((4,), -1, dtype=torch.int32, device=gpu))
        rc = lib.th_ray_sample_train(hip.ctx(gpu), p(dense["ray_o"]), p(dense["ray_d"]), p(dense["near"]), p(dense["far"]), p(rm),
                                     p(msk), p(bound), p(img), 3, 1, H, W, p(draws), nrays, 0.5, 0.25,
                                     *(p(out[k]) for k in ROWS + ("info",)), p(ws), nbytes, hip._stream())
        assert rc == 0, lib.th_last_error()
        assert out["info"].tolist()[:3] == [n, want["iters"], 0]
        _assert_bits({k: out[k][:n] for k in ROWS}, want, ROWS)
        assert all(torch.isnan(out[k][n:]).all() for k in ROWS[:5]) and (out["coord"][n:] == -77).all()    # nothing else is written
        runs.append(out)
        # the test split into dirty rows
        t = dict(rgb=f(H * W, 3), ray_o=f(H * W, 3), ray_d=f(H * W, 3), near=f(H * W), far=f(H * W),
                 info=torch.full((4,), -1, dtype=torch.int32, device=gpu))
        ws = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device=gpu)
        rc = lib.th_ray_sample_test(hip.ctx(gpu), p(dense["ray_o"]), p(dense["ray_d"]), p(dense["near"]), p(dense["far"]), p(rm),
                                    p(img), 3, 1, H, W, *(p(t[k]) for k in ROWS[:5] + ("info",)), p(ws), nbytes, hip._stream())
        assert rc == 0, lib.th_last_error()
        wt = tt.sample_rays_h36m_oracle(split="test", **base)
        nt = wt["rgb"].shape[0]
        assert t["info"].tolist() == [nt, 0, 0, 0] and all(torch.isnan(t[k][nt:]).all() for k in ROWS[:5])
        _assert_bits({k: t[k][:nt] for k in ROWS[:5]}, wt, ROWS[:5])
    for k in ROWS:
        assert torch.equal(runs[0][k][:n], runs[1][k][:n]), k


def test_bad_arguments_are_refused_before_any_launch(tt, gpu, gold):
    from transhuman_amd import hip
    args, _ = golden_case(gold, "one_iter")                                     # 40 x 56
    dense = {k: _dev(gpu, v) for k, v in args["dense_rays"].items()}
    msk, bound, img = (_dev(gpu, args[k]) for k in ("msk", "bound_mask", "img"))
    draws = lambda n: torch.zeros((4, 3, max(n, 0)), dtype=torch.float64, device=gpu)
    for nrays, body, face, what in ((0, 0.5, 0.0, "nrays is"), (65537, 0.5, 0.0, "nrays is"), (8, 0.7, 0.4, "body_ratio"),
                                    (8, -0.1, 0.0, "body_ratio")):
        with pytest.raises(hip.HipError, match=what):
            hip.ray_sample_train(dense, msk, bound, img, draws(nrays), nrays, body, face)
    lib, p = hip._lib, hip._p
    assert lib.th_ray_sample_workspace_bytes(4097, 8, 8) == 0 and lib.th_ray_sample_workspace_bytes(8, 8, 65537) == 0
    out = torch.zeros(1 << 16, dtype=torch.uint8, device=gpu)
    ws = torch.zeros(int(lib.th_ray_sample_workspace_bytes(40, 56, 8)), dtype=torch.uint8, device=gpu)
    rm = dense["mask_at_box"].view(torch.uint8)
    train = lambda H, W, nbytes: lib.th_ray_sample_train(
        hip.ctx(gpu), p(dense["ray_o"]), p(dense["ray_d"]), p(dense["near"]), p(dense["far"]), p(rm), p(msk), p(bound), p(img), 3, 1,
        H, W, p(draws(8)), 8, 0.5, 0.0, *([p(out)] * 7), p(ws), nbytes, None)
    test = lambda H, W, nbytes: lib.th_ray_sample_test(
        hip.ctx(gpu), p(dense["ray_o"]), p(dense["ray_d"]), p(dense["near"]), p(dense["far"]), p(rm), p(img), 3, 1, H, W,
        *([p(out)] * 6), p(ws), nbytes, None)
    assert train(40, 56, ws.numel() - 1) < 0 and b"workspace" in lib.th_last_error()
    assert test(40, 56, ws.numel() - 1) < 0 and b"workspace" in lib.th_last_error()
    assert train(1, 8, ws.numel()) < 0 and b"H, W >= 2" in lib.th_last_error()
    assert train(4097, 2, ws.numel()) < 0 and test(0, 8, ws.numel()) < 0 and b"<= 4096" in lib.th_last_error()
    assert lib.th_ray_acc(hip.ctx(gpu), p(out), -1, p(msk), 40, 56, p(out), None) < 0
    torch.cuda.synchronize()
    assert int(out.sum()) == 0                                                  # nothing ran
    with pytest.raises(ValueError, match="H, W >= 2"):
        tt.sample_rays_h36m(img[:1], msk[:1], np.eye(3), np.eye(3), np.zeros((3, 1)), gold["view_axis_bounds"], "train", nrays=2)
    with pytest.raises(ValueError, match="draws"):
        tt.sample_rays_h36m(img, msk, np.eye(3), np.eye(3), np.zeros((3, 1)), gold["view_axis_bounds"], "train", nrays=2,
                            draws=np.ones((4, 3, 2)))


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def _device_arrays(gpu, gold, view):
    """the fixture view's camera through K9 and th_bound_mask: (camera arguments, dense rays, bound mask as numpy)"""
    from transhuman_amd import hip
    f = lambda k: gold[f"view_{view}_{k}"]
    H, W = f("HW")
    cam = (f("K"), f("R"), f("T"), f("bounds"))
    dense = hip.gen_rays(*cam, H, W, device=gpu, compact=False)
    bound = hip.bound_2d_mask(f("bounds"), f("K"), np.concatenate([f("R"), f("T")], axis=1), H, W, device=gpu)
    return cam, {k: v.cpu().numpy() for k, v in dense.items()}, bound.cpu().numpy()


@pytest.mark.parametrize("name", CASES)
def test_end_to_end_equals_the_restatement_on_the_device_rays(tt, gpu, gold, name):
    args, _ = golden_case(gold, name)
    view = str(gold[f"{name}_view"])
    cam, dense, bound = _device_arrays(gpu, gold, view)
    kw = dict(nrays=args["nrays"], draws=args["draws"], body_ratio=args["body_ratio"], face_ratio=args["face_ratio"])
    try:
        want = tt.sample_rays_h36m_oracle(args["img"], args["msk"], bound, dense, "train", **kw)
    except ValueError as e:                                                     # (the draws were aimed on the fixture's rays)
        with pytest.raises(ValueError, match=str(e)[:20]):
            tt.sample_rays_h36m(args["img"], args["msk"], *cam, "train", **kw)
        return
    got = tt.sample_rays_h36m(_dev(gpu, args["img"]), _dev(gpu, args["msk"]), *cam, "train", **kw)
    assert all(got[k].is_cuda for k in ALL_KEYS)
    _assert_bits(got, want, ALL_KEYS)
    again = tt.sample_rays_h36m(_dev(gpu, args["img"]).permute(2, 0, 1).contiguous(), args["msk"], *cam, "train", **kw)
    for k in ALL_KEYS:
        assert torch.equal(got[k], again[k]), k
    # the test split of the same view
    want = tt.sample_rays_h36m_oracle(args["img"], args["msk"], bound, dense, "test")
    got = tt.sample_rays_h36m(args["img"], args["msk"], *cam, "test")
    _assert_bits(got, want, ALL_KEYS)
    assert got["mask_at_box"].shape == (bound.size,) and got["coord"].shape == (want["rgb"].shape[0], 2)


def test_defaults_come_from_cfg_and_draws_from_the_generator(tt, gpu, gold):
    img, _, _, _ = golden_view(gold, "oblique")
    f = lambda k: gold[f"view_oblique_{k}"]
    cam = (f("K"), f("R"), f("T"), f("bounds"))
    msk = gold["one_iter_msk"]
    got = tt.sample_rays_h36m(img, msk, *cam, "train", generator=torch.Generator().manual_seed(7))
    assert 1024 <= got["rgb"].shape[0] <= 1025
    draws = torch.rand(4, 3, 1024, dtype=torch.float64, generator=torch.Generator().manual_seed(7))
    same = tt.sample_rays_h36m(img, msk, *cam, "train", draws=draws)
    for k in ALL_KEYS:
        assert torch.equal(got[k], same[k]), k


def test_a_loop_that_does_not_end_raises_after_one_launch(tt, gpu, gold, monkeypatch):
    from transhuman_amd import hip
    args, _ = golden_case(gold, "two_iters")
    cam, dense, bound = _device_arrays(gpu, gold, "axis")
    on_device = dict(args, dense_rays=dense, bound_mask=bound)
    later = []
    monkeypatch.setattr(hip, "ray_acc", lambda *a, **kw: later.append(a))
    draws = unfinished_draws(on_device)
    with pytest.raises(ValueError, match="unfinished after MAX_ITERS"):
        tt.sample_rays_h36m(args["img"], args["msk"], *cam, "train", nrays=16, draws=draws, body_ratio=0.0, face_ratio=0.0)
    nothing = np.repeat(draws[:, :, :1], 8, axis=2)                             # every pick on a pixel whose ray misses the box
    with pytest.raises(ValueError, match="added nothing"):
        tt.sample_rays_h36m(args["img"], args["msk"], *cam, "train", nrays=8, draws=nothing, body_ratio=0.0, face_ratio=0.0)
    assert not later                                                            # nothing was started behind the loop's launch
    monkeypatch.undo()
    draws[3, 2, 0] = draws[3, 2, 1]
    got = tt.sample_rays_h36m(args["img"], args["msk"], *cam, "train", nrays=16, draws=draws, body_ratio=0.0, face_ratio=0.0)
    torch.cuda.synchronize()
    assert got["rgb"].shape == (16, 3) and got["acc"].shape == (16,)


# ---- the renderer ----------------------------------------------------------------------------------------------------------
def _camera(target, base):
    """(K, R, T, bounds) of a collated target view, on the host"""
    return [target[k][0].cpu().numpy() for k in ("target_K", "target_R", "target_T")] + [base["can_bounds"][0].cpu().numpy()]


def _restated_targets(tt, gpu, target, base, split, **kw):
    """the restatement's targets for a collated target view (on the device's own dense rays and bound mask), collated"""
    from transhuman_amd import hip
    K, R, T, b = _camera(target, base)
    H, W = (int(n) for n in target["target_msk"].shape[1:])
    dense = hip.gen_rays(K, R, T, b, H, W, device=gpu, compact=False)
    bound = hip.bound_2d_mask(b, K, np.concatenate([R, T], axis=1), H, W, device=gpu)
    want = tt.sample_rays_h36m_oracle(target["target_img"][0], target["target_msk"][0], bound, dense, split, **kw)
    return {k: _dev(gpu, want[k])[None] for k in tt.H36M_KEYS}


RUN_TO_RUN = 4e-5


@pytest.mark.parametrize("mode", ["default", "reproducible"])
def test_training_render_makes_the_dataset_targets_on_the_device(tt, gpu, mode):
    """cfg.patch.use_patch_sampling false, cfg.target_sampler = "dataset": a training Renderer.render through NetworkWrapper (its
    masked-MSE branch) on a batch without ray_o, against the same batch carrying the restatement's targets.  The keys added to the
    batch and the loss are torch.equal (torch on its deterministic algorithms and MIOpen on its deterministic kernels, as
    tests/test_gpu_jitter.py::test_training_step_on_raw_frames_and_a_seed does in both modes).  Gradients, "reproducible": every
    training switch on its device value and the ordered gather backward -- torch.equal.  "default": the backward of the default
    switches (torch's grid_sampler_2d_backward among them) adds with float atomics in an order that changes from run to run, so the
    two runs -- whose inputs are the same bits -- are held to RUN_TO_RUN = 4e-5 of each tensor's largest gradient: a gradient is a
    sum of up to rays x samples x views = 65 x 16 x 3 ~ 3e3 fp32 terms, reordering it moves it by about sqrt(3e3) x 2^-24 ~ 3.3e-6
    of the terms' magnitude, and the bar leaves the factor 10 for cancellation that test_gpu_jitter.py's 1e-4 leaves at its 2e4
    terms."""
    from test_gpu_train_encoder import ALL_DEVICE, _reproducible_torch
    from test_gpu_train_targets import _setup
    from transhuman_amd import config
    from transhuman_amd.train_loss import NetworkWrapper
    switches = dict(ALL_DEVICE, train_encoder="device", train_gather_bwd="ordered") if mode == "reproducible" else {}
    cfg, net, r, base, target, _ = _setup(gpu)
    target.pop("patch_draws")
    base.pop("mask_at_box")                                                     # (synth.make_batch's: a present key is never overwritten)
    draws = torch.rand(1, 4, 3, 64, dtype=torch.float64, generator=torch.Generator().manual_seed(26))
    try:
        cfg.patch.use_patch_sampling = False
        wrapper = NetworkWrapper(net, renderer=r, lpips=lambda a, b: None)
        torch.use_deterministic_algorithms(True, warn_only=True)

        def step(batch):
            net.zero_grad(set_to_none=True)
            ret, loss, stats, _ = wrapper(batch)
            loss.backward()
            return loss.detach().clone(), {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}
        with _reproducible_torch(), config.override(**{**switches, "target_prep": "device", "target_sampler": "dataset", "N_rand": 64}):
            b = {**base, **target, "ray_draws": draws}
            loss, grads = step(b)
            n = b["ray_o"].shape[1]
            assert 64 <= n <= 65 and b["acc"].shape == (1, n) and b["acc"].dtype is torch.uint8
            assert b["mask_at_box"].shape == (1, n) and b["mask_at_box"].dtype is torch.bool and bool(b["mask_at_box"].all())
            assert "coord" not in b and "patch_masks" not in b and b["rgb"].shape == (1, n, 3) and b["rgb"].is_cuda
            fed = {**base, **_restated_targets(tt, gpu, target, base, "train", draws=draws[0])}
            for k in tt.H36M_KEYS:
                assert torch.equal(b[k], fed[k]), k
            want_loss, want_grads = step(fed)
        assert torch.equal(loss, want_loss) and float(loss) > 0 and len(grads) > 20 and grads.keys() == want_grads.keys()
        worst = max((float((grads[k] - want_grads[k]).abs().max()) / max(float(want_grads[k].abs().max()), 1e-30), k) for k in grads)
        print(f"{mode}: loss {float(loss):.6g}, largest gradient difference / largest gradient = {worst[0]:.3g} ({worst[1]}), "
              f"{len(grads)} tensors")
        assert any(float(g.abs().max()) > 0 for g in grads.values())
        if mode == "reproducible":
            differ = [k for k in grads if not torch.equal(grads[k], want_grads[k])]
            assert not differ, differ
        else:
            assert worst[0] <= RUN_TO_RUN, worst
    finally:
        torch.use_deterministic_algorithms(False)
        cfg.patch.use_patch_sampling = True
        cfg.vit_depth, cfg.N_samples = 12, 64


def test_render_fast_makes_the_test_split_on_the_device(tt, gpu, tmp_path):
    from test_gpu_preprocess import _renderer
    from test_gpu_train_targets import _ellipse
    from transhuman_amd import config, hip, synth
    from transhuman_amd.evaluator import Evaluator
    H = W = 64
    with config.override(N_samples=32, num_class=300), torch.no_grad():
        b = synth.make_batch(H, W, 3, seed=0, all_rays=False, focal=100.0)
        cams = synth.make_cameras(H, W, 3, center=tuple(b["Th"][0, 0].tolist()), focal=100.0)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))[None]
        target = dict(target_K=t(cams["K"]), target_R=t(cams["R"]), target_T=t(cams["T"]),
                      target_img=torch.from_numpy(np.random.RandomState(64).uniform(size=(1, H, W, 3)).astype(np.float32)),
                      target_msk=torch.from_numpy(_ellipse(H, W))[None])
        for k in ("ray_o", "ray_d", "near", "far", "mask_at_box"):
            b.pop(k)
        base, target = synth.batch_to(b, gpu), synth.batch_to(target, gpu)
        r = _renderer(gpu)
        render = lambda batch: {k: v.clone() for k, v in r.render_fast(batch, is_train=False).items()}
        rays = hip.gen_rays(*_camera(target, base), H, W, device=gpu, compact=True)
        n = int(rays["mask_at_box"].sum())
        assert n > 0
        fed = {**base, **{k: rays[k][None] for k in ("ray_o", "ray_d", "near", "far")}}
        want = render(fed)
        bare = {**base, **target}
        with config.override(target_prep="device"), pytest.raises(KeyError):    # the default sampler: no rays are made
            r.render_fast(dict(bare), is_train=False)
        with config.override(target_prep="device", target_sampler="dataset"):
            got = render(bare)
            again = {**base, **target}
            r.render(again)                                                     # the no-grad render takes the same route
            seq = [{**base, **target}, {**base, **target}]
            outs = [{k: v.clone() for k, v in o.items()} for o in r.render_sequence(iter(seq))]
            before = dict(fed)
            r.render_fast(fed, is_train=False)                                  # a batch with its rays is left alone
            assert fed.keys() == before.keys() and all(fed[k] is before[k] for k in fed)
        for k in ("rgb_map", "acc_map", "depth_map"):
            assert torch.equal(got[k], want[k]), k
        assert float(want["acc_map"].max()) > 0.05
        restated = _restated_targets(tt, gpu, target, base, "test")
        for k in tt.H36M_KEYS:
            assert torch.equal(bare[k], restated[k]), k
            assert torch.equal(again[k], bare[k]) and all(torch.equal(s[k], bare[k]) for s in seq), k
        assert bare["rgb"].shape == (1, n, 3) and bare["mask_at_box"].shape == (1, H * W) and bare["acc"].shape == (1, n)
        assert len(outs) == 2 and all(torch.equal(o["rgb_map"], want["rgb_map"]) for o in outs)
        res = Evaluator(result_dir=str(tmp_path)).evaluate(got, bare, H=H, W=W, save=False)
        print(res)
        assert np.isfinite(res["mse"]) and np.isfinite(res["psnr"]) and "ssim" in res
