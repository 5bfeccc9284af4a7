"""GPU: the training targets of a step made on the device (csrc/k_patch.hip, transhuman_amd/train_targets.py, K18).  The stage only
selects and copies, so every comparison here is bit for bit: K18 through the C ABI against the reference's own outputs
(tests/golden/g22_patch_rays.npz, fed the fixture's dense rays), ``sample_patch_rays`` end to end against the numpy restatement
fed the device's own dense rays and bound mask (parity of those with the reference is what the K9 tests pin), determinism, the
error returns, the raw-frame route, and the renderer's cfg.target_prep == "device"."""
import numpy as np
import pytest
import torch

from transhuman_amd import synth
from transhuman_amd.config import get_cfg
from test_train_targets_host import CASES, GOLD, ONE, golden_case
from util import can64, synth_assign, SIGMA_BIAS

pytestmark = pytest.mark.gpu
ALL_KEYS = ("rgb", "ray_o", "ray_d", "near", "far", "sub_mask", "patch_masks", "patch_masks_sub", "target_patches",
            "patch_div_indices", "select_inds", "xy_min", "xy_max")
BOX = np.array([[-0.35, -0.9, 2.6], [0.4, 0.85, 3.3]], np.float32)          # the box of the fixture's cases


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


def _ellipse(H, W):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    r = np.sqrt(((y - 0.5 * H) / (0.33 * H)) ** 2 + ((x - 0.45 * W) / (0.22 * W)) ** 2)
    m = np.zeros((H, W), np.uint8)
    m[r <= 1.15] = 100
    m[r <= 1.0] = 1
    return m


def _big_case():
    """512 x 512, N = 6, P = 20: 1024 blocks, more than one per scan lane"""
    H = W = 512
    K = np.array([[600.0, 0, 256.0], [0, 600.0, 256.0], [0, 0, 1]], np.float32)
    img = np.random.RandomState(512).uniform(size=(H, W, 3)).astype(np.float32)
    return dict(img=img, msk=_ellipse(H, W), K=K, R=np.eye(3, dtype=np.float32), T=np.zeros((3, 1), np.float32), bounds=BOX, P=20)


def _view(gold, name):
    if name == "big":
        return _big_case()
    f = lambda k: gold[f"{name}_{k}"]
    return dict(img=f("img"), msk=f("msk"), K=f("K"), R=f("R"), T=f("T"), bounds=f("bounds"), P=int(f("P")))


@pytest.mark.parametrize("layout", ["hwc", "chw"])
@pytest.mark.parametrize("name", CASES)
def test_kernel_on_the_reference_rays_equals_the_reference(tt, gpu, gold, name, layout):
    from transhuman_amd import hip
    args, want = golden_case(gold, name)
    dense = {k: _dev(gpu, v) for k, v in args["dense_rays"].items()}
    img = _dev(gpu, args["img"])
    if layout == "chw":
        img = img.permute(2, 0, 1).contiguous()
    raw = hip.patch_rays(dense, _dev(gpu, args["msk"]), _dev(gpu, args["bound_mask"]), img, _dev(gpu, args["draws"]),
                         args["subject_ratio"], args["patch_size"])
    counts = raw["counts"].cpu().numpy()
    assert counts.dtype == np.int32 and (counts[0] > 0).all()
    assert counts[1].tolist() == np.diff(want["patch_div_indices"]).tolist()
    _assert_bits(tt.assemble(raw, counts), want, want.keys())


@pytest.mark.parametrize("name", CASES + ("big",))
def test_end_to_end_equals_the_restatement_on_the_device_rays(tt, gpu, gold, name):
    from transhuman_amd import hip
    v = _view(gold, name)
    H, W = v["msk"].shape
    draws = gold["draws"]
    got = tt.sample_patch_rays(_dev(gpu, v["img"]), _dev(gpu, v["msk"]), v["K"], v["R"], v["T"], v["bounds"], draws=draws,
                               patch_size=v["P"], subject_ratio=0.8)
    assert all(got[k].is_cuda for k in ALL_KEYS if k != "patch_div_indices") and not got["patch_div_indices"].is_cuda
    dense = hip.gen_rays(v["K"], v["R"], v["T"], v["bounds"], H, W, device=gpu, compact=False)
    bound = hip.bound_2d_mask(v["bounds"], v["K"], np.concatenate([v["R"], v["T"]], axis=1), H, W, device=gpu)
    want = tt.sample_patch_rays_oracle(v["img"], v["msk"], bound, dense, draws, patch_size=v["P"], subject_ratio=0.8)
    counts = np.diff(want["patch_div_indices"])
    print(name, "rays per patch", counts.tolist())
    assert (counts > 0).all() and (counts < v["P"] ** 2).any()                 # windows cut by the box
    _assert_bits(got, want, ALL_KEYS)
    # the same call again, and with the image as K16 lays it out: the same bits
    again = tt.sample_patch_rays(_dev(gpu, v["img"]).permute(2, 0, 1).contiguous(), _dev(gpu, v["msk"]), v["K"], v["R"], v["T"],
                                 v["bounds"], draws=draws, patch_size=v["P"], subject_ratio=0.8)
    for k in ALL_KEYS:
        assert torch.equal(got[k], again[k]), k


def test_defaults_come_from_cfg_and_draws_from_the_generator(tt, gpu):
    v = _big_case()
    g = torch.Generator().manual_seed(7)
    got = tt.sample_patch_rays(v["img"], v["msk"], v["K"], v["R"], v["T"], v["bounds"], generator=g)
    assert got["patch_masks"].shape == (6, 20, 20) and got["target_patches"].shape == (6, 20, 20, 3)
    draws = torch.rand(6, 2, dtype=torch.float64, generator=torch.Generator().manual_seed(7))
    same = tt.sample_patch_rays(v["img"], v["msk"], v["K"], v["R"], v["T"], v["bounds"], draws=draws)
    for k in ALL_KEYS:
        assert torch.equal(got[k], same[k]), k


def test_empty_candidate_set_is_a_clean_error(tt, gpu, gold):
    v = _view(gold, "axis_p8")
    args = (v["K"], v["R"], v["T"], v["bounds"])
    with pytest.raises(ValueError, match="empty"):
        tt.sample_patch_rays(v["img"], np.zeros_like(v["msk"]), *args, draws=[[0.9, 0.5], [0.1, 0.5]], patch_size=8, subject_ratio=0.8)
    got = tt.sample_patch_rays(v["img"], v["msk"], *args, draws=gold["draws"], patch_size=8, subject_ratio=0.8)
    torch.cuda.synchronize()
    assert np.diff(got["patch_div_indices"].numpy()).tolist() == np.diff(gold["axis_p8_patch_div_indices"]).tolist()


def test_bad_arguments_are_refused_before_any_launch(tt, gpu, gold):
    from transhuman_amd import hip
    args, _ = golden_case(gold, "axis_p8")                                      # 64 x 48
    dense = {k: _dev(gpu, v) for k, v in args["dense_rays"].items()}
    msk, bound, img = (_dev(gpu, args[k]) for k in ("msk", "bound_mask", "img"))
    draws = _dev(gpu, args["draws"])
    for P, d, what in ((0, draws, "patch size"), (49, draws, "patch size"), (65, draws, "patch size"),
                       (8, draws[:0], "N is"), (8, draws.repeat(11, 1), "N is")):
        with pytest.raises(hip.HipError, match=what):
            hip.patch_rays(dense, msk, bound, img, d, 0.8, P)
    lib, p = hip._lib, hip._p
    out = torch.zeros(4096, dtype=torch.uint8, device=gpu)
    ws = torch.zeros(int(lib.th_patch_workspace_bytes(64, 48)), dtype=torch.uint8, device=gpu)
    call = lambda nbytes: lib.th_patch_rays(hip.ctx(gpu), p(dense["ray_o"]), p(dense["ray_d"]), p(dense["near"]), p(dense["far"]),
                                            p(dense["mask_at_box"].view(torch.uint8)), p(msk), p(bound), p(img), 3, 1, 64, 48,
                                            p(draws), 0.8, 1, 2, *([p(out)] * 12), p(ws), nbytes, None)
    assert call(ws.numel() - 1) < 0 and b"workspace" in lib.th_last_error()
    torch.cuda.synchronize()
    assert int(out.sum()) == 0                                                  # nothing ran
    with pytest.raises(ValueError):
        tt.sample_patch_rays(img, msk, np.eye(3), np.eye(3), np.zeros((3, 1)), BOX, draws=[[0.5, 0.5]], patch_size=49)
    with pytest.raises(ValueError):
        tt.sample_patch_rays(img, msk, np.eye(3), np.eye(3), np.zeros((3, 1)), BOX, draws=[[0.5, 1.0]], patch_size=8)


def _raw_frame(gold):
    """a raw 128 x 96 target frame whose prepared view (ratio 0.5) has the fixture's axis camera"""
    from test_preprocess_host import D_MINUS, picture
    H0, W0 = 128, 96
    img, _ = picture(H0, W0, seed=9)
    m = _ellipse(H0, W0)
    msk, cihp = ((m == 1) * 255).astype(np.uint8), np.roll(m > 0, 5, axis=1).astype(np.uint8)
    K_raw = gold["axis_p8_K"].copy()
    K_raw[:2] *= 2
    return dict(target_img_raw=img[None], target_msk_raw=msk[None], target_msk_cihp_raw=cihp[None], target_K_raw=K_raw[None],
                target_D=(D_MINUS * np.float32(0.2))[None])


def test_raw_frame_route_equals_the_prepared_route(tt, gpu, gold):
    from transhuman_amd import preprocess
    cfg = get_cfg()
    raw = {k: _dev(gpu, v) for k, v in _raw_frame(gold).items()}
    common = dict(target_R=_dev(gpu, gold["axis_p8_R"])[None], target_T=_dev(gpu, gold["axis_p8_T"])[None],
                  can_bounds=_dev(gpu, gold["axis_p8_bounds"])[None], patch_draws=torch.from_numpy(gold["draws"])[None])
    size = cfg.patch.size
    try:
        cfg.patch.size = 8
        a = tt.add_targets({**raw, **common})
        for with_cihp in (True, False):
            cihp = raw["target_msk_cihp_raw"][0] if with_cihp else None
            m = preprocess.combine_masks(raw["target_msk_raw"][0], cihp, border=5)
            imgs, msks, Ks = preprocess.prepare_views(raw["target_img_raw"], m[None], raw["target_K_raw"], raw["target_D"])
            assert imgs.shape == (1, 3, 64, 48) and (msks == 100).any() and np.array_equal(Ks[0].cpu().numpy(), gold["axis_p8_K"])
            prepared = dict(target_img=imgs.permute(0, 2, 3, 1).contiguous(), target_msk=msks, target_K=Ks)
            b = tt.add_targets({**prepared, **common})
            if not with_cihp:
                a = tt.add_targets({**{k: v for k, v in raw.items() if k != "target_msk_cihp_raw"}, **common})
            for k in tt.REFERENCE_KEYS:
                assert a[k].shape[0] == 1 and torch.equal(a[k], b[k]), k
            assert "target_K" not in a and int(a["patch_div_indices"][0, -1]) == a["ray_o"].shape[1] > 0
    finally:
        cfg.patch.size = size


# ---- the renderer ----------------------------------------------------------------------------------------------------------
def _setup(device):
    """the sizes of tests/test_gpu_train_ops.py::_setup, a 48 x 48 target view"""
    from transhuman_amd.networks.cross_transformer import Network
    from transhuman_amd.networks.renderer.if_clight_renderer import Renderer
    cfg = get_cfg()
    cfg.vit_depth, cfg.N_samples, cfg.num_class, cfg.perturb, cfg.raw_noise_std = 2, 16, 300, 0.0, 0.0
    torch.manual_seed(0)
    net = Network()
    net.load_state_dict(synth.det_state_dict(net.state_dict(), seed=0, sigma_bias=SIGMA_BIAS))
    net.train()
    net = net.to(device)
    r = Renderer(net, vertex_can=can64().numpy(), pc2voxel_ind=synth_assign(300))
    H = W = 48
    b = synth.make_batch(H, W, 3, seed=0, all_rays=False, focal=100.0)
    cams = synth.make_cameras(H, W, 3, center=tuple(b["Th"][0, 0].tolist()), focal=100.0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))[None]
    target = dict(target_K=t(cams["K"]), target_R=t(cams["R"]), target_T=t(cams["T"]),
                  target_img=torch.from_numpy(np.random.RandomState(48).uniform(size=(1, H, W, 3)).astype(np.float32)),
                  target_msk=torch.from_numpy(_ellipse(H, W))[None],
                  patch_draws=torch.tensor([[0.9, 0.0], [0.9, ONE], [0.1, 0.0], [0.1, ONE], [0.5, 0.37], [0.95, 0.6]],
                                           dtype=torch.float64)[None])
    rays = {k: b.pop(k) for k in ("ray_o", "ray_d", "near", "far")}
    return cfg, net, r, synth.batch_to(b, device), synth.batch_to(target, device), synth.batch_to(rays, device)


def test_renderer_makes_its_targets_on_the_device(tt, gpu):
    cfg, net, r, base, target, rays = _setup(gpu)
    size = cfg.patch.size
    try:
        cfg.patch.size, cfg.target_prep = 8, "device"
        b = {**base, **target}
        # (the two renders that are compared bit for bit run with torch's reproducible algorithms: its GEMM library may otherwise
        # add partial sums with atomics, in an order that changes from call to call)
        torch.use_deterministic_algorithms(True, warn_only=True)
        ret = r.render(b)
        n = b["ray_o"].shape[1]
        div = b["patch_div_indices"]
        shapes = dict(rgb=(1, n, 3), ray_o=(1, n, 3), ray_d=(1, n, 3), near=(1, n), far=(1, n), sub_mask=(1, n, 1), patch_masks=(1, 6, 8, 8),
                      patch_masks_sub=(1, 6, 8, 8), target_patches=(1, 6, 8, 8, 3), patch_div_indices=(1, 7))
        for k, s in shapes.items():
            assert tuple(b[k].shape) == s, (k, tuple(b[k].shape))
        assert b["patch_masks"].dtype is torch.bool and b["sub_mask"].dtype is torch.bool and div.dtype is torch.int64
        assert not div.is_cuda and b["ray_o"].is_cuda and int(div[0, 0]) == 0 and int(div[0, -1]) == n > 0
        for i in range(6):
            assert int(b["patch_masks"][0, i].sum()) == int(div[0, i + 1] - div[0, i])
        assert ret["rgb_map"].shape == (1, n, 3) and ret["rgb_map"].requires_grad
        # a "batch"-mode call fed those same rays: the same bits
        cfg.target_prep = "batch"
        fed = {**base, **{k: b[k] for k in ("ray_o", "ray_d", "near", "far")}}
        ref = r.render(fed)
        torch.use_deterministic_algorithms(False)
        print({k: float((ret[k] - ref[k]).abs().max()) for k in ("rgb_map", "acc_map", "depth_map")})
        for k in ("rgb_map", "acc_map", "depth_map"):
            assert torch.equal(ret[k], ref[k]), k
        assert "patch_masks" not in fed
        # the loss reaches the parameters through the rays made here
        cfg.target_prep = "device"
        loss = torch.mean((ret["rgb_map"] - b["rgb"]) ** 2) + 0.1 * ret["acc_map"].mean()
        loss.backward()
        grads = [p.grad for p in net.parameters() if p.grad is not None]
        assert len(grads) > 20 and all(torch.isfinite(g).all() for g in grads) and any(float(g.abs().max()) > 0 for g in grads)
        # a batch that carries its rays is left alone
        own = {**base, **target, **rays}
        before = dict(own)
        r.render(own)
        assert own.keys() == before.keys() and all(own[k] is before[k] for k in own)
        # a key that is present is not overwritten
        marked = {**base, **target, "rgb": torch.zeros(1, 1, 3, device=gpu)}
        r.render(marked)
        assert marked["rgb"].shape == (1, 1, 3) and marked["ray_o"].shape == (1, n, 3)
        # the three refusals
        with pytest.raises(ValueError, match="target"):
            r.render(dict(base))
        cfg.patch.use_patch_sampling = False
        with pytest.raises(ValueError, match="use_patch_sampling"):
            r.render({**base, **target})
        cfg.patch.use_patch_sampling = True
        cfg.target_prep = "host"
        with pytest.raises(ValueError, match="target_prep"):
            r.render({**base, **target, **rays})
    finally:
        torch.use_deterministic_algorithms(False)
        cfg.patch.size, cfg.patch.use_patch_sampling, cfg.target_prep = size, True, "batch"
        cfg.vit_depth, cfg.N_samples = 12, 64
