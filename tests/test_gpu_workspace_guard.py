"""GPU: no entry point writes outside the workspace it asked for.  Inside this module hip._ws and hip._cached_ws hand out the
middle of a larger uint8 tensor -- 64 KiB of 0xA5 on either side, the interior (exactly the bytes asked for) 0xFF, its offset a
multiple of 256 so the alignment is the allocator's own.  Every wrapper that takes a workspace runs once plain and once on
such a buffer, at the smallest shape its own GPU test uses, with odd counts where the entry allows them (33 samples, 50
tokens, 17 x 19 pixels): both guards stay 0xA5 and the results are the plain call's, bit for bit.  The test reads only memory
it allocated itself."""
import numpy as np
import pytest
import torch

from transhuman_amd import synth
from util import body, can64, make_net, synth_assign

pytestmark = pytest.mark.gpu

GUARD = 64 * 1024


@pytest.fixture(scope="module")
def hip(gpu):
    from transhuman_amd import hip as H
    H.load_library()
    return H


class Guarded:
    """the replacement of hip._ws / hip._cached_ws while it is installed"""

    def __init__(self):
        self.blocks = []

    def ws(self, nbytes, device, slot=0):
        n = max(int(nbytes), 256)                                    # (hip._ws's own lower bound)
        big = torch.full((GUARD + n + GUARD,), 0xA5, dtype=torch.uint8, device=device)
        inner = big[GUARD:GUARD + n]
        inner.fill_(0xFF)
        assert inner.data_ptr() % 256 == big.data_ptr() % 256
        self.blocks.append((big, n))
        return inner

    def check(self):
        assert self.blocks, "the wrapper took no workspace through hip._ws / hip._cached_ws"
        for big, n in self.blocks:
            lo, hi = big[:GUARD], big[GUARD + n:]
            assert hi.numel() == GUARD
            assert bool((lo == 0xA5).all()), f"bytes in front of a {n}-byte workspace were written"
            assert bool((hi == 0xA5).all()), f"bytes behind a {n}-byte workspace were written"


def _flat(x, out):
    if torch.is_tensor(x):
        out.append(x.detach().contiguous().reshape(-1).view(torch.uint8).cpu().numpy().tobytes())
    elif isinstance(x, np.ndarray):
        out.append(np.ascontiguousarray(x).tobytes())
    elif isinstance(x, dict):
        for k in sorted(x):
            _flat(x[k], out)
    elif isinstance(x, (tuple, list)):
        for v in x:
            _flat(v, out)
    else:
        out.append(repr(x))
    return out


def _rn(gpu, seed, *shape, scale=1.0):
    return torch.from_numpy((np.random.RandomState(seed).standard_normal(shape) * scale).astype(np.float32)).to(gpu)


# ---- the cases: name -> build(hip, gpu) -> run() -> the call's results (the parts it defines) --------------------------------
CASES = {}


def case(fn):
    CASES[fn.__name__] = fn
    return fn


def _cloud(gpu, P, seed):
    """P points around the synthetic body's vertices"""
    rs = np.random.RandomState(seed)
    v = body()
    return torch.from_numpy((v[rs.randint(0, v.shape[0], P)] + rs.normal(0, 0.05, (P, 3))).astype(np.float32)).to(gpu)


def _tokens_case(gpu, nc=50, V=2):
    rs = np.random.RandomState(3)
    cen = torch.from_numpy(body()[rs.choice(body().shape[0], nc, replace=False)].astype(np.float32)).to(gpu)
    return cen, _rn(gpu, 4, nc, 9), _rn(gpu, 5, V, nc, 192)


@case
def linear(hip, gpu):
    x, w, b = _rn(gpu, 0, 33, 50), _rn(gpu, 1, 17, 50), _rn(gpu, 2, 17)
    return lambda: hip.linear(x, w, b, 1)


@case
def hull_mask(hip, gpu):
    pts, verts = _cloud(gpu, 33 * 19, 0), torch.from_numpy(body()[:1237].astype(np.float32)).to(gpu)
    return lambda: hip.hull_mask(hip.Points(pts=pts), verts, 0.1)


def _cams(hip, gpu, V):
    b = synth.make_batch(32, 32, 3, seed=0)
    return hip.pack_cams(*(b[k][0][0][:V].to(gpu) for k in ("input_R", "input_T", "input_K"))), b


@case
def paint_group_nhwc(hip, gpu):
    V, nv, nc = 2, 50, 7
    cams, b = _cams(hip, gpu, V)
    verts = b["tar_smpl_vertice"][0][:nv].to(gpu)
    scale = torch.tensor([2.0 / 31.0, 2.0 / 31.0], device=gpu)
    off, mem = hip.csr_to_device(*synth.csr_from_assign(np.arange(nv) % nc), gpu)
    m, w, bias = _rn(gpu, 6, V, 17, 19, 384), _rn(gpu, 7, 48, 384, scale=0.05), _rn(gpu, 8, 48)
    viz = torch.from_numpy(np.random.RandomState(9).uniform(size=(V, nv)) < 0.8).to(gpu)
    return lambda: hip.paint_group_nhwc(m, verts, cams, scale, viz, w, bias, off, mem)


@case
def bn_act(hip, gpu):
    x, bn = _rn(gpu, 10, 2, 5, 17, 19), torch.nn.BatchNorm2d(5).to(gpu).train()
    return lambda: hip.bn_act(x, bn, residual=x, relu=True)


@pytest.fixture(scope="module")
def net(gpu, hip):
    return make_net(12).to(gpu)


@case
def vit_forward(hip, gpu, net=None):
    x = _rn(gpu, 11, 2, 50, 192)
    pe = (torch.rand(2, 50, 3, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(gpu)
    return lambda: net.ViT(x, pe, mask=None)


def _qkv(gpu):
    return _rn(gpu, 12, 2, 50, 576)


@case
def attention(hip, gpu):
    q = _qkv(gpu)
    return lambda: hip.attention(q, 3, 0)


@case
def attention_train(hip, gpu):
    q = _qkv(gpu)
    return lambda: hip.attention_train(q, 3, 0)


@case
def attention_bwd(hip, gpu):
    q, g = _qkv(gpu), _rn(gpu, 13, 2, 50, 192)
    out, lse = hip.attention_train(q, 3, 0)
    return lambda: hip.attention_bwd(q, out, lse, g, 3)


@case
def conv2d_wgrad(hip, gpu):
    x, g = _rn(gpu, 14, 2, 64, 17, 19), _rn(gpu, 15, 2, 64, 17, 19)
    return lambda: hip.conv2d_wgrad(x, g, 3, 1)


@case
def bn_act_bwd(hip, gpu):
    y, g, gamma = _rn(gpu, 16, 2, 5, 17, 19), _rn(gpu, 17, 2, 5, 17, 19), _rn(gpu, 18, 5)
    out = torch.relu(y).contiguous()
    return lambda: hip.bn_act_bwd(y, out, g, gamma, 1e-5, need_residual=True)


def _dense(gpu):
    return dict(a=_rn(gpu, 19, 33, 48), W=_rn(gpu, 20, 32, 48, scale=0.2), b=_rn(gpu, 21, 32), g=_rn(gpu, 22, 33, 32),
                lw=_rn(gpu, 23, 48), lb=_rn(gpu, 24, 48))


@case
def linear_train_forward(hip, gpu):
    d = _dense(gpu)
    return lambda: [hip.linear_train_forward(d["a"], d["W"], d["b"], form, d["lw"], d["lb"], 1e-6) for form in (0, 1, 2)]


@case
def linear_bwd(hip, gpu):
    d = _dense(gpu)
    return lambda: [hip.linear_bwd(d["a"], d["W"], d["g"], form, d["lw"], d["lb"], 1e-6) for form in (0, 1, 2)]


@case
def linear_relu_forward(hip, gpu):
    d = _dense(gpu)
    return lambda: hip.linear_relu_forward(d["a"], d["W"], d["b"])


@case
def linear_relu_bwd(hip, gpu):
    d = _dense(gpu)
    y = hip.linear_relu_forward(d["a"], d["W"], d["b"])
    return lambda: hip.linear_relu_bwd(d["a"], y, d["W"], d["g"])


@case
def layernorm_bwd(hip, gpu):
    d = _dense(gpu)
    return lambda: hip.layernorm_bwd(d["a"], d["lw"], _rn(gpu, 25, 33, 48), 1e-6)


@case
def network_forward(hip, gpu, net=None):
    P, V = 33 * 19, 2
    cen, rot, tok = _tokens_case(gpu, 50, V)
    pf, vd, pts = _rn(gpu, 26, V, 384, P), _rn(gpu, 27, P, 27), _cloud(gpu, P, 1)
    mask = torch.from_numpy(np.random.RandomState(28).uniform(size=P) < 0.9).to(gpu)
    return lambda: [hip.network_forward(net, pf, vd, pts, cen, rot, tok, m) for m in (mask, None)]


@case
def dparf_encode_bwd(hip, gpu):
    cen, rot, _ = _tokens_case(gpu, 50, 2)
    pts, g = _cloud(gpu, 129, 2), _rn(gpu, 29, 129, 2, 256)
    return lambda: hip.dparf_encode_bwd(pts, cen, rot, g)


@case
def latent_gather_bwd_ordered(hip, gpu):
    from test_gpu_train_maps import SHAPES, CH, _geometry
    (H, W), dims = SHAPES["33x17"]
    V, P = 2, 129
    _, cams, scale = _geometry(hip, gpu, H, W, V)
    pts = (torch.randn((P, 3), generator=torch.Generator().manual_seed(8)) * 0.6 + torch.tensor([0.0, 0.0, 3.0])).to(gpu)
    shapes = [(V, h, w, C) for (h, w), C in zip(dims, CH)]
    g, rgb_s = _rn(gpu, 30, P, V, 384), torch.rand((P, V, 4), generator=torch.Generator().manual_seed(5)).to(gpu)
    return lambda: hip.latent_gather_bwd_ordered(shapes, (H, W), pts, cams, scale, g, rgb_s=rgb_s)


def _targets(gpu, H=17, W=19):
    rs = np.random.RandomState(31)
    n = H * W
    dense = dict(ray_o=rs.uniform(-1, 1, (n, 3)).astype(np.float32), ray_d=rs.uniform(-1, 1, (n, 3)).astype(np.float32),
                 near=rs.uniform(0, 1, n).astype(np.float32), far=rs.uniform(1, 2, n).astype(np.float32),
                 mask_at_box=(rs.uniform(size=n) < 0.9).astype(np.uint8))
    msk = np.ones((H, W), np.uint8)
    msk[:2], msk[:, :2], msk[5:8, 6:9] = 0, 0, 100
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    return ({k: to(v) for k, v in dense.items()}, to(msk), to(np.ones((H, W), np.uint8)),
            to(rs.uniform(size=(H, W, 3)).astype(np.float32)), rs)


@case
def patch_rays(hip, gpu):
    from transhuman_amd import train_targets
    dense, msk, bound, img, rs = _targets(gpu)
    draws = torch.from_numpy(rs.uniform(size=(3, 2))).to(gpu)

    def run():
        raw = hip.patch_rays(dense, msk, bound, img, draws, 0.5, 5)
        counts = raw["counts"].cpu().numpy()
        return train_targets.assemble(raw, counts), counts
    return run


@case
def ray_sample_train(hip, gpu):
    dense, msk, bound, img, rs = _targets(gpu)
    nrays = 33
    draws = torch.from_numpy(rs.uniform(size=(4, 3, nrays))).to(gpu)

    def run():
        raw = hip.ray_sample_train(dense, msk, bound, img, draws, nrays, 0.5, 0.0)
        n = int(raw["info"][0])
        return {k: (v if k == "info" else v[:n]) for k, v in raw.items()}
    return run


@case
def ray_sample_test(hip, gpu):
    dense, _, _, img, _ = _targets(gpu)

    def run():
        raw = hip.ray_sample_test(dense, img, 17, 19)
        n = int(raw["info"][0])
        return {k: (v if k == "info" else v[:n]) for k, v in raw.items()}
    return run


@case
def truncate_select(hip, gpu):
    cen, _, _ = _tokens_case(gpu, 50, 2)
    pts = _cloud(gpu, 33 * 19, 3)
    return lambda: hip.truncate_select(pts, cen, 0.06)


@case
def ssim(hip, gpu):
    a = torch.rand((17, 19, 3), generator=torch.Generator().manual_seed(6)).to(gpu)
    b = (a + 0.1 * torch.rand((17, 19, 3), generator=torch.Generator().manual_seed(7)).to(gpu)).contiguous()
    return lambda: hip.ssim(a, b)


def _lpips_case(hip, gpu):
    rs = np.random.RandomState(32)
    cw = [torch.from_numpy((rs.standard_normal((co, ci, 3, 3)) * np.sqrt(2.0 / (9 * ci))).astype(np.float32)).to(gpu)
          for co, ci in hip.LPIPS_CONV_SHAPES]
    cb = [torch.from_numpy((rs.standard_normal(co) * 0.05).astype(np.float32)).to(gpu) for co, _ in hip.LPIPS_CONV_SHAPES]
    lin = [torch.from_numpy(rs.uniform(0, 1, (1, c, 1, 1)).astype(np.float32)).to(gpu) for c in hip.LPIPS_TAP_CHANNELS]
    a = torch.from_numpy(rs.uniform(-1, 1, (1, 3, 17, 19)).astype(np.float32)).to(gpu)
    b = torch.from_numpy(rs.uniform(-1, 1, (1, 3, 17, 19)).astype(np.float32)).to(gpu)
    return hip.lpips_pack(cw, cb, lin, gpu), hip.lpips_pack_bwd(cw, gpu), a, b


@case
def lpips(hip, gpu):
    packed, _, a, b = _lpips_case(hip, gpu)
    return lambda: hip.lpips(a, b, packed)


@case
def lpips_train_and_bwd(hip, gpu):
    """the training state and the backward's workspace are the caller's: allocated here, through the same hook"""
    packed, pkb, a, b = _lpips_case(hip, gpu)
    lib = hip.load_library()

    def run():
        state = hip._ws(lib.th_lpips_train_state_bytes(1, 17, 19), gpu)
        out, state = hip.lpips_train(a, b, packed, state=state)
        ws = hip._ws(lib.th_lpips_bwd_workspace_bytes(1, 17, 19), gpu)
        return out, hip.lpips_bwd(torch.ones(1, dtype=torch.float64), a, state, packed, pkb, workspace=ws)
    return run


@case
def marching_cubes(hip, gpu):
    cube = _rn(gpu, 33, 9, 7, 5)
    return lambda: [hip.marching_cubes(cube, 0.0), hip.marching_cubes(cube, 0.0, x_range=(2, 6))]


@case
def smpl_lbs(hip, gpu):
    model = hip.SmplModel(synth.make_smpl_model(), device=gpu)
    pose, beta = synth.make_smpl_pose()
    return lambda: model(torch.from_numpy(pose), beta)


@case
def color_jitter(hip, gpu):
    from transhuman_amd import preprocess
    img = torch.from_numpy(np.random.RandomState(34).randint(0, 256, (3, 17, 19, 3)).astype(np.uint8)).to(gpu)
    return lambda: preprocess.color_jitter(img, ((2, 0, 1, 3), 1.31, 0.58, 1.62, -0.17))


def _mesh(gpu):
    """50 vertices in front of two cameras, 19 + 17 faces in two components that share no vertex"""
    rs = np.random.RandomState(35)
    verts = rs.uniform(-0.5, 0.5, (50, 3))
    faces = np.stack([rs.choice(30, 3, replace=False) for _ in range(19)] + [30 + rs.choice(20, 3, replace=False) for _ in range(17)])
    R = np.stack([np.eye(3, dtype=np.float32)] * 2)
    T = np.array([[[0.0], [0.0], [3.0]], [[0.1], [-0.05], [2.5]]], np.float32)
    K = np.stack([np.array([[40.0, 0, 9.5], [0, 40.0, 8.5], [0, 0, 1]], np.float32)] * 2)
    return torch.from_numpy(verts).to(gpu), torch.from_numpy(faces.astype(np.int32)).to(gpu), R, T, K


@case
def mesh_clean(hip, gpu):
    from transhuman_amd import mesh_clean as mc
    verts, faces, *_ = _mesh(gpu)

    def run():
        v, f, info = mc.filter_components(verts, faces, keep="largest")
        return v, f, info["vert_map"], info["labels"], info["n_components"], info["kept_verts"], info["kept_faces"]
    return run


@case
def visibility(hip, gpu):
    from transhuman_amd import visibility as vz
    verts, faces, R, T, K = _mesh(gpu)
    return lambda: vz.rasterize_mesh(verts.float(), faces, R, T, K, 17, 19)


@case
def mesh_render(hip, gpu):
    from transhuman_amd import mesh_render as mr
    verts, faces, *_ = _mesh(gpu)
    return lambda: mr.vertex_normals(verts, faces)


def _frame(hip, gpu, net):
    """the smallest frame an existing test renders (test_gpu_parity: 32 x 32 rays, V = 3, N_c = 300)"""
    from transhuman_amd.config import get_cfg
    from transhuman_amd.networks.renderer import if_clight_renderer
    get_cfg().N_samples, get_cfg().num_class = 32, 300
    b = synth.batch_to(synth.make_batch(32, 32, 3, seed=0), gpu)
    r = if_clight_renderer.Renderer(net, vertex_can=can64().numpy(), pc2voxel_ind=synth_assign(300))
    return b, r.prepare_frame(b)


@case
def render_rays(hip, gpu, net=None):
    b, frame = _frame(hip, gpu, net)
    rows = slice(352, 352 + 17 * 19)                                       # 17 x 19 rays from the middle of the image, 33 samples each
    pts = lambda: hip.Points(*(b[k][0][rows] for k in ("ray_o", "ray_d", "near", "far")), n_samples=33)
    return lambda: hip.render_rays(net, frame, pts())


@case
def eval_sigma_grid(hip, gpu, net=None):
    b, frame = _frame(hip, gpu, net)
    world = b["tar_smpl_vertice"][0][:33 * 19] + _rn(gpu, 36, 33 * 19, 3, scale=0.03)
    return lambda: hip.eval_sigma_grid(net, frame, world)


@pytest.fixture
def cfg_restored():
    """_frame sets the two config values the renderer reads; later modules see what they were"""
    from transhuman_amd.config import get_cfg
    cfg = get_cfg()
    saved = (cfg.N_samples, cfg.num_class)
    yield
    cfg.N_samples, cfg.num_class = saved


@pytest.mark.parametrize("name", sorted(CASES))
def test_workspace_guards_stay_intact(hip, gpu, net, monkeypatch, cfg_restored, name):
    build = CASES[name]
    run = build(hip, gpu, net) if "net" in build.__code__.co_varnames[:build.__code__.co_argcount] else build(hip, gpu)
    want = _flat(run(), [])
    torch.cuda.synchronize()
    g = Guarded()
    monkeypatch.setattr(hip, "_ws", g.ws)
    monkeypatch.setattr(hip, "_cached_ws", g.ws)
    got = _flat(run(), [])
    torch.cuda.synchronize()
    monkeypatch.undo()
    g.check()
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, f"{name}: result {i} differs from the plain call's"
