"""GPU: adam_step_kernel (K22) through train_optim.DeviceAdam against its numpy definition (adam_step_oracle) bit for bit,
against torch.optim.Adam on the device with both held to float64, the ring of staging buffers, the version counters that make
the renderer re-pack its weights, and one iteration of trainer.Trainer.train.

"Bit for bit" compares the 32-bit patterns of every element that is not a NaN in the oracle (signed zeros, subnormals and
infinities included) and requires a NaN exactly where the oracle has one: IEEE 754 leaves the sign and payload of a NaN that an
operation produces open, and x86 (the oracle) and gfx950 choose differently (inf - inf is 0xffc00000 on one, 0x7fc00000 on the
other)."""
import contextlib
import copy

import numpy as np
import pytest
import torch

from transhuman_amd import config, train_optim as TO
from train_step_case import STEP_CFG, setup

pytestmark = pytest.mark.gpu

BETAS, EPS = (0.9, 0.999), 1e-8
STEPS = 5


@pytest.fixture(scope="module")
def hip(gpu):
    from transhuman_amd import hip as H
    H.load_library()
    return H


def sizes_mixed(chunk):
    """320 element counts: the edges of the float4 path, of a 256-lane round and of a chunk, then seeded fill"""
    edge = [1, 3, 4, 5, 255, 256, 257, chunk - 1, chunk, chunk + 1, 2 * chunk + 5, 3 * chunk]
    rs = np.random.RandomState(22)
    rest = [int(x) for x in np.exp(rs.uniform(0, np.log(3000), 320 - len(edge)))]
    return edge + rest


def grads_of(kind, n, rs):
    g = (rs.standard_normal(n) * np.exp(rs.uniform(-8, 3, n))).astype(np.float32)
    pick = rs.uniform(size=n)
    if kind == "edges":
        vals = np.array([40.0, -40.0, 40.000004, -40.000004, 39.999996, 1e3, -1e3, 3.4e38, -3.4e38, 0.0, -0.0], np.float32)
        g = np.where(pick < 0.6, vals[rs.randint(0, len(vals), n)], g)
    elif kind == "zeros":
        g = np.zeros(n, np.float32)
    elif kind == "subnormal":
        vals = np.array([1e-20, -3e-21, 2e-23, 1e-38, -1e-40, 1.4e-45], np.float32)     # squares: subnormal or 0
        g = np.where(pick < 0.7, vals[rs.randint(0, len(vals), n)], g)
    elif kind == "nonfinite":
        vals = np.array([np.nan, np.inf, -np.inf], np.float32)
        g = np.where(pick < 0.15, vals[rs.randint(0, 3, n)], g)
    return g.astype(np.float32)


# name: (gradient kind, optimiser options, lr)
CASES = {
    "general": ("general", {}, 7e-4),
    "general_clip": ("general", {"clip_value": 40.0}, 7e-4),
    "edges_clip": ("edges", {"clip_value": 40.0}, 7e-4),
    "edges_noclip": ("edges", {}, 7e-4),
    "zeros": ("zeros", {"clip_value": 40.0}, 7e-4),
    "lr0": ("general", {"clip_value": 40.0}, 0.0),
    "subnormal": ("subnormal", {"clip_value": 40.0}, 7e-4),
    "nonfinite_clip": ("nonfinite", {"clip_value": 40.0, "count_nonfinite": True}, 7e-4),
    "nonfinite_noclip": ("nonfinite", {"count_nonfinite": True}, 7e-4),
    "coupled_wd": ("general", {"clip_value": 40.0, "weight_decay": 0.01}, 7e-4),
    "decoupled_wd": ("general", {"clip_value": 40.0, "weight_decay": 0.01, "decoupled_weight_decay": True}, 7e-4),
    "zero_grad": ("general", {"clip_value": 40.0, "zero_grad": True}, 7e-4),
}


def _offset_tensor(a, gpu, off):
    """a device copy of ``a`` that starts ``off`` floats past a 16-byte boundary (a contiguous view of a larger buffer)"""
    buf = torch.zeros(a.size + 4, dtype=torch.float32, device=gpu)
    assert buf.data_ptr() % 16 == 0
    t = buf[off:off + a.size]
    t.copy_(torch.from_numpy(a))
    return t


def make_set(sizes, gpu, seed, kind, steps):
    """initial parameters and per-step gradients (numpy), device parameters; tensor 1 starts 4 bytes past a 16-byte boundary,
    tensor 2's GRADIENT does, tensor 5 never gets a gradient"""
    rs = np.random.RandomState(seed)
    init = [(rs.standard_normal(n) * 0.1).astype(np.float32) for n in sizes]
    grads = [[grads_of(kind, n, rs) for n in sizes] for _ in range(steps)]
    params = []
    for i, a in enumerate(init):
        t = _offset_tensor(a, gpu, 1) if i == 1 else torch.from_numpy(a).to(gpu)
        params.append(t.requires_grad_(True))
    assert params[1].data_ptr() % 16 == 4 and params[1].is_contiguous()
    return init, grads, params


NO_GRAD = 5


def set_grads(params, grads_step, gpu, keep=False):
    for i, (p, g) in enumerate(zip(params, grads_step)):
        if i == NO_GRAD:
            continue
        if keep and p.grad is not None:
            p.grad.copy_(torch.from_numpy(g))
        else:
            p.grad = _offset_tensor(g, gpu, 1) if i == 2 else torch.from_numpy(g).to(gpu)


def run_device(params, grads, gpu, lrs, opts, keep_grads=False):
    opt = TO.DeviceAdam([{"params": [p], "lr": lrs[0]} for p in params], lrs[0], betas=BETAS, eps=EPS, **opts)
    for s, gs in enumerate(grads):
        for group in opt.param_groups:
            group["lr"] = lrs[s]
        set_grads(params, gs, gpu, keep=keep_grads)
        opt.step()
    return opt


def run_oracle(init, grads, lrs, opts, dtype=np.float32):
    state = [[a.astype(dtype), np.zeros(a.size, dtype), np.zeros(a.size, dtype)] for a in init]
    kw = {k: v for k, v in opts.items() if k in ("clip_value", "weight_decay", "decoupled_weight_decay")}
    for s, gs in enumerate(grads):
        for i, g in enumerate(gs):
            if i == NO_GRAD:
                continue
            state[i] = list(TO.adam_step_oracle(*state[i][:1], g, *state[i][1:], lr=lrs[s], step=s + 1, betas=BETAS, eps=EPS,
                                                dtype=dtype, **kw))
    return state


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaNs elsewhere than in the oracle"
    a, b = got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, f"{what}: {bad.size} of {a.size} elements differ, first at {bad[0]}: {a[bad[0]]:#x} != {b[bad[0]]:#x}"


def device_state(opt, params):
    out = []
    for i, p in enumerate(params):
        st = opt.state.get(p, {})
        out.append((p.detach().cpu().numpy(), st["exp_avg"].cpu().numpy() if st else None,
                    st["exp_avg_sq"].cpu().numpy() if st else None, float(st["step"]) if st else None))
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_device_equals_the_oracle_bit_for_bit(hip, gpu, case):
    """320 mixed tensors in one launch, 5 consecutive steps"""
    kind, opts, lr = CASES[case]
    chunk = hip.adam_chunk_elems()
    sizes = sizes_mixed(chunk)
    assert len(sizes) == 320 and {1, 3, 4, 5, 255, 256, 257, chunk - 1, chunk, chunk + 1} <= set(sizes)
    init, grads, params = make_set(sizes, gpu, 100, kind, STEPS)
    lrs = [lr] * STEPS
    versions = [p._version for p in params]
    opt = run_device(params, grads, gpu, lrs, opts, keep_grads=bool(opts.get("zero_grad")))
    want = run_oracle(init, grads, lrs, opts)
    got = device_state(opt, params)
    for i in range(len(sizes)):
        p, m, v, step = got[i]
        if i == NO_GRAD:
            assert m is None and params[i] not in opt.state and params[i]._version == versions[i]
            same_bits(p, init[i], "the parameter without a gradient")
            continue
        assert step == STEPS and params[i]._version > versions[i]
        for name, a, b in (("p", p, want[i][0]), ("exp_avg", m, want[i][1]), ("exp_avg_sq", v, want[i][2])):
            same_bits(a, b, f"{case}: tensor {i} ({sizes[i]} elements) {name}")
    if lr == 0.0:
        for i in range(len(sizes)):
            same_bits(got[i][0], init[i], "lr = 0 leaves the parameters alone")
        assert any(np.abs(got[i][1]).max() > 0 for i in range(len(sizes)) if i != NO_GRAD)
    if opts.get("count_nonfinite"):
        n_bad = sum(int((~np.isfinite(g)).sum()) for gs in grads for i, g in enumerate(gs) if i != NO_GRAD)
        assert n_bad > 100 and opt.nonfinite_count() == n_bad
    if opts.get("zero_grad"):
        for i, p in enumerate(params):
            if i != NO_GRAD:
                assert p.grad is not None and not bool(p.grad.view(torch.int32).any()), f"gradient {i} is not exact zeros"
        ptrs = [p.grad.data_ptr() for i, p in enumerate(params) if i != NO_GRAD]
        opt.zero_grad()
        assert ptrs == [p.grad.data_ptr() for i, p in enumerate(params) if i != NO_GRAD]       # kept allocated
        params[0].grad.fill_(3.0)                                                             # ... and a written one is cleared
        opt.zero_grad()
        assert float(params[0].grad.abs().max()) == 0.0


def test_ring_of_staging_buffers_under_a_running_queue(hip, gpu):
    """40 steps with a different lr each, queued without a host synchronisation behind a few tens of milliseconds of other
    work, so that every copy is still pending when the host reaches the next step: the 16 staging buffers are reused twice
    and a buffer rewritten before its copy has left would hand a later step's lr to an earlier one"""
    n_steps = 40
    sizes = [4 * 4097, 257, 5]
    rs = np.random.RandomState(7)
    init = [(rs.standard_normal(n) * 0.1).astype(np.float32) for n in sizes]
    gsets = [[grads_of("general", n, rs) for n in sizes] for _ in range(4)]
    lrs = [1e-4 * (s + 1) for s in range(n_steps)]
    params = [torch.from_numpy(a).to(gpu).requires_grad_(True) for a in init]
    dgrads = [[torch.from_numpy(g).to(gpu) for g in gs] for gs in gsets]
    opt = TO.DeviceAdam([{"params": [p]} for p in params], 1e-3, betas=BETAS, eps=EPS, clip_value=40.0)
    busy = torch.randn(4096, 4096, device=gpu)
    torch.cuda.synchronize()
    for _ in range(30):
        busy = (busy @ busy) * 1e-4
    for s in range(n_steps):
        for group in opt.param_groups:
            group["lr"] = lrs[s]
        for p, g in zip(params, dgrads[s % 4]):
            p.grad = g
        opt.step()
    state = [[a, np.zeros_like(a), np.zeros_like(a)] for a in init]
    for s in range(n_steps):
        for i in range(len(sizes)):
            state[i] = list(TO.adam_step_oracle(*state[i][:1], gsets[s % 4][i], *state[i][1:], lr=lrs[s], step=s + 1, betas=BETAS,
                                                eps=EPS, clip_value=40.0))
    for i, p in enumerate(params):
        same_bits(p.detach().cpu().numpy(), state[i][0], f"tensor {i} p after {n_steps} queued steps")
        same_bits(opt.state[p]["exp_avg_sq"].cpu().numpy(), state[i][2], f"tensor {i} exp_avg_sq")


def test_two_runs_give_identical_bits(hip, gpu):
    sizes = sizes_mixed(hip.adam_chunk_elems())[:40]
    runs = []
    for _ in range(2):
        init, grads, params = make_set(sizes, gpu, 3, "nonfinite", STEPS)
        opt = run_device(params, grads, gpu, [7e-4] * STEPS, {"clip_value": 40.0, "weight_decay": 0.01})
        runs.append(device_state(opt, params))
    for (p0, m0, v0, _), (p1, m1, v1, _) in zip(*runs):
        for a, b in ((p0, p1), (m0, m1), (v0, v1)):
            assert (a is None and b is None) or np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_against_torch_adam_on_the_device(hip, gpu):
    """5 steps from the same state and gradients: DeviceAdam and torch.optim.Adam + clip_grad_value_, each against the float64
    form of the definition, err <= 4 max(torch's err, 2^-24 max|tensor|)"""
    sizes = [4097, 257, 3 * hip.adam_chunk_elems() + 1, 64]
    init, grads, params = make_set(sizes, gpu, 11, "edges", STEPS)
    lrs = [7e-4, 0.0, 2e-4, 7e-4, 5e-4]
    opts = {"clip_value": 40.0}
    opt = run_device(params, grads, gpu, lrs, opts)
    tparams = [torch.from_numpy(a).to(gpu).requires_grad_(True) for a in init]
    topt = torch.optim.Adam([{"params": [p], "lr": lrs[0], "weight_decay": 0} for p in tparams], lrs[0], betas=BETAS, eps=EPS)
    for s, gs in enumerate(grads):
        for group in topt.param_groups:
            group["lr"] = lrs[s]
        set_grads(tparams, gs, gpu)
        torch.nn.utils.clip_grad_value_(tparams, 40.0)
        topt.step()
    want = run_oracle(init, grads, lrs, opts, dtype=np.float64)
    for i in range(len(sizes)):
        if i == NO_GRAD:
            continue
        mine = (params[i].detach(), opt.state[params[i]]["exp_avg"], opt.state[params[i]]["exp_avg_sq"])
        ref = (tparams[i].detach(), topt.state[tparams[i]]["exp_avg"], topt.state[tparams[i]]["exp_avg_sq"])
        for name, a, b, w in zip(("p", "exp_avg", "exp_avg_sq"), mine, ref, want[i]):
            err = np.abs(a.cpu().numpy().astype(np.float64) - w).max()
            ref_err = np.abs(b.cpu().numpy().astype(np.float64) - w).max()
            bar = 4 * max(ref_err, 2.0 ** -24 * np.abs(w).max())
            print(f"tensor {i} {name}: err {err:.3e}  torch's {ref_err:.3e}  bar {bar:.3e}")
            assert err <= bar, (i, name, err, bar)


def test_refusals_on_the_device(hip, gpu):
    p64 = torch.zeros(8, dtype=torch.float64, device=gpu, requires_grad=True)
    p64.grad = torch.ones_like(p64)
    with pytest.raises(hip.HipError, match="float64"):
        TO.DeviceAdam([p64], 1e-3).step()
    pt = torch.zeros(8, 6, device=gpu).t().requires_grad_(True)                  # not contiguous
    pt.grad = torch.ones_like(pt)
    with pytest.raises(hip.HipError, match="contiguous"):
        TO.DeviceAdam([pt], 1e-3).step()
    # a non-contiguous GRADIENT is made contiguous first
    p = torch.zeros(6, 8, device=gpu, requires_grad=True)
    p.grad = torch.ones(8, 6, device=gpu).t()
    assert not p.grad.is_contiguous()
    opt = TO.DeviceAdam([p], 1e-3)
    opt.step()
    assert p.grad.is_contiguous() and float(p.detach().max()) < 0
    # the C entry refuses a host pointer with an error code
    import ctypes as C
    plan = hip.AdamPlan([p])
    tab = np.zeros(1, dtype=plan.dtype)
    host = np.zeros(48, np.float32)
    tab["p"], tab["g"], tab["m"], tab["v"] = host.ctypes.data, p.grad.data_ptr(), p.grad.data_ptr(), p.grad.data_ptr()
    with pytest.raises(hip.HipError, match="not a device pointer"):
        plan.step(tab, check_pointers=True)
    assert C.sizeof(C.c_void_p) == 8


def test_version_counters_make_the_renderer_take_the_new_weights(hip, gpu):
    """render_fast, one DeviceAdam step through raw pointers, render_fast: the second image is the one a fresh Network loaded
    from the stepped state_dict renders -- hip._sync_weights saw the bumped version counters and re-packed the weight images"""
    from transhuman_amd.networks.cross_transformer import Network
    from transhuman_amd.networks.renderer.if_clight_renderer import Renderer
    from util import can64, synth_assign
    with config.override(**STEP_CFG):
        model, r, b = setup(gpu)
        with torch.no_grad():
            first = r.render_fast(b, is_train=False)["rgb_map"].clone()
        gen = torch.Generator().manual_seed(4)
        for p in model.parameters():
            p.grad = torch.randn(p.shape, generator=gen).to(gpu)
        before = [p._version for p in model.parameters()]
        TO.DeviceAdam([{"params": [p]} for p in model.parameters()], 1e-2, clip_value=40.0).step()
        assert all(p._version > v for p, v in zip(model.parameters(), before))
        with torch.no_grad():
            second = r.render_fast(b, is_train=False)["rgb_map"].clone()
        assert float((second - first).abs().max()) > 1e-4
        torch.manual_seed(1)
        fresh = Network()
        fresh.load_state_dict({k: v.detach().cpu().clone() for k, v in model.state_dict().items()})
        fresh.train()
        r2 = Renderer(fresh.to(gpu), vertex_can=can64().numpy(), pc2voxel_ind=synth_assign(300))
        with torch.no_grad():
            third = r2.render_fast(b, is_train=False)["rgb_map"]
        assert torch.equal(second, third)


def test_one_iteration_of_the_trainer(hip, gpu, tmp_path, monkeypatch):
    """Trainer.train over the golden training step's batch with DeviceAdam and with the reference's form (torch.optim.Adam,
    one group per parameter, clip_grad_value_), on two copies of one net.  Each run's update is held to the float64 form of
    the definition applied to that run's own gradients (captured in front of its step), with the bar
    err <= 4 max(torch's err, 2^-24 max|tensor|); DeviceAdam's is also its fp32 definition bit for bit.

    The two forwards run under torch.use_deterministic_algorithms(True, warn_only=True), as the compared renders of
    tests/test_gpu_train_targets.py do: without it two forwards of ONE net on one batch already differ (measured on an MI355X,
    the same module called twice: loss 0.2975472538485896 and 0.29754725376271673; LOG.md, K18 entry), which says nothing
    about the optimiser."""
    from test_gpu_lpips_grad import SEED
    from test_lpips_host import write_weight_files
    from test_train_loss_host import golden, golden_lin
    from transhuman_amd.lpips import LPIPS
    from transhuman_amd.networks.renderer.if_clight_renderer import Renderer
    from transhuman_amd.train_loss import NetworkWrapper
    from transhuman_amd.trainer import Recorder, Trainer
    from util import can64, synth_assign
    with config.override(**STEP_CFG) as cfg, contextlib.ExitStack() as at_exit:
        at_exit.callback(torch.use_deterministic_algorithms, False)
        model, _, b = setup(gpu)
        monkeypatch.setattr(cfg, "l2rec_weight", 1.0, raising=False)
        monkeypatch.setattr(cfg, "lpips_weight", 0.1, raising=False)
        pv, pl = write_weight_files(str(tmp_path), SEED, golden_lin(golden()))
        lp_mod = LPIPS(net="vgg", vgg16_path=pv, model_path=pl, device=gpu)
        n, P = int(b["ray_o"].shape[1]), 20
        n_patch = -(-n // (P * P))
        masks = torch.zeros(n_patch * P * P, dtype=torch.bool)
        masks[:n] = True
        masks = masks.reshape(n_patch, P, P)
        div = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(masks.reshape(n_patch, -1).sum(1), 0)])
        gen = torch.Generator().manual_seed(0)
        b = dict(b, patch_masks=masks[None].to(gpu), patch_div_indices=div[None],
                 target_patches=torch.rand((1, n_patch, P, P, 3), generator=gen).to(gpu))
        lr = 7e-4
        init = {k: p.detach().cpu().numpy().copy() for k, p in model.named_parameters()}

        def run(make_opt):
            net = copy.deepcopy(model)
            r = Renderer(net, vertex_can=can64().numpy(), pc2voxel_ind=synth_assign(300))
            opt = make_opt(net)
            grads = {}
            opt.register_step_pre_hook(lambda *a: grads.update(
                {k: p.grad.detach().cpu().numpy().copy() for k, p in net.named_parameters() if p.grad is not None}))
            rec = Recorder()
            Trainer(NetworkWrapper(net, renderer=r, lpips=lp_mod), device=gpu).train(0, [b], opt, rec)
            assert rec.step == 1
            return net, opt, grads, rec.loss_stats["loss"].global_avg

        groups = lambda net: [{"params": [p], "lr": lr, "weight_decay": 0} for p in net.parameters()]     # noqa: E731
        torch.use_deterministic_algorithms(True, warn_only=True)
        net_d, opt_d, g_d, loss_d = run(lambda net: TO.DeviceAdam(groups(net), lr))
        net_t, opt_t, g_t, loss_t = run(lambda net: torch.optim.Adam(groups(net), lr))
        torch.use_deterministic_algorithms(False)
        assert opt_d.clip_value == 40.0                                    # the trainer's clip, taken into the kernel
        print(f"loss {loss_d!r} (DeviceAdam run) {loss_t!r} (torch run)")
        assert loss_d == loss_t and np.isfinite(loss_d)
        assert g_d.keys() == g_t.keys() and len(g_d) > 20
        pd, pt = dict(net_d.named_parameters()), dict(net_t.named_parameters())
        worst = 0.0
        for k, p0 in init.items():
            got = pd[k].detach().cpu().numpy()
            if k not in g_d:
                same_bits(got, p0, f"{k} (no gradient)")
                assert pd[k] not in opt_d.state
                continue
            zeros = np.zeros(p0.size, np.float32)
            kw = dict(lr=lr, step=1, betas=BETAS, eps=EPS, clip_value=40.0)
            w32 = TO.adam_step_oracle(p0.reshape(-1), g_d[k].reshape(-1), zeros, zeros, **kw)[0]
            same_bits(got.reshape(-1), w32, k)
            w64_d = TO.adam_step_oracle(p0.reshape(-1), g_d[k].reshape(-1), zeros, zeros, dtype=np.float64, **kw)[0]
            w64_t = TO.adam_step_oracle(p0.reshape(-1), g_t[k].reshape(-1), zeros, zeros, dtype=np.float64, **kw)[0]
            err = np.abs(got.reshape(-1).astype(np.float64) - w64_d).max()
            ref_err = np.abs(pt[k].detach().cpu().numpy().reshape(-1).astype(np.float64) - w64_t).max()
            bar = 4 * max(ref_err, 2.0 ** -24 * np.abs(w64_d).max())
            worst = max(worst, err / bar)
            assert err <= bar, (k, err, bar)
        print(f"worst err / bar over {len(g_d)} parameters: {worst:.3f}")
