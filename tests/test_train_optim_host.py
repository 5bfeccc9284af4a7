"""CPU: the optimiser's definition (train_optim.adam_step_oracle) against the reference's recorded torch.optim.Adam run and its
float64 run (tests/golden/g24_optim.npz, tools/gen_golden_optim.py), the closed-form schedule against the reference's recorded
learning rates, state_dict interchange with torch.optim.Adam, the checkpoint functions and the refusals.

Result of the oracle test on the committed fixture: worst err / bar = 0.364 (each of the 15 recorded arrays holds
err <= 4 max(err of the reference's fp32 run, 2^-24 max|tensor|); 0.25 is an error equal to the reference's own)."""
import copy
import os
import pickle

import numpy as np
import pytest
import torch

from transhuman_amd import hip
from transhuman_amd import train_optim as TO
from transhuman_amd import trainer as TR

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g24_optim.npz")
NAMES = ("w0", "b0", "w1", "b1")
KINDS = ("p", "exp_avg", "exp_avg_sq")


@pytest.fixture(scope="module")
def g24():
    d = np.load(GOLD)
    return {k: d[k] for k in d.files}


def replay(g, dtype):
    """adam_step_oracle over the recorded gradient sequence -> {name_kind: [epochs, n]} like the recorded runs"""
    epochs, spe = int(g["epochs"]), int(g["steps_per_epoch"])
    n_grads = g["grad_w0"].shape[0]
    state = {n: [g[f"init_{n}"].astype(dtype).reshape(-1), np.zeros(g[f"init_{n}"].size, dtype),
                 np.zeros(g[f"init_{n}"].size, dtype)] for n in NAMES}
    rec = {f"{n}_{k}": [] for n in NAMES for k in KINDS}
    step = 0
    for epoch in range(epochs):
        for _ in range(spe):
            step += 1
            for n in NAMES:
                grad = g[f"grad_{n}"][(step - 1) % n_grads].reshape(-1)
                p, m, v = state[n]
                state[n] = list(TO.adam_step_oracle(p, grad, m, v, lr=float(g["lr"][epoch]), step=step,
                                                    betas=tuple(g["betas"]), eps=float(g["eps"]), clip_value=float(g["clip"]),
                                                    dtype=dtype))
        for n in NAMES:
            for k, a in zip(KINDS, state[n]):
                rec[f"{n}_{k}"].append(a.copy())
    return {k: np.stack(v) for k, v in rec.items()}


def recorded(g, tag, n, k):
    """-> [(what, recorded array, selector of the replay's [epochs, n] array)]"""
    out = [(f"{n}.{k}", g[f"{tag}_{n}_{k}"], None)]
    if f"{tag}_{n}_{k}_last" in g:
        stride = int(g["stride"])
        out = [(f"{n}.{k}[::{stride}]", g[f"{tag}_{n}_{k}"], lambda a: a[:, ::stride]),
               (f"{n}.{k} (last epoch, whole)", g[f"{tag}_{n}_{k}_last"], lambda a: a[-1])]
    return out


def bar_ratio(got, ref32, ref64):
    """err / bar of the project's bar: err <= 4 max(error of the reference's own fp32 run, 2^-24 max|tensor|)"""
    ref64 = ref64.astype(np.float64)
    err = np.abs(got.astype(np.float64) - ref64).max()
    ref_err = np.abs(ref32.astype(np.float64) - ref64).max()
    bar = 4 * max(ref_err, 2.0 ** -24 * np.abs(ref64).max())
    return err / bar if bar > 0 else (0.0 if err == 0 else np.inf), err, bar


def test_fixture_holds_the_cases_it_is_for(g24):
    g = g24["grad_w0"].reshape(g24["grad_w0"].shape[0], -1)
    assert g.shape[1] == 4097
    assert (np.abs(g) > 40).any() and (g == 40).any() and (g == -40).any() and (g == 0).any()
    with np.errstate(over="ignore"):
        sq = g.astype(np.float32) ** 2
    tiny = np.finfo(np.float32).tiny
    assert ((sq > 0) & (sq < tiny)).any(), "no gradient whose square is a float32 subnormal"
    assert os.path.getsize(GOLD) < 700 * 1024


def test_oracle_fp32_against_the_reference_and_float64(g24):
    mine = replay(g24, np.float32)
    worst = 0.0
    for n in NAMES:
        for k in KINDS:
            for (what, r32, sel), (_, r64, _) in zip(recorded(g24, "f32", n, k), recorded(g24, "f64", n, k)):
                got = mine[f"{n}_{k}"] if sel is None else sel(mine[f"{n}_{k}"])
                assert got.shape == r64.shape and got.dtype == np.float32 and r64.dtype == np.float64
                ratio, err, bar = bar_ratio(got, r32, r64)
                print(f"{what:32s} err {err:.3e}  bar {bar:.3e}  err/bar {ratio:.3f}")
                assert np.isfinite(got).all()
                assert err <= bar, (what, err, bar)
                worst = max(worst, ratio)
    print(f"worst err / bar = {worst:.3f}")


def test_oracle_float64_form_is_the_reference_float64_run(g24):
    """the float64 form of the definition follows the reference's float64 run to double rounding (it is the yardstick the
    device tests use where no recorded run exists)"""
    mine = replay(g24, np.float64)
    for n in NAMES:
        for k in KINDS:
            for what, r64, sel in recorded(g24, "f64", n, k):
                got = mine[f"{n}_{k}"] if sel is None else sel(mine[f"{n}_{k}"])
                scale = np.abs(r64).max()
                assert np.abs(got - r64).max() <= 2.0 ** -40 * scale, what


def test_schedule_matches_the_recorded_learning_rates(g24):
    base, W, D, end = float(g24["base_lr"]), int(g24["warmup_epochs"]), int(g24["decay_epochs"]), float(g24["end_lr"])
    lr = g24["lr"]
    assert lr[0] == base and lr[1] == 0.0 and lr[W + 1] == base
    net = torch.nn.Linear(3, 2)
    cfg = _cfg(base, W, D, end)
    opt = TO.make_optimizer(cfg, net)
    assert isinstance(opt, TO.DeviceAdam) and len(opt.param_groups) == 2 and opt.clip_value == 40.0
    sch = TO.make_lr_scheduler(cfg, opt)
    for epoch in range(D):
        for group in opt.param_groups:
            got = group["lr"]
            if lr[epoch] == 0.0:
                assert got == 0.0                                        # the exact 0 of epoch 1
            else:
                assert abs(got - lr[epoch]) <= 1e-12 * abs(lr[epoch]), (epoch, got, lr[epoch])
        assert TO.warmup_cosine_lr(epoch, base, W, D, end) == opt.param_groups[0]["lr"]
        sch.step()


def _cfg(lr=7e-4, warmup=3, decay=12, end_lr=1e-6, optim="adam", wd=0.0, **kw):
    from types import SimpleNamespace
    return SimpleNamespace(train=SimpleNamespace(optim=optim, lr=lr, weight_decay=wd, epoch=decay, scheduler=SimpleNamespace(
        type="cosine", warmup_epochs=warmup, decay_epochs=decay, end_lr=end_lr)), **kw)


def test_config_mirrors_the_training_keys():
    from transhuman_amd.config import _defaults
    c = _defaults()
    assert (c.train.optim, c.train.lr, c.train.weight_decay) == ("adam", 7e-4, 0)
    s = c.train.scheduler
    assert (s.type, s.warmup_epochs, s.decay_epochs, s.end_lr) == ("cosine", 300, 3000, 1e-6)
    assert (c.ep_iter, c.save_freq) == (500, 5)


def _mlp(seed=0, dtype=torch.float32):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.ReLU(), torch.nn.Linear(5, 3)).to(dtype)


def _one_group_per_parameter(net, lr=1e-3):
    return [{"params": [p], "lr": lr, "weight_decay": 0} for p in net.parameters()]


def _stepped_torch_adam(net, steps=3, seed=1):
    opt = torch.optim.Adam(_one_group_per_parameter(net), 1e-3)
    gen = torch.Generator().manual_seed(seed)
    for _ in range(steps):
        for p in net.parameters():
            p.grad = torch.randn(p.shape, generator=gen)
        opt.step()
    return opt


def test_state_dict_moves_between_device_adam_and_torch_adam():
    net = _mlp()
    ref = _stepped_torch_adam(net)
    sd_ref = ref.state_dict()
    mine = TO.DeviceAdam(_one_group_per_parameter(net), 1e-3)
    mine.load_state_dict(sd_ref)                                         # torch -> DeviceAdam
    sd = mine.state_dict()                                               # ... and what DeviceAdam writes
    assert sd["state"].keys() == sd_ref["state"].keys()
    for i, st in sd["state"].items():
        assert st.keys() == sd_ref["state"][i].keys() == {"step", "exp_avg", "exp_avg_sq"}
        for k, v in st.items():
            assert v.dtype == sd_ref["state"][i][k].dtype and torch.equal(v, sd_ref["state"][i][k]), (i, k)
        assert float(st["step"]) == 3.0
    assert [g.keys() for g in sd["param_groups"]] == [g.keys() for g in sd_ref["param_groups"]]
    # DeviceAdam -> torch.optim.Adam on a CPU copy, which then continues exactly as the original does
    net2 = _mlp()
    net2.load_state_dict(net.state_dict())
    cont = torch.optim.Adam(_one_group_per_parameter(net2), 1e-3)
    cont.load_state_dict(copy.deepcopy(sd))               # (load_state_dict adopts the tensors it is given)
    gen = torch.Generator().manual_seed(5)
    for (p, q) in zip(net.parameters(), net2.parameters()):
        p.grad = torch.randn(p.shape, generator=gen)
        q.grad = p.grad.clone()
    ref.step()
    cont.step()
    for p, q in zip(net.parameters(), net2.parameters()):
        assert torch.equal(p, q)
    assert all(float(cont.state[q]["step"]) == 4.0 for q in net2.parameters())
    # a checkpoint of an older torch, whose step is a plain number, is adopted too
    sd_old = ref.state_dict()
    for st in sd_old["state"].values():
        st["step"] = int(st["step"])
    mine.load_state_dict(sd_old)
    assert mine.state_dict()["state"].keys() == sd_ref["state"].keys()


def test_checkpoint_round_trip(tmp_path):
    cfg = _cfg()
    net = _mlp()
    ref = _stepped_torch_adam(net)
    opt = TO.make_optimizer(cfg, net)
    opt.load_state_dict({"state": ref.state_dict()["state"], "param_groups": opt.state_dict()["param_groups"]})
    sch = TO.make_lr_scheduler(cfg, opt)
    for _ in range(3):
        sch.step()                                                       # the state behind epoch 2: epoch 3 trains next
    rec = TR.Recorder()
    rec.step = 1500
    path = TR.save_model(net, opt, sch, rec, str(tmp_path), epoch=2)
    assert os.path.basename(path) == "3.pth"
    assert os.path.basename(TR.save_model(net, opt, sch, rec, str(tmp_path), epoch=2, last=True)) == "latest.pth"
    model = torch.load(path, map_location="cpu", weights_only=True)      # plain numbers and tensors only
    assert set(model) == {"net", "optim", "scheduler", "recorder", "epoch"} and model["epoch"] == 2

    net2 = _mlp(seed=9)
    opt2 = TO.make_optimizer(cfg, net2)
    sch2 = TO.make_lr_scheduler(cfg, opt2)
    rec2 = TR.Recorder()
    begin = TR.load_model(net2, opt2, sch2, rec2, str(tmp_path))
    assert begin == 3 and rec2.step == 1500
    for (k, a), (_, b) in zip(net.state_dict().items(), net2.state_dict().items()):
        assert torch.equal(a, b), k
    s1, s2 = opt.state_dict(), opt2.state_dict()
    assert s1["state"].keys() == s2["state"].keys()
    for i in s1["state"]:
        for k in s1["state"][i]:
            assert torch.equal(s1["state"][i][k], s2["state"][i][k])
    want = TO.warmup_cosine_lr(3, cfg.train.lr, 3, 12, 1e-6)
    assert [g["lr"] for g in opt2.param_groups] == [want] * len(opt2.param_groups) == [g["lr"] for g in opt.param_groups]
    sch.step()
    sch2.step()
    assert opt2.param_groups[0]["lr"] == opt.param_groups[0]["lr"] == TO.warmup_cosine_lr(4, cfg.train.lr, 3, 12, 1e-6)
    # resume=False starts from scratch and leaves the directory alone
    assert TR.load_model(_mlp(), TO.make_optimizer(cfg, _mlp()), sch2, TR.Recorder(), str(tmp_path), resume=False) == 0
    assert sorted(os.listdir(tmp_path)) == ["3.pth", "latest.pth"]
    assert TR.load_model(net2, opt2, sch2, rec2, str(tmp_path / "absent")) == 0


class _ForeignScheduler:
    """stands for the reference's WarmupLR: its state_dict holds a bound method of its own class"""

    def _warmup_linear(self, start, end, pct):
        return (end - start) * pct + start

    def state_dict(self):
        return {"wrapped": {"T_max": 9, "last_epoch": 0}, "wrapper": {"_warmup_func": self._warmup_linear, "_step_count": 6}}


def test_checkpoint_with_an_unreadable_scheduler_entry_resumes_from_epoch(tmp_path):
    cfg = _cfg()
    net = _mlp()
    ref = _stepped_torch_adam(net)                                       # a torch.optim.Adam checkpoint, as the reference writes
    model = {"net": net.state_dict(), "optim": ref.state_dict(), "scheduler": _ForeignScheduler().state_dict(),
             "recorder": {"step": 2500}, "epoch": 4}
    torch.save(model, str(tmp_path / "latest.pth"))
    with pytest.raises(pickle.UnpicklingError):
        torch.load(str(tmp_path / "latest.pth"), map_location="cpu", weights_only=True)
    net2 = _mlp(seed=9)
    opt2 = TO.make_optimizer(cfg, net2)
    sch2 = TO.make_lr_scheduler(cfg, opt2)
    rec2 = TR.Recorder()
    assert TR.load_model(net2, opt2, sch2, rec2, str(tmp_path)) == 5
    assert rec2.step == 2500 and sch2.last_epoch == 5
    assert opt2.param_groups[0]["lr"] == TO.warmup_cosine_lr(5, cfg.train.lr, 3, 12, 1e-6)
    for p, q in zip(net.parameters(), net2.parameters()):
        assert torch.equal(p, q)
        assert torch.equal(ref.state[p]["exp_avg_sq"], opt2.state[q]["exp_avg_sq"])
        assert float(opt2.state[q]["step"]) == 3.0


def test_refusals():
    net = _mlp()
    for flag in ("amsgrad", "maximize", "capturable", "differentiable"):
        with pytest.raises(ValueError, match=flag):
            TO.DeviceAdam(net.parameters(), 1e-3, **{flag: True})
    with pytest.raises(ValueError):
        TO.make_optimizer(_cfg(optim="sgd"), net)
    for bad in (_mlp(), _mlp(dtype=torch.float64)):                      # a CPU parameter, a float64 parameter
        opt = TO.DeviceAdam(bad.parameters(), 1e-3)
        for p in bad.parameters():
            p.grad = torch.ones_like(p)
        before = [p.detach().clone() for p in bad.parameters()]
        with pytest.raises(hip.HipError):
            opt.step()
        assert all(torch.equal(a, b) for a, b in zip(before, bad.parameters())) and len(opt.state) == 0
    # a group that arrives through load_state_dict asking for amsgrad is refused by the step, not ignored
    opt = TO.DeviceAdam(net.parameters(), 1e-3)
    opt.param_groups[0]["amsgrad"] = True
    with pytest.raises(ValueError, match="amsgrad"):
        opt.step()


def test_table_sizes_are_pure_host_calls():
    lib = hip.load_library()
    chunk = hip.adam_chunk_elems()
    assert chunk % 1024 == 0 and chunk >= 1024
    assert lib.th_adam_table_bytes(0, 10) == 0 and lib.th_adam_table_bytes(3, 0) == 0
    small, large = lib.th_adam_table_bytes(293, 10_000_000), lib.th_adam_table_bytes(293, 20_000_000)
    assert 293 * 72 < small < large
    assert np.dtype(hip.ADAM_TENSOR_FIELDS).itemsize == 72


def test_recorder_smooths_and_counts():
    rec = TR.Recorder()
    for i in range(30):
        rec.update_loss_stats({"loss": torch.tensor(float(i))})
        rec.step += 1
    assert rec.loss_stats["loss"].avg == pytest.approx(sum(range(10, 30)) / 20) and rec.loss_stats["loss"].global_avg == 14.5
    assert rec.state_dict() == {"step": 30} and "loss" in str(rec)
