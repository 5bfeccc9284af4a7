"""Write tests/golden/g24_optim.npz: a recorded run of the reference's own optimiser and schedule.

    python tools/gen_golden_optim.py --reference <reference checkout> [--seed 24]

CPU only, where the reference checkout exists.  The reference's ``make_optimizer`` (lib/train/optimizer.py: torch.optim.Adam,
one parameter group per tensor) and ``make_lr_scheduler`` (lib/train/scheduler.py: CosineAnnealingLR inside the WarmupLR wrapper
of lib/utils/optimizer/lr_scheduler.py) are built on a small seeded MLP -- Linear(241, 17) -> Linear(17, 3); the first weight
has 4097 elements -- with lr 7e-4, warmup_epochs 3, decay_epochs 12, end_lr 1e-6, and driven for 16 epochs of two steps each
(``clip_grad_value_(., 40)`` + ``step()``, then ``scheduler.step()`` per epoch, as train_net.py does), once with the module in
float32 and once in float64.  The four modules are loaded by file path: importing the ``lib.train`` package would pull in the
whole training stack.

The gradients are inputs, not functions of the parameters: N_GRADS seeded sets, step s taking set s % N_GRADS.  They hold
values beyond +-40, exactly +-40, zeros and magnitudes whose square is a float32 subnormal.

Stored, as plain arrays only: the initial parameters, the gradient sets, the learning rate of every epoch and the two recorded
runs (p, exp_avg, exp_avg_sq after every epoch).  To stay well under the size limit of a committed file, the per-epoch record of
the 4097-element tensor holds every 8th element (the update is elementwise; the last element, 4096, is one of them) and the
full tensor is stored after the last epoch; the small tensors are stored whole at every epoch.
"""
import argparse
import importlib.util
import os
import sys
import types
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPOCHS, STEPS_PER_EPOCH, N_GRADS, STRIDE = 16, 2, 8, 8
LR, WARMUP, DECAY, END_LR, CLIP = 7e-4, 3, 12, 1e-6, 40.0
SHAPES = [("w0", (17, 241)), ("b0", (17,)), ("w1", (3, 17)), ("b1", (3,))]


def _load_reference(reference):
    """the reference's optimizer.py / scheduler.py and the two files they import, by path, under their own module names"""
    for pkg in ("lib", "lib.train", "lib.utils", "lib.utils.optimizer"):
        m = types.ModuleType(pkg)
        m.__path__ = []
        sys.modules[pkg] = m

    def load(name, rel):
        spec = importlib.util.spec_from_file_location(name, os.path.join(reference, rel))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod

    load("lib.utils.optimizer.radam", "lib/utils/optimizer/radam.py")
    load("lib.utils.optimizer.lr_scheduler", "lib/utils/optimizer/lr_scheduler.py")
    return load("lib.train.optimizer", "lib/train/optimizer.py"), load("lib.train.scheduler", "lib/train/scheduler.py")


def make_inputs(seed):
    rs = np.random.RandomState(seed)
    init = {n: (rs.standard_normal(s) * 0.1).astype(np.float32) for n, s in SHAPES}
    grads = {}
    for n, s in SHAPES:
        g = (rs.standard_normal((N_GRADS,) + s) * np.exp(rs.uniform(-6, 2, (N_GRADS,) + s))).astype(np.float32)
        f = g.reshape(N_GRADS, -1)
        for k in range(N_GRADS):
            sign = np.float32(1 if k % 2 == 0 else -1)
            special = [55.5, -1000.0, 40.0, -40.0, 0.0, 1e-20, -3e-21, 40.000004, 3.4e38]
            if f.shape[1] >= 8 * len(special):
                for j, val in enumerate(special):
                    f[k, 8 * j] = sign * np.float32(val)
                f[k, -1] = sign * np.float32(77.0)                          # the 4097th element: past the last float4
                f[k, 1:8] = [41.0, -40.0, 40.0, 0.0, -0.0, 2e-20, -1e3]     # ... and some off the stride
            else:
                for j, val in enumerate(special[:f.shape[1]]):
                    f[k, j] = sign * np.float32(val) if (j + k) % 3 == 0 else f[k, j]
        if f.shape[1] > 64:
            f[3] = 0.0                                                       # one all-zero gradient for the large tensor
        grads[n] = f.reshape((N_GRADS,) + s)
    return init, grads


class MLP(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.l0 = torch.nn.Linear(241, 17)
        self.l1 = torch.nn.Linear(17, 3)


def run(ref_opt, ref_sch, init, grads, dtype):
    net = MLP().to(dtype)
    params = [net.l0.weight, net.l0.bias, net.l1.weight, net.l1.bias]
    with torch.no_grad():
        for p, (n, _) in zip(params, SHAPES):
            p.copy_(torch.from_numpy(init[n]).to(dtype))
    cfg = SimpleNamespace(train=SimpleNamespace(optim="adam", lr=LR, weight_decay=0, scheduler=SimpleNamespace(
        type="cosine", warmup_epochs=WARMUP, decay_epochs=DECAY, end_lr=END_LR)))
    opt = ref_opt.make_optimizer(cfg, net)
    sch = ref_sch.make_lr_scheduler(cfg, opt)
    assert len(opt.param_groups) == len(params)
    lrs, rec = [], {f"{n}_{k}": [] for n, _ in SHAPES for k in ("p", "exp_avg", "exp_avg_sq")}
    step = 0
    for epoch in range(EPOCHS):
        assert len({g["lr"] for g in opt.param_groups}) == 1
        lrs.append(opt.param_groups[0]["lr"])
        for _ in range(STEPS_PER_EPOCH):
            opt.zero_grad()
            for p, (n, _) in zip(params, SHAPES):
                p.grad = torch.from_numpy(grads[n][step % N_GRADS]).to(dtype).clone()
            torch.nn.utils.clip_grad_value_(net.parameters(), CLIP)
            opt.step()
            step += 1
        sch.step()
        for p, (n, _) in zip(params, SHAPES):
            st = opt.state[p]
            assert int(st["step"]) == step
            rec[f"{n}_p"].append(p.detach().numpy().copy())
            rec[f"{n}_exp_avg"].append(st["exp_avg"].numpy().copy())
            rec[f"{n}_exp_avg_sq"].append(st["exp_avg_sq"].numpy().copy())
    return np.array(lrs, dtype=np.float64), {k: np.stack(v) for k, v in rec.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference checkout (holds lib/train and lib/utils/optimizer)")
    ap.add_argument("--seed", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "g24_optim.npz"))
    args = ap.parse_args()
    ref_opt, ref_sch = _load_reference(args.reference)
    init, grads = make_inputs(args.seed)
    lr32, rec32 = run(ref_opt, ref_sch, init, grads, torch.float32)
    lr64, rec64 = run(ref_opt, ref_sch, init, grads, torch.float64)
    assert np.array_equal(lr32, lr64)
    out = {"seed": np.int64(args.seed), "epochs": np.int64(EPOCHS), "steps_per_epoch": np.int64(STEPS_PER_EPOCH),
           "stride": np.int64(STRIDE), "clip": np.float64(CLIP), "base_lr": np.float64(LR), "warmup_epochs": np.int64(WARMUP),
           "decay_epochs": np.int64(DECAY), "end_lr": np.float64(END_LR), "betas": np.array([0.9, 0.999]),
           "eps": np.float64(1e-8), "lr": lr32}
    for n, s in SHAPES:
        out[f"init_{n}"] = init[n]
        out[f"grad_{n}"] = grads[n]
        big = int(np.prod(s)) > 1024
        for k in ("p", "exp_avg", "exp_avg_sq"):
            for tag, rec in (("f32", rec32), ("f64", rec64)):
                a = rec[f"{n}_{k}"].reshape(EPOCHS, -1)
                if big:
                    out[f"{tag}_{n}_{k}"] = a[:, ::STRIDE].copy()
                    out[f"{tag}_{n}_{k}_last"] = a[-1].copy()
                else:
                    out[f"{tag}_{n}_{k}"] = a
    np.savez_compressed(args.out, **out)
    print(f"wrote {args.out}: {os.path.getsize(args.out) / 1024:.0f} KiB; lr per epoch: {lr32}")


if __name__ == "__main__":
    main()
