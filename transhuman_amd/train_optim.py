"""The optimiser of the training loop: value clipping and the Adam / AdamW update of every parameter in ONE kernel launch
(csrc/k_optim.hip, K22), the reference's schedule in closed form, and its two factories.

The reference (lib/train/optimizer.py:11-28, lib/train/scheduler.py:5-46, lib/train/trainers/trainer.py:82-86) builds
torch.optim.Adam over one parameter group PER TENSOR (293 groups), clips every gradient to [-40, 40] in a pass of its own and
wraps CosineAnnealingLR in a linear warm-up.  ``DeviceAdam`` keeps that interface -- the group list, ``group['lr']`` read at
every step, torch's ``state_dict`` layout -- and replaces the per-tensor launches with one table copy and one launch.

The arithmetic is this project's definition (fp32, every operation rounded once, in this order; it is torch's
``_single_tensor_adam`` order without FMA contraction):

    g  = clamp(g, -c, c)                                  when a clip value is given; NaN stays NaN
    p  = p * (1 - lr wd)                                  decoupled weight decay (AdamW), else
    g  = g + wd * p                                       when wd != 0
    m' = m + (1 - b1) * (g - m)
    v' = b2 * v + ((1 - b2) * g) * g
    p' = p - step_size * (m' / (sqrt(v') / bc2_sqrt + eps))

with step_size = lr / (1 - b1^t), bc2_sqrt = (1 - b2^t)^0.5, 1 - b1, 1 - b2 and 1 - lr wd computed in Python floats and
rounded to fp32 once.  ``adam_step_oracle`` restates it in numpy (float32: the kernel's bits; float64: the yardstick).
"""
import math

import numpy as np
import torch

from . import hip


# ---------------------------------------------------------------------------
# the definition
# ---------------------------------------------------------------------------
def adam_scalars(lr, beta1, beta2, eps, weight_decay, step):
    """The per-tensor scalars of one step as Python floats, in the order of the device table's columns:
    (lr, step_size, bc2_sqrt, 1 - beta1, beta2, 1 - beta2, eps, weight_decay, decay_mul)."""
    lr, beta1, beta2, eps, weight_decay = float(lr), float(beta1), float(beta2), float(eps), float(weight_decay)
    step = int(step)
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    return (lr, lr / bc1, bc2 ** 0.5, 1 - beta1, beta2, 1 - beta2, eps, weight_decay, 1 - lr * weight_decay)


def adam_step_oracle(p, g, m, v, *, lr, step, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled_weight_decay=False,
                     clip_value=None, dtype=np.float32):
    """One step of the definition above on numpy arrays -> (p', m', v'); ``step`` is the 1-based step count of this update.
    dtype=np.float32 is what adam_step_kernel computes, bit for bit (the scalars rounded to fp32 once, every operation
    rounded once); dtype=np.float64 is the same expression in double precision with unrounded scalars."""
    dt = np.dtype(dtype).type
    p, g, m, v = (np.asarray(a).astype(dt) for a in (p, g, m, v))
    _, step_size, bc2_sqrt, omb1, beta2, omb2, eps_, wd, decay_mul = (dt(x) for x in adam_scalars(
        lr, betas[0], betas[1], eps, weight_decay, step))
    with np.errstate(all="ignore"):
        if clip_value is not None:
            c = dt(clip_value)
            g = np.where(g < -c, -c, np.where(g > c, c, g))             # (comparisons are false on NaN: it stays)
        if decoupled_weight_decay:
            p = p * decay_mul
        elif wd != 0:
            g = g + wd * p
        m = m + omb1 * (g - m)
        v = beta2 * v + (omb2 * g) * g
        p = p - step_size * (m / (np.sqrt(v) / bc2_sqrt + eps_))
    assert p.dtype == dt and m.dtype == dt and v.dtype == dt
    return p, m, v


# ---------------------------------------------------------------------------
# the optimiser
# ---------------------------------------------------------------------------
class DeviceAdam(torch.optim.Optimizer):
    """Adam / AdamW whose step is one launch of adam_step_kernel over every parameter tensor.

    Accepts what torch.optim.Adam accepts for ``params`` (the reference's list of one group per parameter included), reads
    each group's ``lr`` / ``betas`` / ``eps`` / ``weight_decay`` at every step, and keeps ``state[p] = {step, exp_avg,
    exp_avg_sq}`` as torch.optim.Adam does (``step`` a float32 scalar on the host), so ``state_dict()`` /
    ``load_state_dict()`` are interchangeable with torch.optim.Adam / AdamW in both directions.

    clip_value: clamp every gradient element to [-clip_value, clip_value] inside the kernel (clip_grad_value_ without its pass).
    zero_grad:  the kernel writes 0 over each gradient after reading it; ``zero_grad()`` then keeps the gradients allocated
                and touches only those that were written since.
    count_nonfinite: the kernel counts NaN / +-inf gradient elements; ``nonfinite_count()`` reads the running total.

    Parameters must be contiguous fp32 device tensors (hip.HipError otherwise, raised by the first step: there is no CPU
    path); a parameter whose ``grad`` is None is skipped and gets no state; a non-contiguous gradient is replaced by a
    contiguous copy.  After the update the in-place version counter of every updated parameter is bumped
    (torch.autograd.graph.increment_version: host bookkeeping, no launch), which is what hip._sync_weights reads to
    re-pack the renderer's weight images.  Device work per step: the table copy and the kernel."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, decoupled_weight_decay=False,
                 clip_value=None, zero_grad=False, *, count_nonfinite=False, amsgrad=False, maximize=False, capturable=False,
                 differentiable=False, foreach=None, fused=None):
        for name, val in (("amsgrad", amsgrad), ("maximize", maximize), ("capturable", capturable),
                          ("differentiable", differentiable)):
            if val:
                raise ValueError(f"DeviceAdam: {name}=True is not implemented by adam_step_kernel")
        if isinstance(lr, torch.Tensor):
            raise ValueError("DeviceAdam: lr must be a Python number (the step's scalars are computed on the host)")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameters: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if clip_value is not None and not clip_value >= 0:
            raise ValueError(f"Invalid clip value: {clip_value}")
        # (the keys of torch.optim.Adam's groups, so that a state_dict moves either way without a missing key)
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None,
                        decoupled_weight_decay=bool(decoupled_weight_decay))
        super().__init__(params, defaults)
        self.clip_value = clip_value
        self.zero_grad_in_step = bool(zero_grad)
        self.count_nonfinite = bool(count_nonfinite)
        self._plan = None

    # -- bookkeeping -------------------------------------------------------------------------------------------------
    def _drop_plan(self):
        self._plan = None

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._plan = None

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._plan = None                                                  # (new moment tensors, new step counts)

    def _build(self):
        flat = [(p, gi) for gi, group in enumerate(self.param_groups) for p in group["params"]]
        if not flat:
            raise hip.HipError("DeviceAdam: no parameters")
        for i, (p, _) in enumerate(flat):
            hip.adam_check_tensor(p, f"parameter {i}")
        plan = hip.AdamPlan([p for p, _ in flat])
        n = len(flat)
        self._flat = flat
        self._params = [p for p, _ in flat]
        self._group_of = [gi for _, gi in flat]
        self._table = np.zeros(n, dtype=plan.dtype)
        self._steps = [0] * n                 # host mirror of state[p]['step']
        # every state[p]['step'] is a 0-dim view of this one host tensor: a step adds 1 to all of them in one operation
        # (torch._foreach_add_ over hundreds of host scalars costs more than the kernel)
        self._step_buf = torch.zeros(n, dtype=torch.float32)
        self._state_of = [None] * n           # state dicts (None until the parameter's first gradient)
        self._zeroed = {}                     # index -> (grad tensor, its version) as the kernel left it, all zeros
        self._scalar_cache = {}
        self._fresh = True
        self._plan = plan
        for i, p in enumerate(self._params):
            st = self.state.get(p)
            if st:
                self._adopt(i, p, st)

    def _adopt(self, i, p, st):
        m, v = st["exp_avg"], st["exp_avg_sq"]
        for t, what in ((m, "exp_avg"), (v, "exp_avg_sq")):
            hip.adam_check_tensor(t, f"{what} of parameter {i}")
            if t.shape != p.shape:
                raise hip.HipError(f"DeviceAdam: {what} of parameter {i} has shape {tuple(t.shape)}, not {tuple(p.shape)}")
        # (a number in checkpoints of old torch versions, a device tensor in a capturable / fused optimiser's)
        self._steps[i] = int(st["step"].item() if isinstance(st["step"], torch.Tensor) else st["step"])
        self._step_buf[i] = self._steps[i]
        st["step"] = self._step_buf[i]
        self._state_of[i] = st
        self._table["m"][i] = m.data_ptr()
        self._table["v"][i] = v.data_ptr()
        self._fresh = True

    # -- the step ----------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        groups = []
        for gi, group in enumerate(self.param_groups):
            for name in ("amsgrad", "maximize", "capturable", "differentiable"):
                if group.get(name):
                    raise ValueError(f"DeviceAdam: group {gi} asks for {name}, which adam_step_kernel does not implement")
            b1, b2 = group["betas"]
            groups.append((float(group["lr"]), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]),
                           bool(group.get("decoupled_weight_decay", False))))
        if self._plan is None:
            self._build()
        params, tab, steps, states = self._params, self._table, self._steps, self._state_of
        cache = self._scalar_cache
        if len(cache) > 4096:
            cache.clear()
        n = len(params)
        ptr_p, ptr_g, cols, updated, active = [0] * n, [0] * n, [None] * n, [], []
        fresh, group_of = self._fresh, self._group_of
        for i in range(n):
            p = params[i]
            g = p.grad
            if g is None:
                continue
            if not g.is_contiguous():
                g = p.grad = g.contiguous()
            if fresh or g.dtype is not torch.float32:
                if g.is_sparse:
                    raise RuntimeError("DeviceAdam does not support sparse gradients")
                hip.adam_check_tensor(p, f"parameter {i}")
                hip.adam_check_tensor(g, f"the gradient of parameter {i}")
            st = states[i]
            if st is None:
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = 0.0
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                self._adopt(i, p, st)
            t = steps[i] + 1
            key = (groups[group_of[i]], t)
            sc = cache.get(key)
            if sc is None:
                lr, b1, b2, eps, wd, dec = key[0]
                sc = cache[key] = adam_scalars(lr, b1, b2, eps, wd, t) + (hip.ADAM_T_DECOUPLED if dec else 0,)
            cols[i] = sc
            ptr_p[i] = p.data_ptr()
            ptr_g[i] = g.data_ptr()
            updated.append(p)
            active.append(i)
        if not updated:
            return loss
        tab["p"] = ptr_p
        tab["g"] = ptr_g
        names = ("lr", "step_size", "bc2_sqrt", "one_minus_beta1", "beta2", "one_minus_beta2", "eps", "weight_decay",
                 "decay_mul", "flags")
        distinct = {id(cols[i]): cols[i] for i in active}
        if len(distinct) == 1:                                             # the usual case: one setting, one step count
            sc = next(iter(distinct.values()))                             # (rows of skipped tensors are never read)
            for k, name in enumerate(names):
                tab[name] = sc[k]                                          # -> fp32 once, on assignment
        else:
            blank = (0.0,) * 9 + (0,)
            c = np.array([x if x is not None else blank for x in cols], dtype=np.float64)
            for k, name in enumerate(names):
                tab[name] = c[:, k]
        self._plan.step(tab, clip=self.clip_value, zero_grad=self.zero_grad_in_step, count_nonfinite=self.count_nonfinite,
                        check_pointers=self._fresh)
        self._fresh = False
        for i in active:
            steps[i] += 1
        if len(active) == n:
            self._step_buf += 1
        else:
            self._step_buf[active] += 1
        # the kernel wrote through raw pointers: tell autograd (and hip._sync_weights, which reads p._version)
        torch.autograd.graph.increment_version(updated)
        if self.zero_grad_in_step:
            grads = [p.grad for p in updated]
            torch.autograd.graph.increment_version(grads)
            self._zeroed = {id(p): (g, g._version) for p, g in zip(updated, grads)}
        return loss

    def zero_grad(self, set_to_none=None):
        """With zero_grad=True at construction the gradients stay allocated (set_to_none defaults to False) and one the
        kernel cleared, untouched since, is left alone; otherwise torch's zero_grad (set_to_none defaults to True)."""
        if not self.zero_grad_in_step:
            return super().zero_grad(True if set_to_none is None else set_to_none)
        if set_to_none:
            self._zeroed = {}
            return super().zero_grad(True)
        zeroed = getattr(self, "_zeroed", {})
        for group in self.param_groups:
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                z = zeroed.get(id(p))
                if z is not None and z[0] is g and z[1] == g._version:
                    continue
                if g.grad_fn is not None:
                    g.detach_()
                else:
                    g.requires_grad_(False)
                g.zero_()

    def nonfinite_count(self):
        """NaN / +-inf gradient elements seen by the steps so far (count_nonfinite=True); waits for the device."""
        if not self.count_nonfinite:
            raise ValueError("DeviceAdam: built without count_nonfinite=True")
        return 0 if self._plan is None else self._plan.nonfinite()


# ---------------------------------------------------------------------------
# the schedule
# ---------------------------------------------------------------------------
def warmup_cosine_lr(epoch, base_lr, warmup_epochs, decay_epochs, end_lr):
    """The learning rate the reference's schedule (CosineAnnealingLR(T_max = decay_epochs - warmup_epochs, eta_min = end_lr)
    inside WarmupLR(init_lr = 0, num_warmup = warmup_epochs, 'linear'); lib/train/scheduler.py:22-30) has set when epoch
    ``epoch`` trains, in closed form.  Its quirks are kept: the wrapper takes no step of its own at construction, so

        epoch 0                          base_lr              (the optimiser's own value: nothing has been scheduled yet)
        1 <= epoch <= warmup_epochs + 1  base_lr (epoch - 1) / warmup_epochs          (exactly 0 at epoch 1)
        epoch > warmup_epochs + 1        end_lr + (base_lr - end_lr) (1 + cos(pi t / T)) / 2,  t = epoch - warmup_epochs - 1,
                                                                                               T = decay_epochs - warmup_epochs

    The reference reaches the cosine part by torch's recursive update; the two agree to rounding for epoch < decay_epochs, the
    epochs the reference trains (cfg.train.epoch = decay_epochs).  Past that the closed form simply continues the cosine."""
    epoch = int(epoch)
    if warmup_epochs <= 0:                                                  # (no wrapper: plain cosine from epoch 0)
        t, T = epoch, decay_epochs
        return end_lr + (base_lr - end_lr) * (1 + math.cos(math.pi * t / T)) / 2
    if epoch == 0:
        return base_lr
    if epoch <= warmup_epochs + 1:
        return (base_lr - 0.0) * ((epoch - 1) / warmup_epochs) + 0.0
    t, T = epoch - warmup_epochs - 1, decay_epochs - warmup_epochs
    return end_lr + (base_lr - end_lr) * (1 + math.cos(math.pi * t / T)) / 2


class WarmupCosineLR:
    """``step()`` once per epoch, as the reference's loop does (train_net.py:73): writes warmup_cosine_lr(epoch) of each
    group's base lr into ``group['lr']``.  ``state_dict()`` holds plain numbers only (it loads with weights_only=True)."""

    def __init__(self, optimizer, warmup_epochs, decay_epochs, end_lr, last_epoch=0):
        self.optimizer = optimizer
        self.warmup_epochs = int(warmup_epochs)
        self.decay_epochs = int(decay_epochs)
        self.end_lr = float(end_lr)
        self.base_lrs = [float(g["lr"]) for g in optimizer.param_groups]
        self.last_epoch = 0
        if last_epoch:
            self.set_epoch(last_epoch)

    def lr_at(self, epoch):
        return [warmup_cosine_lr(epoch, b, self.warmup_epochs, self.decay_epochs, self.end_lr) for b in self.base_lrs]

    def set_epoch(self, epoch):
        """the state in front of training epoch ``epoch`` (what ``epoch`` calls of step() leave)"""
        self.last_epoch = int(epoch)
        for group, lr in zip(self.optimizer.param_groups, self.lr_at(self.last_epoch)):
            group["lr"] = lr

    def step(self):
        self.set_epoch(self.last_epoch + 1)

    def get_last_lr(self):
        return [g["lr"] for g in self.optimizer.param_groups]

    def state_dict(self):
        return {"last_epoch": self.last_epoch, "warmup_epochs": self.warmup_epochs, "decay_epochs": self.decay_epochs,
                "end_lr": self.end_lr, "base_lrs": list(self.base_lrs)}

    def load_state_dict(self, sd):
        if len(sd["base_lrs"]) != len(self.base_lrs):
            raise ValueError("WarmupCosineLR: the checkpoint's schedule has another number of parameter groups")
        self.warmup_epochs, self.decay_epochs = int(sd["warmup_epochs"]), int(sd["decay_epochs"])
        self.end_lr = float(sd["end_lr"])
        self.base_lrs = [float(x) for x in sd["base_lrs"]]
        self.set_epoch(int(sd["last_epoch"]))


# ---------------------------------------------------------------------------
# the reference's factories
# ---------------------------------------------------------------------------
def _train_cfg(cfg):
    from .config import _STANDALONE
    return getattr(cfg, "train", None) or _STANDALONE.train


def make_optimizer(cfg, net, lr=None, weight_decay=None, clip_value=40.0):
    """lib/train/optimizer.py:11-28 for cfg.train.optim in {'adam', 'adamw'}: one group per parameter that requires a
    gradient, in named_parameters() order.  clip_value is the trainer's clip_grad_value_(., 40), done inside the step."""
    tr = _train_cfg(cfg)
    lr = tr.lr if lr is None else lr
    weight_decay = tr.weight_decay if weight_decay is None else weight_decay
    params = [{"params": [value], "lr": lr, "weight_decay": weight_decay}
              for _, value in net.named_parameters() if value.requires_grad]
    if tr.optim not in ("adam", "adamw"):
        raise ValueError(f"make_optimizer: cfg.train.optim = {tr.optim!r}; DeviceAdam implements 'adam' and 'adamw'")
    return DeviceAdam(params, lr, weight_decay=weight_decay, decoupled_weight_decay=tr.optim == "adamw", clip_value=clip_value)


def make_lr_scheduler(cfg, optimizer):
    """lib/train/scheduler.py:5-30 for cfg.train.scheduler.type == 'cosine' (the only type the reference still builds)"""
    sch = _train_cfg(cfg).scheduler
    if sch.type != "cosine":
        raise ValueError(f"make_lr_scheduler: cfg.train.scheduler.type = {sch.type!r}; only 'cosine' is implemented")
    return WarmupCosineLR(optimizer, sch.warmup_epochs, sch.decay_epochs, sch.end_lr)
