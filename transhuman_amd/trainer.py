"""The training loop around NetworkWrapper (train_loss.py): the reference's Trainer (lib/train/trainers/trainer.py:19-150),
its checkpoint functions (lib/utils/net_utils.py:288-348), a small Recorder (lib/train/recorder.py without tensorboard) and
the epoch loop of train_net.py:31-87, restated for this project.

One process per GPU: with a process group (``Trainer(..., group=)``, ``fit(..., group=)``; ``python -m torch.distributed.run -m
transhuman_amd.trainer`` sets one up from RANK / WORLD_SIZE / LOCAL_RANK) every rank starts from rank 0's parameters and
buffers, trains on its own batches, and the gradients are averaged between ``loss.backward()`` and the step by
train_dist.GradExchange -- one pack launch, one all-reduce, DeviceAdam stepping out of the flat buffer -- in the place of the
reference's DistributedDataParallel(find_unused_parameters=True) (lib/train/trainers/trainer.py:23-33).  The reference also
converts every BatchNorm to SyncBatchNorm; ``sync_bn`` does the same (default: when distributed on a device).  With
cfg.train_encoder = "device" the converted encoder trunk runs under torch autograd unless cfg.train_sync_bn = "device", which
keeps it on the HIP backward of the trunk (K23) with the ranks' statistics combined in rank order (train_ops.SyncBnActFn,
DESIGN.md section 4).  ``reduce`` is GradExchange's: "rank_ordered" makes an N-rank step the rank-ordered oracle bit for bit.
Without a group nothing differs from a single process.  The data loaders
are out of scope; a ``data_loader`` is any sized iterable of batches (train_dist.DistributedSampler deals a data set to the
ranks as the reference's sampler does).

Checkpoints keep the reference's layout ``{net, optim, scheduler, recorder, epoch}`` and names (``latest.pth``,
``{epoch + 1}.pth``).  Ours hold tensors and plain numbers only and load with ``weights_only=True``.  The ``net`` and ``optim``
entries of a checkpoint written by the reference load the same way; its ``scheduler`` entry pickles a bound method of the
reference's own class, which is neither loadable without that class nor needed: the schedule is a function of the epoch
(train_optim.warmup_cosine_lr), so it is rebuilt from ``epoch``.
"""
import os
import pickle
import time
from collections import defaultdict, deque

import torch

from .config import get_cfg, _STANDALONE
from .train_optim import DeviceAdam, make_lr_scheduler, make_optimizer


def _cfg_get(cfg, name):
    return getattr(cfg, name) if hasattr(cfg, name) else getattr(_STANDALONE, name)


# ---------------------------------------------------------------------------
# recorder
# ---------------------------------------------------------------------------
class SmoothedValue:
    """the last ``window_size`` values and the running total (recorder.py:10-37)"""

    def __init__(self, window_size=20):
        self.deque = deque(maxlen=window_size)
        self.total = 0.0
        self.count = 0

    def update(self, value):
        value = float(value)
        self.deque.append(value)
        self.count += 1
        self.total += value

    @property
    def median(self):
        d = sorted(self.deque)
        return d[(len(d) - 1) // 2] if d else 0.0            # (torch.median's choice: the lower of two middle values)

    @property
    def avg(self):
        return sum(self.deque) / len(self.deque) if self.deque else 0.0

    @property
    def global_avg(self):
        return self.total / max(self.count, 1)


class Recorder:
    """Smoothed loss statistics and the global step; ``state_dict()`` is ``{'step': n}`` as the reference's."""

    def __init__(self):
        self.epoch = 0
        self.step = 0
        self.loss_stats = defaultdict(SmoothedValue)
        self.batch_time = SmoothedValue()
        self.data_time = SmoothedValue()

    def update_loss_stats(self, loss_dict):
        # ONE transfer for all the statistics of a step (a .item() per entry is a device round trip each)
        keys = list(loss_dict)
        if not keys:
            return
        vals = torch.stack([loss_dict[k].detach().to(torch.float64).reshape(()) for k in keys]).cpu().tolist()
        for k, v in zip(keys, vals):
            self.loss_stats[k].update(v)

    def state_dict(self):
        return {"step": self.step}

    def load_state_dict(self, sd):
        self.step = int(sd["step"])

    def __str__(self):
        stats = "  ".join(f"{k}: {v.avg:.4f}" for k, v in self.loss_stats.items())
        return "  ".join([f"epoch: {self.epoch}", f"step: {self.step}", stats, f"data: {self.data_time.avg:.4f}",
                          f"batch: {self.batch_time.avg:.4f}"])


# ---------------------------------------------------------------------------
# trainer
# ---------------------------------------------------------------------------
class Trainer:
    """Trainer(network_wrapper): ``network_wrapper(batch) -> (output, loss, loss_stats, image_stats)``.

    group: a torch.distributed process group (``dist.group.WORLD`` for the default one) makes the trainer one rank of a
    data-parallel job (:23-33): construction -- a collective, every rank builds its trainer at the same point -- copies rank
    0's parameters and buffers to every rank, and ``train`` averages the gradients over the ranks before the clip and the
    step, so DeviceAdam's in-kernel clip clips the averaged gradient as :84-86 does.  Only rank 0 records and logs (:88-89).
    With DeviceAdam(zero_grad=True) a tensor that once had a gradient keeps its slot (train_dist.GradExchange, "Liveness").
    sync_bn: convert BatchNorm to SyncBatchNorm (:24-26); None: when distributed and on a device, as the reference.  A
    converted encoder trunk under cfg.train_encoder = "device" follows cfg.train_sync_bn (autograd_path.trunk_device).
    reduce: passed to GradExchange (None: its default, one all_reduce)."""

    clip_value = 40.0                                          # trainer.py:85

    def __init__(self, network, device=None, group=None, sync_bn=None, reduce=None):
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        self.device = torch.device(device)
        self.network = network.to(self.device)
        self.group, self.exchange, self.rank = group, None, 0
        if sync_bn is None:
            sync_bn = group is not None and self.device.type == "cuda"
        if group is None:
            if sync_bn:
                raise ValueError("Trainer: sync_bn needs a process group")
            return
        import torch.distributed as dist
        from .train_dist import GradExchange
        self.rank = dist.get_rank(group)
        if sync_bn:
            self.network = torch.nn.SyncBatchNorm.convert_sync_batchnorm(self.network, process_group=group)
        self.exchange = GradExchange([p for p in self.network.parameters() if p.requires_grad], group=group, reduce=reduce)
        self.exchange.broadcast_parameters(self.network, src=dist.get_global_rank(group, 0))

    @staticmethod
    def reduce_loss_stats(loss_stats):
        return {k: torch.mean(v) for k, v in loss_stats.items()}

    def to_device(self, batch):
        """to_cuda (:43-59): tensors and lists of tensors move, everything else (meta data, paths, names) stays"""
        out = {}
        for k, v in batch.items():
            if isinstance(v, torch.Tensor):
                out[k] = v.to(self.device)
            elif isinstance(v, (tuple, list)) and v and all(isinstance(b, torch.Tensor) for b in v):
                out[k] = [b.to(self.device) for b in v]
            else:
                out[k] = v
        return out

    def _parameters(self):
        return self.network.parameters()

    def train(self, epoch, data_loader, optimizer, recorder, log=None):
        """One epoch (:61-125): forward, zero_grad, loss.mean().backward(), [the gradient exchange,] clip at 40, step.  A
        DeviceAdam clips inside its kernel (its clip_value is set to the trainer's when it has none); any other optimiser gets
        clip_grad_value_."""
        cfg = get_cfg()
        max_iter = len(data_loader)
        log_interval = int(_cfg_get(cfg, "log_interval"))
        self.network.train()
        in_kernel = isinstance(optimizer, DeviceAdam)
        if in_kernel and optimizer.clip_value is None:
            optimizer.clip_value = self.clip_value
        end = time.time()
        for iteration, batch in enumerate(data_loader):
            data_time = time.time() - end
            iteration = iteration + 1
            batch = self.to_device(batch)
            output, loss, loss_stats, image_stats = self.network(batch)
            optimizer.zero_grad()
            loss = loss.mean()
            loss.backward()
            if self.exchange is not None:
                self.exchange.exchange()
            if not in_kernel:
                torch.nn.utils.clip_grad_value_(self._parameters(), self.clip_value)
            optimizer.step()
            if self.rank > 0:
                continue

            recorder.step += 1
            recorder.update_loss_stats(self.reduce_loss_stats(loss_stats))
            batch_time = time.time() - end
            end = time.time()
            recorder.batch_time.update(batch_time)
            recorder.data_time.update(data_time)
            if log is not None and (iteration % log_interval == 0 or iteration == max_iter - 1):
                lr = optimizer.param_groups[0]["lr"]
                log(f"{recorder}  lr: {lr:.6f}")

    def val(self, epoch, data_loader, evaluator=None, recorder=None, log=None):
        """:127-150: eval mode, no gradients, the mean of every loss statistic over the loader"""
        self.network.eval()
        sums = {}
        n = 0
        for batch in data_loader:
            batch = self.to_device(batch)
            with torch.no_grad():
                output, loss, loss_stats, image_stats = self.network(batch)
                if evaluator is not None:
                    evaluator.evaluate(output, batch)
            for k, v in self.reduce_loss_stats(loss_stats).items():
                sums[k] = sums.get(k, 0) + v.detach().to(torch.float64)
            n += 1
        stats = {k: float(v) / max(n, 1) for k, v in sums.items()}
        if log is not None:
            log("  ".join(f"{k}: {v:.4f}" for k, v in stats.items()))
        if evaluator is not None and hasattr(evaluator, "summarize"):
            evaluator.summarize()
        return stats


# ---------------------------------------------------------------------------
# checkpoints
# ---------------------------------------------------------------------------
def save_model(net, optim, scheduler, recorder, model_dir, epoch, last=False):
    """net_utils.py:335-348 -> the path written"""
    os.makedirs(model_dir, exist_ok=True)
    model = {"net": net.state_dict(), "optim": optim.state_dict(), "scheduler": scheduler.state_dict(),
             "recorder": recorder.state_dict(), "epoch": int(epoch)}
    path = os.path.join(model_dir, "latest.pth" if last else f"{epoch + 1}.pth")
    tmp = path + ".tmp"
    torch.save(model, tmp)
    os.replace(tmp, path)                                      # (a run killed while writing leaves the old file whole)
    return path


def find_checkpoint(model_dir, epoch=-1):
    """net_utils.py:303-318: latest.pth, else the highest numbered file; ``epoch`` picks one.  None when there is none."""
    if not os.path.isdir(model_dir):
        return None
    names = os.listdir(model_dir)
    pths = [int(n.split(".")[0]) for n in names if n.endswith(".pth") and n != "latest.pth" and n.split(".")[0].isdigit()]
    if not pths and "latest.pth" not in names:
        return None
    if epoch == -1:
        name = "latest" if "latest.pth" in names else str(max(pths))
    else:
        name = str(epoch)
    return os.path.join(model_dir, f"{name}.pth")


class _Opaque:
    """stands in for any class a foreign checkpoint pickled (never called, never inspected)"""

    def __init__(self, *a, **k):
        pass

    def __setstate__(self, state):
        pass


def _read_checkpoint(path):
    """The entries of a checkpoint file.  Ours -- and a reference checkpoint's tensors and numbers -- load with
    weights_only=True.  A file that does not (the reference's scheduler entry holds a bound method of lib.utils.optimizer.
    lr_scheduler.WarmupLR) is read with a restricted unpickler: torch's tensor rebuild
    functions and the standard containers are real, every other global becomes an inert placeholder, and the scheduler entry is
    dropped.  No code from the file runs."""
    try:
        return torch.load(path, map_location="cpu", weights_only=True)
    except pickle.UnpicklingError:
        pass
    import collections
    from torch import _utils as tu

    allowed = {("collections", "OrderedDict"): collections.OrderedDict, ("collections", "Counter"): collections.Counter,
               ("collections", "defaultdict"): collections.defaultdict,
               ("torch._utils", "_rebuild_tensor_v2"): tu._rebuild_tensor_v2,
               ("torch._utils", "_rebuild_parameter"): tu._rebuild_parameter,
               ("torch", "Size"): torch.Size, ("torch", "device"): torch.device}
    for name in ("FloatStorage", "DoubleStorage", "HalfStorage", "BFloat16Storage", "LongStorage", "IntStorage",
                 "ShortStorage", "CharStorage", "ByteStorage", "BoolStorage"):
        allowed[("torch", name)] = getattr(torch, name)

    class Unpickler(pickle.Unpickler):
        def find_class(self, module, name):
            return allowed.get((module, name), _Opaque)

    model = torch.load(path, map_location="cpu", weights_only=False, pickle_module=_PickleShim(Unpickler))
    if isinstance(model, dict):
        model = dict(model)
        model["scheduler"] = None
    return model


class _PickleShim:
    """the two names torch.load takes from ``pickle_module``"""

    def __init__(self, unpickler):
        self.Unpickler = unpickler
        self.__name__ = "pickle"

    def load(self, f, **kw):
        return self.Unpickler(f, **kw).load()


def load_model(net, optim, scheduler, recorder, model_dir, resume=True, epoch=-1, specified_resume=""):
    """net_utils.py:288-332 -> the epoch to begin with.  resume=False starts from scratch WITHOUT touching model_dir (the
    reference removes the directory; this never deletes anything).  A checkpoint whose scheduler entry is missing or not plain
    numbers resumes the schedule from ``epoch`` -- the schedule is a function of the epoch."""
    if not resume:
        return 0
    path = specified_resume if specified_resume else find_checkpoint(model_dir, epoch)
    if path is None:
        return 0
    model = _read_checkpoint(path)
    net.load_state_dict(model["net"])
    optim.load_state_dict(model["optim"])
    begin = int(model["epoch"]) + 1
    sd = model.get("scheduler")
    try:
        if not isinstance(sd, dict) or "last_epoch" not in sd:
            raise KeyError("scheduler")
        scheduler.load_state_dict(sd)
    except (KeyError, TypeError, ValueError):
        scheduler.set_epoch(begin)
    rec = model.get("recorder")
    if isinstance(rec, dict) and "step" in rec:
        recorder.load_state_dict(rec)
    return begin


# ---------------------------------------------------------------------------
# the epoch loop
# ---------------------------------------------------------------------------
def fit(cfg, network, data_loader, log=print, group=None, reduce=None):
    """train_net.py:31-87: ``network`` is a NetworkWrapper (its ``net`` holds the trained parameters, as in the reference,
    where the optimiser and the checkpoints are built on network.net), ``data_loader`` a sized iterable that yields at most
    cfg.ep_iter batches per pass (train_dist.iterations_per_rank of them on each rank of a job).  With a process group every
    rank loads the checkpoint, only rank 0 writes one (:76-82) and logs, and the loader's sampler is told the epoch (:68-69).
    ``reduce`` is the Trainer's."""
    net = network.net if hasattr(network, "net") else network
    trainer = Trainer(network, group=group, reduce=reduce)
    optimizer = make_optimizer(cfg, net)
    scheduler = make_lr_scheduler(cfg, optimizer)
    recorder = Recorder()
    model_dir = _cfg_get(cfg, "trained_model_dir")
    begin_epoch = load_model(net, optimizer, scheduler, recorder, model_dir, resume=bool(_cfg_get(cfg, "resume")))
    tr = getattr(cfg, "train", None) or _STANDALONE.train
    save_freq, save_latest = int(_cfg_get(cfg, "save_freq")), int(_cfg_get(cfg, "save_latest_ep"))
    writes = trainer.rank == 0
    for epoch in range(begin_epoch, int(tr.epoch)):
        recorder.epoch = epoch
        if hasattr(getattr(data_loader, "dataset", None), "set_epoch"):
            data_loader.dataset.set_epoch(epoch)
        if group is not None:
            for sampler in (getattr(data_loader, "sampler", None),
                            getattr(getattr(data_loader, "batch_sampler", None), "sampler", None)):
                if hasattr(sampler, "set_epoch"):
                    sampler.set_epoch(epoch)
                    break
        trainer.train(epoch, data_loader, optimizer, recorder, log=log if writes else None)
        scheduler.step()
        if writes and (epoch + 1) % save_freq == 0:
            save_model(net, optimizer, scheduler, recorder, model_dir, epoch)
        if writes and (epoch + 1) % save_latest == 0:
            save_model(net, optimizer, scheduler, recorder, model_dir, epoch, last=True)
    if group is not None:
        import torch.distributed as dist
        dist.barrier(group=group)                             # (a rank that returns finds rank 0's last checkpoint written)
    return network


# ---------------------------------------------------------------------------
# one process per GPU
# ---------------------------------------------------------------------------
def init_distributed(backend=None, timeout_s=1800):
    """The process group of a ``torch.distributed.run`` launch (train_net.py:116-123): RANK, WORLD_SIZE and LOCAL_RANK select
    it, LOCAL_RANK the device.  -> (group, device), or (None, None) when the variables are absent: a single process.
    backend: "nccl" (RCCL) on a device, "gloo" without one, unless given."""
    if not all(k in os.environ for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK")):
        return None, None
    import datetime
    import torch.distributed as dist
    on_device = torch.cuda.is_available()
    device = torch.device("cuda", int(os.environ["LOCAL_RANK"])) if on_device else torch.device("cpu")
    if on_device:
        torch.cuda.set_device(device)
    if not dist.is_initialized():
        dist.init_process_group(backend or ("nccl" if on_device else "gloo"), rank=int(os.environ["RANK"]),
                                world_size=int(os.environ["WORLD_SIZE"]), timeout=datetime.timedelta(seconds=timeout_s))
    return dist.group.WORLD, device


def main(argv=None):
    """``python -m transhuman_amd.trainer --steps N``: N steps per epoch on a seeded synthetic subject (synth.make_batch) with
    target patches seeded per rank and step (the data loaders are out of scope) through ``fit`` -- under ``torch.distributed.run`` as one rank of
    a data-parallel job, otherwise as a single process.  The MSE term alone unless cfg names the LPIPS weights."""
    import argparse
    from . import synth
    from .networks.cross_transformer import Network
    from .networks.renderer.if_clight_renderer import Renderer
    from .train_loss import NetworkWrapper
    ap = argparse.ArgumentParser(description=main.__doc__)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--epochs", type=int, default=1)
    ap.add_argument("--patch", type=int, default=20)
    ap.add_argument("--backend", default=None)
    ap.add_argument("--model-dir", default=None, help="where checkpoints go (default: cfg.trained_model_dir)")
    args = ap.parse_args(argv)
    group, device = init_distributed(args.backend)
    rank, world = 0, 1
    if group is not None:
        import torch.distributed as dist
        rank, world = dist.get_rank(), dist.get_world_size()
    if device is None:
        device = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
    cfg = get_cfg()
    P = args.patch
    masks = torch.ones((1, 1, P, P), dtype=torch.bool)
    div = torch.tensor([[0, P * P]], dtype=torch.int64)

    base = synth.make_batch(P, P, 3, seed=0)                    # one subject and pose; the targets differ per rank and step

    def batch(k):
        gen = torch.Generator().manual_seed(k)
        return dict(base, patch_masks=masks, patch_div_indices=div, target_patches=torch.rand((1, 1, P, P, 3), generator=gen))

    loader = [batch(1 + e * world + rank) for e in range(args.steps)]
    from .config import override
    keep = dict(lpips_weight=float(_cfg_get(cfg, "lpips_weight")) if getattr(cfg, "lpips_vgg16_path", None) else 0.0,
                trained_model_dir=args.model_dir or _cfg_get(cfg, "trained_model_dir"))
    with override(**keep):
        torch.manual_seed(0)
        net = Network().train().to(device)
        body = loader[0]["tar_smpl_vertice_smplcoord"][0].numpy()
        n_class = int(_cfg_get(cfg, "num_class"))
        renderer = Renderer(net, vertex_can=body.astype("float64") * 1.02 + 0.001, pc2voxel_ind=synth.kmeans_assign(body, n_class))
        tr = getattr(cfg, "train", None) or _STANDALONE.train
        epochs, tr.epoch = tr.epoch, args.epochs
        try:
            fit(cfg, NetworkWrapper(net, renderer=renderer), loader, group=group)
        finally:
            tr.epoch = epochs
    if group is not None:
        import torch.distributed as dist
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
