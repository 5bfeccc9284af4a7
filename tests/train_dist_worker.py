"""One rank of the jobs tests/test_gpu_train_dist.py starts (not a test file).

    python -m torch.distributed.run --nproc-per-node N tests/train_dist_worker.py --out DIR [--sync-bn] [--reduce ordered]     (gloo, every rank on cuda:0)
    RANK=0 WORLD_SIZE=1 LOCAL_RANK=0 python tests/train_dist_worker.py --out DIR --rccl                      (one rank over "nccl")

Default mode: the golden training step's small case (train_step_case.setup) under every training switch's device value.  Rank r
perturbs its parameters and buffers with seed r, builds the distributed trainer.Trainer (which makes them rank 0's again) and runs
STEPS iterations on batches whose target patches are seeded by (rank, step), with a DeviceAdam that zeroes the gradients in its
kernel -- so the first exchange packs out of autograd's own tensors and the later ones in place.  Written to DIR/rank<r>.npz:
the parameters as perturbed ("own") and as started ("start") and after every step as SHA-256 digests of their bytes, the local
gradients of every step in full, the exchanged ones as digests (rank 0: in full as well), which tensors have optimiser state,
and the losses.  Rank 0 of a run without --sync-bn also trains a copy of the started network alone on its own batches
("solo" digests).

--rccl: a GradExchange over the real transport with one rank: the flat device buffer goes through all_reduce on "nccl" and the
exchanged gradients must be the local ones, bit for bit; broadcast_parameters must leave the tensors as they are."""
import argparse
import copy
import datetime
import hashlib
import json
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

STEPS = 3
LR = 7e-4


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def rccl(args):
    from transhuman_amd import train_dist as TD
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, timeout=datetime.timedelta(seconds=120))
    try:
        gen = torch.Generator().manual_seed(3)
        sizes = [1, 3, 4096, 5, 4097, 300]
        m = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(n, generator=gen).to(dev)) for n in sizes])
        params = list(m)
        local = [torch.randn(n, generator=gen).to(dev) for n in sizes]
        local[2][:4] = torch.tensor([float("inf"), -0.0, 1e-42, -float("inf")])
        for i, (p, g) in enumerate(zip(params, local)):
            p.grad = None if i == 3 else g.clone()
        ex = TD.GradExchange(params)
        assert ex.backend == "device" and ex.world == 1 and dist.get_backend() == "nccl"
        before = [p.detach().clone() for p in params]
        ex.broadcast_parameters(m)
        flat = ex.exchange()
        torch.cuda.synchronize()
        ok = all(torch.equal(a, b) for a, b in zip(before, params)) and params[3].grad is None
        for i, (p, g) in enumerate(zip(params, local)):
            if i != 3:
                ok = ok and p.grad.data_ptr() == flat.data_ptr() + 4 * int(ex.layout.offsets[i])
                ok = ok and bool((p.grad.view(torch.int32) == g.view(torch.int32)).all())
        with open(os.path.join(args.out, "rccl.json"), "w") as f:
            json.dump({"ok": bool(ok), "flat_elems": int(flat.numel())}, f)
    finally:
        dist.destroy_process_group()


def train(args):
    from train_step_case import STEP_CFG, setup
    from transhuman_amd import config, train_optim as TO
    from transhuman_amd.networks.renderer.if_clight_renderer import Renderer
    from transhuman_amd.train_loss import NetworkWrapper
    from transhuman_amd.trainer import Recorder, Trainer
    from util import can64, synth_assign
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    switches = {k: v[1] for k, v in config.TRAIN_SWITCHES.items()}
    out = {}
    try:
        with config.override(**STEP_CFG, **switches, l2rec_weight=1.0, lpips_weight=0.0):
            net, r, b = setup(dev)
            names = [k for k, _ in net.named_parameters()]
            gen = torch.Generator().manual_seed(1000 + rank)
            with torch.no_grad():
                for t in list(net.parameters()) + [x for x in net.buffers() if x.dtype is torch.float32]:
                    t.add_((torch.randn(t.shape, generator=gen) * 1e-3 * (rank + 1)).to(dev))
            for k, p in net.named_parameters():
                out[f"own:{k}"] = digest(p)
            n, P = int(b["ray_o"].shape[1]), 20
            n_patch = -(-n // (P * P))
            masks = torch.zeros(n_patch * P * P, dtype=torch.bool)
            masks[:n] = True
            masks = masks.reshape(n_patch, P, P)
            div = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(masks.reshape(n_patch, -1).sum(1), 0)])

            def batch(rk, step):
                g = torch.Generator().manual_seed(7 + 10 * step + rk)
                return dict(b, patch_masks=masks[None].to(dev), patch_div_indices=div[None],
                            target_patches=torch.rand((1, n_patch, P, P, 3), generator=g).to(dev))

            wrapper = NetworkWrapper(net, renderer=r)
            losses = []
            wrapper.register_forward_hook(lambda m, i, o: losses.append(o[1].detach().reshape(())))
            trainer = Trainer(wrapper, device=dev, group=dist.group.WORLD, sync_bn=args.sync_bn)
            assert trainer.exchange.reduce == "collective"                 # one all_reduce, whatever the transport
            if args.reduce:
                from transhuman_amd.train_dist import GradExchange
                trainer.exchange = GradExchange(trainer.exchange.params, group=dist.group.WORLD, reduce=args.reduce)
            out["reduce"] = np.array(trainer.exchange.reduce)
            assert trainer.exchange.backend == "device" and trainer.exchange.world == world
            for k, p in net.named_parameters():
                out[f"start:{k}"] = digest(p)
            for k, t in net.named_buffers():
                out[f"startbuf:{k}"] = digest(t)
            solo = None
            if rank == 0 and not args.sync_bn:
                solo = copy.deepcopy(net)
            params = list(net.parameters())
            assert [id(p) for p in trainer.exchange.params] == [id(p) for p in params]
            opt = TO.DeviceAdam([{"params": [p], "lr": LR, "weight_decay": 0} for p in params], LR, zero_grad=True)
            inner = trainer.exchange.exchange
            step_no = [0]

            def recording_exchange():
                s = step_no[0]
                for k, p in zip(names, params):
                    if p.grad is not None:
                        out[f"local{s}:{k}"] = p.grad.detach().cpu().numpy().copy()
                flat = inner()
                for k, p in zip(names, params):
                    if p.grad is not None:
                        out[f"exdig{s}:{k}"] = digest(p.grad)
                        if rank == 0:
                            out[f"ex{s}:{k}"] = p.grad.detach().cpu().numpy().copy()
                return flat

            trainer.exchange.exchange = recording_exchange
            rec = Recorder()
            for step in range(STEPS):
                step_no[0] = step
                trainer.train(0, [batch(rank, step)], opt, rec)
                for k, p in zip(names, params):
                    out[f"param{step}:{k}"] = digest(p)
            out["recorder_step"] = np.int64(rec.step)
            out["inplace"] = np.int64(trainer.exchange.layout.view_ptrs is not None)
            out["state"] = np.array([k for k, p in zip(names, params) if len(opt.state.get(p, {}))])
            out["no_grad"] = np.array([k for k, p in zip(names, params) if p.grad is None])
            out["losses"] = torch.stack(losses).double().cpu().numpy()
            if solo is not None:
                r2 = Renderer(solo, vertex_can=can64().numpy(), pc2voxel_ind=synth_assign(300))
                sp = list(solo.parameters())
                opt2 = TO.DeviceAdam([{"params": [p], "lr": LR, "weight_decay": 0} for p in sp], LR, zero_grad=True)
                alone = Trainer(NetworkWrapper(solo, renderer=r2), device=dev)
                for step in range(STEPS):
                    alone.train(0, [batch(0, step)], opt2, Recorder())
                for k, p in zip(names, sp):
                    out[f"solo:{k}"] = digest(p)
            torch.cuda.synchronize()
        np.savez(os.path.join(args.out, f"rank{rank}.npz"), **out)
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--sync-bn", action="store_true")
    ap.add_argument("--reduce", default=None, help="'ordered': the trainer's exchange is replaced by GradExchange(reduce='ordered')")
    ap.add_argument("--rccl", action="store_true")
    a = ap.parse_args()
    (rccl if a.rccl else train)(a)
