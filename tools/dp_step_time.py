"""Time the gradient exchange of data-parallel training (transhuman_amd/train_dist.py) on one MI355X, in one process:

    timeout -k 10 900 python tools/dp_step_time.py [--rounds 5] [--reps 20] [--steps 5] [--warmup 2] [--only pack|rank_sum|sync_bn|step]

(a) "pack": adam_pack_kernel alone on the product Network's parameter list with a seeded gradient on every tensor, once for the
    live set (the tensors the reference trains: no layer3 / layer4, dead tokens or PE buffers) and once for all tensors, at
    world = 2 (a real division): out of place (4 B read + 4 B written per element) and in place (the steady state), as device
    time per call (events around --reps calls queued back to back) and GB/s, beside tools/fill_bw.py's stream figures for the
    same bytes (fill_ of the flat buffer, copy_ of a buffer of its size) and the torch form of the same work
    (torch._foreach_div + torch.cat).
(b) "step": a whole training step at the reference's training shape (tools/train_step_time.py's set-up, every training switch on
    its device value) at world = 1 over RCCL ("nccl"), three forms on three copies of one network:
      exchange   forward + backward, GradExchange.exchange (pack, all_reduce, views), DeviceAdam(clip 40)
      ddp        torch DistributedDataParallel(find_unused_parameters=True) around the same computation, clip_grad_value_(., 40)
                 + torch.optim.Adam over one group per tensor: the reference's form (lib/train/trainers/trainer.py:23-33, :84-86)
      single     the single-process step: forward + backward, DeviceAdam(clip 40)
      rank_ordered_sync   as "exchange" with GradExchange(reduce="rank_ordered") on a network converted to SyncBatchNorm under
                 cfg.train_sync_bn = "device": at world 1 no collective runs, what differs from "exchange" (the step as it was
                 before these options) is the BatchNorm backward's split launches (train_ops.SyncBnActFn)
(c) "rank_sum": th_rank_sum (K28) at world 2, 3 and 8 on the live set's flat buffer -- the parts emulated on one device, the sum
    written over rank 0's part -- as device time per call and GB/s over (world + 1) * slice * 4 bytes, beside a copy_ that moves
    the same bytes.  As in (a), buffers of this size live in the Infinity Cache: these are its rates, not HBM's.
(d) "sync_bn": th_bn_act_bwd_sums + th_bn_act_bwd_apply (world 1) against th_bn_act_bwd at the trunk's five BatchNorm sites'
    shapes for V = 3 views of 512 x 512.
Per figure: the median of --rounds alternating rounds with the lowest and the highest round beside it.  Prints one JSON line.
No threshold on any figure.  One rank on one device: what a multi-GPU node adds is the transport, which this does not measure."""
import argparse
import copy
import datetime
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]


def spread(v, digits=4):
    return {"median": round(float(np.median(v)), digits), "min": round(float(np.min(v)), digits), "max": round(float(np.max(v)), digits)}


def device_ms(fn, reps):
    import torch
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def pack_times(dev, rounds, reps):
    import torch
    from transhuman_amd import hip
    from transhuman_amd.networks.cross_transformer import Network
    from transhuman_amd.train_dist import flat_layout
    torch.manual_seed(0)
    net = Network().to(dev)
    names = [k for k, _ in net.named_parameters()]
    params = list(net.parameters())
    dead = [k.endswith(("cls_token", "mask_token")) or ".layer3." in k or ".layer4." in k or "PE" in k for k in names]
    gen = torch.Generator().manual_seed(1)
    grads = [torch.randn(p.shape, generator=gen).to(dev) for p in params]
    plan = hip.AdamPlan(params)
    counts = [p.numel() for p in params]
    out = {}
    for label, live in (("live", [not d for d in dead]), ("all", [True] * len(params))):
        offsets, n = flat_layout(counts, live)
        flat, other = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        views = [flat[int(o):int(o) + c] if o >= 0 else None for o, c in zip(offsets, counts)]
        src = [g if l else None for g, l in zip(grads, live)]
        have = [g for g in src if g is not None]
        src_ptrs = plan.pack(src, offsets, 2, flat, n)                   # (checked once; the timed calls hand over the addresses)
        view_ptrs = plan.pack(views, offsets, 2, flat, n)
        forms = {
            "pack": lambda: plan.pack(src_ptrs, offsets, 2, flat, n),
            "pack_in_place": lambda: plan.pack(view_ptrs, offsets, 2, flat, n),
            "torch_foreach_div_cat": lambda: torch.cat([g.reshape(-1) for g in torch._foreach_div(have, 2.0)]),
            "fill": lambda: flat.fill_(1.0),
            "copy": lambda: other.copy_(flat),
        }
        ms = {f: [] for f in forms}
        for f in forms.values():
            f()
        for r in range(rounds):
            order = list(forms) if r % 2 == 0 else list(forms)[::-1]
            for f in order:
                ms[f].append(device_ms(forms[f], reps))
        moved = {"pack": 8, "pack_in_place": 8, "torch_foreach_div_cat": 16, "fill": 4, "copy": 8}      # bytes per element
        out[label] = {"tensors": int(sum(live)), "flat_elems": int(n), "flat_MB": round(n * 4 / 1e6, 2)}
        for f in forms:
            med = float(np.median(ms[f]))
            out[label][f] = {"device_ms": spread(ms[f]), "GB_per_s": round(moved[f] * n / med / 1e6, 1), "bytes_per_element": moved[f]}
    return out


def live_flat_elems():
    import torch
    from transhuman_amd.networks.cross_transformer import Network
    from transhuman_amd.train_dist import flat_layout
    torch.manual_seed(0)
    net = Network()
    names = [k for k, _ in net.named_parameters()]
    dead = [k.endswith(("cls_token", "mask_token")) or ".layer3." in k or ".layer4." in k or "PE" in k for k in names]
    return flat_layout([p.numel() for p in net.parameters()], [not d for d in dead])[1]


def timed_rounds(forms, rounds, reps):
    ms = {f: [] for f in forms}
    for f in forms.values():
        f()
    for r in range(rounds):
        for f in (list(forms) if r % 2 == 0 else list(forms)[::-1]):
            ms[f].append(device_ms(forms[f], reps))
    return ms


def rank_sum_times(dev, rounds, reps):
    import torch
    from transhuman_amd import hip
    from transhuman_amd.train_dist import rank_slice
    n = live_flat_elems()
    out = {"flat_elems": int(n)}
    gen = torch.Generator().manual_seed(2)
    for world in (2, 3, 8):
        sl = rank_slice(n, world)
        parts = torch.randn(world * sl, generator=gen).to(dev)
        half = (world + 1) * sl // 2                                          # a copy_ that reads and writes the same bytes in all
        a, b = torch.zeros(half, device=dev), torch.zeros(half, device=dev)
        ms = timed_rounds({"rank_sum": lambda: hip.rank_sum(parts, world, sl, parts[:sl]), "copy": lambda: b.copy_(a)}, rounds, reps)
        moved = (world + 1) * sl * 4
        out[f"world{world}"] = {"slice_elems": int(sl), "MB_moved": round(moved / 1e6, 2)}
        for f, v in ms.items():
            out[f"world{world}"][f] = {"device_ms": spread(v), "GB_per_s": round(moved / float(np.median(v)) / 1e6, 1)}
    return out


def sync_bn_times(dev, rounds, reps):
    import torch
    from transhuman_amd import hip
    sites = {"bn1 64@256x256 relu": (64, 256, True, False), "layer1.bn1 64@128x128 relu": (64, 128, True, False),
             "layer1.bn2 64@128x128 residual relu": (64, 128, True, True), "layer2.bn2 128@64x64 residual relu": (128, 64, True, True),
             "layer2.downsample 128@64x64": (128, 64, False, False)}
    gen = torch.Generator().manual_seed(3)
    out = {}
    for label, (C, hw, relu, res) in sites.items():
        y, g = (torch.randn((3, C, hw, hw), generator=gen).to(dev) for _ in range(2))
        o = torch.relu(torch.randn((3, C, hw, hw), generator=gen)).to(dev) if relu else None
        gamma = torch.rand(C, generator=gen).to(dev) + 0.5

        def split():
            rec = hip.bn_act_bwd_sums(y, o, g)
            return hip.bn_act_bwd_apply(y, o, g, gamma, 1e-5, rec[None], 0, need_residual=res and relu)

        ms = timed_rounds({"bn_act_bwd": lambda: hip.bn_act_bwd(y, o, g, gamma, 1e-5, need_residual=res and relu),
                           "sums_apply": split}, rounds, reps)
        assert all(a is None or torch.equal(a, b) for a, b in zip(split(), hip.bn_act_bwd(y, o, g, gamma, 1e-5,
                                                                                            need_residual=res and relu)))
        out[label] = {f: {"device_ms": spread(v)} for f, v in ms.items()}
    return out


def step_times(dev, rounds, steps, warmup):
    import torch
    import torch.distributed as dist
    from train_step_time import RAYS, setup
    from transhuman_amd.config import TRAIN_SWITCHES, override
    from transhuman_amd.networks.renderer.if_clight_renderer import Renderer
    from transhuman_amd.train_dist import GradExchange
    from transhuman_amd.train_optim import DeviceAdam
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29517")
    dist.init_process_group("nccl", rank=0, world_size=1, timeout=datetime.timedelta(seconds=300))
    try:
        net0, r0, b = setup(dev)
        target = torch.rand((1, RAYS, 3), device=dev)

        class Step(torch.nn.Module):
            def __init__(self, net, renderer):
                super().__init__()
                self.net = net
                self.renderer = [renderer]                                   # (not a submodule: it holds the same net)

            def forward(self, batch, tgt):
                ret = self.renderer[0].render(batch)
                return torch.mean((ret["rgb_map"] - tgt) ** 2) + 0.1 * ret["acc_map"].mean() + 0.01 * ret["depth_map"].mean()

        from transhuman_amd import synth
        body, _ = synth.make_body(0)
        d = np.load(os.path.join(ROOT, "tests", "golden", "synth_assign.npz"))
        assign = d["assign_500"].astype(np.int64) if "assign_500" in d.files else synth.kmeans_assign(body, 500).astype(np.int64)
        forms = {}
        for form in ("exchange", "ddp", "single", "rank_ordered_sync"):
            net = net0 if form == "single" else copy.deepcopy(net0)
            if form == "rank_ordered_sync":
                net = torch.nn.SyncBatchNorm.convert_sync_batchnorm(net)
            r = r0 if form == "single" else Renderer(net, vertex_can=body.astype(np.float64) * 1.02 + 0.001, pc2voxel_ind=assign)
            mod = Step(net, r)
            params = [p for p in net.parameters() if p.requires_grad]
            groups = [{"params": [p], "lr": 7e-4, "weight_decay": 0} for p in params]
            if form == "ddp":
                ddp = torch.nn.parallel.DistributedDataParallel(mod, device_ids=[dev.index], output_device=dev.index,
                                                                find_unused_parameters=True)
                opt = torch.optim.Adam(groups, 7e-4)

                def one(ddp=ddp, opt=opt, params=params):
                    loss = ddp(b, target)
                    opt.zero_grad()
                    loss.backward()
                    torch.nn.utils.clip_grad_value_(params, 40.0)
                    opt.step()
            else:
                opt = DeviceAdam(groups, 7e-4, clip_value=40.0)
                ex = None
                if form != "single":
                    ex = GradExchange(params, reduce="rank_ordered" if form == "rank_ordered_sync" else None)

                def one(mod=mod, opt=opt, ex=ex):
                    loss = mod(b, target)
                    opt.zero_grad()
                    loss.backward()
                    if ex is not None:
                        ex.exchange()
                    opt.step()
            forms[form] = one
        ms = {f: [] for f in forms}
        with override(**{k: v[1] for k, v in TRAIN_SWITCHES.items()}, train_sync_bn="device"):
            for f in forms.values():
                for _ in range(warmup):
                    f()
            for rnd in range(rounds):
                for f in (list(forms) if rnd % 2 == 0 else list(forms)[::-1]):
                    per = []
                    for _ in range(steps):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        forms[f]()
                        torch.cuda.synchronize()
                        per.append((time.perf_counter() - t0) * 1e3)
                    ms[f].append(float(np.median(per)))
        return {"backend": dist.get_backend(), "world": 1, "steps_per_round": steps,
                **{f: {"step_ms": spread(v, 2)} for f, v in ms.items()}}
    finally:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20, help="pack: calls per timed round")
    ap.add_argument("--steps", type=int, default=5, help="step: steps per timed round")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="", help="'pack', 'rank_sum', 'sync_bn' or 'step'")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("dp_step_time.py needs an MI355X: a time taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    res = {"gpu": torch.cuda.get_device_name(0), "rounds": args.rounds}
    if args.only in ("", "pack"):
        res["pack"] = pack_times(dev, args.rounds, args.reps)
    if args.only in ("", "rank_sum"):
        res["rank_sum"] = rank_sum_times(dev, args.rounds, args.reps)
    if args.only in ("", "sync_bn"):
        res["sync_bn"] = sync_bn_times(dev, args.rounds, args.reps)
    if args.only in ("", "step"):
        res["step"] = step_times(dev, args.rounds, args.steps, args.warmup)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
