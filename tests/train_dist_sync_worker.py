"""One rank of the jobs tests/test_gpu_train_dist_rank_ordered.py starts (not a test file), and the definitions that test shares
with it.

    python -m torch.distributed.run --nproc-per-node N tests/train_dist_sync_worker.py --out DIR --trunk          (gloo, every rank on cuda:0)
    python -m torch.distributed.run --nproc-per-node N tests/train_dist_sync_worker.py --out DIR --sync-bn --reduce rank_ordered

--trunk: the encoder trunk alone.  A seeded SpatialEncoder is converted to SyncBatchNorm; under cfg.train_encoder = "device" and
cfg.train_sync_bn = "device" rank r runs autograd_path.trunk_device on its r + 1 images of 3 x 40 x 56 (its part of the batch
``trunk_inputs`` makes) and back-propagates its part of the seeded cotangents.  Written to DIR/trunk<r>.npz: the 30 LOCAL parameter
gradients, the gradient arriving at conv1's output (the finest per-rank quantity there is: K23 builds conv1's weight gradient only,
the images have no gradient on the device path), the running statistics, and how often train_ops.SyncBnActFn ran its backward.

Otherwise: train_dist_worker.train -- the golden step's small case under every training switch's device value, the distributed
Trainer, three steps -- under cfg.train_sync_bn = "device" with MIOpen's deterministic kernels; DIR/rank<r>.npz as that worker writes
it, and DIR/sync<r>.json with the SyncBnActFn count."""
import argparse
import datetime
import json
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

IMAGE = (3, 40, 56)
TRUNK = ("model.conv1.", "model.bn1.", "model.layer1.", "model.layer2.")


# ---- shared with the test process -----------------------------------------------------------------------------------------
def make_encoder(dtype=torch.float32):
    """a seeded SpatialEncoder in train mode whose BatchNorm weights and biases matter (fresh ones are 1 and 0)"""
    from transhuman_amd.networks.encoder import SpatialEncoder
    torch.manual_seed(3)
    enc = SpatialEncoder()
    rs = np.random.RandomState(9)
    with torch.no_grad():
        for b in enc._bn_sites():
            b.weight.copy_(torch.from_numpy(rs.uniform(0.5, 1.5, size=b.weight.shape).astype(np.float32)))
            b.bias.copy_(torch.from_numpy(rs.normal(scale=0.2, size=b.bias.shape).astype(np.float32)))
    return enc.to(dtype).train()


def rank_parts(world):
    """rank r holds r + 1 images: its slice of the concatenated batch"""
    cuts = np.cumsum([0] + [r + 1 for r in range(world)])
    return [slice(int(a), int(b)) for a, b in zip(cuts[:-1], cuts[1:])]


def trunk_inputs(world):
    """the concatenated batch of a ``world``-rank job and a cotangent per latent, fp32, on the host"""
    n = world * (world + 1) // 2
    rs = np.random.RandomState(40 + world)
    images = torch.from_numpy(rs.uniform(size=(n, *IMAGE)).astype(np.float32))
    H, W = IMAGE[1:]
    sizes = [(n, 64, (H + 1) // 2, (W + 1) // 2), (n, 64, (H + 3) // 4, (W + 3) // 4), (n, 128, (H + 7) // 8, (W + 7) // 8)]
    return images, [torch.from_numpy(rs.normal(size=s).astype(np.float32)) for s in sizes]


def trunk_names(enc):
    return [k for k, _ in enc.named_parameters() if k.startswith(TRUNK)]


# ---- the jobs ---------------------------------------------------------------------------------------------------------------
def _conv1_node(lat, weight):
    """the backward node of the convolution whose weight is ``weight``: its arriving gradient is the gradient of conv1's output"""
    seen, todo = set(), [l.grad_fn for l in lat]
    while todo:
        node = todo.pop()
        if node is None or node in seen:
            continue
        seen.add(node)
        nxt = [f for f, _ in node.next_functions if f is not None]
        if type(node).__name__ == "ConvFnBackward" and any(getattr(f, "variable", None) is weight for f in nxt):
            return node
        todo += nxt
    raise RuntimeError("conv1's backward node was not found")


def trunk(args):
    from transhuman_amd import config
    from transhuman_amd.networks import autograd_path, train_ops
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    try:
        enc = torch.nn.SyncBatchNorm.convert_sync_batchnorm(make_encoder().to(dev), process_group=dist.group.WORLD)
        sites = enc._bn_sites()
        assert len(sites) == 10 and all(isinstance(b, torch.nn.SyncBatchNorm) for b in sites)
        images, seeds = trunk_inputs(world)
        part = rank_parts(world)[rank]
        out = {}
        with config.override(train_encoder="device", train_sync_bn="device"):
            lat = autograd_path.trunk_device(enc, images[part].to(dev))
            out["site"] = np.array(type(lat[0].grad_fn).__name__)
            kept = []
            _conv1_node(lat, enc.model.conv1.weight).register_prehook(lambda g: kept.append(g[0].detach().clone()))
            torch.autograd.backward(lat, [s[part].to(dev) for s in seeds])
        torch.cuda.synchronize()
        for k, p in enc.named_parameters():
            if p.grad is not None:
                out["grad:" + k] = p.grad.detach().cpu().numpy()
        out["g_conv1"] = kept[0].cpu().numpy()
        for k, v in enc.state_dict().items():
            if "running_" in k or "num_batches" in k:
                out["stat:" + k] = v.detach().cpu().numpy()
        for i, l in enumerate(lat):
            out[f"lat{i}"] = l.detach().cpu().numpy()
        out["sync_calls"] = np.int64(train_ops.SyncBnActFn.calls)
        np.savez(os.path.join(args.out, f"trunk{rank}.npz"), **out)
    finally:
        dist.destroy_process_group()


def trainer(args):
    import train_dist_worker as W
    from transhuman_amd import config
    from transhuman_amd.networks import train_ops
    torch.backends.cudnn.deterministic = True
    with config.override(train_sync_bn="device"):
        W.train(args)
    with open(os.path.join(args.out, f"sync{os.environ['RANK']}.json"), "w") as f:
        json.dump({"sync_calls": int(train_ops.SyncBnActFn.calls)}, f)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--trunk", action="store_true")
    ap.add_argument("--sync-bn", action="store_true")
    ap.add_argument("--reduce", default=None)
    a = ap.parse_args()
    (trunk if a.trunk else trainer)(a)
