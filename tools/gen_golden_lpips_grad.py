"""Write tests/golden/g23_lpips_grad.npz: the gradient of the vendored LPIPS module (third_parties/lpips of the reference
checkout, net "vgg", version 0.1, ``.double()``) with respect to in0, and one case of the trainer's loss
(lib/train/trainers/if_nerf_clight.py:43-106) made with the reference's own _unpack_imgs and scale_for_lpips.

    python tools/gen_golden_lpips_grad.py --reference <reference checkout> [--seed 20]

As tools/gen_golden_lpips.py: CPU only, where the reference checkout exists; the same torchvision stub, pnet_rand=True, and
the seeded He-normal VGG16 weights of tests/test_lpips_host.py (vgg_weights), which the tests regenerate -- the fixture holds
plain arrays only: the lin weights, the images, the values and the gradients.

Every image is ``RandomState(seed).uniform(-1, 1)`` of a seed found by search: the first seeds, from 1000 up, whose float64
forward keeps every pre-activation and every pool decision of the in0 branch 2^-16 of the layer's rms away from its boundary
(tests/test_train_loss_host.py: lpips_margins), so that no decision can differ between an fp32 and a float64 evaluation.  The
seeds are recorded."""
import argparse
import ast
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gen_golden_lpips import _stub_torchvision  # noqa: E402
from test_lpips_host import VGG_CONV_INDICES, vgg_weights  # noqa: E402
from test_train_loss_host import MARGIN, lpips_margins, pair_of_seed  # noqa: E402

PAIRS = [(1, 16, 16, 0.05), (1, 17, 23, None), (1, 16, 33, 0.3), (2, 20, 20, None)]   # (n, h, w, noise; None: unrelated)
L2REC_WEIGHT, LPIPS_WEIGHT = 1.0, 0.1                                                 # train_or_eval.yaml
PATCH = 16


def _clean(in0, w):
    act, pool = lpips_margins(in0, w)
    return act >= MARGIN and pool >= MARGIN


def _trainer_functions(reference):
    """_unpack_imgs and scale_for_lpips of the reference's trainer, taken from its source file (importing the module would pull in
    the whole training stack)"""
    path = os.path.join(reference, "lib", "train", "trainers", "if_nerf_clight.py")
    tree = ast.parse(open(path).read())
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("_unpack_imgs", "scale_for_lpips")]
    assert len(keep) == 2
    ns = {"torch": torch}
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return ns["_unpack_imgs"], ns["scale_for_lpips"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference checkout (holds third_parties/lpips and lib/train)")
    ap.add_argument("--seed", type=int, default=20, help="seed of the VGG16 weights")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "g23_lpips_grad.npz"))
    args = ap.parse_args()
    _stub_torchvision()
    sys.path.insert(0, args.reference)
    from third_parties.lpips import LPIPS

    lin_path = os.path.join(args.reference, "third_parties", "lpips", "weights", "v0.1", "vgg.pth")
    m = LPIPS(net="vgg", pnet_rand=True, model_path=lin_path, verbose=False)
    ws, bs = vgg_weights(args.seed)
    feats = m.net.slice1, m.net.slice2, m.net.slice3, m.net.slice4, m.net.slice5
    mods = {name: mod for s in feats for name, mod in s.named_children()}
    for i, w, b in zip(VGG_CONV_INDICES, ws, bs):
        mods[str(i)].weight.data.copy_(torch.from_numpy(w))
        mods[str(i)].bias.data.copy_(torch.from_numpy(b))
    m = m.double().eval()
    for p in m.parameters():
        p.requires_grad_(False)
    lin_sd = torch.load(lin_path, map_location="cpu", weights_only=True)
    rec = {"seed": np.int64(args.seed), "n_pairs": np.int64(len(PAIRS))}
    for k in range(5):
        rec[f"lin{k}"] = lin_sd[f"lin{k}.model.1.weight"].reshape(-1).numpy().astype(np.float32)

    seed = 1000
    for i, (n, h, w, noise) in enumerate(PAIRS):
        while not _clean(pair_of_seed(seed, n, h, w, noise)[0], (ws, bs)):
            seed += 1
        a, b = pair_of_seed(seed, n, h, w, noise)
        x0 = torch.from_numpy(a).double().requires_grad_(True)
        val = m(x0, torch.from_numpy(b).double())
        val.sum().backward()
        rec[f"in0_{i}"], rec[f"in1_{i}"] = a, b
        rec[f"seed_{i}"], rec[f"noise_{i}"] = np.int64(seed), np.float64(-1.0 if noise is None else noise)
        rec[f"val64_{i}"] = val.detach().reshape(-1).numpy()
        rec[f"grad64_{i}"] = x0.grad.numpy()
        print(f"pair {i}: N {n} {h} x {w} seed {seed} noise {noise}  lpips {rec[f'val64_{i}']}  max |grad| "
              f"{np.abs(rec[f'grad64_{i}']).max():.3e}")
        seed += 1

    # the loss: 2 patches of 16 x 16, the first mask all-false, the second partly true
    unpack, scale_for_lpips = _trainer_functions(args.reference)
    while True:
        rs = np.random.RandomState(seed)
        masks = np.zeros((2, PATCH, PATCH), bool)
        masks[1] = rs.uniform(size=(PATCH, PATCH)) < 0.7
        div = np.array([0, 0, int(masks[1].sum())], np.int64)
        rgb = rs.uniform(size=(int(div[-1]), 3)).astype(np.float32)
        targets = rs.uniform(size=(2, PATCH, PATCH, 3)).astype(np.float32)
        leaf = torch.from_numpy(rgb).double().requires_grad_(True)
        fake = unpack(leaf, torch.from_numpy(masks), bgcolor=torch.zeros(3, dtype=torch.float64),
                      targets=torch.from_numpy(targets).double(), div_indices=torch.from_numpy(div))
        x0 = scale_for_lpips(fake.permute(0, 3, 1, 2))
        if _clean(x0[1:2].detach().float().numpy(), (ws, bs)):
            break
        seed += 1
    t64 = torch.from_numpy(targets).double()
    mse_loss = L2REC_WEIGHT * torch.mean((fake - t64) ** 2)
    lpips_loss = LPIPS_WEIGHT * torch.mean(m(x0, scale_for_lpips(t64.permute(0, 3, 1, 2))))
    loss = mse_loss + lpips_loss
    loss.backward()
    rec.update(loss_seed=np.int64(seed), loss_masks=masks, loss_div=div, loss_rgb=rgb, loss_targets=targets,
               l2rec_weight=np.float64(L2REC_WEIGHT), lpips_weight=np.float64(LPIPS_WEIGHT),
               loss_mse_loss=np.float64(mse_loss.item()), loss_lpips_loss=np.float64(lpips_loss.item()),
               loss_loss=np.float64(loss.item()), loss_grad_rgb=leaf.grad.numpy())
    print(f"loss case: seed {seed}  {int(div[-1])} rays  mse {mse_loss.item():.6f}  lpips {lpips_loss.item():.6f}  "
          f"loss {loss.item():.6f}")
    np.savez_compressed(args.out, **rec)
    print(f"wrote {args.out} ({os.path.getsize(args.out)} bytes)")


if __name__ == "__main__":
    main()
