"""The golden training step (tests/golden/g18_train_step.npz, made by oracle/gen_golden_train.py from the REAL reference's
Renderer.render + the trainer's image loss): its network, renderer and batch, the cfg keys it runs under, and the assertions
every variant of it holds -- outputs, loss and the gradients of 20 parameters spread over the encoder, TransHE and the per-point
network.

Shared by tests/test_train_path.py (CPU, every switch at its default) and the GPU files that run the step under the training
switches (test_gpu_train_ops, _train_attention, _train_vit_dense, _train_maps, _train_point_net, _train_encoder,
_latgather_ordered).  A test sets the keys with ``config.override(**STEP_CFG, **switches)`` around ``setup`` AND the step: Network()
reads cfg.vit_depth when it is built."""
import os

import numpy as np
import torch

from transhuman_amd import synth
from util import GOLD, SIGMA_BIAS, can64, synth_assign

STEP_CFG = dict(vit_depth=2, N_samples=16, num_class=300, perturb=0.0, raw_noise_std=0.0)


def golden():
    return np.load(os.path.join(GOLD, "g18_train_step.npz"))


def setup(device="cpu"):
    """-> net (train mode, the deterministic weights of the golden), its Renderer, the synthetic patch of 400 rays; under STEP_CFG"""
    from transhuman_amd.networks.cross_transformer import Network
    from transhuman_amd.networks.renderer.if_clight_renderer import Renderer
    torch.manual_seed(0)
    net = Network()
    net.load_state_dict(synth.det_state_dict(net.state_dict(), seed=0, sigma_bias=SIGMA_BIAS))
    net.train()
    net = net.to(device)
    r = Renderer(net, vertex_can=can64().numpy(), pc2voxel_ind=synth_assign(300))
    b = synth.batch_to(synth.make_batch(20, 20, 3, seed=0, all_rays=False, focal=62.5), device)
    return net, r, b


def loss(ret, target):
    return torch.mean((ret["rgb_map"] - target) ** 2) + 0.1 * ret["acc_map"].mean() + 0.01 * ret["depth_map"].mean()


def check_step(g, net, renderer, batch):
    """one forward / backward of autograd_path.render under the cfg the caller has set, against the golden ``g``: outputs to 2e-5,
    loss to 1e-6, the 20 golden gradients to 2e-3 of their maximum, and a gradient on every parameter the reference trains"""
    from transhuman_amd.networks import autograd_path
    assert batch["ray_o"].shape[1] == int(g["rays"])
    ret = autograd_path.render(renderer, batch)
    for k, name in (("rgb_map", "rgb"), ("acc_map", "acc"), ("depth_map", "depth")):
        d = float((ret[k][0].detach().cpu() - torch.from_numpy(g[name])).abs().max())
        print(k, d)
        assert d < 2e-5, (k, d)
    step_loss = loss(ret, torch.from_numpy(g["target"])[None].to(ret["rgb_map"].device))
    assert abs(float(step_loss) - float(g["loss"])) < 1e-6
    step_loss.backward()
    params = dict(net.named_parameters())
    keys = [k[5:] for k in g.files if k.startswith("grad:")]
    assert len(keys) == 20
    for k in keys:
        ref = torch.from_numpy(g["grad:" + k])
        got = params[k].grad
        assert got is not None and got.shape == ref.shape, k
        err = float((got.cpu() - ref).abs().max()) / float(ref.abs().max())
        print(k, err)
        assert err < 2e-3, (k, err)
    # every parameter the reference trains receives a gradient (the dead cls / mask tokens and PE buffers do not)
    missing = [k for k, p in params.items() if p.grad is None and not k.endswith(("cls_token", "mask_token"))
               and ".layer3." not in k and ".layer4." not in k and "PE" not in k]
    assert not missing, missing
