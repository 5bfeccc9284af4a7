"""The training entry (Renderer.render with gradients -> transhuman_amd.networks.autograd_path) against a forward /
backward of the REAL reference (tests/golden/g18_train_step.npz, made by oracle/gen_golden_train.py from the reference's
own Renderer.render + the trainer's image loss): outputs, loss and the gradients of 20 parameters spread over the
encoder, TransHE and the per-point network.  The path is plain torch, so this pin runs on CPU; the GPU test checks that
Renderer.render dispatches to it under autograd and to the HIP kernels under no_grad, and that both agree."""
import pytest
import torch

from transhuman_amd import config
from train_step_case import STEP_CFG, check_step, golden, loss as _loss, setup


def test_training_step_matches_the_reference():
    with config.override(**STEP_CFG):
        check_step(golden(), *setup())


def test_training_randomisations_are_live():
    """cfg.perturb (stratified depth jitter, :276-283) and cfg.raw_noise_std (density noise, nerf_net_utils.py:39-46) change
    the result from call to call in train() mode and leave it alone in eval() / at 0"""
    from transhuman_amd.networks import autograd_path
    with config.override(**STEP_CFG) as cfg:
        net, r, b = setup()
        with torch.no_grad():
            base = autograd_path.render(r, b)["rgb_map"]
            cfg.perturb = 1.0
            a1 = autograd_path.render(r, b)["rgb_map"]
            a2 = autograd_path.render(r, b)["rgb_map"]
            assert float((a1 - a2).abs().max()) > 1e-6 and float((a1 - base).abs().max()) > 1e-6
            net.eval()
            e1 = autograd_path.render(r, b)["rgb_map"]
            e2 = autograd_path.render(r, b)["rgb_map"]
            assert torch.equal(e1, e2)
            net.train()
            cfg.perturb, cfg.raw_noise_std = 0.0, 1.0
            n1 = autograd_path.render(r, b)["rgb_map"]
            n2 = autograd_path.render(r, b)["rgb_map"]
            assert float((n1 - n2).abs().max()) > 1e-7


@pytest.mark.gpu
def test_render_dispatch_on_the_gpu(gpu):
    """Renderer.render: under autograd the differentiable path (loss.backward() reaches the encoder), under no_grad the
    HIP kernels -- and the two agree within the parity bar on the same patch"""
    with config.override(**STEP_CFG) as cfg:
        net, r, b = setup(gpu)
        ret = r.render(b)
        assert ret["rgb_map"].requires_grad
        target = torch.rand(ret["rgb_map"].shape, device=gpu)
        _loss(ret, target).backward()
        g = net.encoder.model.conv1.weight.grad
        assert g is not None and torch.isfinite(g).all() and float(g.abs().max()) > 0
        with torch.no_grad():
            fast = r.render(b)
        assert not fast["rgb_map"].requires_grad
        for k in ("rgb_map", "acc_map", "depth_map"):
            assert float((fast[k] - ret[k].detach()).abs().max()) < 1e-4, k
        # the training-time randomisations are served too (stratified sampling in train() mode)
        cfg.perturb = 1.0
        with torch.no_grad():
            j1, j2 = r.render(b)["rgb_map"], r.render(b)["rgb_map"]
        assert float((j1 - j2).abs().max()) > 1e-6
