"""LPIPS (VGG16) of the evaluator -- lib/evaluators/if_nerf.py:19, :29-32, :110-117 -- on the device (csrc/k_lpips.hip).

The metric is the vendored third_parties/lpips/lpips.py:81-124 with net="vgg", version "0.1", lpips=True, spatial=False,
eval mode (dropout is the identity): ScalingLayer, VGG16 features[0:30] with the taps relu1_2 .. relu5_3, per tap
normalize_tensor (third_parties/lpips/__init__.py:40-42: x / (sqrt(sum_c x^2 + 1e-10) + 1e-10), the eps twice),
(f0 - f1)^2, the 1x1 lin_k without bias, the spatial mean, the sum of the five taps.  The reference's evaluator imports the
PyPI `lpips` package instead, which (as far as its published source goes; not checked here, it is absent) differs only in
normalize_tensor: it has no eps inside the sqrt.  That changes a value only where sum_c x^2 is near 1e-10.

The convolutions run in fp32 on the fp32-input MFMA and the head in fp64, so the value is checked against the float64
evaluation of the formula (tests/test_lpips_host.py: lpips_oracle), not against a cuDNN run of the reference.

Weights: torchvision's pretrained VGG16 (`vgg16-397923af.pth`, keys features.{0,2,5,...,28}.{weight,bias}) and LPIPS's
`weights/v0.1/vgg.pth` (keys lin{k}.model.1.weight).  Nothing is downloaded: both files are read from the given paths.

As the training loss (lib/train/trainers/if_nerf_clight.py:68-72): called under enabled grad on an in0 that requires grad,
``forward`` goes through ``train_ops.LpipsFn`` (th_lpips_train / th_lpips_bwd) and the value carries the gradient into in0.
"""
import torch

from . import hip

VGG16_CONV_INDICES = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)


def _load(path):
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if isinstance(sd, dict) and "state_dict" in sd and isinstance(sd["state_dict"], dict):
        sd = sd["state_dict"]
    if not isinstance(sd, dict):
        raise ValueError(f"{path}: expected a state dict, got {type(sd).__name__}")
    return sd


def _take(sd, key, shape, path):
    if key not in sd:
        raise KeyError(f"{path}: missing key {key!r}")
    t = sd[key]
    if not torch.is_tensor(t) or tuple(t.shape) != tuple(shape):
        got = tuple(t.shape) if torch.is_tensor(t) else type(t).__name__
        raise ValueError(f"{path}: key {key!r} has shape {got}, expected {tuple(shape)}")
    return t


def load_lpips_weights(vgg16_path, lin_path, device=None):
    """Read the 13 VGG16 conv layers (torchvision key names; `classifier.*` is ignored) and the 5 LPIPS lin layers with
    torch.load(weights_only=True); every shape is checked, and a missing or misshaped key is an error naming it.
    -> (conv_w [13], conv_b [13], lin_w [5]) float32 tensors on `device` (CPU if None)."""
    vgg, lin = _load(vgg16_path), _load(lin_path)
    conv_w, conv_b, lin_w = [], [], []
    for i, (co, ci) in zip(VGG16_CONV_INDICES, hip.LPIPS_CONV_SHAPES):
        conv_w.append(_take(vgg, f"features.{i}.weight", (co, ci, 3, 3), vgg16_path))
        conv_b.append(_take(vgg, f"features.{i}.bias", (co,), vgg16_path))
    for k, c in enumerate(hip.LPIPS_TAP_CHANNELS):
        lin_w.append(_take(lin, f"lin{k}.model.1.weight", (1, c, 1, 1), lin_path))
    dev = torch.device(device) if device is not None else torch.device("cpu")
    cvt = [[t.detach().to(dev, torch.float32).contiguous() for t in ts] for ts in (conv_w, conv_b, lin_w)]
    return tuple(cvt)


class LPIPS:
    """lpips.LPIPS(net="vgg") as the reference's evaluator builds it (if_nerf.py:19), backed by th_lpips.

    forward(in0, in1, retPerLayer=False, normalize=False) takes NCHW [N, 3, H, W] images in [-1, 1] (in [0, 1] with
    normalize=True) and returns [N, 1, 1, 1] (and with retPerLayer the list of the five [N, 1, 1, 1] tap values), as the
    reference does; the values are float64 (the head's precision).  (The reference's forward sums the taps into res[0] in
    place, lpips.py:109-111, so its list holds the total in place of the first tap; this list holds the tap itself.)
    Needs a HIP device; H and W must be >= 16."""

    def __init__(self, net="vgg", version="0.1", lpips=True, spatial=False, vgg16_path=None, model_path=None,
                 device=None, verbose=False):
        if net not in ("vgg", "vgg16"):
            raise NotImplementedError(f"LPIPS net {net!r}: only 'vgg' is implemented")
        if version != "0.1":
            raise NotImplementedError(f"LPIPS version {version!r}: only '0.1' is implemented")
        if not lpips:
            raise NotImplementedError("LPIPS lpips=False (the uncalibrated baseline) is not implemented")
        if spatial:
            raise NotImplementedError("LPIPS spatial=True is not implemented")
        if vgg16_path is None or model_path is None:
            raise ValueError("LPIPS needs vgg16_path (torchvision's vgg16-397923af.pth) and model_path (LPIPS's "
                             "weights/v0.1/vgg.pth): nothing is downloaded")
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        conv_w, conv_b, lin_w = load_lpips_weights(vgg16_path, model_path, dev)
        self.device = dev
        self.packed = hip.lpips_pack(conv_w, conv_b, lin_w, dev)
        self._vgg16_path, self._model_path = vgg16_path, model_path     # the input-gradient image (as large again) is packed
        self.packed_bwd = None                                          # from the files on first use
        if verbose:
            print(f"LPIPS (vgg, v0.1) from {vgg16_path} and {model_path}")

    def forward(self, in0, in1, retPerLayer=False, normalize=False):
        if normalize:                                        # lpips.py:82-84
            in0 = 2 * in0 - 1
            in1 = 2 * in1 - 1
        if torch.is_grad_enabled() and in0.requires_grad:
            return self._forward_train(in0, in1, retPerLayer)
        out = hip.lpips(in0.to(self.device), in1.to(self.device), self.packed)
        val = out[:, 5].reshape(-1, 1, 1, 1)
        if retPerLayer:
            return val, [out[:, k].reshape(-1, 1, 1, 1) for k in range(5)]
        return val

    def _forward_train(self, in0, in1, retPerLayer):
        from .networks.train_ops import LpipsFn
        if retPerLayer:
            raise NotImplementedError("LPIPS: retPerLayer has no gradient path (only the total does)")
        if self.packed_bwd is None:
            conv_w, _, _ = load_lpips_weights(self._vgg16_path, self._model_path)
            self.packed_bwd = hip.lpips_pack_bwd(conv_w, self.device)
        if in0.dim() == 3:
            in0, in1 = in0[None], in1[None]
        return LpipsFn.apply(in0.to(self.device), in1.to(self.device), self.packed, self.packed_bwd).reshape(-1, 1, 1, 1)

    __call__ = forward
