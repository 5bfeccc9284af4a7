"""Evaluator of the rendered images -- the consumer of `renderer.render_fast` in `run.py --type evaluate`
("the evaluator's PSNR / PNG path").

Mirrors /root/reference/lib/evaluators/if_nerf.py: ``evaluate(output, batch)`` appends the frame's MSE and PSNR
(:34-37, :121-130), rebuilds the H x W image from the rays inside the body box (`mask_at_box`, :41-57), crops it to the
mask's bounding rectangle (:60-62) and writes `pred/frame{i}_view{v}.png` and `gt/..._gt.png` under
`<result_dir>/<human>/` (:64-99); ``summarize()`` stores `mse.npy` / `psnr.npy` / `ssim.npy` (and `lpips.npy` when
LPIPS runs, below) and returns the means (:146-175).
PNG files are written with PIL (cv2 is absent; `cv2.imwrite` of a float image = round-to-nearest, saturate to uint8,
and the reference's RGB -> BGR swap followed by cv2's BGR file order is the identity on the stored RGB).

SSIM (:108, `structural_similarity(img_pred, img_gt, multichannel=True)` on the cropped float64 images) is computed on
the device by `hip.ssim` (csrc/k_metrics.hip) from cropped float32 images assembled on the device with the same fill and
crop as ``images()``.  skimage is third-party and absent, so the metric is pinned by its formula -- skimage 0.19's, the
releases that take data_range from the float64 dtype: 7 x 7 uniform window, sample covariance, data_range 2, mean over the
window-interior pixels of each channel, then over the channels -- not by a run of skimage.  Like skimage, a crop smaller
than 7 x 7 raises ValueError.  Without a visible HIP device SSIM is skipped (the list stays empty: there is no CPU path).

LPIPS (:110-117, `lpips.LPIPS(net="vgg")` of the same crops mapped to [-1, 1] with `2 x - 1`) is computed on the device
by `transhuman_amd.lpips.LPIPS` (csrc/k_lpips.hip) from the same device-side crops, permuted to [1, 3, h, w].  It needs two
weight files, which are never downloaded: torchvision's VGG16 (`lpips_vgg16` / `cfg.lpips_vgg16_path`, by default
`<torch.hub.get_dir()>/checkpoints/vgg16-397923af.pth` when that file exists) and LPIPS's `weights/v0.1/vgg.pth`
(`lpips_lin` / `cfg.lpips_lin_path`, no default).  It runs when both are found and a HIP device is visible; then
``evaluate`` returns ``"lpips"`` and ``summarize`` writes `lpips.npy`.  A configured path that does not exist raises
FileNotFoundError; a crop smaller than 16 x 16 raises ValueError.  Without the weights nothing changes: no ``"lpips"`` key
and no `lpips.npy`.  The metric is the vendored third_parties/lpips (see transhuman_amd/lpips.py for how it may differ
from the PyPI package the reference's evaluator imports).
"""
import os

import numpy as np
import torch

from . import hip
from .config import cfg_get, get_cfg
from .mesh import psnr_metric


def _np(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def bounding_rect(mask):
    """cv2.boundingRect of a binary mask -> (x, y, w, h)"""
    ys, xs = np.nonzero(mask)
    if ys.size == 0:
        return 0, 0, 0, 0
    return int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)


def to_uint8(img):
    """what cv2.imwrite does to a float image: saturate_cast<uchar>(x) = round to nearest, clamp to [0, 255]"""
    return np.clip(np.rint(img * 255.0), 0, 255).astype(np.uint8)


def _weight_path(given, key, default=None):
    """an explicitly given or configured path must exist; the default is used only when it does"""
    p = given if given is not None else cfg_get(key)
    if p is not None:
        p = os.path.expanduser(str(p))
        if not os.path.isfile(p):
            raise FileNotFoundError(f"LPIPS weights: {key} = {p!r} does not exist")
        return p
    return default if default is not None and os.path.isfile(default) else None


class Evaluator:
    def __init__(self, result_dir=None, lpips_vgg16=None, lpips_lin=None):
        cfg = get_cfg()
        self.result_dir = result_dir if result_dir is not None else os.path.join(
            getattr(cfg, "result_dir", "data/result"), "epoch_" + str(getattr(getattr(cfg, "test", None), "epoch", -1)),
            str(getattr(getattr(cfg, "test", None), "exp_folder_name", "debug")))
        self.mse, self.psnr, self.ssim, self.lpips = [], [], [], []
        self.lpips_vgg16 = _weight_path(lpips_vgg16, "lpips_vgg16_path",
                                        os.path.join(torch.hub.get_dir(), "checkpoints", "vgg16-397923af.pth"))
        self.lpips_lin = _weight_path(lpips_lin, "lpips_lin_path")
        self.lpips_on = self.lpips_vgg16 is not None and self.lpips_lin is not None
        self._lpips_net = None

    def psnr_metric(self, img_pred, img_gt):
        return psnr_metric(img_pred, img_gt)

    def images(self, rgb_pred, rgb_gt, batch, H=None, W=None):
        """(:41-62) full-frame prediction / ground truth from the masked ray list, cropped to the box's rectangle"""
        cfg = get_cfg()
        if H is None:
            H, W = int(cfg.H * cfg.ratio), int(cfg.W * cfg.ratio)
        m = _np(batch["mask_at_box"][0]).reshape(H, W).astype(bool)
        fill = 1.0 if cfg.white_bkgd else 0.0
        pred = np.full((H, W, 3), fill)
        gt = np.full((H, W, 3), fill)
        pred[m] = rgb_pred
        gt[m] = rgb_gt
        x, y, w, h = bounding_rect(m)
        return pred[y:y + h, x:x + w], gt[y:y + h, x:x + w]

    def device_images(self, rgb_pred, rgb_gt, batch, H=None, W=None):
        """(:39-62) the cropped images of ``images()``, assembled as float32 [h, w, 3] on the device"""
        cfg = get_cfg()
        if H is None:
            H, W = int(cfg.H * cfg.ratio), int(cfg.W * cfg.ratio)
        dev = rgb_pred.device if torch.is_tensor(rgb_pred) and rgb_pred.is_cuda else \
            torch.device("cuda", torch.cuda.current_device())
        m = torch.as_tensor(batch["mask_at_box"][0], device=dev).reshape(H, W).bool()
        x, y, w, h = bounding_rect(_np(m))
        m = m[y:y + h, x:x + w]
        fill = 1.0 if cfg.white_bkgd else 0.0
        pred = torch.full((h, w, 3), fill, dtype=torch.float32, device=dev)
        gt = torch.full((h, w, 3), fill, dtype=torch.float32, device=dev)
        pred[m] = torch.as_tensor(rgb_pred, device=dev).to(torch.float32)
        gt[m] = torch.as_tensor(rgb_gt, device=dev).to(torch.float32)
        return pred, gt

    def ssim_metric(self, rgb_pred, rgb_gt, batch, H=None, W=None):
        """(:108) SSIM of the cropped images of ``images()``, assembled on the device -> hip.ssim"""
        return hip.ssim(*self.device_images(rgb_pred, rgb_gt, batch, H, W))

    def lpips_metric(self, rgb_pred, rgb_gt, batch, H=None, W=None):
        """(:110-117) LPIPS (VGG16) of the cropped images of ``images()`` mapped to [-1, 1], [1, 3, h, w] -> th_lpips"""
        return self._lpips_of(*self.device_images(rgb_pred, rgb_gt, batch, H, W))

    def _lpips_of(self, pred, gt):
        if self._lpips_net is None:
            from .lpips import LPIPS
            self._lpips_net = LPIPS(net="vgg", vgg16_path=self.lpips_vgg16, model_path=self.lpips_lin, device=pred.device)
        p, g = (t.permute(2, 0, 1)[None] * 2.0 - 1.0 for t in (pred, gt))
        return float(self._lpips_net(p, g).item())

    def evaluate(self, output, batch, H=None, W=None, save=True):
        from PIL import Image
        rgb_pred = _np(output["rgb_map"][0])
        rgb_gt = _np(batch["rgb"][0])
        mse = float(np.mean((rgb_pred - rgb_gt) ** 2))                     # :124
        self.mse.append(mse)
        self.psnr.append(self.psnr_metric(rgb_pred, rgb_gt))               # :127
        out = {"mse": mse, "psnr": self.psnr[-1]}
        if "mask_at_box" in batch and hip._gpu_visible():
            crops = self.device_images(output["rgb_map"][0], batch["rgb"][0], batch, H, W)
            self.ssim.append(hip.ssim(*crops))                              # :108, :131-133
            out["ssim"] = self.ssim[-1]
            if self.lpips_on:
                self.lpips.append(self._lpips_of(*crops))                  # :110-117
                out["lpips"] = self.lpips[-1]
        if save and "mask_at_box" in batch:
            pred, gt = self.images(rgb_pred, rgb_gt, batch, H, W)
            human = batch["human_name"][0] if "human_name" in batch else "human"
            frame = int(_np(batch["frame_index"]).reshape(-1)[0]) if "frame_index" in batch else len(self.mse) - 1
            view = int(_np(batch["cam_ind"]).reshape(-1)[0]) if "cam_ind" in batch else 0
            for sub, img, suffix in (("pred", pred, ""), ("gt", gt, "_gt")):
                d = os.path.join(self.result_dir, human, sub)
                os.makedirs(d, exist_ok=True)
                Image.fromarray(to_uint8(img)).save(os.path.join(d, f"frame{frame}_view{view}{suffix}.png"))
        return out

    def summarize(self):
        os.makedirs(self.result_dir, exist_ok=True)
        np.save(os.path.join(self.result_dir, "mse.npy"), self.mse)
        np.save(os.path.join(self.result_dir, "psnr.npy"), self.psnr)
        np.save(os.path.join(self.result_dir, "ssim.npy"), self.ssim)
        out = {"mse": float(np.mean(self.mse)) if self.mse else float("nan"),
               "psnr": float(np.mean(self.psnr)) if self.psnr else float("nan"),
               "ssim": float(np.mean(self.ssim)) if self.ssim else float("nan")}
        if self.lpips_on:                                                   # (like ssim: empty without a device)
            np.save(os.path.join(self.result_dir, "lpips.npy"), self.lpips)
            out["lpips"] = float(np.mean(self.lpips)) if self.lpips else float("nan")
        self.mse, self.psnr, self.ssim, self.lpips = [], [], [], []
        return out
