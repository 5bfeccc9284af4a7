"""The input views of a frame, prepared on the device from the raw camera pictures (csrc/k_prep.hip, K16): union and border marking
of the raw masks, lens undistortion, area resize, background masking.

The reference's dataset does this on the host with OpenCV for every view of every frame (lib/datasets/light_stage/can_smpl.py:
``get_mask`` / ``get_input_mask`` :118-200 and ``process_loaded`` :629-660: the uint8 picture / 255, ``cv2.undistort`` of picture and
mask, ``cv2.resize`` by ``cfg.ratio`` with INTER_AREA / INTER_NEAREST, the picture set to the background colour where the resized
mask is 0; the target view's mask gets the border between its 5 x 5 erosion and dilation marked with 100).  OpenCV is third-party
and absent wherever this project builds or runs, so no picture of cv2's own exists to compare with.  The image is therefore
DEFINED BY THIS PROJECT, written after OpenCV's documented algorithm; BIT PARITY WITH cv2 IS UNPINNED: OpenCV's
SIMD paths may fuse the four-tap sum, and its 15-bit integer weight table has a saturation fix-up that is not reproduced here.

Definition.  Every step is ONE correctly rounded IEEE operation in the order written (no contraction), so the device equals the
numpy restatement below bit for bit, not approximately.

  inputs      per view: img uint8 [H0,W0,3], msk uint8 [H0,W0], K fp32 [3,3], D fp32 [5] = (k1, k2, p1, p2, k3);
              n = 1 / ratio must be 1, 2 or 4 and divide H0 and W0 (ValueError otherwise); H = H0 / n, W = W0 / n.
  map         float64 on the exactly promoted fp32 K and D, for source pixel (col j, row i):
              x = (j - cx) / fx, y = (i - cy) / fy, x2 = x x, y2 = y y, r2 = x2 + y2, t = (2 x) y,
              kr = 1 + ((k3 r2 + k2) r2 + k1) r2, xd = (x kr + p1 t) + p2 (r2 + 2 x2), yd = (y kr + p1 (r2 + 2 y2)) + p2 t,
              u = fx xd + cx, v = fy yd + cy, iu = rint(32 u), iv = rint(32 v), half to even (a coordinate that is not finite or
              has |32 u| >= 2^30 is taken as -2^20: every tap outside); X = iu >> 5, a = iu & 31, Y = iv >> 5, b = iv & 31.
  weights     of the taps (X,Y), (X+1,Y), (X,Y+1), (X+1,Y+1): W00 = (32-b)(32-a), W01 = (32-b) a, W10 = b (32-a), W11 = b a (their
              sum is 1024).  A tap outside the image contributes the constant 0.
  picture     per channel, fp32: s = float(u8) / 255.0f (a 256-entry table made here with numpy's fp32 division),
              w = float(W) / 1024.0f (exact), o = ((s00 w00 + s01 w01) + s10 w10) + s11 w11.
  mask        m' = (W00 m00 + W01 m01 + W10 m10 + W11 m11 + 512) >> 10 in integers, for any uint8 values (100 included).
  resize      picture: the n x n block summed in fp32 in row-major order from 0, times float(1 / (n n)); mask: m'[n y, n x].
  background  with ``mask_bkgd`` a pixel whose resized mask is 0 becomes 0 on all three channels (1 with ``white_bkgd``).
  outputs     imgs fp32 [V,3,H,W] (what ``batch['input_imgs'][t][0]`` is), msk uint8 [V,H,W], K_out = K with its first two rows
              multiplied by ratio in fp32.
  raw masks   m = (a != 0) | (b != 0) of one or two raw masks; with ``border`` (odd, <= 15; the reference uses 5) ero / dil are
              the minimum / maximum of m over the border x border window, over the pixels of it that lie inside the image, and
              m = 100 where dil - ero == 1; ``border = 0`` skips this.

``prepare_views`` / ``combine_masks`` run on the device (no host wait); ``prepare_views_oracle`` / ``combine_masks_oracle`` restate the
definition in numpy and import without a GPU.  tests/test_preprocess_host.py checks the restatement against scipy.ndimage
(map_coordinates on the quantised coordinates, minimum_filter / maximum_filter); tests/test_gpu_preprocess.py holds the device to
the restatement at every pixel.

Colour jitter (training only; the reference applies it to the raw frames before all of the above) is K25, further down:
``jitter_params`` / ``color_jitter`` (device) / ``color_jitter_oracle`` (numpy), with its own definition there.
"""
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import hip
from .config import cfg_get

RATIOS = (1, 2, 4)
MAX_BORDER = 15
Q_MAX = float(1 << 30)
Q_OUT = -(1 << 20)
MAX_DIM = 16384


def unit_table():
    """fp32 [256]: float(i) / 255.0f, numpy's fp32 division"""
    return np.arange(256, dtype=np.float32) / np.float32(255.0)


def block_factor(ratio):
    """n = 1 / ratio, which must be 1, 2 or 4"""
    r = float(ratio)
    n = int(round(1.0 / r)) if r > 0.0 else 0
    if n not in RATIOS or n * r != 1.0:
        raise ValueError(f"ratio is {ratio}: 1 / ratio must be 1, 2 or 4")
    return n


def _check_sizes(H0, W0, n):
    if not (1 <= H0 <= MAX_DIM and 1 <= W0 <= MAX_DIM):
        raise ValueError(f"image size {H0} x {W0}: 1 <= H0, W0 <= {MAX_DIM}")
    if H0 % n or W0 % n:
        raise ValueError(f"image size {H0} x {W0} is not divisible by 1 / ratio = {n}")


def _check_border(border):
    b = int(border)
    if b != border or b < 0 or b > MAX_BORDER or (b > 0 and b % 2 == 0):
        raise ValueError(f"border is {border}: 0 or an odd value up to {MAX_BORDER}")
    return b


def scale_K(K, ratio):
    """K with its first two rows multiplied by ratio, in fp32 (torch tensor or ndarray; a copy)"""
    if torch.is_tensor(K):
        out = K.to(torch.float32).clone()
        out[..., :2, :] = out[..., :2, :] * float(ratio)
        return out
    out = np.array(K, np.float32)
    out[..., :2, :] = out[..., :2, :] * np.float32(ratio)
    return out


# ---------------------------------------------------------------------------
# device
# ---------------------------------------------------------------------------
_lut = {}


def _table(device):
    key = str(device)
    if key not in _lut:
        _lut[key] = torch.from_numpy(unit_table()).to(device)
    return _lut[key]


def _u8_dev(x, name, device=None, allow_bool=False):
    """a contiguous uint8 device tensor; anything but uint8 (or bool, for masks) is rejected: a float picture would have to be
    guessed to be 0..1 or 0..255"""
    t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
    if t.dtype is torch.bool and allow_bool:
        t = t.to(torch.uint8)
    if t.dtype is not torch.uint8:
        raise TypeError(f"{name} must be uint8, not {t.dtype}")
    if not t.is_cuda:
        t = t.to(device if device is not None else torch.device("cuda", torch.cuda.current_device()))
    return t.contiguous()


def _f32_dev(x, device):
    t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
    return t.detach().to(device=device, dtype=torch.float32).contiguous()


def combine_masks(msk, msk_cihp=None, border=0):
    """th_prep_mask: one or two raw masks uint8 (or bool) [V,H0,W0] or [H0,W0] (device tensor or ndarray) -> uint8 of the same
    shape on the device: (msk != 0) | (msk_cihp != 0), and with ``border`` (odd, <= 15) 100 on the border between the erosion and
    the dilation by a border x border window.  No host wait."""
    border = _check_border(border)
    a = _u8_dev(msk, "msk", allow_bool=True)
    b = None if msk_cihp is None else _u8_dev(msk_cihp, "msk_cihp", a.device, allow_bool=True)
    if a.dim() not in (2, 3) or a.numel() == 0:
        raise ValueError(f"msk has shape {tuple(a.shape)}: [V,H0,W0] or [H0,W0]")
    if b is not None and b.shape != a.shape:
        raise ValueError(f"msk {tuple(a.shape)} and msk_cihp {tuple(b.shape)} differ in shape")
    H0, W0 = a.shape[-2:]
    V = a.numel() // (H0 * W0)
    _check_sizes(H0, W0, 1)
    lib = hip.load_library()
    out = torch.empty_like(a)
    hip._check(lib.th_prep_mask(hip.ctx(a.device), hip._p(a), hip._p(b), V, H0, W0, border, hip._p(out), hip._stream()))
    return out


def prepare_views(imgs_u8, msks_u8, K, D, ratio=None, mask_bkgd=True, white_bkgd=None):
    """th_prep_views: imgs_u8 uint8 [V,H0,W0,3], msks_u8 uint8 [V,H0,W0] (any values; 100 survives), K [V,3,3], D [V,5] or
    [V,5,1] (device tensors or ndarrays) -> (imgs fp32 [V,3,H,W], msk uint8 [V,H,W], K_out fp32 [V,3,3]) on the device.
    ``ratio`` defaults to cfg.ratio, ``white_bkgd`` to cfg.white_bkgd.  No host wait."""
    ratio = cfg_get("ratio", 0.5) if ratio is None else ratio
    white_bkgd = bool(cfg_get("white_bkgd", False)) if white_bkgd is None else bool(white_bkgd)
    n = block_factor(ratio)
    img = _u8_dev(imgs_u8, "imgs_u8")
    dev = img.device
    msk = _u8_dev(msks_u8, "msks_u8", dev, allow_bool=True)
    if img.dim() != 4 or img.shape[-1] != 3 or img.numel() == 0:
        raise ValueError(f"imgs_u8 has shape {tuple(img.shape)}: [V,H0,W0,3]")
    V, H0, W0 = img.shape[:3]
    if tuple(msk.shape) != (V, H0, W0):
        raise ValueError(f"msks_u8 has shape {tuple(msk.shape)}: {(V, H0, W0)} for these pictures")
    _check_sizes(H0, W0, n)
    Kd, Dd = _f32_dev(K, dev), _f32_dev(D, dev)
    if Kd.numel() != V * 9 or Dd.numel() != V * 5:
        raise ValueError(f"K {tuple(Kd.shape)} / D {tuple(Dd.shape)}: [V,3,3] and [V,5] (or [V,5,1]) for V = {V} views")
    Kd = Kd.reshape(V, 3, 3)
    H, W = H0 // n, W0 // n
    lib = hip.load_library()
    out = torch.empty((V, 3, H, W), dtype=torch.float32, device=dev)
    out_msk = torch.empty((V, H, W), dtype=torch.uint8, device=dev)
    hip._check(lib.th_prep_views(hip.ctx(dev), hip._p(img), hip._p(msk), V, H0, W0, hip._p(Kd), hip._p(Dd), n, int(bool(mask_bkgd)),
                                 int(white_bkgd), hip._p(_table(dev)), hip._p(out), hip._p(out_msk), hip._stream()))
    return out, out_msk, scale_K(Kd, ratio)


# ---------------------------------------------------------------------------
# colour jitter of the raw frames (csrc/k_jitter.hip, K25)
# ---------------------------------------------------------------------------
# The reference trains with ``jitter: True``: process_loaded (can_smpl.py:629-637) puts the RAW uint8 frame of the target view and of
# every input view through torchvision's ColorJitter(brightness=(0.2, 2), contrast=(0.3, 2), saturation=(0.2, 2), hue=(-0.5, 0.5))
# before it undistorts them, reseeded with the same number for all views of an item.  torchvision is absent wherever this project
# builds or runs: the draws and the order of operations follow its documented ColorJitter and PARITY WITH torchvision IS UNPINNED;
# the image arithmetic is Pillow's (ImageEnhance.Brightness / Contrast / Color, convert("HSV") / convert("RGB")), which
# tests/test_jitter_host.py holds ``color_jitter_oracle`` to byte for byte.  Definition, per uint8 pixel:
#   grey        L = (19595 R + 38470 G + 7471 B + 32768) >> 16
#   blend       blend(d, x, f) = d + f (x - d) in fp32 (x - d in integers, f rounded to fp32, product and sum rounded one by one);
#               0 <= f <= 1: truncated; otherwise 0 where <= 0, 255 where >= 255, else truncated
#   brightness  blend(0, x, f) per channel          saturation  blend(L, x, f) per channel, L of that pixel
#   contrast    blend(m, x, f), m = int(sum L / n + 0.5) = (2 sum L + n) // (2 n) over the n pixels of THAT image as it stands then
#   hue h       RGB -> HSV, H <- (H + d) mod 256 with d = trunc(255 h) mod 256, HSV -> RGB; d = 0 is no shortcut (the round trip is
#               lossy).  RGB -> HSV: V = max; max == min: H = S = 0; else in fp32 c = max - min, s = c / max, rc, gc, bc = (max - R) / c,
#               ...; h = bc - gc if R == max, else 2.0 + rc - bc if G == max, else 4.0 + gc - rc, evaluated in double and rounded to
#               fp32; h <- fp32(fmod(double(h) / 6.0 + 1.0, 1.0)); H = clip(int(double(h) 255.0)), S = clip(int(double(s) 255.0)).
#               HSV -> RGB: S == 0: R = G = B = V; else in double x = H 6.0 / 255.0, i = floor(x), f = x - i, fs = S / 255.0,
#               p = round(V (1 - fs)), q = round(V (1 - fs f)), t = round(V (1 - fs (1 - f))) (half away from zero, clipped to
#               0..255, every product and difference rounded on its own: no fused multiply-add), (R, G, B) by i mod 6:
#               (V,t,p) (q,V,p) (p,V,t) (p,q,V) (t,p,V) (V,p,q)
#   parameters  ``order`` = randperm(4), then b, c, s, h uniform in their ranges, on a local generator seeded with the item's seed;
#               the operations run in ``order`` (0 brightness, 1 contrast, 2 saturation, 3 hue); None switches one off
JITTER_RANGES = dict(brightness=(0.2, 2), contrast=(0.3, 2), saturation=(0.2, 2), hue=(-0.5, 0.5))
JITTER_MODES = ("batch", "device")
BRIGHTNESS, CONTRAST, SATURATION, HUE = range(4)


class JitterParams(NamedTuple):
    """``order``: the four operation numbers in the order they run; a factor that is None switches its operation off"""
    order: tuple
    brightness: Optional[float]
    contrast: Optional[float]
    saturation: Optional[float]
    hue: Optional[float]


def jitter_params(seed, brightness=JITTER_RANGES["brightness"], contrast=JITTER_RANGES["contrast"],
                  saturation=JITTER_RANGES["saturation"], hue=JITTER_RANGES["hue"]):
    """The parameter set of one item: torchvision's ColorJitter.get_params on a LOCAL generator seeded with ``seed`` (the global
    generator is neither reseeded nor advanced): order = randperm(4), then one uniform draw per range that is not None."""
    g = torch.Generator().manual_seed(int(seed))
    order = tuple(int(i) for i in torch.randperm(4, generator=g))
    draw = lambda r: None if r is None else float(torch.empty(1).uniform_(float(r[0]), float(r[1]), generator=g))
    return JitterParams(order, draw(brightness), draw(contrast), draw(saturation), draw(hue))


def hue_shift(h):
    """d = trunc(255 h) mod 256: what is added to the H plane"""
    return int(float(h) * 255.0) % 256


def _jitter_args(params):
    """(order, [b, c, s] as fp32 or None, d or None) of a JitterParams or a plain 5-tuple, checked"""
    order, b, c, s, h = params
    order = tuple(int(i) for i in order)
    if sorted(order) != [0, 1, 2, 3]:
        raise ValueError(f"jitter order is {order}: a permutation of 0, 1, 2, 3")
    factors = []
    for name, f in (("brightness", b), ("contrast", c), ("saturation", s)):
        if f is not None and not (0.0 <= float(f) < float("inf")):
            raise ValueError(f"{name} factor is {f}: a finite value >= 0, or None")
        factors.append(None if f is None else np.float32(f))
    if h is not None and not -0.5 <= float(h) <= 0.5:
        raise ValueError(f"hue is {h}: -0.5 <= hue <= 0.5, or None")
    return order, factors, None if h is None else hue_shift(h)


def batch_jitter(batch):
    """The parameter set that cfg.input_jitter asks for on this batch, or None.  "batch" (default): None -- the dataset did it, as
    in the reference.  "device": ``jitter_params(batch['jitter_seed'])`` -- the seed a Python int or a CPU int64 tensor, the
    reference's ``index + epoch * cfg.seed`` (no device read is made for it); a batch without a seed (the reference's test split)
    is not jittered."""
    mode = cfg_get("input_jitter", "batch")
    if mode not in JITTER_MODES:
        raise ValueError(f'cfg.input_jitter is {mode!r}: "batch" or "device"')
    if mode == "batch" or "jitter_seed" not in batch:
        return None
    seed = batch["jitter_seed"]
    if torch.is_tensor(seed):
        if seed.is_cuda or seed.numel() != 1 or seed.dtype.is_floating_point:
            raise TypeError("batch['jitter_seed'] must be a Python int or a CPU integer tensor of one element")
        seed = seed.item()
    return jitter_params(int(seed))


def _frames(shape):
    if len(shape) < 3 or shape[-1] != 3 or 0 in shape:
        raise ValueError(f"imgs_u8 has shape {tuple(shape)}: [V,H,W,3] or [H,W,3]")
    H, W = (int(n) for n in shape[-3:-1])
    _check_sizes(H, W, 1)
    V = int(np.prod(shape[:-3], dtype=np.int64))
    if V > 65535:
        raise ValueError(f"{V} images: at most 65535")
    return V, H, W


def color_jitter(imgs_u8, params):
    """th_color_jitter: imgs_u8 uint8 [V,H,W,3] (or [H,W,3], or more leading dimensions; device tensor or ndarray), ``params`` a
    JitterParams or a plain (order, brightness, contrast, saturation, hue) -> a new uint8 device tensor of the same shape, every
    image with the definition above applied (the contrast mean is each image's own).  No host wait."""
    order, factors, d = _jitter_args(params)
    img = _u8_dev(imgs_u8, "imgs_u8")
    V, H, W = _frames(img.shape)
    lib = hip.load_library()
    out = torch.empty_like(img)
    ws = hip._ws(lib.th_color_jitter_workspace_bytes(V, H, W), img.device)
    enabled = sum(1 << op for op, f in enumerate(factors + [d]) if f is not None)
    b, c, s = (0.0 if f is None else float(f) for f in factors)
    hip._check(lib.th_color_jitter(hip.ctx(img.device), hip._p(img), V, H, W, sum(op << (2 * k) for k, op in enumerate(order)), b, c, s,
                                   d or 0, enabled, hip._p(out), hip._p(ws), ws.numel(), hip._stream()))
    return out


# ---------------------------------------------------------------------------
# numpy restatement of the definition
# ---------------------------------------------------------------------------
def _np(x, dtype=None):
    a = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return a if dtype is None else a.astype(dtype)


def _u8_np(x, name, allow_bool=False):
    a = _np(x)
    if a.dtype == np.bool_ and allow_bool:
        a = a.astype(np.uint8)
    if a.dtype != np.uint8:
        raise TypeError(f"{name} must be uint8, not {a.dtype}")
    return a


def undistort_map_oracle(K, D, H0, W0):
    """(iu, iv) int64 [H0,W0]: rint(32 u), rint(32 v) of the definition's map for one view"""
    k = _np(K, np.float32).reshape(3, 3).astype(np.float64)
    k1, k2, p1, p2, k3 = _np(D, np.float32).reshape(5).astype(np.float64)
    fx, fy, cx, cy = k[0, 0], k[1, 1], k[0, 2], k[1, 2]
    j = np.broadcast_to(np.arange(W0, dtype=np.float64)[None, :], (H0, W0))
    i = np.broadcast_to(np.arange(H0, dtype=np.float64)[:, None], (H0, W0))
    with np.errstate(all="ignore"):
        x, y = (j - cx) / fx, (i - cy) / fy
        x2, y2 = x * x, y * y
        r2, t = x2 + y2, (2.0 * x) * y
        kr = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
        xd = (x * kr + p1 * t) + p2 * (r2 + 2.0 * x2)
        yd = (y * kr + p1 * (r2 + 2.0 * y2)) + p2 * t
        u, v = fx * xd + cx, fy * yd + cy

        def quant(c):
            q = 32.0 * c
            ok = np.abs(q) < Q_MAX
            return np.where(ok, np.rint(np.where(ok, q, 0.0)), float(Q_OUT)).astype(np.int64)
        return quant(u), quant(v)


def _taps(iu, iv, H0, W0):
    """[(row, col, inside, weight int64)] of the four taps, in the definition's order"""
    X, Y, a, b = iu >> 5, iv >> 5, iu & 31, iv & 31
    out = []
    for ty, tx, w in ((0, 0, (32 - b) * (32 - a)), (0, 1, (32 - b) * a), (1, 0, b * (32 - a)), (1, 1, b * a)):
        r, c = Y + ty, X + tx
        inside = (r >= 0) & (r < H0) & (c >= 0) & (c < W0)
        out.append((np.clip(r, 0, H0 - 1), np.clip(c, 0, W0 - 1), inside, w))
    return out


def taps_outside_oracle(K, D, H0, W0):
    """int [H0,W0]: how many of a source pixel's four taps lie outside the image"""
    return sum((~inside).astype(np.int64) for _, _, inside, _ in _taps(*undistort_map_oracle(K, D, H0, W0), H0, W0))


def undistort_oracle(img_u8, msk_u8, K, D):
    """One view at full resolution: (o fp32 [H0,W0,3], m' uint8 [H0,W0])"""
    img, msk = _u8_np(img_u8, "img"), _u8_np(msk_u8, "msk", allow_bool=True)
    H0, W0 = msk.shape
    s = unit_table()[img]                                                    # fp32 [H0,W0,3]
    o, m = None, np.full((H0, W0), 512, np.int64)
    for r, c, inside, w in _taps(*undistort_map_oracle(K, D, H0, W0), H0, W0):
        wf = w.astype(np.float32) / np.float32(1024.0)
        p = np.where(inside[..., None], s[r, c], np.float32(0.0)) * wf[..., None]
        o = p if o is None else o + p
        m = m + w * np.where(inside, msk[r, c].astype(np.int64), 0)
    assert o.dtype == np.float32
    return o, (m >> 10).astype(np.uint8)


def area_resize_oracle(o, n):
    """fp32 [H0,W0,...] -> [H0/n,W0/n,...]: the n x n block summed in row-major order from 0, times float(1 / (n n))"""
    o = np.asarray(o, np.float32)
    acc = np.zeros((o.shape[0] // n, o.shape[1] // n) + o.shape[2:], np.float32)
    for dy in range(n):
        for dx in range(n):
            acc = acc + o[dy::n, dx::n]
    return acc * np.float32(1.0 / (n * n))


def prepare_views_oracle(imgs_u8, msks_u8, K, D, ratio=None, mask_bkgd=True, white_bkgd=None):
    """The definition on the host: (imgs fp32 [V,3,H,W], msk uint8 [V,H,W], K_out fp32 [V,3,3]) as numpy arrays."""
    ratio = cfg_get("ratio", 0.5) if ratio is None else ratio
    white_bkgd = bool(cfg_get("white_bkgd", False)) if white_bkgd is None else bool(white_bkgd)
    n = block_factor(ratio)
    imgs, msks = _u8_np(imgs_u8, "imgs_u8"), _u8_np(msks_u8, "msks_u8", allow_bool=True)
    if imgs.ndim != 4 or imgs.shape[-1] != 3 or imgs.size == 0:
        raise ValueError(f"imgs_u8 has shape {imgs.shape}: [V,H0,W0,3]")
    V, H0, W0 = imgs.shape[:3]
    if msks.shape != (V, H0, W0):
        raise ValueError(f"msks_u8 has shape {msks.shape}: {(V, H0, W0)} for these pictures")
    _check_sizes(H0, W0, n)
    Ks, Ds = _np(K, np.float32).reshape(V, 3, 3), _np(D, np.float32).reshape(V, 5)
    out = np.empty((V, 3, H0 // n, W0 // n), np.float32)
    out_msk = np.empty((V, H0 // n, W0 // n), np.uint8)
    for view in range(V):
        o, m = undistort_oracle(imgs[view], msks[view], Ks[view], Ds[view])
        small, m = area_resize_oracle(o, n), m[::n, ::n]
        if mask_bkgd:
            small[m == 0] = np.float32(1.0 if white_bkgd else 0.0)
        out[view] = small.transpose(2, 0, 1)
        out_msk[view] = m
    return out, out_msk, scale_K(Ks, ratio)


def combine_masks_oracle(msk, msk_cihp=None, border=0):
    """The definition's raw-mask rule on the host: uint8, the shape of ``msk``."""
    border = _check_border(border)
    a = _u8_np(msk, "msk", allow_bool=True)
    m = a != 0
    if msk_cihp is not None:
        b = _u8_np(msk_cihp, "msk_cihp", allow_bool=True)
        if b.shape != a.shape:
            raise ValueError(f"msk {a.shape} and msk_cihp {b.shape} differ in shape")
        m = m | (b != 0)
    out = m.astype(np.uint8)
    if border:
        H0, W0 = m.shape[-2:]
        r = border // 2
        # windows clipped to the image: pad the erosion with 1 and the dilation with 0, which never decide a minimum / maximum
        pad = [(0, 0)] * (m.ndim - 2) + [(r, r), (r, r)]
        lo, hi = np.pad(out, pad, constant_values=1), np.pad(out, pad, constant_values=0)
        ero, dil = np.ones_like(out), np.zeros_like(out)
        for dy in range(border):
            for dx in range(border):
                ero = np.minimum(ero, lo[..., dy:dy + H0, dx:dx + W0])
                dil = np.maximum(dil, hi[..., dy:dy + H0, dx:dx + W0])
        out[(dil - ero) == 1] = 100
    return out


def grey_oracle(x):
    """L of int64 [...,3] pixels"""
    return (19595 * x[..., 0] + 38470 * x[..., 1] + 7471 * x[..., 2] + 32768) >> 16


def blend_oracle(d, x, f):
    """blend(d, x, f) of the definition: d, x int64 arrays (broadcast), f a float -> int64"""
    f = np.float32(f)
    t = d.astype(np.float32) + f * (x - d).astype(np.float32)
    assert t.dtype == np.float32
    if 0.0 <= f <= 1.0:
        return t.astype(np.int64)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.clip(t, 0, 255).astype(np.int64)))


def rgb_to_hsv_oracle(x):
    """int64 [...,3] RGB -> int64 [...,3] HSV, Pillow's integer HSV"""
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    mx, mn = x.max(-1), x.min(-1)
    flat = mx == mn
    f32 = lambda a: a.astype(np.float32)
    with np.errstate(all="ignore"):
        c = f32(np.where(flat, 1, mx - mn))
        s = c / f32(np.maximum(mx, 1))
        rc, gc, bc = (f32(mx - ch) / c for ch in (r, g, b))
        d = lambda a: a.astype(np.float64)
        h = np.where(r == mx, d(bc) - d(gc), np.where(g == mx, (2.0 + d(rc)) - d(bc), (4.0 + d(gc)) - d(rc))).astype(np.float32)
        h = np.fmod(d(h) / 6.0 + 1.0, 1.0).astype(np.float32)
        H = np.clip((d(h) * 255.0).astype(np.int64), 0, 255)
        S = np.clip((d(s) * 255.0).astype(np.int64), 0, 255)
    return np.stack([np.where(flat, 0, H), np.where(flat, 0, S), mx], -1)


def _round_u8(v):
    """half away from zero (v >= 0 here), clipped to 0..255"""
    lo = np.floor(v)
    return np.clip((lo + ((v - lo) >= 0.5)).astype(np.int64), 0, 255)


def hsv_to_rgb_oracle(x):
    """int64 [...,3] HSV -> int64 [...,3] RGB, Pillow's"""
    H, S, V = (x[..., k].astype(np.float64) for k in range(3))
    t6 = H * 6.0 / 255.0
    i = np.floor(t6)
    f = t6 - i
    fs = S / 255.0
    p = _round_u8(V * (1.0 - fs))
    q = _round_u8(V * (1.0 - fs * f))
    t = _round_u8(V * (1.0 - fs * (1.0 - f)))
    v = x[..., 2]
    sextant = i.astype(np.int64) % 6
    table = ((v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q))
    out = np.stack([np.choose(sextant, [row[k] for row in table]) for k in range(3)], -1)
    return np.where((x[..., 1] == 0)[..., None], v[..., None], out)


def hue_oracle(x, d):
    """the hue operation with the integer shift d on int64 [...,3] pixels"""
    hsv = rgb_to_hsv_oracle(x)
    hsv[..., 0] = (hsv[..., 0] + int(d)) % 256
    return hsv_to_rgb_oracle(hsv)


def color_jitter_oracle(imgs_u8, params):
    """The definition on the host: uint8 ndarray of the shape of ``imgs_u8`` ([V,H,W,3], [H,W,3] or more leading dimensions)."""
    order, (b, c, s), d = _jitter_args(params)
    imgs = _u8_np(imgs_u8, "imgs_u8")
    V, H, W = _frames(imgs.shape)
    out = np.empty((V, H, W, 3), np.uint8)
    for v, img in enumerate(imgs.reshape(V, H, W, 3)):
        x = img.astype(np.int64)
        for op in order:
            if op == BRIGHTNESS and b is not None:
                x = blend_oracle(np.zeros_like(x), x, b)
            elif op == CONTRAST and c is not None:
                total, n = int(grey_oracle(x).sum()), H * W
                x = blend_oracle(np.full_like(x, (2 * total + n) // (2 * n)), x, c)
            elif op == SATURATION and s is not None:
                x = blend_oracle(np.broadcast_to(grey_oracle(x)[..., None], x.shape), x, s)
            elif op == HUE and d is not None:
                x = hue_oracle(x, d)
        out[v] = x
    return out.reshape(imgs.shape)
