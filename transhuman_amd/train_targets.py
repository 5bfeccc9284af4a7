"""The training targets of a step, made on the device (csrc/k_patch.hip, K18): the rays of ``cfg.patch.N_patches`` random
``size x size`` patches of the target view and what the loss reads beside them.

The reference builds them per step in numpy inside its dataset: the train split of ``sample_ray_patch``
(lib/utils/if_nerf/if_nerf_data_utils.py:445-499 with its helpers :287-443, called at lib/datasets/light_stage/can_smpl.py:507-516);
the trainer reads ``target_patches``, ``patch_masks`` and ``patch_div_indices`` from the batch
(lib/train/trainers/if_nerf_clight.py:54-62).

Definition.  Inputs are the dense per-pixel arrays of ``hip.gen_rays(..., compact=False)`` (K9: ray_o, ray_d, near, far and the
3-D box test ``ray_mask``), ``msk`` uint8 [H,W] (any values, 100 marks the silhouette border), ``bound_mask`` uint8 [H,W]
(``hip.bound_2d_mask``), the float32 image and ``draws`` float64 [N,2] in [0, 1), which stand for the reference's two random
numbers per patch (``np.random.rand(1)[0]`` :383 and ``np.random.choice(n)`` :302).

  m = msk * bound_mask in uint8 (:455); human = m > 0 (:461); background = ray_mask & ~human (:368-371, :482)
  patch i   candidate set = human if draws[i,0] < subject_ratio else background (:383-386); n = its pixel count (0: ValueError, as
            np.random.choice raises); centre = its k-th pixel in np.where order, k = min(floor(draws[i,1] n), n - 1), the product in
            float64; x_min = clip(cx - P // 2, 0, W - P), y_min likewise (:307-315)
  window    patch_masks[i] = ray_mask, patch_masks_sub[i] = human, target_patches[i] = the image, on [y_min, y_min + P) x
            [x_min, x_min + P) (:329-344, :433-438)
  rays      the window's ray_mask pixels in row-major order (:328-330), the patches one after the other (:402), overlapping
            patches repeating their rays; select_inds = cumsum(ray_mask) - 1 at those pixels (:336-337); rgb, ray_o, ray_d, near,
            far and sub_mask (= human) gathered there (:347-353, :429-431); patch_div_indices = the running ray count (:379-400)

Only selection and copies: ``sample_patch_rays`` (device) equals ``sample_patch_rays_oracle`` (numpy, imports without a GPU) bit for
bit.  tests/test_train_targets_host.py holds the restatement to the reference's own outputs (tests/golden/g22_patch_rays.npz);
tests/test_gpu_train_targets.py holds the device to the restatement.  The non-patch train split (sample_ray_h36m) is not part of this.
"""
import numpy as np
import torch

from . import hip
from .config import cfg_get

MAX_DIM = 4096
MAX_PATCH = 64
MAX_PATCHES = 64
REFERENCE_KEYS = ("rgb", "ray_o", "ray_d", "near", "far", "sub_mask", "patch_masks", "patch_masks_sub", "target_patches",
                  "patch_div_indices")


def _patch_cfg(n_patches, patch_size, subject_ratio):
    p = cfg_get("patch")
    n = p.N_patches if n_patches is None else n_patches
    size = p.size if patch_size is None else patch_size
    ratio = p.sample_subject_ratio if subject_ratio is None else subject_ratio
    return int(n), int(size), float(ratio)


def check_limits(H, W, N, P):
    """the limits of th_patch_rays, as ValueError"""
    if not (1 <= H <= MAX_DIM and 1 <= W <= MAX_DIM):
        raise ValueError(f"image size {H} x {W}: 1 <= H, W <= {MAX_DIM}")
    if not (1 <= P <= MAX_PATCH and P <= min(H, W)):
        raise ValueError(f"patch size {P}: 1 <= P <= {MAX_PATCH} and P <= min(H, W) = {min(H, W)}")
    if not 1 <= N <= MAX_PATCHES:
        raise ValueError(f"{N} patches: 1 <= N <= {MAX_PATCHES}")


def _np(x, dtype=None):
    a = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return a if dtype is None else np.ascontiguousarray(a, dtype=dtype)


def _check_draws(d, N=None):
    d = np.asarray(d, np.float64)
    if d.ndim != 2 or d.shape[1] != 2 or (N is not None and d.shape[0] != N):
        raise ValueError(f"draws has shape {d.shape}: [N,2]" + (f" for N = {N} patches" if N is not None else ""))
    if not ((d >= 0.0) & (d < 1.0)).all():
        raise ValueError("draws must lie in [0, 1)")
    return d


# ---------------------------------------------------------------------------
# numpy restatement of the definition
# ---------------------------------------------------------------------------
def sample_patch_rays_oracle(img, msk, bound_mask, dense_rays, draws, patch_size=None, subject_ratio=None):
    """The definition on the host.  img float32 [H,W,3]; msk, bound_mask uint8 [H,W]; dense_rays {ray_o, ray_d [H*W,3], near, far
    [H*W], mask_at_box [H*W]}; draws float64 [N,2].  Returns numpy arrays with the reference's dtypes: rgb, ray_o, ray_d [R',3], near,
    far [R'] float32, sub_mask bool [R',1], patch_masks, patch_masks_sub bool [N,P,P], target_patches float32 [N,P,P,3],
    patch_div_indices, select_inds int64, xy_min, xy_max int64 [N,2]."""
    img, msk, bound = _np(img, np.float32), _np(msk), _np(bound_mask)
    if msk.dtype != np.uint8 or bound.dtype != np.uint8:
        raise TypeError(f"msk and bound_mask must be uint8, not {msk.dtype} / {bound.dtype}")
    H, W = msk.shape
    draws = _check_draws(_np(draws))
    N, P, ratio = _patch_cfg(draws.shape[0], patch_size, subject_ratio)
    check_limits(H, W, N, P)
    if img.shape != (H, W, 3) or bound.shape != (H, W):
        raise ValueError(f"img {img.shape} / bound_mask {bound.shape}: [H,W,3] / [H,W] for a {H} x {W} msk")
    ray_mask = _np(dense_rays["mask_at_box"]).reshape(-1) != 0
    ray_o, ray_d = (_np(dense_rays[k], np.float32).reshape(-1, 3) for k in ("ray_o", "ray_d"))
    near, far = (_np(dense_rays[k], np.float32).reshape(-1) for k in ("near", "far"))
    if not (ray_mask.size == H * W and ray_o.shape[0] == H * W and ray_d.shape[0] == H * W and near.size == H * W and far.size == H * W):
        raise ValueError(f"dense_rays must hold one row per pixel of the {H} x {W} image")
    human = (msk * bound) > 0                                                       # :455, :461 (uint8 product)
    background = ray_mask.reshape(H, W) & ~human                                    # :368-371
    masked_indices = np.cumsum(ray_mask) - 1                                        # :336
    pix, masks, masks_sub, xy_min, div = [], [], [], [], [0]
    for u0, u1 in draws:
        cand = human if u0 < ratio else background                                  # :383-386
        ys, xs = np.where(cand)                                                     # :299
        n = ys.shape[0]
        if n == 0:
            raise ValueError("a patch's candidate set (" + ("subject" if u0 < ratio else "background") + " pixels) is empty")
        k = min(int(np.floor(u1 * np.float64(n))), n - 1)
        x0 = int(np.clip(xs[k] - P // 2, 0, W - P))                                 # :307-315
        y0 = int(np.clip(ys[k] - P // 2, 0, H - P))
        rows = (np.arange(y0, y0 + P)[:, None] * W + np.arange(x0, x0 + P)[None, :]).reshape(-1)
        sel = rows[ray_mask[rows]]                                                  # :328-330 (row-major)
        pix.append(sel)
        masks.append(ray_mask[rows].reshape(P, P))
        masks_sub.append(human.reshape(-1)[rows].reshape(P, P))
        xy_min.append([x0, y0])
        div.append(div[-1] + sel.size)
    pix = np.concatenate(pix)
    xy_min = np.asarray(xy_min, np.int64)
    flat = img.reshape(-1, 3)
    return dict(rgb=flat[pix], ray_o=ray_o[pix], ray_d=ray_d[pix], near=near[pix], far=far[pix],
                sub_mask=human.reshape(-1, 1)[pix], patch_masks=np.stack(masks), patch_masks_sub=np.stack(masks_sub),
                target_patches=np.stack([img[y:y + P, x:x + P] for x, y in xy_min]),
                patch_div_indices=np.asarray(div, np.int64), select_inds=masked_indices[pix].astype(np.int64),
                xy_min=xy_min, xy_max=xy_min + P)


# ---------------------------------------------------------------------------
# device
# ---------------------------------------------------------------------------
def _device_of(*xs):
    for x in xs:
        if torch.is_tensor(x) and x.is_cuda:
            return x.device
    hip.ctx()                                                                       # (raises without a device)
    return torch.device("cuda", torch.cuda.current_device())


def assemble(raw, counts):
    """The dict ``sample_patch_rays`` returns, from ``hip.patch_rays``' raw outputs and their ``counts`` read to the host (int
    [2,N]): ValueError for an empty candidate set, the ray rows cut to R', masks as bool."""
    counts = np.asarray(counts, np.int64)
    if (counts[0] == 0).any():
        raise ValueError(f"the candidate set of patch {int(np.argmax(counts[0] == 0))} is empty")
    div = np.concatenate([[0], np.cumsum(counts[1])]).astype(np.int64)
    n = int(div[-1])
    P = raw["patch_masks"].shape[-1]
    xy_min = raw["xy_min"].to(torch.int64)
    out = {k: raw[k][:n] for k in ("rgb", "ray_o", "ray_d", "near", "far", "select_inds")}
    out.update(sub_mask=raw["sub_mask"][:n].bool()[:, None], patch_masks=raw["patch_masks"].bool(),
               patch_masks_sub=raw["patch_masks_sub"].bool(), target_patches=raw["target_patches"],
               patch_div_indices=torch.from_numpy(div), xy_min=xy_min, xy_max=xy_min + P)
    return out


def sample_patch_rays(img, msk, K, R, T, bounds, draws=None, n_patches=None, patch_size=None, subject_ratio=None, generator=None):
    """The train split of sample_ray_patch for one target view, on the device.  img float32 [H,W,3] or [3,H,W] (K16's layout) and msk
    uint8 [H,W]: device tensors (host arrays are uploaded); K [3,3], R [3,3], T [3,1], bounds [2,3]: host values, read like
    ``hip.gen_rays`` reads them.  ``draws`` float64 [N,2] in [0, 1) (default: ``torch.rand(N, 2, dtype=float64,
    generator=generator)`` on the host); N, P and subject_ratio default to cfg.patch.{N_patches, size, sample_subject_ratio}.

    Chains th_gen_rays, th_bound_mask and th_patch_rays on the current stream, then reads the 2 N counts to the host (the one wait
    of the call): they size R' and fill ``patch_div_indices``.  Returns device tensors under the reference's keys -- rgb, ray_o,
    ray_d [R',3], near, far [R'], sub_mask bool [R',1], patch_masks, patch_masks_sub bool [N,P,P], target_patches [N,P,P,3],
    patch_div_indices (int64, on the host) -- plus xy_min, xy_max int64 [N,2] and select_inds int64 [R'].  ValueError for an empty
    candidate set (np.random.choice raises there) and for sizes outside 1 <= P <= 64, P <= min(H, W), 1 <= N <= 64, H, W <= 4096."""
    if n_patches is None and draws is not None:
        n_patches = len(draws)
    N, P, ratio = _patch_cfg(n_patches, patch_size, subject_ratio)
    if msk.ndim != 2:
        raise ValueError(f"msk has shape {tuple(msk.shape)}: [H,W]")
    H, W = (int(n) for n in msk.shape)
    check_limits(H, W, N, P)
    if tuple(img.shape) not in ((H, W, 3), (3, H, W)):
        raise ValueError(f"img has shape {tuple(img.shape)}: [H,W,3] or [3,H,W] for a {H} x {W} msk")
    if draws is None:
        draws = torch.rand(N, 2, dtype=torch.float64, generator=generator)
    if not (torch.is_tensor(draws) and draws.is_cuda):
        draws = torch.from_numpy(_check_draws(_np(draws), N))
    elif tuple(draws.shape) != (N, 2):
        raise ValueError(f"draws has shape {tuple(draws.shape)}: [N,2] for N = {N} patches")
    dev = _device_of(img, msk)
    as_dev = lambda x, dt: (x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))).to(device=dev, dtype=dt)
    img, msk, draws = as_dev(img, torch.float32), as_dev(msk, torch.uint8), as_dev(draws, torch.float64)
    Kh, Rh, Th, bh = (_np(a, np.float32) for a in (K, R, T, bounds))
    with torch.cuda.device(dev):
        dense = hip.gen_rays(Kh, Rh, Th, bh, H, W, device=dev, compact=False)
        pose = np.concatenate([Rh.reshape(3, 3), Th.reshape(3, 1)], axis=1)                     # :452
        bound = hip.bound_2d_mask(bh.reshape(2, 3), Kh.reshape(3, 3), pose, H, W, device=dev)
        raw = hip.patch_rays(dense, msk, bound, img, draws, ratio, P)
        counts = raw["counts"].cpu().numpy()
    return assemble(raw, counts)


def add_targets(batch):
    """cfg.target_prep == "device" (Renderer.render's training entry): the reference's target keys, made here and ADDED TO
    ``batch`` with the collated leading 1 -- the one place this package mutates a batch, because the unchanged trainer reads
    ``patch_masks`` / ``target_patches`` / ``patch_div_indices`` from it after ``render`` returns.  A key that is present is
    never overwritten, and a batch that carries ``ray_o`` is left as it is.

    Reads ``target_R``, ``target_T`` [1,3,3] / [1,3,1], ``can_bounds`` [1,2,3] and either ``target_K`` [1,3,3] with the prepared view
    ``target_img`` float32 [1,H,W,3] + ``target_msk`` uint8 [1,H,W], or the raw frame ``target_img_raw`` uint8 [1,H0,W0,3],
    ``target_msk_raw`` [1,H0,W0], optional ``target_msk_cihp_raw``, ``target_K_raw`` [1,3,3], ``target_D`` [1,5], which goes through
    ``combine_masks(border=5)`` and ``prepare_views`` (can_smpl.py:118-158, :629-660; the scaled K is used in place of target_K);
    with cfg.input_jitter == "device" and ``jitter_seed`` in the batch the raw frame first gets the colour jitter of that seed, the
    parameter set the input views get (can_smpl.py:629-637; ``preprocess.batch_jitter``, K25).
    Optional ``patch_draws`` float64 [1,N,2]."""
    patch = cfg_get("patch")
    if not bool(patch.use_patch_sampling):
        raise ValueError('cfg.target_prep = "device" makes the patch targets only: cfg.patch.use_patch_sampling is false')
    if "ray_o" in batch:
        return batch
    raw_keys = ("target_img_raw", "target_msk_raw", "target_K_raw", "target_D")
    has_raw = all(k in batch for k in raw_keys)
    has_prepared = all(k in batch for k in ("target_img", "target_msk", "target_K"))
    if not (has_raw or has_prepared) or any(k not in batch for k in ("target_R", "target_T", "can_bounds")):
        raise ValueError('cfg.target_prep = "device": the batch has no ray_o and lacks the target view (target_R, target_T, '
                         "can_bounds and target_img + target_msk + target_K, or target_img_raw + target_msk_raw + target_K_raw + "
                         "target_D)")
    if has_prepared:
        img, msk, K = batch["target_img"][0], batch["target_msk"][0], batch["target_K"][0]
    else:
        from . import preprocess
        cihp = batch.get("target_msk_cihp_raw")
        m = preprocess.combine_masks(batch["target_msk_raw"][0], None if cihp is None else cihp[0], border=5)
        jitter = preprocess.batch_jitter(batch)
        frame = batch["target_img_raw"] if jitter is None else preprocess.color_jitter(batch["target_img_raw"], jitter)
        imgs, msks, Ks = preprocess.prepare_views(frame, m[None], batch["target_K_raw"], batch["target_D"],
                                                  mask_bkgd=bool(cfg_get("mask_bkgd", True)))
        img, msk, K = imgs[0], msks[0], Ks[0]
    draws = batch.get("patch_draws")
    out = sample_patch_rays(img, msk, K, batch["target_R"][0], batch["target_T"][0], batch["can_bounds"][0],
                            draws=None if draws is None else draws[0])
    for k in REFERENCE_KEYS:
        if k not in batch:
            batch[k] = out[k][None]
    return batch
