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
tests/test_gpu_train_targets.py holds the device to the restatement.

The dataset's other targets (csrc/k_raysample.hip, K26; cfg.target_sampler = "dataset"): ``sample_ray_h36m`` followed by ``get_acc``
(if_nerf_data_utils.py:516-614, :635-641, called at can_smpl.py:518-535) -- every test / evaluation / visualisation batch, and the
training batch when cfg.patch.use_patch_sampling is false.

Definition.  The dense arrays, ``msk``, ``bound_mask`` and the image as above; ``nrays``, ``body_ratio``, ``face_ratio``
(cfg.N_rand, cfg.body_sample_ratio, cfg.face_sample_ratio) and ``draws`` float64 [MAX_ITERS,3,nrays] in [0, 1).

  m = msk * bound_mask in uint8 (:527); rand_set = (bound_mask == 1) & (m != 100) (:530); body = (m == 1), face = (m == 13)
  test      mask_at_box = the box test [H*W]; rgb, ray_o, ray_d, near, far = the dense rows where it holds, in row-major order;
            coord = zeros [R',2] int64 (:600-612)
  train     n = 0; while n < nrays (:545): rem = nrays - n; n_body = int(rem body_ratio), n_face = int(rem face_ratio), the products
            in float64, truncated; n_rand = rem - n_body - n_face.  Each class picks that many of its pixels, in np.argwhere
            (row-major) order, with replacement: pick j of class c (0 body, 1 face, 2 rand) in iteration i is member
            min(floor(draws[i,c,j] n_c), n_c - 1), the product in float64 (np.random.randint(0, n_c, k), :554, :562, :568).  An empty
            body class contributes the SINGLE coordinate (1,1) (:557), an empty rand_set the single coordinate (0,0) (:570), an empty
            face class nothing (:572-575) -- so an iteration can offer fewer coordinates than rem, or one more, and the final count
            can be nrays + 1.  Body, face, rand in that order (:573); the coordinates whose ray hits the box (the dense mask_at_box
            there: get_near_far is elementwise per ray) are appended -- rgb, rays, near, far, coord (row, col) int64 -- and n grows
            by their number (:581-590).  mask_at_box = ones [n] bool (:589).
            The reference never ends when an iteration adds nothing; here that is a ValueError, as are a loop still unfinished
            after MAX_ITERS = 4 iterations, H < 2 or W < 2 (the (1,1) fallback), and ratios outside 0 <= body, face,
            body + face <= 1 (np.random.randint raises for a negative count).
  acc       get_acc(coord, msk) with the caller's msk, not the product (can_smpl.py:525): 1 where any pixel of msk is nonzero in
            the 25 x 25 window centred on coord[i] and clipped to the image, uint8 [n].  In the test split coord is all zeros, so
            acc is one value repeated: the reference's behaviour, kept.

The reference's random stream depends on the class sizes (``np.random.randint(0, n_c, k)``), so it cannot be drawn ahead of time:
as for the patches the definition takes recorded uniforms, and parity with numpy's own bit stream is unpinned.  get_acc is
``cv2.dilate`` with a 25 x 25 kernel of ones, centre anchor and cv2's default border, restated after OpenCV's documented rule; cv2
is absent here, so parity with cv2 itself is unpinned (tests/test_ray_sample_host.py cross-checks the restatement against
scipy.ndimage.maximum_filter).  ``sample_rays_h36m`` (device) equals ``sample_rays_h36m_oracle`` (numpy) bit for bit:
tests/test_ray_sample_host.py holds the restatement to the reference's own outputs (tests/golden/g26_ray_sample.npz),
tests/test_gpu_ray_sample.py holds the device to the restatement.
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
# sample_ray_h36m + get_acc (K26)
MAX_RAYS = 65536
MAX_ITERS = 4
ACC_BORDER = 25
STATUS_ADDED_NOTHING, STATUS_UNFINISHED, STATUS_NEGATIVE_COUNT = 1, 2, 4            # th_ray_sample_train's info[2]
H36M_KEYS = ("rgb", "ray_o", "ray_d", "near", "far", "acc", "mask_at_box")          # can_smpl.py:527-535


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


# ---------------------------------------------------------------------------
# sample_ray_h36m + get_acc (K26)
# ---------------------------------------------------------------------------
def _h36m_cfg(nrays, body_ratio, face_ratio):
    n = cfg_get("N_rand", 1024) if nrays is None else nrays
    body = cfg_get("body_sample_ratio", 0.5) if body_ratio is None else body_ratio
    face = cfg_get("face_sample_ratio", 0.0) if face_ratio is None else face_ratio
    return int(n), float(body), float(face)


def check_h36m_limits(H, W, split, nrays, body_ratio, face_ratio):
    """the limits of th_ray_sample_train / th_ray_sample_test, as ValueError"""
    if split not in ("train", "test"):
        raise ValueError(f'split is {split!r}: "train" or "test"')
    if not (1 <= H <= MAX_DIM and 1 <= W <= MAX_DIM):
        raise ValueError(f"image size {H} x {W}: 1 <= H, W <= {MAX_DIM}")
    if split == "train":
        if H < 2 or W < 2:
            raise ValueError(f"image size {H} x {W}: the train split needs H, W >= 2 (an empty body class samples pixel (1,1))")
        if not 1 <= nrays <= MAX_RAYS:
            raise ValueError(f"nrays = {nrays}: 1 <= nrays <= {MAX_RAYS}")
        if not (body_ratio >= 0.0 and face_ratio >= 0.0 and body_ratio + face_ratio <= 1.0):
            raise ValueError(f"body_ratio = {body_ratio}, face_ratio = {face_ratio}: both >= 0 and their sum <= 1")


def _check_h36m_draws(d, nrays):
    d = np.asarray(d, np.float64)
    if d.shape != (MAX_ITERS, 3, nrays):
        raise ValueError(f"draws has shape {d.shape}: [{MAX_ITERS},3,nrays] for nrays = {nrays}")
    if not ((d >= 0.0) & (d < 1.0)).all():
        raise ValueError("draws must lie in [0, 1)")
    return d


def _loop_error(status, n, nrays, iters):
    """the ValueError of a train loop that did not end, from the status bits of th_ray_sample_train's info (None: it ended)"""
    if status & STATUS_NEGATIVE_COUNT:
        return ValueError("a class count came out negative (body_ratio + face_ratio rounds above 1): np.random.randint raises")
    if status & STATUS_ADDED_NOTHING:
        return ValueError(f"iteration {iters} of the sampling loop added nothing ({n} of {nrays} rays): the reference never ends "
                          "here")
    if status & STATUS_UNFINISHED:
        return ValueError(f"the sampling loop is unfinished after MAX_ITERS = {MAX_ITERS} iterations ({n} of {nrays} rays)")
    return None


def get_acc_oracle(coord, msk):
    """get_acc (:635-641) on the host: uint8 [n], 1 where any pixel of ``msk`` [H,W] is nonzero in the 25 x 25 window centred on
    coord[i] = (row, col) and clipped to the image -- cv2.dilate with a 25 x 25 kernel of ones (centre anchor, default border: the
    outside never wins a maximum), read at the coordinates."""
    msk, coord = _np(msk), _np(coord).astype(np.int64).reshape(-1, 2)
    H, W = msk.shape
    if coord.size and not ((coord >= 0).all() and (coord[:, 0] < H).all() and (coord[:, 1] < W).all()):
        raise ValueError(f"coord must lie inside the {H} x {W} image")
    table = np.zeros((H + 1, W + 1), np.int64)                                      # summed-area table of msk != 0
    table[1:, 1:] = np.cumsum(np.cumsum(msk != 0, axis=0, dtype=np.int64), axis=1)
    half = ACC_BORDER // 2
    y0, y1 = np.maximum(coord[:, 0] - half, 0), np.minimum(coord[:, 0] + half, H - 1) + 1
    x0, x1 = np.maximum(coord[:, 1] - half, 0), np.minimum(coord[:, 1] + half, W - 1) + 1
    return ((table[y1, x1] - table[y0, x1] - table[y1, x0] + table[y0, x0]) != 0).astype(np.uint8)


def sample_rays_h36m_oracle(img, msk, bound_mask, dense_rays, split, nrays=None, draws=None, body_ratio=None, face_ratio=None):
    """The definition on the host.  img float32 [H,W,3]; msk, bound_mask uint8 [H,W]; dense_rays {ray_o, ray_d [H*W,3], near, far
    [H*W], mask_at_box [H*W]}; split "train" (``draws`` float64 [MAX_ITERS,3,nrays]) or "test".  Returns numpy arrays with the
    reference's dtypes: rgb, ray_o, ray_d [n,3], near, far [n] float32, coord int64 [n,2], mask_at_box bool ([H*W] test, [n] train),
    acc uint8 [n]; the train split adds iters (the iterations used)."""
    img, msk, bound = _np(img, np.float32), _np(msk), _np(bound_mask)
    if msk.dtype != np.uint8 or bound.dtype != np.uint8:
        raise TypeError(f"msk and bound_mask must be uint8, not {msk.dtype} / {bound.dtype}")
    H, W = msk.shape
    nrays, body_ratio, face_ratio = _h36m_cfg(nrays, body_ratio, face_ratio)
    check_h36m_limits(H, W, split, nrays, body_ratio, face_ratio)
    if img.shape != (H, W, 3) or bound.shape != (H, W):
        raise ValueError(f"img {img.shape} / bound_mask {bound.shape}: [H,W,3] / [H,W] for a {H} x {W} msk")
    ray_mask = _np(dense_rays["mask_at_box"]).reshape(-1) != 0
    ray_o, ray_d = (_np(dense_rays[k], np.float32).reshape(-1, 3) for k in ("ray_o", "ray_d"))
    near, far = (_np(dense_rays[k], np.float32).reshape(-1) for k in ("near", "far"))
    if not (ray_mask.size == H * W and ray_o.shape[0] == H * W and ray_d.shape[0] == H * W and near.size == H * W and far.size == H * W):
        raise ValueError(f"dense_rays must hold one row per pixel of the {H} x {W} image")
    flat = img.reshape(-1, 3)
    if split == "test":                                                             # :600-612
        pix = np.flatnonzero(ray_mask)
        coord = np.zeros((pix.size, 2), np.int64)
        return dict(rgb=flat[pix], ray_o=ray_o[pix], ray_d=ray_d[pix], near=near[pix], far=far[pix], coord=coord,
                    mask_at_box=ray_mask, acc=get_acc_oracle(coord, msk))
    draws = _check_h36m_draws(_np(draws), nrays)
    m = msk * bound                                                                 # :527 (uint8 product)
    classes = [np.flatnonzero(c.reshape(-1)) for c in (m == 1, m == 13, (bound == 1) & (m != 100))]    # :551, :560, :530 + :566
    fallback = (np.array([W + 1]), np.zeros(0, np.int64), np.array([0]))            # (1,1) :557, nothing :572-575, (0,0) :570
    pix, n, iters = [], 0, 0
    while n < nrays:                                                                # :545
        if iters == MAX_ITERS:
            raise _loop_error(STATUS_UNFINISHED, n, nrays, iters)
        rem = nrays - n
        n_body, n_face = int(rem * body_ratio), int(rem * face_ratio)               # :546-547
        counts = (n_body, n_face, rem - n_body - n_face)                            # :548
        if min(counts) < 0:
            raise _loop_error(STATUS_NEGATIVE_COUNT, n, nrays, iters)
        cand = []
        for c, (members, k) in enumerate(zip(classes, counts)):
            if members.size == 0:
                cand.append(fallback[c])
                continue
            size = np.float64(members.size)
            picks = np.minimum(np.floor(draws[iters, c, :k] * size).astype(np.int64), members.size - 1)
            cand.append(members[picks])
        cand = np.concatenate(cand).astype(np.int64)                                # :573 (body, face, rand)
        hit = cand[ray_mask[cand]]                                                  # :581-588
        iters += 1
        if hit.size == 0:
            raise _loop_error(STATUS_ADDED_NOTHING, n, nrays, iters)
        pix.append(hit)
        n += hit.size                                                               # :590
    pix = np.concatenate(pix)
    coord = np.stack([pix // W, pix % W], axis=1).astype(np.int64)
    return dict(rgb=flat[pix], ray_o=ray_o[pix], ray_d=ray_d[pix], near=near[pix], far=far[pix], coord=coord,
                mask_at_box=np.ones(n, np.bool_), acc=get_acc_oracle(coord, msk), iters=iters)


def sample_rays_h36m(img, msk, K, R, T, bounds, split, nrays=None, draws=None, body_ratio=None, face_ratio=None, generator=None):
    """sample_ray_h36m + get_acc for one target view, on the device.  The arguments of ``sample_patch_rays``; ``split`` is "train"
    or "test" (what the reference's dataset calls every split but 'train').  Train: ``draws`` float64 [MAX_ITERS,3,nrays] in [0, 1)
    (default: ``torch.rand(MAX_ITERS, 3, nrays, dtype=float64, generator=generator)`` on the host -- parity with numpy's own bit
    stream is unpinned, see the module docstring); nrays, body_ratio and face_ratio default to cfg.N_rand, cfg.body_sample_ratio
    and cfg.face_sample_ratio.

    Chains th_gen_rays, th_bound_mask (train) and th_ray_sample_train / th_ray_sample_test on the current stream, reads the 4-int
    ``info`` record to the host (the one wait of the call: the ray count, and for the train split the loop's status), then queues
    th_ray_acc.  Returns device tensors under the reference's keys: rgb, ray_o, ray_d [n,3], near, far [n], coord int64 [n,2],
    mask_at_box bool ([H*W] test, ones [n] train), acc uint8 [n].  ValueError for a train loop that adds nothing in an iteration
    or is unfinished after MAX_ITERS iterations (nothing is launched after that read), and for sizes outside the limits."""
    if msk.ndim != 2:
        raise ValueError(f"msk has shape {tuple(msk.shape)}: [H,W]")
    H, W = (int(n) for n in msk.shape)
    nrays, body_ratio, face_ratio = _h36m_cfg(nrays, body_ratio, face_ratio)
    check_h36m_limits(H, W, split, nrays, body_ratio, face_ratio)
    if tuple(img.shape) not in ((H, W, 3), (3, H, W)):
        raise ValueError(f"img has shape {tuple(img.shape)}: [H,W,3] or [3,H,W] for a {H} x {W} msk")
    dev = _device_of(img, msk)
    as_dev = lambda x, dt: (x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))).to(device=dev, dtype=dt)
    img, msk = as_dev(img, torch.float32), as_dev(msk, torch.uint8)
    Kh, Rh, Th, bh = (_np(a, np.float32) for a in (K, R, T, bounds))
    with torch.cuda.device(dev):
        dense = hip.gen_rays(Kh, Rh, Th, bh, H, W, device=dev, compact=False)
        if split == "test":
            raw = hip.ray_sample_test(dense, img, H, W)
            n = int(raw["info"][0])                                                 # (the one wait)
            acc = hip.ray_acc(torch.zeros((1, 2), dtype=torch.int64, device=dev), msk)      # (coord is all zeros: one value)
            out = {k: raw[k][:n] for k in ("rgb", "ray_o", "ray_d", "near", "far")}
            out.update(coord=torch.zeros((n, 2), dtype=torch.int64, device=dev), mask_at_box=dense["mask_at_box"],
                       acc=acc.expand(n).contiguous())
            return out
        if draws is None:
            draws = torch.rand(MAX_ITERS, 3, nrays, dtype=torch.float64, generator=generator)
        if not (torch.is_tensor(draws) and draws.is_cuda):
            draws = torch.from_numpy(_check_h36m_draws(_np(draws), nrays))
        elif tuple(draws.shape) != (MAX_ITERS, 3, nrays):
            raise ValueError(f"draws has shape {tuple(draws.shape)}: [{MAX_ITERS},3,nrays] for nrays = {nrays}")
        pose = np.concatenate([Rh.reshape(3, 3), Th.reshape(3, 1)], axis=1)                     # :524
        bound = hip.bound_2d_mask(bh.reshape(2, 3), Kh.reshape(3, 3), pose, H, W, device=dev)
        raw = hip.ray_sample_train(dense, msk, bound, img, as_dev(draws, torch.float64), nrays, body_ratio, face_ratio)
        n, iters, status, _ = (int(v) for v in raw["info"].cpu())                   # (the one wait)
        err = _loop_error(status, n, nrays, iters)
        if err is not None:
            raise err
        out = {k: raw[k][:n] for k in ("rgb", "ray_o", "ray_d", "near", "far", "coord")}
        out.update(mask_at_box=torch.ones(n, dtype=torch.bool, device=dev), acc=hip.ray_acc(out["coord"], msk))
    return out


def _target_view(batch):
    """-> (img, msk, K) of the batch's target view: the prepared view as it is, a raw frame through K16 / K25"""
    raw_keys = ("target_img_raw", "target_msk_raw", "target_K_raw", "target_D")
    has_raw = all(k in batch for k in raw_keys)
    has_prepared = all(k in batch for k in ("target_img", "target_msk", "target_K"))
    if not (has_raw or has_prepared) or any(k not in batch for k in ("target_R", "target_T", "can_bounds")):
        raise ValueError('cfg.target_prep = "device": the batch has no ray_o and lacks the target view (target_R, target_T, '
                         "can_bounds and target_img + target_msk + target_K, or target_img_raw + target_msk_raw + target_K_raw + "
                         "target_D)")
    if has_prepared:
        return batch["target_img"][0], batch["target_msk"][0], batch["target_K"][0]
    from . import preprocess
    cihp = batch.get("target_msk_cihp_raw")
    m = preprocess.combine_masks(batch["target_msk_raw"][0], None if cihp is None else cihp[0], border=5)
    jitter = preprocess.batch_jitter(batch)
    frame = batch["target_img_raw"] if jitter is None else preprocess.color_jitter(batch["target_img_raw"], jitter)
    imgs, msks, Ks = preprocess.prepare_views(frame, m[None], batch["target_K_raw"], batch["target_D"],
                                              mask_bkgd=bool(cfg_get("mask_bkgd", True)))
    return imgs[0], msks[0], Ks[0]


def add_targets(batch, split=None):
    """cfg.target_prep == "device" (Renderer.render's training entry): the reference's target keys, made here and ADDED TO
    ``batch`` with the collated leading 1 -- the one place this package mutates a batch, because the unchanged trainer reads
    ``patch_masks`` / ``target_patches`` / ``patch_div_indices`` from it after ``render`` returns.  A key that is present is
    never overwritten, and a batch that carries ``ray_o`` is left as it is.

    cfg.target_sampler: "patch" (default) makes the patch targets only, ``split`` is not read.  "dataset" makes what the
    reference's dataset makes for the call's split (can_smpl.py:507-535; ``split`` None: "train" with gradients enabled, else
    "test"): the patch targets for a training call with cfg.patch.use_patch_sampling, else ``sample_rays_h36m`` of that split --
    rgb, ray_o, ray_d, near, far, acc and mask_at_box (H36M_KEYS); the renderer's no-grad entries call this too, so that an
    evaluation loop fed target views needs no host dataset.  Optional ``ray_draws`` float64 [1,MAX_ITERS,3,cfg.N_rand].

    Reads ``target_R``, ``target_T`` [1,3,3] / [1,3,1], ``can_bounds`` [1,2,3] and either ``target_K`` [1,3,3] with the prepared view
    ``target_img`` float32 [1,H,W,3] + ``target_msk`` uint8 [1,H,W], or the raw frame ``target_img_raw`` uint8 [1,H0,W0,3],
    ``target_msk_raw`` [1,H0,W0], optional ``target_msk_cihp_raw``, ``target_K_raw`` [1,3,3], ``target_D`` [1,5], which goes through
    ``combine_masks(border=5)`` and ``prepare_views`` (can_smpl.py:118-158, :629-660; the scaled K is used in place of target_K);
    with cfg.input_jitter == "device" and ``jitter_seed`` in the batch the raw frame first gets the colour jitter of that seed, the
    parameter set the input views get (can_smpl.py:629-637; ``preprocess.batch_jitter``, K25).
    Optional ``patch_draws`` float64 [1,N,2]."""
    sampler = cfg_get("target_sampler", "patch")
    if sampler not in ("patch", "dataset"):
        raise ValueError(f'cfg.target_sampler is {sampler!r}: "patch" or "dataset"')
    patches = bool(cfg_get("patch").use_patch_sampling)
    if sampler == "patch":
        if not patches:
            raise ValueError('cfg.target_prep = "device" makes the patch targets only: cfg.patch.use_patch_sampling is false '
                             '(cfg.target_sampler = "dataset" makes the others)')
    else:
        if split is None:
            split = "train" if torch.is_grad_enabled() else "test"
        if split not in ("train", "test"):
            raise ValueError(f'split is {split!r}: "train" or "test"')
        patches = patches and split == "train"                                      # can_smpl.py:507
    if "ray_o" in batch:
        return batch
    img, msk, K = _target_view(batch)
    view = (img, msk, K, batch["target_R"][0], batch["target_T"][0], batch["can_bounds"][0])
    if patches:
        draws = batch.get("patch_draws")
        out, keys = sample_patch_rays(*view, draws=None if draws is None else draws[0]), REFERENCE_KEYS
    else:
        draws = batch.get("ray_draws")
        out, keys = sample_rays_h36m(*view, split, draws=None if draws is None else draws[0]), H36M_KEYS
    for k in keys:
        if k not in batch:
            batch[k] = out[k][None]
    return batch
