"""Write tests/golden/g22_patch_rays.npz: the outputs of the reference's own ``sample_ray_patch(..., 'train')``
(lib/utils/if_nerf/if_nerf_data_utils.py:445-499) on small target views, with its two random calls replaced for the call by
functions that consume recorded ``draws`` (the rule of transhuman_amd/train_targets.py: ``np.random.rand(1)[0]`` returns
draws[i,0]; ``np.random.choice(n)`` returns min(floor(draws[i,1] n), n - 1)) and ``get_bound_2d_mask`` replaced with
``oracle.th_oracle.bound_2d_mask`` (cv2 is absent; fillPoly parity stays unpinned).

    python tools/gen_golden_patch_rays.py --reference <reference checkout>

Runs on the CPU, only where the reference checkout exists.  Stored per case: the inputs, ``draws``, ``bound_mask``, the
reference's dense ray_o / ray_d / near / far / ray_mask (near / far scattered back to one value per pixel, 0 off the box, the
layout th_gen_rays writes) and every output.  The generator asserts the properties the cases were chosen for."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ONE = 1.0 - 2.0 ** -53
DRAWS = np.array([[0.9, 0.0], [0.9, ONE], [0.1, 0.0], [0.1, ONE], [0.5, 0.37], [0.5, 0.37]], np.float64)
SUBJECT_RATIO = 0.8
COUNTS = {"axis_p8": [16, 25, 48, 40, 48, 48], "axis_p5": [9, 9, 25, 15, 25, 25], "oblique_p8": [32, 64, 56, 64, 64, 64],
          "wide_p20": [140, 132, 304, 280, 400, 400]}


def ellipse_mask(H, W):
    """1 inside the ellipse centred at (0.5 H, 0.45 W) with radii (0.33 H, 0.22 W), 100 on the ring up to 1.15, else 0"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    r = np.sqrt(((y - 0.5 * H) / (0.33 * H)) ** 2 + ((x - 0.45 * W) / (0.22 * W)) ** 2)
    m = np.zeros((H, W), np.uint8)
    m[r <= 1.15] = 100
    m[r <= 1.0] = 1
    return m


def cases():
    """(name, H, W, P, K, R, T, bounds): the cameras and the box of oracle/gen_golden_rays.py, and one wider view"""
    from oracle.gen_golden_rays import cases as ray_cases
    (_, H1, W1, K1, R1, T1, b), (_, H2, W2, K2, R2, T2, _) = ray_cases()
    K3 = np.array([[120.0, 0, 40.0], [0, 120.0, 48.0], [0, 0, 1]], np.float32)
    return [("axis_p8", H1, W1, 8, K1, R1, T1, b), ("axis_p5", H1, W1, 5, K1, R1, T1, b),
            ("oblique_p8", H2, W2, 8, K2, R2, T2, b),
            ("wide_p20", 96, 80, 20, K3, np.eye(3, dtype=np.float32), np.zeros((3, 1), np.float32), b)]


class _Draws:
    """stands in for numpy.random inside the reference module for one call"""

    def __init__(self, draws):
        self.draws, self.i = draws, 0

    def rand(self, n):
        assert n == 1
        return np.array([self.draws[self.i, 0]])

    def choice(self, n, size=None, replace=True):
        assert list(size) == [1] and n > 0
        k = min(int(np.floor(self.draws[self.i, 1] * np.float64(n))), n - 1)
        self.i += 1
        return np.array([k])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference checkout")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "g22_patch_rays.npz"))
    args = ap.parse_args()
    from oracle import ref_harness, th_oracle
    ref_harness.REF = args.reference
    mods = ref_harness.load_reference()
    from lib.utils.if_nerf import if_nerf_data_utils as du
    cfg = mods["cfg"]
    du.get_bound_2d_mask = th_oracle.bound_2d_mask
    real_random = du.np.random
    rec = {"names": np.array([c[0] for c in cases()]), "draws": DRAWS, "subject_ratio": np.float64(SUBJECT_RATIO)}
    fully, empty = False, 0
    try:
        for name, H, W, P, K, R, T, b in cases():
            rs = np.random.RandomState(H * 100 + W)
            img = rs.uniform(size=(H, W, 3)).astype(np.float32)
            msk = ellipse_mask(H, W)
            cfg.defrost()
            cfg.patch.N_patches, cfg.patch.size, cfg.patch.sample_subject_ratio = len(DRAWS), P, SUBJECT_RATIO
            # the dense rays of the call, recomputed by the same functions (:450, :465-470)
            ray_o, ray_d = du.get_rays(H, W, K, R, T)
            ray_o, ray_d = ray_o.reshape(-1, 3).astype(np.float32), ray_d.reshape(-1, 3).copy()
            assert ray_d.dtype == np.float32
            near_c, far_c, ray_mask = du.get_near_far(b, ray_o, ray_d)                # mutates ray_d (:70)
            near, far = np.zeros(H * W, np.float32), np.zeros(H * W, np.float32)
            near[ray_mask], far[ray_mask] = near_c.astype(np.float32), far_c.astype(np.float32)
            bound = th_oracle.bound_2d_mask(b, K, np.concatenate([R, T], axis=1), H, W)

            class _NP:                                                                # numpy, with the recorded draws as .random
                random = _Draws(DRAWS)

                def __getattr__(self, k):
                    return getattr(np, k)
            du.np = _NP()
            try:
                rgb, o, d, nr, fr, meta = du.sample_ray_patch(img.copy(), msk.copy(), K, R, T, b, 1024, "train")
            finally:
                du.np = np
            div = np.asarray(meta["patch_div_indices"])
            counts = np.diff(div).tolist()
            print(name, H, W, "P", P, "rays in box", int(ray_mask.sum()), "per patch", counts)
            # the properties the cases were chosen for
            assert counts == COUNTS[name], (name, counts)
            assert rgb.dtype == o.dtype == d.dtype == nr.dtype == fr.dtype == np.float32
            assert meta["patch_masks"].dtype == np.bool_ and meta["sub_mask"].dtype == np.bool_ and div.dtype == np.int64
            assert any(0 < c < P * P for c in counts), "no window cut by the box"
            sub = meta["patch_masks_sub"].reshape(len(DRAWS), -1)
            rays = meta["patch_masks"].reshape(len(DRAWS), -1)
            # (a window inside the subject can still be cut by the box: "full" is every ray of the window on the subject)
            covers = (sub | ~rays).all(1) & rays.any(1)
            assert covers.any() and not covers.all(), "patch_masks_sub never covers its window's rays / always does"
            empty += int((~sub.any(1)).any())
            fully = fully or bool(sub.all(1).any())
            human = (msk * bound) > 0
            background = ray_mask.reshape(H, W) & ~human
            clipped = False
            for cand, u1, slot in ((background, 0.0, 0), (background, ONE, 1), (human, 0.0, 2), (human, ONE, 3)):
                ys, xs = np.where(cand)
                k = 0 if u1 == 0.0 else len(ys) - 1
                x0, y0 = np.clip(xs[k] - P // 2, 0, W - P), np.clip(ys[k] - P // 2, 0, H - P)
                assert np.array_equal(meta["target_patches"][slot], img[y0:y0 + P, x0:x0 + P]), (name, slot)
                clipped = clipped or x0 != xs[k] - P // 2 or y0 != ys[k] - P // 2
            if name == "oblique_p8":
                assert clipped, "no window clipped at the image border"
                assert ray_mask.reshape(H, W)[0].any() and ray_mask.reshape(H, W)[:, W - 1].any() and (H * W) % 256
            assert np.array_equal(meta["target_patches"][4], meta["target_patches"][5])
            rec.update({f"{name}_{k}": v for k, v in dict(
                HW=np.array([H, W]), P=np.int64(P), K=K, R=R, T=T, bounds=b, img=img, msk=msk, bound_mask=bound,
                dense_ray_o=ray_o, dense_ray_d=ray_d, dense_near=near, dense_far=far, dense_mask=ray_mask,
                rgb=rgb, ray_o=o, ray_d=d, near=nr, far=fr, sub_mask=meta["sub_mask"], patch_masks=meta["patch_masks"],
                patch_masks_sub=meta["patch_masks_sub"], target_patches=meta["target_patches"], patch_div_indices=div).items()})
    finally:
        du.np = np
        assert du.np.random is real_random
        os.chdir(mods["old_cwd"])
    assert empty >= 3, "fewer than three cases have a window without a subject pixel"
    assert fully, "no case has a window that lies on the subject with all its P x P pixels"
    np.savez_compressed(args.out, **rec)
    print(f"wrote {args.out} ({os.path.getsize(args.out)} bytes)")


if __name__ == "__main__":
    main()
