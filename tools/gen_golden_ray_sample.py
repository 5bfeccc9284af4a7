"""Write tests/golden/g26_ray_sample.npz: the outputs of the reference's own ``sample_ray_h36m``
(lib/utils/if_nerf/if_nerf_data_utils.py:516-614) for both splits on small target views, with ``np.random`` inside that module
replaced for the call by a stand-in that feeds recorded ``draws`` (the rule of transhuman_amd/train_targets.py:
``np.random.randint(0, n, k)`` of iteration i and class c returns min(floor(draws[i,c,:k] n), n - 1)) and ``get_bound_2d_mask``
replaced with ``oracle.th_oracle.bound_2d_mask`` (cv2 is absent; fillPoly parity stays unpinned).  ``get_acc`` is cv2.dilate and
cannot run here: the fixture holds no ``acc``.

    python tools/gen_golden_ray_sample.py --reference <reference checkout>

Runs on the CPU, only where the reference checkout exists.  The stand-in attributes a ``randint(0, n, k)`` call to its class by
``n`` (the non-empty classes of every case have pairwise different sizes; asserted) and to its iteration by counting the calls of
that class.  Stored per view: the camera, the box, the image, the bound mask, the reference's dense ray_o / ray_d / near / far /
mask (near / far scattered back to one value per pixel, 0 off the box, the layout th_gen_rays writes) and the test split's
outputs; per case: its view, msk, nrays, the two ratios, draws and the train split's outputs.  The generator asserts the
properties the cases were chosen for, and that every case ends within MAX_ITERS by the reference's own run."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ONE = 1.0 - 2.0 ** -53
MAX_ITERS = 4
BOX = np.array([[-0.35, -0.9, 2.6], [0.4, 0.85, 3.3]], np.float32)
BIG_BOX = np.array([[-2.0, -2.0, 2.6], [2.0, 2.0, 3.3]], np.float32)          # every pixel of the axis view hits it


def views():
    """name -> (H, W, K, R, T, bounds): the axis camera of oracle/gen_golden_rays.py at half its size, its oblique camera, and
    the axis camera with a box that covers the image"""
    from oracle.gen_golden_rays import cases as ray_cases
    (_, _, _, _, R1, T1, _), (_, H2, W2, K2, R2, T2, _) = ray_cases()
    K1 = np.array([[37.5, 0, 12.0], [0, 37.5, 16.0], [0, 0, 1]], np.float32)
    return {"axis": (32, 24, K1, R1, T1, BOX), "oblique": (H2, W2, K2, R2, T2, BOX), "inside": (32, 24, K1, R1, T1, BIG_BOX)}


def ellipse_mask(H, W, face=False):
    """1 inside the ellipse centred at (0.5 H, 0.45 W) with radii (0.33 H, 0.22 W), 100 on the ring up to 1.15, else 0; ``face``:
    13 on its rows above 0.3 H"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    r = np.sqrt(((y - 0.5 * H) / (0.33 * H)) ** 2 + ((x - 0.45 * W) / (0.22 * W)) ** 2)
    m = np.zeros((H, W), np.uint8)
    m[r <= 1.15] = 100
    m[r <= 1.0] = 1
    if face:
        m[(r <= 1.0) & (y < 0.3 * H)] = 13
    return m


def masks(name, H, W):
    if name == "ellipse":
        return ellipse_mask(H, W)
    if name == "face":
        return ellipse_mask(H, W, face=True)
    if name == "no_body":                                                     # border pixels only: body and face are empty
        m = ellipse_mask(H, W)
        m[m == 1] = 0
        return m
    assert name == "all_border"                                               # rand_set is empty
    return np.full((H, W), 100, np.uint8)


# name -> (view, mask, nrays, body_ratio, face_ratio, misses forced per iteration, iterations, final count - nrays)
CASES = {
    "one_iter": ("oblique", "ellipse", 64, 0.5, 0.0, [0], 1, 0),
    "two_iters": ("axis", "ellipse", 48, 0.5, 0.0, [3], 2, 0),
    "three_iters": ("axis", "ellipse", 40, 0.5, 0.0, [5, 2], 3, 0),
    "face": ("oblique", "face", 32, 0.5, 0.25, [0], 1, 0),
    "empty_body": ("inside", "no_body", 4, 0.5, 0.0, [0, 0], 2, 1),
    "empty_rand": ("inside", "all_border", 3, 0.5, 0.0, [0, 0], 2, 1),
    "nrays_1": ("oblique", "ellipse", 1, 0.5, 0.0, [0], 1, 0),
}


def classes_of(msk, bound):
    """the flat pixel indices of body / face / rand_set (:527-530, :551, :560, :566)"""
    m = msk * bound
    return [np.flatnonzero(c.reshape(-1)) for c in (m == 1, m == 13, (bound == 1) & (m != 100))]


def craft_draws(seed, classes, ray_mask, W, nrays, body_ratio, face_ratio, plan):
    """seeded draws [MAX_ITERS,3,nrays], re-aimed so that iteration i has exactly plan[i] picks (of the rand class) whose ray
    misses the box and every other pick hits; draws of exactly 0 and 1 - 2^-53 are put where the first / last member hits"""
    draws = np.random.RandomState(seed).uniform(size=(MAX_ITERS, 3, nrays))
    aim = lambda k, n: (k + 0.5) / n
    n, extremes = 0, []
    for i in range(MAX_ITERS):
        if n >= nrays:
            break
        rem = nrays - n
        n_body, n_face = int(rem * body_ratio), int(rem * face_ratio)
        counts = (n_body, n_face, rem - n_body - n_face)
        misses = plan[i] if i < len(plan) else 0
        added = 0
        for c, (members, k) in enumerate(zip(classes, counts)):
            if members.size == 0:
                added += int(ray_mask[W + 1]) if c == 0 else int(ray_mask[0]) if c == 2 else 0      # (1,1) / (0,0)
                continue
            hit = np.flatnonzero(ray_mask[members])
            miss = np.flatnonzero(~ray_mask[members])
            assert hit.size > 0
            for j in range(k):
                want_miss = c == 2 and j < misses
                if want_miss:
                    assert miss.size > 0, "no rand_set pixel whose ray misses the box"
                    draws[i, c, j] = aim(miss[j % miss.size], members.size)
                    continue
                if i == 0 and c in (0, 2) and j - (misses if c == 2 else 0) in (0, 1):
                    first = j - (misses if c == 2 else 0) == 0
                    if ray_mask[members[0 if first else -1]]:
                        draws[i, c, j] = 0.0 if first else ONE
                        extremes.append((c, first))
                pick = min(int(np.floor(draws[i, c, j] * np.float64(members.size))), members.size - 1)
                if not ray_mask[members[pick]]:
                    draws[i, c, j] = aim(hit[pick % hit.size], members.size)
                added += 1
            if c == 2:
                assert misses <= k
        n += added
    return draws, extremes


class _Draws:
    """stands in for numpy.random inside the reference module for one call"""

    def __init__(self, draws, sizes):
        self.draws, self.sizes, self.calls = draws, sizes, [0, 0, 0]

    def randint(self, lo, n, k):
        assert lo == 0 and n > 0 and self.sizes.count(n) == 1, (n, self.sizes)
        c = self.sizes.index(n)
        i = self.calls[c]
        self.calls[c] += 1
        assert i < MAX_ITERS, "the reference's loop runs past MAX_ITERS"
        return np.minimum(np.floor(self.draws[i, c, :k] * np.float64(n)).astype(np.int64), n - 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference checkout")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "g26_ray_sample.npz"))
    args = ap.parse_args()
    from oracle import ref_harness, th_oracle
    ref_harness.REF = args.reference
    mods = ref_harness.load_reference()
    from lib.utils.if_nerf import if_nerf_data_utils as du
    cfg = mods["cfg"]
    du.get_bound_2d_mask = th_oracle.bound_2d_mask
    real_random = du.np.random
    rec = {"names": np.array(list(CASES)), "views": np.array(list(views()))}
    seen = dict(extremes=set(), iters=set(), plus_one=0)

    def call(draws, sizes, *a):
        class _NP:                                                            # numpy, with the recorded draws as .random
            random = _Draws(draws, sizes)

            def __getattr__(self, k):
                return getattr(np, k)
        du.np = _NP()
        try:
            return du.sample_ray_h36m(*a), _NP.random.calls
        finally:
            du.np = np

    try:
        dense = {}
        for vname, (H, W, K, R, T, b) in views().items():
            img = (np.random.RandomState(H * 100 + W).randint(0, 256, size=(H, W, 3)) / 255.0).astype(np.float32)
            # the dense rays of the call, recomputed by the same functions (:522, :601-608)
            ray_o, ray_d = du.get_rays(H, W, K, R, T)
            ray_o, ray_d = ray_o.reshape(-1, 3).astype(np.float32), ray_d.reshape(-1, 3).astype(np.float32)
            near_c, far_c, ray_mask = du.get_near_far(b, ray_o, ray_d)            # mutates ray_d (:70)
            near, far = np.zeros(H * W, np.float32), np.zeros(H * W, np.float32)
            near[ray_mask], far[ray_mask] = near_c.astype(np.float32), far_c.astype(np.float32)
            bound = th_oracle.bound_2d_mask(b, K, np.concatenate([R, T], axis=1), H, W)
            assert bound.dtype == np.uint8 and set(np.unique(bound)) <= {0, 1}
            dense[vname] = (img, bound, ray_mask)
            (rgb, o, d, nr, fr, coord, mab), _ = call(None, [], img.copy(), ellipse_mask(H, W), K, R, T, b, 1024, "test")
            assert rgb.dtype == o.dtype == d.dtype == nr.dtype == fr.dtype == np.float32 and coord.dtype == np.int64
            assert mab.dtype == np.bool_ and np.array_equal(mab, ray_mask) and coord.shape == (len(rgb), 2) and not coord.any()
            print(vname, H, W, "rays in box", int(ray_mask.sum()), "bound", int(bound.sum()),
                  "bound pixels off the box", int(((bound.reshape(-1) == 1) & ~ray_mask).sum()))
            rec.update({f"view_{vname}_{k}": v for k, v in dict(
                HW=np.array([H, W]), K=K, R=R, T=T, bounds=b, img=img, bound_mask=bound, dense_ray_o=ray_o, dense_ray_d=ray_d,
                dense_near=near, dense_far=far, dense_mask=ray_mask, test_rgb=rgb, test_ray_o=o, test_ray_d=d, test_near=nr,
                test_far=fr, test_coord=coord, test_mask_at_box=mab).items()})
        for seed, (name, (vname, mname, nrays, body_ratio, face_ratio, plan, want_iters, extra)) in enumerate(CASES.items()):
            H, W, K, R, T, b = views()[vname]
            img, bound, ray_mask = dense[vname]
            msk = masks(mname, H, W)
            classes = classes_of(msk, bound)
            sizes = [int(c.size) for c in classes]
            live = [s for s in sizes if s > 0]
            assert len(set(live)) == len(live), (name, sizes)                  # n identifies the class
            draws, extremes = craft_draws(26 + seed, classes, ray_mask, W, nrays, body_ratio, face_ratio, plan)
            assert ((draws >= 0.0) & (draws < 1.0)).all()
            cfg.defrost()
            cfg.body_sample_ratio, cfg.face_sample_ratio = body_ratio, face_ratio
            (rgb, o, d, nr, fr, coord, mab), calls = call(draws, sizes, img.copy(), msk.copy(), K, R, T, b, nrays, "train")
            iters = max(calls) if any(calls) else len(rgb) // 2      # (no class: each iteration offers the two fallbacks)
            n = len(rgb)
            print(name, vname, mname, "nrays", nrays, "class sizes", sizes, "iterations", iters, "rays", n, "extremes", extremes)
            # the properties the cases were chosen for
            assert rgb.dtype == o.dtype == d.dtype == nr.dtype == fr.dtype == np.float32 and mab.dtype == np.bool_
            assert o.shape == d.shape == rgb.shape == (n, 3) and nr.shape == fr.shape == (n,) and coord.shape == (n, 2)
            assert mab.shape == (n,) and mab.all() and n >= nrays
            assert iters == want_iters <= MAX_ITERS and n == nrays + extra, (name, iters, n)
            # (two uint8 fallbacks concatenate to a uint8 coord: only then is the reference's coord not int64)
            assert coord.dtype == (np.uint8 if sizes[2] == 0 else np.int64), coord.dtype
            if mname == "no_body":
                assert sizes[0] == sizes[1] == 0 and sizes[2] > 0 and (coord == 1).all(1).any()
            if mname == "all_border":
                assert sizes == [0, 0, 0] and coord.tolist() == [[1, 1], [0, 0]] * 2
            if name == "face":
                assert sizes[1] > 0 and int(nrays * face_ratio) > 0 and (msk[coord[:, 0], coord[:, 1]] == 13).sum() >= 8
            seen["extremes"].update(extremes)
            seen["iters"].add(iters)
            seen["plus_one"] += int(extra == 1)
            rec.update({f"{name}_{k}": v for k, v in dict(
                view=np.array(vname), msk=msk, nrays=np.int64(nrays), body_ratio=np.float64(body_ratio),
                face_ratio=np.float64(face_ratio), draws=draws, iters=np.int64(iters), rgb=rgb, ray_o=o, ray_d=d, near=nr, far=fr,
                coord=coord.astype(np.int64), coord_dtype=np.array(coord.dtype.name), mask_at_box=mab).items()})
    finally:
        du.np = np
        assert du.np.random is real_random
        os.chdir(mods["old_cwd"])
    assert seen["iters"] >= {1, 2, 3} and seen["plus_one"] >= 1
    assert seen["extremes"] >= {(0, True), (0, False), (2, True), (2, False)}, seen["extremes"]    # draws of 0 and 1 - 2^-53
    np.savez_compressed(args.out, **rec)
    size = os.path.getsize(args.out)
    print(f"wrote {args.out} ({size} bytes)")
    assert size < 300 * 1024


if __name__ == "__main__":
    main()
