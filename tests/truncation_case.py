"""cfg.use_truncation (K27): the recording of the real reference (tests/golden/g27_truncation.npz and its gradient parts, made by
tools/gen_golden_truncation.py) and the point sets the select kernel is held to.

Shared by tests/test_truncation_host.py (CPU) and tests/test_gpu_truncation.py."""
import functools
import glob
import os

import numpy as np

from util import GOLD

F = np.float32


class Recording(dict):
    """the parts of the recording as one mapping with the ``files`` of an npz (train_step_case.check_step reads it so)"""

    @property
    def files(self):
        return list(self)


@functools.lru_cache(maxsize=None)
def golden():
    rec = Recording()
    for path in [os.path.join(GOLD, "g27_truncation.npz")] + sorted(glob.glob(os.path.join(GOLD, "g27_truncation_grads*.npz"))):
        d = np.load(path)
        rec.update({k: d[k] for k in d.files})
    return rec


def step_cfg():
    """the cfg keys of the recorded training step beyond train_step_case.STEP_CFG"""
    return dict(use_truncation=True, KNN_SIGMA=float(golden()["step_sigma"]))


def threshold_case(sigma):
    """dyadic centres and points at distance ``sigma`` (a dyadic fp32 value), one ulp below and one ulp above it, along each
    axis in both directions from the centre at the origin (the seven others are far corners): d^2 and its root are exact -> (pts, centres, expected keep)"""
    s = F(sigma)
    cen = np.array([[0, 0, 0]] + [[8 * (i & 1), 8 * ((i >> 1) & 1), 8 * ((i >> 2) & 1)] for i in range(1, 8)], F)
    pts, keep = [], []
    for d, k in ((np.nextafter(s, F(0)), True), (s, False), (np.nextafter(s, F(1)), False)):
        for a in range(3):
            for sign in (1, -1):
                p = np.zeros(3, F)
                p[a] = sign * d
                pts.append(p)
                keep.append(k)
    return np.array(pts, F), cen, np.array(keep)


def body_case(P, nc, seed=0):
    """``nc`` centres spread like a body, ``P`` points around them and a few far outside the box -> (pts, centres)"""
    rs = np.random.RandomState(1000 * seed + 7 * nc + P % 997)
    cen = (rs.normal(size=(nc, 3)) * np.array([0.18, 0.45, 0.10])).astype(F)
    pts = (cen[rs.randint(0, nc, size=P)] + rs.normal(0, 0.08, (P, 3))).astype(F)
    pts[::97] += F(3.0)
    return pts, cen
