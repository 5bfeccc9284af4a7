"""cfg.use_truncation: which samples keep their per-point network (cross_transformer.py:175-180, :247-264).

``truncation_mask_oracle`` is the numpy restatement of K27's test (transhuman_amd/csrc/k_truncate.hip), in fp32 and in K4's
operation order: d2 = (dx dx + dy dy) + dz dz with every product and sum rounded on its own, d = sqrt(min d2) correctly rounded,
kept = d < fp32(sigma).  The reference compares its float32 distances with the Python float ``cfg.KNN_SIGMA`` in float32 --
the scalar rounds to fp32 first (recorded from the reference in tests/golden/g27_truncation.npz, a sigma of 0.7 whose fp32 value
lies below its double value and a point at exactly that fp32 distance: dropped) -- so the device equals this at every sample.
"""
import numpy as np

from .config import get_cfg

F = np.float32


def nearest_d2_oracle(pts, centres, block=4096):
    """min over the centres of K4's fp32 squared distance; 3e38 where no distance compares below it (a NaN coordinate)"""
    p, c = np.ascontiguousarray(pts, F).reshape(-1, 3), np.ascontiguousarray(centres, F).reshape(-1, 3)
    out = np.empty(p.shape[0], F)
    for s in range(0, p.shape[0], block):
        d = p[s:s + block, None, :] - c[None]
        d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
        d2 = d2 + d[..., 2] * d[..., 2]
        with np.errstate(invalid="ignore"):
            out[s:s + block] = np.where(d2 < F(3.0e38), d2, F(3.0e38)).min(1)
    return out


def truncation_mask_oracle(pts, centres, sigma):
    """bool [P]: True where K27 keeps the sample"""
    with np.errstate(invalid="ignore"):
        return np.sqrt(nearest_d2_oracle(pts, centres)) < F(sigma)


def sigma_in_force(cfg=None):
    """cfg.KNN_SIGMA where cfg.use_truncation is set, else 0 (off): what the frame paths hand to hip.set_truncation"""
    cfg = cfg or get_cfg()
    return float(cfg.KNN_SIGMA) if getattr(cfg, "use_truncation", False) else 0.0
