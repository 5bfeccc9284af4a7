"""cfg.KNN / cfg.KNN_FREQ / cfg.KNN_DIST_ALPHA: the recording of the real reference (tests/golden/g28_dparf_params.npz and its
parts, made by tools/gen_golden_dparf_params.py) and the networks built under its triples.

Shared by tests/test_dparf_params_host.py (CPU) and tests/test_gpu_dparf_params_frames.py."""
import functools
import glob
import os

import numpy as np
import torch

from transhuman_amd import config, synth
from util import GOLD, SIGMA_BIAS

TRIPLES = {"A": (1, 1, 0.5), "B": (3, 6, 0.25), "C": (5, 10, 2.0), "D": (7, 4, 0.5), "E": (7, 10, 0.1)}


class Recording(dict):
    """the parts of the recording as one mapping with the ``files`` of an npz (train_step_case.check_step reads it so)"""

    @property
    def files(self):
        return list(self)


@functools.lru_cache(maxsize=None)
def golden():
    rec = Recording()
    for path in [os.path.join(GOLD, "g28_dparf_params.npz")] + sorted(glob.glob(os.path.join(GOLD, "g28_dparf_params_part*.npz"))):
        d = np.load(path)
        rec.update({k: d[k] for k in d.files})
    assert np.array_equal(rec["triples"], np.array([TRIPLES[t] for t in "ABCDE"], np.float64))
    return rec


def step_recording(t="B"):
    """the recorded training step under triple ``t`` with the key names of g18_train_step.npz"""
    g, p = golden(), f"step_{t}_"
    return Recording({k[len(p):]: v for k, v in g.items() if k.startswith(p)})


def cfg_of(t):
    K, F_, alpha = TRIPLES[t]
    return dict(KNN=K, KNN_FREQ=F_, KNN_DIST_ALPHA=alpha)


def under(t, **more):
    """``with under("B"): ...`` -- the live cfg holds the triple (and ``more``) for the block"""
    return config.override(**cfg_of(t), **more)


def build_cfg(t):
    """what Network() is constructed under: the triple's octave count and temperature.  cfg.KNN is a per-call key (the
    constructor takes it at its default only, tests/test_dropin.py), so it is set around the calls, not the construction"""
    return dict(KNN_FREQ=TRIPLES[t][1], KNN_DIST_ALPHA=TRIPLES[t][2])


def make_net(t, depth=12):
    """Product Network built under triple ``t`` (CPU, train mode) with the deterministic weights of the recording"""
    from transhuman_amd.networks.cross_transformer import Network
    with config.override(vit_depth=depth, **build_cfg(t)):
        torch.manual_seed(0)
        net = Network()
        net.load_state_dict(synth.det_state_dict(net.state_dict(), seed=0, sigma_bias=SIGMA_BIAS))
        net.train()
    return net


def forward_inputs():
    """g8's inputs as the recording used them -> (pixel_feat [3,384,P], viewdir [P,27], pts [P,3], mask [P], centres, blend, tokens)"""
    g8, g7 = np.load(os.path.join(GOLD, "g8_forward.npz")), np.load(os.path.join(GOLD, "g7_dparf.npz"))
    tok = torch.from_numpy(np.load(os.path.join(GOLD, "g6_vit.npz"))["out"])
    pf = torch.from_numpy(synth.smooth_noise((3, 384, g8["pts_s"].shape[0]), 23, passes=0))
    return (pf, torch.from_numpy(g8["viewdir"]), torch.from_numpy(g8["pts_s"]), torch.from_numpy(g8["mask"]),
            torch.from_numpy(g7["centres"]), torch.from_numpy(g7["blend"]), tok)


# ---- the derived bounds of a K4 row (tests/test_gpu_dparf_params.py states the derivation) -------------------------------------
ULP, HALF = 2.0 ** -23, 2.0 ** -24


def row_bounds(pts, cen, rot, tok, K, F_, alpha):
    """pts [P,3], cen [N,3], rot [N,9] fp32 arrays, tok [V,N,192] tensor -> (tol_tok [P,V,192], tol_pe [P,3 + 6 F]) on the oracle's
    selection: the weights' relative bound on every term + K roundings of the fma chain; sum_k w_k * 5 * 2^-23 |a_k| + 2e-6"""
    from oracle import th_oracle as O
    d2, idx = O.knn_points_exact(torch.from_numpy(np.ascontiguousarray(pts)), torch.from_numpy(np.ascontiguousarray(cen)), K)
    d2, idx = d2.numpy(), idx.numpy()
    x = -np.sqrt(d2.astype(np.float64)) / float(np.float32(alpha))
    t = x - x.max(1, keepdims=True)
    e = np.exp(t)
    w = e / e.sum(1, keepdims=True)
    rho = HALF * (2 * np.abs(x) + 2 * np.abs(x).min(1, keepdims=True) + np.abs(t)) + ULP
    rel = (rho + rho.max(1, keepdims=True) + (K + 1) * HALF) * 1.001
    tmag = np.abs(tok.double().numpy()[:, idx])                                                  # [V,P,K,192]
    tol_tok = np.moveaxis((((rel + K * HALF) * w)[None, :, :, None] * tmag).sum(2), 0, 1)
    r = pts.astype(np.float64)[:, None, :] - cen.astype(np.float64)[idx]
    R = rot.astype(np.float64).reshape(-1, 3, 3)[idx]
    de = np.einsum("pkj,pkjc->pkc", r, R)
    f32pi, f32hpi = float(np.float32(np.pi)), float(np.float32(np.pi * 0.5))
    lit = [4 * ULP * np.abs(de)]
    for o in range(F_):
        for ph in (0.0, f32hpi):
            lit.append(5 * ULP * np.abs(de * (f32pi * 2.0 ** o) + ph))
    return tol_tok, (w[..., None] * np.concatenate(lit, -1)).sum(1) + 2e-6
