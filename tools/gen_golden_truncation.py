"""Write tests/golden/g27_truncation.npz (and its g27_truncation_grads<i>.npz parts): the reference's own ``cfg.use_truncation`` (lib/networks/cross_transformer.py:175-180,
:247-264), recorded from the real reference imported with the stand-ins of oracle/ref_harness.py.

    python tools/gen_golden_truncation.py --reference <reference checkout>

Runs on the CPU, only where the reference checkout exists.  Four recordings:
  mask_*   ``get_human_representation``'s mask_preserve on dyadic points at distance sigma, one ulp below and one ulp above, for
           sigma in {0.25, 0.5, 0.7}.  fp32(0.7) lies below the double 0.7 and one point sits at exactly fp32(0.7): the reference
           DROPS it, so ``knn_dist_min < sigma`` compares in fp32 (the Python float rounds to fp32 first) -- asserted here, and
           what transhuman_amd.truncation.truncation_mask_oracle and K27 do.
  fwd_*    ``Network.forward`` under truncation on the inputs of g8_forward.npz, pts_mask in {None, random, all-false}, V in {1, 3}.
  step_*   the golden training step of tests/train_step_case.py (oracle/gen_golden_train.py) with use_truncation: outputs, loss and
           the same 20 gradients.
  frame_*  ``render_fast`` on the g11_render_small frame.
Every KNN_SIGMA but the mask recording's is moved until no sample's float64 distance to its nearest centre lies within 1e-4 of
it (asserted): a sample on the threshold flips a whole term whatever computes it.  The frame's 4015 hull-valid samples leave no
gap that wide (the widest is 1.86e-4); its KNN_SIGMA sits in the middle of that gap, 9.1e-5 from the nearer neighbour (asserted
at 9e-5, recorded as frame_margin)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F = np.float32
MARGIN = 1e-4
FRAME_MARGIN = 9e-5
PART_BYTES = 900_000           # uncompressed bytes per written file (each stays below 1 MiB)
SIGMA_BIAS = -1.7


def mask_case():
    """centres: the origin and seven far corners; points on the axes and on a 3-4-5 triangle, all dyadic"""
    cen = np.array([[0, 0, 0]] + [[8 * ((i >> 0) & 1), 8 * ((i >> 1) & 1), 8 * ((i >> 2) & 1)] for i in range(1, 8)], F)
    pts = []
    for s in (F(0.25), F(0.5), F(0.7)):
        lo, hi = np.nextafter(s, F(0)), np.nextafter(s, F(1))
        for d in (lo, s, hi):
            pts += [[d, 0, 0], [0, -d, 0], [0, 0, d]]
    for k in (0.25, 0.5, 1.0):                              # |p| = 5 k / 16 exactly: 0.078125, 0.15625, 0.3125
        pts += [[3 * k / 16, 4 * k / 16, 0], [0, -3 * k / 16, 4 * k / 16]]
    pts += [[8 + 0.25, 8, 8], [8, 8 - 0.5, 8], [4, 4, 4]]    # at sigma from another centre; far from all
    return np.array(pts, F), cen


def nearest64(pts, cen):
    d = np.asarray(pts, np.float64)[:, None, :] - np.asarray(cen, np.float64)[None]
    return np.sqrt((d * d).sum(-1).min(1))


def settle(sigma, dist64, what, margin=MARGIN):
    """the value nearest to ``sigma`` that no distance lies within ``margin`` of: ``sigma`` itself if it is one, else the middle of
    the nearest wide enough gap between neighbouring distances; between 10 % and 90 % of the samples lie on either side"""
    d = np.sort(dist64)
    n = len(d)
    ok = lambda s: np.abs(dist64 - s).min() > margin and 0.1 < (dist64 < s).mean() < 0.9
    if not ok(sigma):
        band = (np.arange(n - 1) + 1 > 0.1 * n) & (np.arange(n - 1) + 1 < 0.9 * n)
        width = d[1:] - d[:-1]
        gap = np.where((width > 2.0 * margin + 2e-6) & band)[0]
        assert len(gap), f"{what}: no KNN_SIGMA with a {margin} margin: {n} samples, widest gap {width[band].max():.3e}"
        mid = 0.5 * (d[gap] + d[gap + 1])
        sigma = float(mid[np.argmin(np.abs(mid - sigma))])
    assert ok(sigma)
    print(f"  {what}: KNN_SIGMA {sigma:.7f}, nearest sample {np.abs(dist64 - sigma).min():.2e} away, "
          f"kept {100.0 * (dist64 < sigma).mean():.1f} %")
    return float(sigma)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference checkout")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "g27_truncation.npz"))
    args = ap.parse_args()
    from oracle import ref_harness as rh
    from oracle.gen_golden_train import GRAD_KEYS
    from transhuman_amd import synth
    from transhuman_amd.truncation import truncation_mask_oracle
    rh.REF = args.reference
    torch.set_num_threads(8)
    mods = rh.load_reference(num_class=300, n_samples=32)
    cfg, CT = mods["cfg"], mods["cross_transformer"]
    gold = lambda n: np.load(os.path.join(ROOT, "tests", "golden", n + ".npz"))
    assign = gold("synth_assign")["assign_300"].astype(np.int64)
    body, _ = synth.make_body(0)
    can64 = body.astype(np.float64) * 1.02 + 0.001
    rec = {}

    feat_size = cfg.img_feat_size            # (Network() overwrites the key its encoder is sized from, cross_transformer.py:123)

    def ref_net(depth):
        cfg.vit_depth, cfg.img_feat_size = depth, feat_size
        torch.manual_seed(0)
        net = CT.Network()
        net.load_state_dict(synth.det_state_dict(net.state_dict(), seed=0, sigma_bias=SIGMA_BIAS))
        net.train()
        return net

    try:
        net = ref_net(12)
        cfg.use_truncation = True

        # ---- 1: the mask, and how the comparison rounds sigma ----
        pts, cen = mask_case()
        sigmas = np.array([0.25, 0.5, 0.7], np.float64)
        keep = []
        blend = torch.eye(4, dtype=torch.float64)[None].repeat(len(cen), 1, 1)
        tok = torch.zeros((1, len(cen), 192))
        for s in sigmas:
            cfg.KNN_SIGMA = float(s)
            with torch.no_grad():
                _, m = net.get_human_representation(torch.from_numpy(pts)[None], torch.from_numpy(cen)[None], blend[None], tok)
            keep.append(m.numpy())
        keep = np.stack(keep)
        for i, s in enumerate(sigmas):
            d32 = np.sqrt((pts.astype(F) ** 2).sum(1, dtype=F))[:9 * 3].reshape(3, 3, 3)[i]      # [below | at | above][axis]
            assert keep[i][9 * i:9 * i + 9].reshape(3, 3).tolist() == [[True] * 3, [False] * 3, [False] * 3], (s, keep[i])
            assert (d32[1] == F(s)).all()
        # fp32(0.7) < 0.7: a double comparison would keep the points at fp32(0.7); the reference drops them
        assert float(F(0.7)) < 0.7 and not keep[2][9 * 2 + 3:9 * 2 + 6].any(), "the reference compares in double: change the oracle"
        for i, s in enumerate(sigmas):
            assert np.array_equal(truncation_mask_oracle(pts, cen, s), keep[i]), s
        rec.update(mask_pts=pts, mask_centres=cen, mask_sigmas=sigmas, mask_keep=keep)
        print("  mask: the comparison runs in fp32; kept per sigma", keep.sum(1).tolist(), "of", len(pts))

        # ---- 2: Network.forward on g8's inputs ----
        g8, g7, tok = gold("g8_forward"), gold("g7_dparf"), torch.from_numpy(gold("g6_vit")["out"])
        pts8, centres, blend = torch.from_numpy(g8["pts_s"]), torch.from_numpy(g7["centres"]), torch.from_numpy(g7["blend"])
        vd, mask = torch.from_numpy(g8["viewdir"])[None], torch.from_numpy(g8["mask"])[None]
        pf = torch.from_numpy(synth.smooth_noise((3, 384, pts8.shape[0]), 23, passes=0))
        d8 = nearest64(pts8.numpy(), centres.numpy())
        cfg.KNN_SIGMA = settle(0.08, d8, "forward")
        share = float((d8 < cfg.KNN_SIGMA).mean())
        assert 0.1 < share < 0.9
        rec.update(fwd_sigma=np.float64(cfg.KNN_SIGMA), fwd_kept_share=np.float64(share))
        dd = lambda: {"pts_smplcoord": pts8[None], "obs_smpl_smplcoord": centres[None], "blend_mtx": blend[None]}
        with torch.no_grad():
            for tag, mk in (("none", None), ("rand", mask), ("zero", torch.zeros_like(mask))):
                rec["fwd_raw_" + tag] = net(pf, vd, dd(), holder=tok, face_idx=None, pts_mask=mk)[0].numpy()
            rec["fwd_raw_v1_rand"] = net(pf[:1], vd, dd(), holder=tok[:1], face_idx=None, pts_mask=mask)[0].numpy()
            rec["fwd_raw_v1_none"] = net(pf[:1], vd, dd(), holder=tok[:1], face_idx=None, pts_mask=None)[0].numpy()
        far = d8 >= cfg.KNN_SIGMA
        assert (rec["fwd_raw_none"][far] == 0).all() and (rec["fwd_raw_none"][~far, 3] != 0).all()
        assert (rec["fwd_raw_zero"] == 0).all()

        # ---- 4: render_fast on the g11_render_small frame ----
        cfg.N_samples = 32
        r = rh.make_ref_renderer(mods, net, can64, assign)
        bb = synth.make_batch(32, 32, 3, seed=0)
        cap, orig = {}, r._render

        def spy(batch, pts, z_vals, is_train=True, pts_mask=None):
            cap["mask"], cap["pts"] = pts_mask.clone(), pts.clone()
            cap["Rh"], cap["Th"] = batch["Rh"].clone(), batch["Th"].clone()
            return orig(batch, pts, z_vals, is_train=is_train, pts_mask=pts_mask)
        r._render = spy
        clone = lambda b: {k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.items()}
        cfg.use_truncation = False
        with torch.no_grad():
            r.render_fast(clone(bb), is_train=False)                         # (for the samples only)
        cfg.use_truncation = True
        valid = cap["mask"][0].numpy().reshape(-1)
        w = cap["pts"][0].reshape(-1, 3)
        smpl = torch.matmul(w - cap["Th"][0].reshape(1, 3), cap["Rh"][0]).numpy()[valid]
        cen_f = r.voxelization(r.dict_voxel2pc_ind, bb["tar_smpl_vertice_smplcoord"][0]).numpy()
        dv = nearest64(smpl, cen_f)
        # (4015 hull-valid samples: the widest gap between neighbouring distances that leaves 10 % .. 90 % on either side is 1.86e-4,
        # so no KNN_SIGMA keeps 1e-4 on this frame; FRAME_MARGIN is three orders above the fp32 rounding of a distance, < 1e-7)
        cfg.KNN_SIGMA = settle(0.05, dv, "frame", margin=FRAME_MARGIN)
        dropped = float((dv >= cfg.KNN_SIGMA).mean())
        assert 0.1 < dropped < 0.9, dropped
        with torch.no_grad():
            ret = r.render_fast(clone(bb), is_train=False)
        r._render = orig
        rec.update(frame_sigma=np.float64(cfg.KNN_SIGMA), frame_dropped_share=np.float64(dropped),
                   frame_valid=np.int64(valid.sum()), frame_margin=np.float64(np.abs(dv - cfg.KNN_SIGMA).min()), frame_rgb=ret["rgb_map"][0].numpy(), frame_acc=ret["acc_map"][0].numpy(),
                   frame_depth=ret["depth_map"][0].numpy())
        print(f"  frame: {int(valid.sum())} hull-valid samples, {100 * dropped:.1f} % dropped")

        # ---- 3: the golden training step under truncation ----
        cfg.N_samples, cfg.perturb, cfg.raw_noise_std = 16, 0.0, 0.0
        net = ref_net(2)
        r = rh.make_ref_renderer(mods, net, can64, assign)
        b = synth.make_batch(20, 20, 3, seed=0, all_rays=False, focal=62.5)
        R = b["ray_o"].shape[1]
        g18 = gold("g18_train_step")
        assert R == int(g18["rays"])
        pts_w, _ = r.get_sampling_points(b["ray_o"], b["ray_d"], b["near"], b["far"])
        smpl = torch.matmul(pts_w[0].reshape(-1, 3) - b["Th"][0].reshape(1, 3), b["Rh"][0]).numpy()
        cen_s = r.voxelization(r.dict_voxel2pc_ind, b["tar_smpl_vertice_smplcoord"][0]).numpy()
        ds = nearest64(smpl, cen_s)
        cfg.KNN_SIGMA = settle(0.1, ds, "step")
        target = torch.from_numpy(g18["target"])[None]
        ret = r.render(clone(b))
        loss = torch.mean((ret["rgb_map"] - target) ** 2) + 0.1 * ret["acc_map"].mean() + 0.01 * ret["depth_map"].mean()
        loss.backward()
        params = dict(net.named_parameters())
        rec.update(step_sigma=np.float64(cfg.KNN_SIGMA), step_kept_share=np.float64((ds < cfg.KNN_SIGMA).mean()),
                   step_kept=np.int64((ds < cfg.KNN_SIGMA).sum()), rays=np.int64(R), rgb=ret["rgb_map"][0].detach().numpy(),
                   acc=ret["acc_map"][0].detach().numpy(), depth=ret["depth_map"][0].detach().numpy(),
                   loss=np.float64(loss.item()), target=target[0].numpy())
        for k in GRAD_KEYS:
            g = params[k].grad
            assert g is not None and float(g.abs().max()) > 0.0, k
            rec["grad:" + k] = g.numpy()
        assert abs(float(loss) - float(g18["loss"])) > 1e-5, "truncation changed nothing"
        print("  step: loss", float(loss), "without truncation", float(g18["loss"]))
    finally:
        cfg.use_truncation = False
        os.chdir(mods["old_cwd"])
    # no committed file above 1 MiB: the gradients that do not fit beside the rest go to g27_truncation_grads<i>.npz, first fit in
    # descending size (tests/truncation_case.py reads the parts back as one recording)
    parts = [{k: v for k, v in rec.items() if not k.startswith("grad:")}]
    for k in sorted((k for k in rec if k.startswith("grad:")), key=lambda k: -rec[k].nbytes):
        fit = [p for p in parts if sum(v.nbytes for v in p.values()) + rec[k].nbytes <= PART_BYTES]
        if not fit:
            parts.append({})
            fit = parts[-1:]
        fit[0][k] = rec[k]
    for i, part in enumerate(parts):
        path = args.out if i == 0 else args.out[:-4] + f"_grads{i}.npz"
        np.savez_compressed(path, **part)
        assert os.path.getsize(path) < (1 << 20), path
        print(f"wrote {path} ({os.path.getsize(path)} bytes, {len(part)} arrays)")


if __name__ == "__main__":
    main()
