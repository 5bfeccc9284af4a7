"""Write tests/golden/g28_dparf_params.npz (and its g28_dparf_params_part<i>.npz parts): the reference under DPaRF's own
hyper-parameters cfg.KNN, cfg.KNN_FREQ and cfg.KNN_DIST_ALPHA (lib/networks/cross_transformer.py:106, :154, :170), recorded from
the real reference imported with the stand-ins of oracle/ref_harness.py.

    python tools/gen_golden_dparf_params.py --reference <reference checkout>

Runs on the CPU, only where the reference checkout exists.  The triples (KNN, KNN_FREQ, KNN_DIST_ALPHA):
  A = (1, 1, 0.5)   B = (3, 6, 0.25)   C = (5, 10, 2.0)   D = (7, 4, 0.5)   E = (7, 10, 0.1)
Four recordings:
  rep_<t>    ``get_human_representation`` on the inputs of g7_dparf.npz, all five triples.  Asserted here, on the CPU:
             oracle.th_oracle.dparf with the same K, n_freq, alpha equals each recording to fp32 rounding -- the oracle's
             parametrisation is what the GPU tests lean on.
  fwd_<t>_*  ``Network.forward`` on the inputs of g8_forward.npz, pts_mask in {None, random}, V = 3 for all five triples and
             V = 1 for B; weights: synth.det_state_dict on a network built under the triple (fc_0 is 256 x (195 + 6 KNN_FREQ)).
  frame_<t>_* ``render_fast`` on the g11_render_small frame, B and D.
  step_B_*   the golden training step of tests/train_step_case.py (oracle/gen_golden_train.py) under B: outputs, loss and the same
             20 gradients as g18 / g27.
Also recorded (freq0_runs, freq0_note): what the reference does at KNN_FREQ = 0.  PositionalEncoding.forward
(vision_transformer.py:131-133) ends in view(n, -1) of an empty [n, 0, 3] tensor.  The torch releases the reference was written
for reject that ("cannot reshape tensor of 0 elements into shape [n, -1]"); torch 2.10, under which this recording was made,
infers 0 and the reference runs with the three raw offsets as its whole encoding.  The tool does not assert either outcome: it
writes down the one it saw, and transhuman_amd/dparf_params.py words its refusal of that value accordingly."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TRIPLES = {"A": (1, 1, 0.5), "B": (3, 6, 0.25), "C": (5, 10, 2.0), "D": (7, 4, 0.5), "E": (7, 10, 0.1)}
PART_BYTES = 900_000           # uncompressed bytes per written file (each stays below 1 MiB)
SIGMA_BIAS = -1.7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference checkout")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "g28_dparf_params.npz"))
    args = ap.parse_args()
    from oracle import ref_harness as rh
    from oracle import th_oracle as O
    from oracle.gen_golden_train import GRAD_KEYS
    from transhuman_amd import synth
    rh.REF = args.reference
    torch.set_num_threads(8)
    mods = rh.load_reference(num_class=300, n_samples=32)
    cfg, CT = mods["cfg"], mods["cross_transformer"]
    gold = lambda n: np.load(os.path.join(ROOT, "tests", "golden", n + ".npz"))
    assign = gold("synth_assign")["assign_300"].astype(np.int64)
    body, _ = synth.make_body(0)
    can64 = body.astype(np.float64) * 1.02 + 0.001
    rec = {"triples": np.array([TRIPLES[t] for t in "ABCDE"], np.float64)}
    feat_size = cfg.img_feat_size            # (Network() overwrites the key its encoder is sized from, cross_transformer.py:123)
    saved = {k: cfg[k] for k in ("KNN", "KNN_FREQ", "KNN_DIST_ALPHA", "N_samples", "perturb", "raw_noise_std", "vit_depth")}

    def under(t):
        cfg.KNN, cfg.KNN_FREQ, cfg.KNN_DIST_ALPHA = TRIPLES[t]

    def ref_net(depth):
        cfg.vit_depth, cfg.img_feat_size = depth, feat_size
        torch.manual_seed(0)
        net = CT.Network()
        net.load_state_dict(synth.det_state_dict(net.state_dict(), seed=0, sigma_bias=SIGMA_BIAS))
        net.train()
        return net

    clone = lambda b: {k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.items()}
    try:
        g8, g7, tok = gold("g8_forward"), gold("g7_dparf"), torch.from_numpy(gold("g6_vit")["out"])
        pts7, centres, blend = torch.from_numpy(g7["pts_s"]), torch.from_numpy(g7["centres"]), torch.from_numpy(g7["blend"])
        pts8 = torch.from_numpy(g8["pts_s"])
        vd, mask = torch.from_numpy(g8["viewdir"])[None], torch.from_numpy(g8["mask"])[None]
        pf = torch.from_numpy(synth.smooth_noise((3, 384, pts8.shape[0]), 23, passes=0))
        dd = lambda: {"pts_smplcoord": pts8[None], "obs_smpl_smplcoord": centres[None], "blend_mtx": blend[None]}

        # ---- the reference without an octave: written down, not asserted (see the module's text) ----
        cfg.KNN, cfg.KNN_FREQ, cfg.KNN_DIST_ALPHA = 7, 0, 0.5
        try:
            with torch.no_grad():
                rep0, _ = ref_net(12).get_human_representation(pts7[None], centres[None], blend[None], tok)
            note = f"torch {torch.__version__}: runs, rows of {rep0.shape[1]} channels"
            rec["freq0_runs"] = np.bool_(True)
        except Exception as e:                                     # noqa: BLE001 (whatever it raises is the finding)
            note = f"torch {torch.__version__}: {type(e).__name__}: {str(e).splitlines()[0][:160]}"
            rec["freq0_runs"] = np.bool_(False)
        print("  KNN_FREQ = 0, the reference:", note)
        rec["freq0_note"] = np.array(note)

        for t in "ABCDE":
            K, nf, alpha = TRIPLES[t]
            under(t)
            net = ref_net(12)
            assert tuple(net.fc_0.weight.shape[:2]) == (256, 195 + 6 * nf)
            # ---- 1: get_human_representation on g7's inputs, and the oracle's parametrisation ----
            with torch.no_grad():
                rep, _ = net.get_human_representation(pts7[None], centres[None], blend[None], tok)
            rec[f"rep_{t}"] = rep.numpy()                                                      # [V, 195 + 6 F, P]
            mine = O.dparf(pts7, centres, blend, tok, K=K, n_freq=nf, alpha=alpha).permute(1, 2, 0).numpy()
            err = float(np.abs(mine - rec[f"rep_{t}"]).max())
            scale = float(np.abs(rec[f"rep_{t}"]).max())
            print(f"  rep_{t}: K={K} F={nf} alpha={alpha}: oracle - reference max {err:.2e} (values up to {scale:.2f})")
            assert mine.shape == rec[f"rep_{t}"].shape and err <= 2e-6 * max(1.0, scale), (t, err)
            # ---- 2: Network.forward on g8's inputs ----
            with torch.no_grad():
                rec[f"fwd_{t}_none"] = net(pf, vd, dd(), holder=tok, face_idx=None, pts_mask=None)[0].numpy()
                rec[f"fwd_{t}_rand"] = net(pf, vd, dd(), holder=tok, face_idx=None, pts_mask=mask)[0].numpy()
                if t == "B":
                    rec["fwd_B_v1_none"] = net(pf[:1], vd, dd(), holder=tok[:1], face_idx=None, pts_mask=None)[0].numpy()
                    rec["fwd_B_v1_rand"] = net(pf[:1], vd, dd(), holder=tok[:1], face_idx=None, pts_mask=mask)[0].numpy()
            assert np.abs(rec[f"fwd_{t}_none"] - g8["raw_none"]).max() > 1e-3, "the triple changed nothing"
            # ---- 3: render_fast on the g11_render_small frame ----
            if t in "BD":
                cfg.N_samples = 32
                r = rh.make_ref_renderer(mods, net, can64, assign)
                with torch.no_grad():
                    ret = r.render_fast(clone(synth.make_batch(32, 32, 3, seed=0)), is_train=False)
                rec.update({f"frame_{t}_rgb": ret["rgb_map"][0].numpy(), f"frame_{t}_acc": ret["acc_map"][0].numpy(),
                            f"frame_{t}_depth": ret["depth_map"][0].numpy()})
                assert float(ret["acc_map"].max()) > 0.1

        # ---- 4: the golden training step under B ----
        under("B")
        cfg.N_samples, cfg.perturb, cfg.raw_noise_std = 16, 0.0, 0.0
        net = ref_net(2)
        r = rh.make_ref_renderer(mods, net, can64, assign)
        b = synth.make_batch(20, 20, 3, seed=0, all_rays=False, focal=62.5)
        g18 = gold("g18_train_step")
        assert b["ray_o"].shape[1] == int(g18["rays"])
        target = torch.from_numpy(g18["target"])[None]
        ret = r.render(clone(b))
        loss = torch.mean((ret["rgb_map"] - target) ** 2) + 0.1 * ret["acc_map"].mean() + 0.01 * ret["depth_map"].mean()
        loss.backward()
        params = dict(net.named_parameters())
        rec.update(step_B_rays=np.int64(b["ray_o"].shape[1]), step_B_rgb=ret["rgb_map"][0].detach().numpy(),
                   step_B_acc=ret["acc_map"][0].detach().numpy(), step_B_depth=ret["depth_map"][0].detach().numpy(),
                   step_B_loss=np.float64(loss.item()), step_B_target=target[0].numpy())
        for k in GRAD_KEYS:
            g = params[k].grad
            assert g is not None and float(g.abs().max()) > 0.0, k
            rec["step_B_grad:" + k] = g.numpy()
        assert abs(float(loss) - float(g18["loss"])) > 1e-5, "the triple changed nothing"
        print("  step B: loss", float(loss), "at the defaults", float(g18["loss"]))
    finally:
        for k, v in saved.items():
            cfg[k] = v
        cfg.img_feat_size = feat_size
        os.chdir(mods["old_cwd"])
    # no committed file above 1 MiB: first fit in descending size (tests/dparf_params_case.py reads the parts back as one recording)
    parts = [{}]
    for k in sorted(rec, key=lambda k: -np.asarray(rec[k]).nbytes):
        fit = [p for p in parts if sum(np.asarray(v).nbytes for v in p.values()) + np.asarray(rec[k]).nbytes <= PART_BYTES]
        if not fit:
            parts.append({})
            fit = parts[-1:]
        fit[0][k] = rec[k]
    for i, part in enumerate(parts):
        path = args.out if i == 0 else args.out[:-4] + f"_part{i}.npz"
        np.savez_compressed(path, **part)
        assert os.path.getsize(path) < (1 << 20), path
        print(f"wrote {path} ({os.path.getsize(path)} bytes, {len(part)} arrays)")


if __name__ == "__main__":
    main()
