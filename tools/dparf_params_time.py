"""What cfg.KNN / cfg.KNN_FREQ cost on the frame path: K4's device time (TH_ROWS_NBR, the frame paths' default hand-over) on the
valid samples of the benchmark's "real" frame, and the whole frame through Renderer.render_sequence, under
(KNN, KNN_FREQ, KNN_DIST_ALPHA) = (7, 10, 0.5), (5, 10, 0.5), (3, 6, 0.25) and (1, 1, 0.5).

    python tools/dparf_params_time.py [--frames 20] [--rounds 5] [--out profiles/r16_dparf_params_time.json]

One MI355X, one process.  Every round runs the four settings one after the other (alternating, so drift of the clock or of the
card's temperature reaches all of them alike); per setting the median over the rounds is reported with the lowest and the
highest round beside it.  K4's time is the context's own event pair around its launches (hip.profile_read, phase "dparf"),
read in a pass of its own: the frame time is taken with the profiler off."""
import argparse
import itertools
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETTINGS = [(7, 10, 0.5), (5, 10, 0.5), (3, 6, 0.25), (1, 1, 0.5)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_dparf_params_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dparf_params_time.py needs an MI355X: no HIP device visible")
    import bench
    from transhuman_amd import config, hip, synth
    from transhuman_amd.networks.renderer.if_clight_renderer import Renderer
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    cfg = config.get_cfg()
    cfg.N_samples, cfg.num_class = 64, 500
    bc = synth.make_batch(args.res, args.res, 3, seed=0, all_rays=True)
    body = bc["tar_smpl_vertice_smplcoord"][0].numpy()
    assign = bench.load_assign(500, body)
    b = synth.batch_to(bc, dev)
    keys = lambda s: dict(KNN=s[0], KNN_FREQ=s[1], KNN_DIST_ALPHA=s[2])
    renderers = {}
    for s in SETTINGS:
        with config.override(KNN_FREQ=s[1], KNN_DIST_ALPHA=s[2]):        # (cfg.KNN is a per-call key: set in run())
            renderers[s] = Renderer(bench.build_net(dev), vertex_can=body.astype(np.float64) * 1.02 + 0.001, pc2voxel_ind=assign)

    def run(s, n, profile):
        """n frames of the pipeline under setting s -> (ms per frame, K4 ms per frame, valid samples)"""
        with config.override(**keys(s)):
            r = renderers[s]
            seq = r.render_sequence(itertools.repeat(b))
            for _ in range(args.warmup):
                next(seq)
            torch.cuda.synchronize()
            hip.profile_enable(profile)
            hip.profile_read()
            t0 = time.perf_counter()
            for _ in range(n):
                next(seq)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / n
            k4 = hip.profile_read()["dparf"][0] / n if profile else None
            hip.profile_enable(False)
            valid = int(r.last_stats["valid_samples"])
            seq.close()
        return ms, k4, valid

    rows = {s: dict(frame_ms=[], k4_ms=[], valid_samples=None) for s in SETTINGS}
    for s in SETTINGS:                                            # (uploads, graphs, workspaces: once, outside the rounds)
        run(s, 2, False)
    for _ in range(args.rounds):
        for s in SETTINGS:
            ms, _, valid = run(s, args.frames, False)
            _, k4, _ = run(s, args.frames, True)
            rows[s]["frame_ms"].append(ms)
            rows[s]["k4_ms"].append(k4)
            rows[s]["valid_samples"] = valid
    stat = lambda v: dict(median=float(np.median(v)), lowest=float(min(v)), highest=float(max(v)))
    out = dict(tool="tools/dparf_params_time.py", device=torch.cuda.get_device_name(0), res=args.res, samples=64, n_clusters=500,
               frames_per_round=args.frames, rounds=args.rounds,
               settings=[dict(KNN=s[0], KNN_FREQ=s[1], KNN_DIST_ALPHA=s[2], valid_samples=rows[s]["valid_samples"],
                              k4_nbr_ms_per_frame=stat(rows[s]["k4_ms"]), frame_ms=stat(rows[s]["frame_ms"])) for s in SETTINGS])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
