"""Time one training step (tools/train_step_time.py's step: 2 400 rays x 64 samples, V = 3 views of 512 x 512, N_c = 500) with every
training switch on its device value, under cfg.use_truncation off, at KNN_SIGMA = 0.25 (the reference's default) and at 0.1 --
one process, the forms in alternating order round by round -- and K27's own device time at P = 153 600.

    timeout -k 10 900 python tools/truncation_time.py [--steps 8] [--warmup 2] [--rounds 3] [--sigmas off,0.25,0.1]

Prints one JSON line.  Per form: the median of the rounds' median step times with the lowest and the highest round (host clock around
forward + backward with a device synchronisation at both ends), the share of the samples K27 keeps, and the largest difference of the
outputs from the form before it.  "k27": device events around 50 consecutive th_truncate_select / th_truncate_scatter /
th_truncate_scatter_bwd calls on the step's own samples, per call, median of 5 windows.  `--sigmas off` runs on a commit without K27
too: that run is the yardstick of the off form (same tool, same step).  No threshold on any figure."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import train_step_time as T                      # noqa: E402

ALL_DEVICE = dict(train_kernels="device", train_attention="device", train_vit_dense="device", train_maps="latents",
                  train_gather_bwd="ordered", train_point_net="device", train_encoder="device")


def step_samples(r, b):
    """pts_smpl [P,3] and the token centres of the step, as autograd_path.render forms them"""
    import torch
    from transhuman_amd.config import get_cfg
    from transhuman_amd.networks import autograd_path as ap
    ray_o, ray_d = b["ray_o"][0], b["ray_d"][0]
    z = ap.sample_depths(b["near"][0], b["far"][0], int(get_cfg().N_samples), False)
    xyz = (ray_o[:, None] + ray_d[:, None] * z[..., None]).reshape(-1, 3)
    pts_s = torch.matmul(xyz - b["Th"][0].reshape(1, 3), b["Rh"][0])
    M = ap.pooling_matrix_cached(r, b["input_smpl_vertice"][0][0].shape[0], ray_o.device, torch.float32)
    return pts_s.contiguous(), (M @ b["tar_smpl_vertice_smplcoord"][0]).contiguous()


def k27_times(pts_s, centres, sigma, calls=50, windows=5):
    import torch
    from transhuman_amd import hip
    mask, sel, n = hip.truncate_select(pts_s, centres, sigma)
    rows, g = torch.randn((n, 4), device=pts_s.device), torch.randn((pts_s.shape[0], 4), device=pts_s.device)
    lib, P, nc = hip.load_library(), pts_s.shape[0], centres.shape[0]
    ws = torch.empty(int(lib.th_truncate_select_workspace_bytes(P, nc)), dtype=torch.uint8, device=pts_s.device)
    cnt = torch.empty(1, dtype=torch.int32, device=pts_s.device)
    sel_all = torch.empty(P, dtype=torch.int32, device=pts_s.device)
    forms = {
        "select_us": lambda: hip._check(lib.th_truncate_select(hip.ctx(pts_s.device), hip._p(pts_s), P, hip._p(centres), nc, float(sigma),
                                                               hip._p(mask), hip._p(sel_all), hip._p(cnt), hip._p(ws), ws.numel(),
                                                               hip._stream())),
        "scatter_us": lambda: hip.truncate_scatter(rows, mask, sel),
        "scatter_bwd_us": lambda: hip.truncate_scatter_bwd(g, sel)}
    out = {"P": P, "n_centres": nc, "kept": n}
    forms["select_full_scan_us"] = forms["select_us"]                # (TH_DPARF_NOGRID=1: no grid build, all centres per sample)
    for name, fn in forms.items():
        os.environ.pop("TH_DPARF_NOGRID", None)
        if name == "select_full_scan_us":
            os.environ["TH_DPARF_NOGRID"] = "1"
        fn()
        per = []
        for _ in range(windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            per.append(e0.elapsed_time(e1) * 1e3 / calls)
        out[name] = round(float(np.median(per)), 2)
    os.environ.pop("TH_DPARF_NOGRID", None)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sigmas", default="off,0.25,0.1", help="comma list of KNN_SIGMA values, 'off' = cfg.use_truncation false")
    args = ap.parse_args()
    import torch
    from transhuman_amd import hip
    from transhuman_amd.config import override
    dev = torch.device("cuda:0")
    res = {"shape": {"rays": T.RAYS, "samples": T.SAMPLES, "views": T.VIEWS, "n_clusters": T.NC, "image": [T.SIZE, T.SIZE]},
           "device": torch.cuda.get_device_name(0), "switches": ALL_DEVICE}
    net, r, b = T.setup(dev)
    target = torch.rand((1, T.RAYS, 3), device=dev)
    forms = [(s, dict(use_truncation=False) if s == "off" else dict(use_truncation=True, KNN_SIGMA=float(s)))
             for s in args.sigmas.split(",")]
    rounds, outs = {}, {}
    with override(**ALL_DEVICE):
        for rnd in range(max(args.rounds, 1)):
            for key, keys in (forms if rnd % 2 == 0 else forms[::-1]):
                with override(**keys):
                    one, o, _ = T.run_mode(net, r, b, target, args.steps, args.warmup)
                rounds.setdefault(key, []).append(one)
                outs[key] = o
        have_k27 = hasattr(hip, "truncate_select")
        pts_s, centres = step_samples(r, b) if have_k27 else (None, None)
    prev = None
    for key, _ in forms:
        med = [x["step_ms_median"] for x in rounds[key]]
        res[key] = {"step_ms_median": round(float(np.median(med)), 2), "step_ms_lowest_round": min(med),
                    "step_ms_highest_round": max(med), "step_ms_min": min(x["step_ms_min"] for x in rounds[key]),
                    "rounds": len(med), "steps": args.steps, "peak_allocated_MiB": max(x["peak_allocated_MiB"] for x in rounds[key])}
        if key != "off" and have_k27:
            res[key]["kept_share"] = round(hip.truncate_select(pts_s, centres, float(key))[2] / pts_s.shape[0], 4)
        if prev is not None:
            res[key]["outputs_max_abs_vs_" + prev] = max(float((outs[key][k] - outs[prev][k]).abs().max()) for k in outs[key])
        prev = key
    if have_k27:
        res["k27"] = {s: k27_times(pts_s, centres, float(s)) for s, _ in forms if s != "off"}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
