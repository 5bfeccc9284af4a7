"""Time the encoder's part of a training step in both modes of cfg.train_maps on the same box in the same process, at the
reference's training shape: V = 3 input views of 512 x 512, 6 890 input vertices (painting), 2 400 rays x 64 samples =
153 600 points (pixel-aligned features).

    timeout -k 10 600 python tools/encoder_tail_time.py [--rounds 5] [--warmup 2] [--size 512]

One step = forward + backward of: trunk -> painting rows [V,6890,192] -> pixel rows [153600,V,384], with a seeded upstream
gradient on both row tensors standing in for the rest of the network.
  "full"     autograd_path.encode (upsample, concatenate, 1 x 1 reduction: the two full-size maps) + sample_map twice
  "latents"  autograd_path.latent_features (K19, train_ops.LatentGatherFn on the three latents) + the reduction on the rows
--encoder torch,device repeats every mode with cfg.train_encoder's "device" form of the trunk (K23: autograd_path.trunk_device, the
same forward, HIP backwards; keys gain '+encoder'); --encoder-fwd torch,device repeats the '+encoder' modes with cfg.train_encoder_fwd's
"device" form of the trunk's forward (K29: th_conv2d_fwd32, th_bn_act, th_maxpool3x3s2; keys gain '+fwd', and the "torch" value --
MIOpen's forward -- is the yardstick in the same process); --gather-bwd atomic,ordered repeats the "latents" modes with
cfg.train_gather_bwd's "ordered" form of K19's backward (k_latgather_ord.hip: no float atomic; keys gain '+ordered', before '+encoder'); --maps picks the
modes.  --rocprof DIR first runs a fresh child process under
`rocprofv3 --kernel-trace` (last --maps value, last --encoder value) and reports, per step, the number of kernel launches of the
stage and the device time of its ten slowest kernel names (DIR keeps the trace).
Prints one JSON line.  Per mode: the median of --rounds alternating rounds with the lowest and the highest (device events around
the step, no host synchronisation inside; one synchronisation after the closing event), torch.cuda.max_memory_allocated of a
step above what is allocated before it, and the largest difference of every encoder gradient between the modes.  The two
kernels' own time: device events around th_latent_gather / th_latent_gather_bwd (and, with --gather-bwd ordered, all the kernels of
th_latent_gather_bwd_ordered, with its workspace size and the peak allocation of a call) at the pixel shape, median of 20 calls.
No threshold on any figure."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RAYS, SAMPLES, VIEWS = 2400, 64, 3


def setup(dev, size):
    import torch
    from transhuman_amd import hip, synth
    from transhuman_amd.networks import autograd_path
    from transhuman_amd.networks.encoder import SpatialEncoder
    torch.manual_seed(0)
    enc = SpatialEncoder().to(dev).train()
    b = synth.make_batch(size, size, VIEWS, seed=0, all_rays=False)
    n = b["ray_o"].shape[1]
    pick = torch.from_numpy(np.sort(np.random.RandomState(0).choice(n, RAYS, replace=n < RAYS)))
    for k in ("ray_o", "ray_d", "near", "far"):
        b[k] = b[k][:, pick].contiguous()
    b = synth.batch_to(b, dev)
    z = autograd_path.sample_depths(b["near"][0], b["far"][0], SAMPLES, False)
    xyz = (b["ray_o"][0][:, None] + b["ray_d"][0][:, None] * z[..., None]).reshape(-1, 3).contiguous()
    images = b["input_imgs"][0].reshape(-1, *b["input_imgs"][0].shape[2:])
    R, T, K = (b[k][0].reshape(VIEWS, *sh) for k, sh in (("input_R", (3, 3)), ("input_T", (3, 1)), ("input_K", (3, 3))))
    verts = b["input_smpl_vertice"][0][0]
    gen = torch.Generator().manual_seed(1)
    g_paint = torch.randn((VIEWS, verts.shape[0], 192), generator=gen).to(dev)
    g_pix = torch.randn((xyz.shape[0], VIEWS, 384), generator=gen).to(dev)
    cams = hip.pack_cams(R, T, K)
    scale = hip.feat_scale(enc.feat_scale(size, size), (size, size), dev)
    return enc, images, verts, xyz, (R, T, K), cams, scale, g_paint, g_pix


def step(mode, enc, images, verts, xyz, rtk, cams, scale, g_paint, g_pix):
    from transhuman_amd.config import override
    parts = mode.split("+")
    maps, encoder, gather_bwd = parts[0], "device" if "encoder" in parts else "torch", "ordered" if "ordered" in parts else "atomic"
    enc.zero_grad(set_to_none=True)
    image_shape = images.shape[-2:]
    with override(train_encoder_fwd="device" if "fwd" in parts else "torch"):
        return _step(maps, encoder, gather_bwd, image_shape, enc, images, verts, xyz, rtk, cams, scale, g_paint, g_pix)


def _step(maps, encoder, gather_bwd, image_shape, enc, images, verts, xyz, rtk, cams, scale, g_paint, g_pix):
    from transhuman_amd.networks import autograd_path as A
    if maps == "latents":
        gather = A.latent_features(enc, images, cams, scale, encoder=encoder, gather_bwd=gather_bwd)
        painted, f = A._lin(enc.reduction_layer, gather(verts)).permute(1, 0, 2), gather(xyz)
    else:
        hol, pix = A.encode(enc, images, encoder=encoder)
        painted = A.sample_map(hol, A.project(verts, *rtk), enc, image_shape).permute(0, 2, 1)
        f = A.sample_map(pix, A.project(xyz, *rtk), enc, image_shape).permute(2, 0, 1)
    ((painted * g_paint).sum() + (f * g_pix).sum()).backward()


def kernel_times(enc, images, xyz, cams, scale, g_pix, reps=20, ordered=False):
    """device time of th_latent_gather and th_latent_gather_bwd on their own at the pixel shape; ordered: also of
    th_latent_gather_bwd_ordered (latents and lift), with its workspace and the peak allocation of one call"""
    import torch
    from transhuman_amd import hip
    with torch.no_grad():
        lat = [l.permute(0, 2, 3, 1).contiguous() for l in enc.trunk(images, fused_bn=False)]
        w, b = enc.upsample_color.weight.reshape(128, 3).contiguous(), enc.upsample_color.bias
        shapes = [tuple(l.shape) for l in lat]
        out = tuple(torch.empty_like(l) for l in lat)
        fwd = lambda: hip.latent_gather(*lat, w, b, images, xyz, cams, scale)
        bwd = lambda: hip.latent_gather_bwd(shapes, images.shape[2:], xyz, cams, scale, g_pix, out=out)
        res = {}
        calls = [("th_latent_gather", fwd), ("th_latent_gather_bwd (with its three clears)", bwd)]
        if ordered:
            rgb_s = fwd()[1]
            V, (H, W) = images.shape[0], images.shape[2:]
            ws = torch.empty(hip.load_library().th_latent_gather_bwd_ordered_ws(V, H, W, xyz.shape[0]), dtype=torch.uint8,
                             device=xyz.device)
            calls.append(("th_latent_gather_bwd_ordered (all its kernels, latents only)",
                          lambda: hip.latent_gather_bwd_ordered(shapes, (H, W), xyz, cams, scale, g_pix, out=out, workspace=ws)))
            calls.append(("th_latent_gather_bwd_ordered (all its kernels, latents and lift)",
                          lambda: hip.latent_gather_bwd_ordered(shapes, (H, W), xyz, cams, scale, g_pix, rgb_s=rgb_s, out=out,
                                                                workspace=ws)))
        for name, fn in calls:
            for _ in range(3):
                fn()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
            for a, e in ev:
                a.record()
                fn()
                e.record()
            torch.cuda.synchronize()
            ms = [a.elapsed_time(e) for a, e in ev]
            res[name] = {"ms_median": round(float(np.median(ms)), 4), "ms_min": round(float(np.min(ms)), 4),
                         "ms_max": round(float(np.max(ms)), 4), "calls": reps}
        if ordered:
            del ws
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            hip.latent_gather_bwd_ordered(shapes, (H, W), xyz, cams, scale, g_pix, rgb_s=rgb_s, out=out)
            torch.cuda.synchronize()
            res["th_latent_gather_bwd_ordered memory"] = {
                "workspace_MiB": round(hip.load_library().th_latent_gather_bwd_ordered_ws(V, H, W, xyz.shape[0]) / 2 ** 20, 2),
                "peak_allocated_MiB_of_a_call": round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 2)}
    return res


MARKER = "rank_sum_kernel"          # the gradient exchange's kernel (K28): no stage of a single-process step launches it


def traced_child(mode, size, steps):
    """the body of the child that --rocprof traces: `steps` steps of `mode`, each between two launches of the marker kernel"""
    import torch
    from transhuman_amd import hip
    dev = torch.device("cuda:0")
    a = setup(dev, size)
    mark = torch.zeros(4, device=dev)
    step(mode, *a)
    for _ in range(steps):
        hip.rank_sum(mark, 1, 4, mark)
        step(mode, *a)
    hip.rank_sum(mark, 1, 4, mark)
    torch.cuda.synchronize()


def trace_summary(out_dir):
    """launches per step and device time per kernel name between the marker launches of the child's kernel trace"""
    import csv
    import glob
    from collections import defaultdict
    rows = []
    for path in glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True):
        rows += [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(path))]
    rows.sort()
    marks = [i for i, r in enumerate(rows) if MARKER in r[2]]
    if len(marks) < 2:
        return {"error": f"{len(marks)} marker launches in the trace"}
    steps = len(marks) - 1
    agg = defaultdict(lambda: [0, 0])
    for i in range(marks[0], marks[-1]):
        if i not in marks:
            key = rows[i][2].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0][:70]
            agg[key][0] += 1
            agg[key][1] += rows[i][1] - rows[i][0]
    top = sorted(agg.items(), key=lambda kv: -kv[1][1])[:10]
    return {"steps": steps, "launches_per_step": round(sum(c for c, _ in agg.values()) / steps, 1),
            "kernel_us_per_step": round(sum(t for _, t in agg.values()) / 1e3 / steps, 1),
            "slowest": {k: {"calls_per_step": round(c / steps, 2), "us_per_step": round(t / 1e3 / steps, 1)} for k, (c, t) in top}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--maps", default="full,latents", help="comma list of cfg.train_maps values")
    ap.add_argument("--encoder", default="torch", help="comma list of cfg.train_encoder values (results of 'device' are keyed "
                                                       "'<maps>+encoder')")
    ap.add_argument("--encoder-fwd", default="torch", help="comma list of cfg.train_encoder_fwd values, for the '+encoder' modes "
                                                           "(results of 'device' are keyed '<maps>...+encoder+fwd')")
    ap.add_argument("--gather-bwd", default="atomic", help="comma list of cfg.train_gather_bwd values, for the 'latents' modes "
                                                           "(results of 'ordered' are keyed '<maps>+ordered')")
    ap.add_argument("--rocprof", default=None, metavar="DIR", help="also trace a short run of the last mode under rocprofv3 into DIR")
    ap.add_argument("--traced-child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    modes = tuple(m + ("" if g == "atomic" else "+ordered") + ("" if e == "torch" else "+encoder") + ("" if f == "torch" else "+fwd")
                  for m in args.maps.split(",") for g in (args.gather_bwd.split(",") if m == "latents" else ["atomic"])
                  for e in args.encoder.split(",") for f in (args.encoder_fwd.split(",") if e == "device" else ["torch"]))
    if args.traced_child:
        return traced_child(args.traced_child, args.size, 3)
    traced = None
    if args.rocprof:
        # (first, before this process opens the GPU; the traced program is a fresh child behind `--`)
        import subprocess
        os.makedirs(args.rocprof, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", args.rocprof, "-o", "encoder_tail", "--",
               sys.executable, os.path.abspath(__file__), "--traced-child", modes[-1], "--size", str(args.size)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        traced = dict(trace_summary(args.rocprof), mode=modes[-1]) if p.returncode == 0 else {"error": p.stderr[-400:]}
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("encoder_tail_time.py needs an MI355X: a time taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    enc, images, verts, xyz, rtk, cams, scale, g_paint, g_pix = setup(dev, args.size)
    a = (enc, images, verts, xyz, rtk, cams, scale, g_paint, g_pix)
    res = {"device": torch.cuda.get_device_name(0),
           "shape": {"views": VIEWS, "image": [args.size, args.size], "vertices": int(verts.shape[0]), "points": int(xyz.shape[0])}}
    if traced is not None:
        res["traced"] = traced
    grads = {}
    for m in modes:
        for _ in range(args.warmup):
            step(m, *a)
        grads[m] = {k: p.grad.detach().clone() for k, p in enc.named_parameters() if p.grad is not None}
    enc.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    ms, peak = {m: [] for m in modes}, {m: 0 for m in modes}
    for r in range(args.rounds):
        for m in (modes if r % 2 == 0 else modes[::-1]):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            step(m, *a)
            t1.record()
            torch.cuda.synchronize()
            ms[m].append(t0.elapsed_time(t1))
            peak[m] = max(peak[m], torch.cuda.max_memory_allocated() - base)
            enc.zero_grad(set_to_none=True)
    for m in modes:
        res[m] = {"step_ms_median": round(float(np.median(ms[m])), 2), "step_ms_min": round(float(np.min(ms[m])), 2),
                  "step_ms_max": round(float(np.max(ms[m])), 2), "rounds": args.rounds,
                  "peak_allocated_MiB": round(peak[m] / 2 ** 20, 1)}
    rel = lambda p, q: max(float((grads[p][k] - grads[q][k]).abs().max()) / max(float(grads[p][k].abs().max()), 1e-30)
                           for k in grads[p])
    if "full" in grads and "latents" in grads:
        assert set(grads["full"]) == set(grads["latents"])
        res["latents_vs_full"] = {"grads_max_rel_to_own_max": rel("full", "latents")}
    for m in modes:
        if m.endswith("+encoder") and m[:-8] in grads:
            assert set(grads[m]) == set(grads[m[:-8]])
            res[m + "_vs_torch_encoder"] = {"grads_max_rel_to_own_max": rel(m[:-8], m)}
    for m in modes:
        if m.endswith("+fwd") and m[:-4] in grads:
            assert set(grads[m]) == set(grads[m[:-4]])
            res[m + "_vs_torch_forward"] = {"grads_max_rel_to_own_max": rel(m[:-4], m)}
    for m in modes:
        q = m.replace("+ordered", "")
        if q != m and q in grads:
            assert set(grads[m]) == set(grads[q])
            res[m + "_vs_atomic"] = {"grads_max_rel_to_own_max": rel(q, m)}
    if any(m.startswith("latents") for m in modes):
        res["kernels"] = kernel_times(enc, images, xyz, cams, scale, g_pix, ordered=any("+ordered" in m for m in modes))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
