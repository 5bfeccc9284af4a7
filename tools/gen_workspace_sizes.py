"""Record what every pure-host size function of include/transhuman_hip.h answers -> tests/golden/workspace_sizes.json.

    python tools/gen_workspace_sizes.py [--lib PATH] [--out PATH]

Needs no GPU.  The file pins the sizes of the commit BEFORE the workspaces moved onto layout functions (LOG.md, "one layout
per workspace"): check that commit out, build it, run this script there and the committed file comes back byte for byte.
It is never regenerated from later code; tests/test_workspace_sizes.py compares the built library with it row by row.

Per function: the smallest shape it accepts, the headline frame (512 x 512 rays x 64 samples, V = 3, N_c = 500, 6890
vertices), a ragged shape (odd counts, no multiple of 64), the largest shape where that is a plain limit, and shapes it
refuses (0) where it refuses any.  th_shade_pool_bytes (needs a context) and th_sizeof (no workspace) are left out.
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

R, S, V, NC, NV, H, W = 512 * 512, 64, 3, 500, 6890, 512, 512
P = R * S
BIG = 1 << 24

ATTN = [(1, 1, 1), (V, NC, 3), (3, 333, 5), (2, 4096, 3), (65535, BIG, 1024), (0, 1, 1), (65536, 1, 1), (1, BIG + 1, 1), (1, 1, 1025)]
DENSE = [(1, 16, 16), (V * NC, 192, 192), (V * NC, 768, 192), (1237, 48, 80), (333, 192, 768), (BIG, 65536, 65536), (0, 16, 16),
         (BIG + 1, 16, 16), (5, 17, 16), (5, 16, 65552)]
MESH = [(0, 0), (1, 1), (NV, 13776), (6891, 13777), (100003, 200001), (-1, 1), (1, -1)]
IMG = [(1, 1), (H, W), (17, 19), (333, 77), (4096, 4096), (0, 5), (5, 0), (4097, 4), (4, 4097)]
LPIPS = [(1, 16, 16), (1, H, W), (2, 256, 256), (3, 33, 47), (1, 15, 16), (1, 16, 15), (0, 16, 16)]

SHAPES = {
    "th_linear_workspace_bytes": [(1, 1), (256, 384), (256, 255), (283, 129), (3, 128), (0, 0)],
    "th_hull_workspace_bytes": [(0,), (1,), (NV,), (6891,), (100003,)],
    "th_map_demand_bytes": [(1, 1, 64), (V, H, W), (3, 77, 192), (2, 333, 320), (0, 0, 0)],
    "th_paint_group_nhwc_workspace_bytes": [(1, 1, 384, 16), (V, NV, 256, 192), (V, NV, 260, 192), (V, NV, 384, 192), (2, 6891, 260, 48),
                                            (0, 0, 256, 0)],
    "th_conv_pack_bytes": [(64, 3, 7), (64, 64, 3), (128, 64, 3), (128, 128, 3), (128, 64, 1), (256, 128, 3), (256, 256, 3),
                           (256, 128, 1), (5, 5, 5), (0, 0, 0)],
    "th_bn_workspace_bytes": [(1, 1, 1), (V, 64, 256 * 256), (V, 128, 64 * 64), (3, 65, 333 * 7), (0, 0, 0)],
    "th_vit_workspace_bytes": [(1, 1, 64, 1), (V, NC, 192, 3), (3, 333, 192, 3), (1, 4096, 192, 3), (2, 50, 320, 5), (0, 0, 0, 0)],
    "th_attention_workspace_bytes": ATTN,
    "th_attention_train_workspace_bytes": ATTN,
    "th_attention_bwd_workspace_bytes": ATTN,
    "th_linear_train_workspace_bytes": [s + (f,) for f in (0, 1, 2) for s in DENSE] + [(5, 16, 16, 3), (5, 16, 16, -1), (8193, 16, 16, 1),
                                                                                        (8192, 16, 256, 1), (5, 16, 272, 1)],
    "th_linear_bwd_workspace_bytes": [s + (f,) for f in (0, 1, 2) for s in DENSE] + [(5, 16, 16, 3), (5, 16, 16, -1), (8193, 16, 16, 1),
                                                                                      (8192, 16, 256, 1), (5, 16, 272, 1)],
    "th_layernorm_bwd_workspace_bytes": [(1, 16), (V * NC, 192), (1237, 80), (BIG, 256), (0, 16), (BIG + 1, 16), (5, 17), (5, 272), (5, 0)],
    "th_linear_relu_workspace_bytes": DENSE,
    "th_linear_relu_bwd_workspace_bytes": DENSE,
    "th_pixel_texlist_bytes": [(1, 1), (V, 5 * 524288), (V, 524288), (3, 1237), (2, 33), (1, 0), (0, 0)],
    "th_network_workspace_bytes": [(1, 1), (V, 524288), (V, 32768), (3, 1237), (2, 33), (4, 600001), (1, 0), (1, -5)],
    "th_dparf_encode_bwd_workspace_bytes": [(1, 1, 7), (32768, V, NC), (524288, V, NC), (1237, 3, 333), (33, 2, 4096), (0, 3, 500),
                                            (5, 0, 500), (5, 3, 0)],
    "th_latent_gather_bwd_ordered_ws": [(1, 16, 16, 1), (V, H, W, 32768), (V, H, W, 524288), (3, 77, 95, 1237), (2, 333, 191, 33),
                                        (1, 16, 16, 0), (0, 16, 16, 5), (1, 0, 16, 5), (1, 16, 0, 5), (1, 16, 16, -1)],
    "th_marching_cubes_workspace_bytes": [(2, 2, 2), (256, 256, 256), (77, 33, 19), (171, 203, 95), (1, 1, 1), (0, 0, 0)],
    "th_mesh_components_workspace_bytes": MESH,
    "th_ssim_workspace_bytes": [(7, 7, 1), (H, W, 3), (33, 47, 3), (333, 77, 1), (6, 7, 3), (7, 6, 3), (7, 7, 0)],
    "th_lpips_pack_bytes": [()],
    "th_lpips_workspace_bytes": LPIPS,
    "th_lpips_bwd_pack_bytes": [()],
    "th_lpips_train_state_bytes": LPIPS,
    "th_lpips_bwd_workspace_bytes": LPIPS,
    "th_rasterize_workspace_bytes": [(1, 1, 1, 1, 1), (V, NV, 13776, H, W), (3, 6891, 13777, 333, 77), (2, 33, 50, 17, 19),
                                     (0, 1, 1, 1, 1), (1, 0, 1, 1, 1), (1, 1, 0, 1, 1), (1, 1, 1, 0, 1), (1, 1, 1, 1, 0)],
    "th_vertex_normals_workspace_bytes": MESH,
    "th_color_jitter_workspace_bytes": [(1, 1, 1), (V, 1002, 1000), (V, H, W), (3, 17, 19), (2, 333, 77), (0, 1, 1), (1, 0, 1), (1, 1, 0),
                                        (65535, 1, 1), (1, 16384, 16384), (65535, 16384, 16384), (65536, 1, 1), (1, 16385, 1),
                                        (1, 1, 16385)],
    "th_patch_workspace_bytes": IMG,
    "th_smpl_workspace_bytes": [(0,), (1,), (NV,), (6891,), (100003,)],
    "th_adam_table_bytes": [(1, 1), (300, 23_000_000), (37, 1_000_003), (1, 1 << 40), (0, 1), (1, 0), (-1, 5), (1 << 30, 1 << 50)],
    "th_bn_act_bwd_workspace_bytes": [(1, 1, 1), (V, 64, 256 * 256), (V, 128, 64 * 64), (3, 65, 333 * 7), (0, 1, 1), (1, 0, 1), (1, 1, 0),
                                      (1, 65535, 1), (1, 65535, 32767), (1, 1, (1 << 31) - 1), (1, 65536, 1), (1, 65535, 32769),
                                      (2, 1, 1 << 30)],
    "th_conv2d_dgrad_pack_bytes": [(3, 64, 7, 2), (64, 64, 3, 1), (64, 128, 3, 2), (128, 128, 3, 1), (64, 128, 1, 2), (128, 256, 3, 2),
                                   (256, 256, 3, 1), (128, 256, 1, 2), (5, 5, 5, 1), (64, 64, 3, 3)],
    "th_conv2d_wgrad_workspace_bytes": [(1, 64, 64, 3, 1, 1, 1), (V, 3, 64, 7, 2, H, W), (V, 64, 64, 3, 1, 128, 128), (V, 64, 128, 3, 2, 128, 128),
                                        (3, 64, 128, 1, 2, 33, 47), (2, 128, 256, 3, 2, 17, 19), (1, 5, 5, 5, 1, 8, 8), (0, 64, 64, 3, 1, 8, 8),
                                        (1, 64, 64, 3, 1, 0, 8), (16383, 64, 64, 3, 1, 8, 8), (16384, 64, 64, 3, 1, 8, 8),
                                        (1, 64, 64, 3, 1, 4096, 8191), (1, 64, 64, 3, 1, 4096, 8192), (16383, 64, 128, 3, 2, 45, 45)],
    "th_ray_sample_workspace_bytes": [s + (n,) for s in IMG for n in (0, 1024)] + [(H, W, 1), (333, 77, 1237), (H, W, -1), (H, W, 1 << 30),
                                                                                            (H, W, 65536), (4096, 4096, 65536),
                                                                                            (H, W, 65537)],
    "th_truncate_select_workspace_bytes": [(0, 1), (1, 1), (524288, NC), (32768, NC), (1237, 333), (33, 7), (5, 4096), (5, 4097), (-3, 0)],
}
# th_frame rows: (V, H, W, map_channels, n_verts, n_clusters) + the call's own counts
FRAMES = [(V, H, W, 256, NV, n) for n in (NC, 0, 7, 1500, 4096)] + [(1, 16, 16, 384, 1, 7), (3, 333, 77, 260, 6891, 333),
                                                                    (4, 64, 64, 256, 100, 4097)]
FRAME_SHAPES = {
    "th_render_workspace_bytes": [(1, 1), (R, S), (32 * 32, 32), (17 * 19, 33), (1237, 63), (0, 0)],
    "th_sigma_grid_workspace_bytes": [(1,), (256 * 256 * 64,), (32768,), (1237,), (17 * 19 * 33,), (0,)],
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(ROOT, "transhuman_amd", "libtranshuman_hip.so"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "workspace_sizes.json"))
    a = ap.parse_args()
    from transhuman_amd import cheader
    hdr = cheader.load()
    lib = C.CDLL(a.lib)
    sized = sorted(n for n, (res, _) in hdr.prototypes.items() if res is C.c_size_t and n not in ("th_sizeof", "th_shade_pool_bytes"))
    assert sized == sorted(list(SHAPES) + list(FRAME_SHAPES)), sorted(set(sized) ^ set(list(SHAPES) + list(FRAME_SHAPES)))
    for n in sized:
        getattr(lib, n).restype, getattr(lib, n).argtypes = hdr.prototypes[n]
    rows = []
    for name, shapes in SHAPES.items():
        for s in shapes:
            rows.append({"fn": name, "args": list(s), "bytes": int(getattr(lib, name)(*s))})
    ThFrame = hdr.structs["th_frame"]
    for name, shapes in FRAME_SHAPES.items():
        for fr in FRAMES:
            f = ThFrame()
            f.V, f.H, f.W, f.map_channels, f.n_verts, f.n_clusters = fr
            for s in shapes:
                rows.append({"fn": name, "frame": list(fr), "args": list(s), "bytes": int(getattr(lib, name)(C.byref(f), *s))})
    with open(a.out, "w") as fh:
        fh.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    print(f"{len(rows)} rows of {len(sized)} functions -> {a.out}")


if __name__ == "__main__":
    main()
