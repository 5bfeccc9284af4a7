"""The two forms of the texel filling of the 8-wave fused MLP kernel (fill_tex, k_mlp_fused8_kernel.h).

Every form requests the listed texel rows by LDS-DMA.  STAGED: V = 3, one-pass tiles -- view 0's operand rows are blended while
the last 2 - 6 requests of every wave (rows of views 1 and 2) are still landing, the other views behind a second barrier; how many
requests stay in flight follows from the number of rows view 0 lists.  SINGLE-STAGE: everything else (V < 3, 2- / 4-pass tiles).
Both blend with the same instructions in the same order, so an image must not depend on which form a tile took; the 4-wave
kernel (rows through registers, untouched) is the outside reference at the bar of test_fused_kernel_8_waves_equals_4_waves
(5e-6: fp32 summation order of the dense layers).
Small frames (64 - 97 px, 32 samples) through render_fast; everything through the C ABI."""
import os

import pytest
import torch

from transhuman_amd import synth
from util import make_net, synth_assign, can64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip(gpu):
    from transhuman_amd import hip as H
    H.load_library()
    yield H
    H.set_fused_waves(8)
    os.environ.pop("TH_TEX_CAP", None)


@pytest.fixture(scope="module")
def renderer(gpu):
    from transhuman_amd.config import get_cfg
    from transhuman_amd.networks.renderer import if_clight_renderer
    cfg = get_cfg()
    cfg.N_samples, cfg.num_class = 32, 300
    return if_clight_renderer.Renderer(make_net(12).to(gpu), vertex_can=can64().numpy(), pc2voxel_ind=synth_assign(300))


def _image(r, b):
    o = r.render_fast(b, is_train=False)
    return torch.cat([o["rgb_map"][0], o["acc_map"][0][:, None], o["depth_map"][0][:, None]], dim=1).cpu(), dict(r.last_stats)


def _both_forms(hip, r, b):
    """the frame through the 8-wave and the 4-wave kernel"""
    out = {}
    try:
        for w in (8, 4):
            hip.set_fused_waves(w)
            out[w] = _image(r, b)
    finally:
        hip.set_fused_waves(8)
    (i8, s8), (i4, s4) = out[8], out[4]
    assert s8["valid_samples"] == s4["valid_samples"] > 500
    assert bool(torch.isfinite(i8).all()) and float(i8[:, 3].max()) > 0.05
    return i8, i4, s8


def tile_paths(hip, r, b, samples=32):
    """K5t's headers of the frame's masked sample list, read back: the share of 32-sample tiles that are staged (one pass) /
    multi-pass, the share of one-pass tiles with a view of more than 32 rows (lists spread unevenly over the views) and the
    fewest / most rows a view of a one-pass tile has (view 0's count decides how many requests stay in flight).
    NOT the renderer's own K5t buffer: the hull-masked sample list is rebuilt here in the frame's documented order and K5t is run on
    it a second time (th_pixel_texlist), so the shares describe that list's 32-sample tiles; callers tie it to the render by the
    sample count where the frame takes the masked branch."""
    gpu = b["ray_o"].device
    frame = r.prepare_frame(b)
    pts = hip.Points(b["ray_o"][0], b["ray_d"][0], b["near"][0], b["far"][0], n_samples=samples)
    mask, _ = hip.hull_mask(pts, b["tar_smpl_vertice"][0])
    rr, ss = torch.nonzero(mask, as_tuple=True)
    order = torch.argsort((rr // 16) * (samples * 16) + ss * 16 + (rr % 16))      # (the frame's order: depth-major in 16-ray groups)
    rr, ss = rr[order], ss[order]
    z = pts.near[rr] * pts.omt[ss] + pts.far[rr] * pts.t[ss]
    world = (pts.ray_o[rr] + pts.ray_d[rr] * z[:, None]).contiguous()
    t = hip.pixel_texlist(frame.map, world, frame.cams, frame.scale)
    torch.cuda.synchronize()
    lists = t["lists"].long()
    V, HW = frame.map.V, frame.map.H * frame.map.W
    npass, U = lists[:, 0, 0] >> 16, lists[:, 0, 0] & 0xffff
    view = lists[:, 0, 8:8 + 103] // HW
    live = torch.arange(103, device=gpu)[None, :] < U[:, None]
    per_view = torch.stack([((view == v) & live).sum(1) for v in range(V)], dim=1)      # [T, V] rows of pass 0
    one = npass == 1
    wide = (per_view > 32).any(1)
    T = float(lists.shape[0])
    return dict(tiles=int(T), samples=int(world.shape[0]), staged=float(one.sum()) / T if V == 3 else 0.0,
                multipass=float((~one).sum()) / T, staged_wide=float((one & wide).sum()) / T,
                min_rows=int(per_view[one].min()) if bool(one.any()) else 0, max_rows=int(per_view[one].max()) if bool(one.any()) else 0)


@pytest.mark.parametrize("V,H,W", [(3, 97, 83), (2, 81, 97), (1, 65, 91)])
def test_every_view_count_ragged_tiles(hip, gpu, renderer, V, H, W):
    """V = 3 (staged tiles) and V = 1 / 2 (single-stage only), odd sizes and the masked branch (focal 200: more than 2400 hit rays,
    a ragged last tile): 8 waves against 4 waves"""
    b = synth.batch_to(synth.make_batch(H, W, V, seed=3, all_rays=True, focal=200.0), gpu)
    i8, i4, st = _both_forms(hip, renderer, b)
    d = float((i8 - i4).abs().max())
    print(f"V={V} {H}x{W}x32: valid {st['valid_samples']} unmasked {st['unmasked']}  max |8w - 4w| = {d:.2e}")
    assert st["unmasked"] == 0 and st["valid_samples"] % 32 != 0
    assert d < 5e-6, d


@pytest.fixture(scope="module")
def cap_frame(hip, gpu, renderer):
    """one V = 3 frame, rendered with K5t's full row budget (8 and 4 waves)"""
    b = synth.batch_to(synth.make_batch(96, 96, 3, seed=2, all_rays=True), gpu)
    os.environ.pop("TH_TEX_CAP", None)
    i8, i4, st = _both_forms(hip, renderer, b)
    return b, i8, i4, st, tile_paths(hip, renderer, b)


@pytest.mark.parametrize("cap", [8, 24, 56])
def test_row_budget_does_not_change_the_image(hip, gpu, renderer, cap_frame, cap):
    """TH_TEX_CAP = 8 / 24 / 56 sends (nearly) all / nearly all / most of the tiles down the 4- and 2-pass forms, which stay
    single-stage; with the full budget 99 % of this frame's tiles are staged.  The blend of a row is the same instructions in
    every form, so the 8-wave image is IDENTICAL to the one with the full budget -- it is identical across the caps on the
    parent commit's kernel as well (checked there with this test) -- and stays within 5e-6 of the 4-wave kernel's."""
    # `capped` comes from tile_paths' own K5t launch under the same TH_TEX_CAP, not from the launch inside render_fast: K5t reads the
    # variable at every launch (th_pixtex_launch), which is why the render sees the cap as well.  If that launch is ever replayed
    # from a captured graph the cap would no longer reach it and this test would compare the full-budget image with itself.
    b, ref8, ref4, st, paths = cap_frame
    assert paths["staged"] > 0.5, paths                    # (with the full budget most tiles of this frame are staged)
    os.environ["TH_TEX_CAP"] = str(cap)
    try:
        i8, s8 = _image(renderer, b)
        capped = tile_paths(hip, renderer, b)
    finally:
        os.environ.pop("TH_TEX_CAP", None)
    print(f"cap {cap}: {capped}  (full budget: {paths})")
    assert s8["valid_samples"] == st["valid_samples"]
    assert capped["multipass"] > 0.5, capped
    assert torch.equal(i8, ref8), float((i8 - ref8).abs().max())
    assert float((i8 - ref4).abs().max()) < 5e-6


def test_long_lists_take_both_forms(hip, gpu, renderer):
    """A long lens spreads the samples' footprints over the reference views: long, uneven lists (a view with 2 rows next to one
    with 66: every length of the in-flight tail, none included) next to tiles whose rows exceed a pass and take the 2- / 4-pass
    single-stage form, in ONE frame.  The shares are read back from K5t's headers; each form must serve at least a tenth of the
    tiles.  (The staged form as built has no fixed group a view could overflow -- the tail follows view 0's row count -- so the two
    forms of a frame are staged and multi-pass.)  Measured on an MI355X: LONG_LENS_SHARES below."""
    b = synth.batch_to(synth.make_batch(96, 96, 3, seed=2, all_rays=True, focal=LONG_LENS_FOCAL), gpu)
    paths = tile_paths(hip, renderer, b)
    print(f"focal {LONG_LENS_FOCAL}: {paths}")
    assert paths["staged"] >= 0.1 and paths["multipass"] >= 0.1 and paths["staged_wide"] >= 0.1, paths
    i8, i4, st = _both_forms(hip, renderer, b)
    assert st["unmasked"] == 0 and st["valid_samples"] == paths["samples"], (st, paths)
    d = float((i8 - i4).abs().max())
    print(f"max |8w - 4w| = {d:.2e}")
    assert d < 5e-6, d


LONG_LENS_FOCAL = 1400.0
LONG_LENS_SHARES = ("focal 1400 at 96 x 96 x 32: 8140 tiles (260 462 samples); staged 89.2 %, of which 72.2 % of all tiles have a view "
                    "with more than 32 rows; multi-pass 10.8 %; rows per view of a one-pass tile 2 .. 66")


def test_unmasked_branch(hip, gpu, renderer):
    """focal 40: few hit rays, every sample of a hit ray is shaded (the un-masked branch: samples outside the hull, whose footprints
    lie anywhere in the reference views)"""
    b = synth.batch_to(synth.make_batch(97, 97, 3, seed=3, all_rays=True, focal=40.0), gpu)
    i8, i4, st = _both_forms(hip, renderer, b)
    d = float((i8 - i4).abs().max())
    print(f"focal 40: valid {st['valid_samples']} unmasked {st['unmasked']}  max |8w - 4w| = {d:.2e}")
    assert st["unmasked"] != 0
    assert d < 5e-6, d


def test_sigma_grid_32(hip, gpu):
    """the sigma-only use of K6 (rgb_all = 2: the pixel branch's filling only, no RGB filling) on a 32^3 grid"""
    from transhuman_amd.config import get_cfg
    from transhuman_amd.networks.renderer import if_mesh_renderer
    cfg = get_cfg()
    cfg.N_samples, cfg.num_class = 32, 300
    bc = synth.make_batch(64, 64, 3, seed=0)
    bc["pts"] = synth.make_grid_pts(bc, 32)
    b = synth.batch_to(bc, gpu)
    r = if_mesh_renderer.Renderer(make_net(12).to(gpu), vertex_can=can64().numpy(), pc2voxel_ind=synth_assign(300))
    frame = r.prepare_frame(b)
    sl = torch.arange(32 ** 3, device=gpu)
    sig = {}
    try:
        for w in (8, 4):
            hip.set_fused_waves(w)
            sig[w] = r.render(b, frame=frame, pts_slice=sl)["sigma"].cpu()
    finally:
        hip.set_fused_waves(8)
    assert int((sig[8] != 0).sum()) > 300
    assert float((sig[8] - sig[4]).abs().max()) <= 2e-5 * max(1.0, float(sig[4].abs().max()))
