"""K1 (transhuman_amd/csrc/k_hull.hip) on the adversarial cases of hull_cases.py.

The reference of every result is oracle.th_oracle.hull_mask: exact brute force, (dx*dx + dy*dy) + dz*dz in fp32, correctly
rounded sqrt, < fp32 thresh.  The device equals it bit for bit on every sample of every case, in both forms of the kernel (the
wave-cooperative default and TH_HULL_SEQ=1): no tolerance, no allowed count of differing samples.  tests/test_hull_cases_host.py
proves on the CPU that the cases reach what they are named for: samples a few ulp either side of the threshold, the layer of
cells around the grid, cells of 1 .. 200 vertices around the sizes 8 (HULL_PROBE) and 64 (a wave step), grids whose cell the
extent rule enlarged, degenerate vertex sets, samples that are not finite.

Then: the result does not depend on what the workspace held, and the small-frame rule (R' <= small_frame_rays, :551) switches
exactly at its boundary -- count_hits_kernel counts the rays with a hit sample into info[0], cmp_rule_on reads
`info[0] <= thr`, as the header says (th_render_prepass_wait: "R' <= small_frame_rays"); under the rule every sample of a hit
ray is listed, without it the masked ones."""
import ctypes as C

import numpy as np
import pytest
import torch

import hull_cases as Hc

pytestmark = pytest.mark.gpu
FORMS = ("wave", "seq")


@pytest.fixture(scope="module")
def hip(gpu):
    from transhuman_amd import hip as H
    H.load_library()
    return H


def _form(monkeypatch, form):
    if form == "seq":
        monkeypatch.setenv("TH_HULL_SEQ", "1")
    else:
        monkeypatch.delenv("TH_HULL_SEQ", raising=False)


def _same(name, form, got, ref, verts, pts, thresh):
    """torch.equal, with a message that names the case and the first differing sample"""
    got, ref = got.reshape(-1).cpu(), torch.from_numpy(np.array(ref)).reshape(-1)
    assert got.dtype == torch.bool and got.shape == ref.shape
    if not torch.equal(got, ref):
        bad = torch.nonzero(got != ref).reshape(-1)
        i = int(bad[0])
        raise AssertionError(f"{name} ({form}): {bad.numel()} of {ref.numel()} samples differ; device {bool(got[i])}, reference "
                             f"{bool(ref[i])} at " + Hc.describe(verts, pts, thresh, i))


# ---- every case, both forms, against the reference -----------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", Hc.CASES)
def test_points_equal_the_reference(hip, gpu, monkeypatch, name, form):
    """explicit points; run twice: the order of the vertices inside a cell comes from atomics and must not matter"""
    c = Hc.case(name)
    ref = Hc.ref_of(name)
    _form(monkeypatch, form)
    pts, verts = torch.from_numpy(np.array(c.pts)).to(gpu), torch.from_numpy(np.array(c.verts)).to(gpu)
    m, hit = hip.hull_mask(hip.Points(pts=pts), verts, c.thresh)
    m2, hit2 = hip.hull_mask(hip.Points(pts=pts), verts, c.thresh)
    print(f"{name} ({form}): {c.pts.shape[0]} samples x {c.verts.shape[0]} vertices, hits {int(m.sum())} (reference {int(ref.sum())})")
    _same(name, form, m, ref, c.verts, c.pts, c.thresh)
    _same(name, form, hit, ref, c.verts, c.pts, c.thresh)                # (S = 1: the per-"ray" flag is the mask)
    assert torch.equal(m, m2) and torch.equal(hit, hit2), name


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", Hc.RAY_FORM)
def test_rays_equal_the_reference(hip, gpu, monkeypatch, name, form):
    """the ray form (samples placed by the kernel, for one set from explicit z_vals): the mask, and ray_hit = any sample of the ray"""
    c = Hc.ray_case(name)
    ref = Hc.ray_ref_of(name)
    _form(monkeypatch, form)
    z = Hc.ray_z(name)
    P = hip.Points(c.ray_o.to(gpu), c.ray_d.to(gpu), c.near.to(gpu), c.far.to(gpu), n_samples=c.S,
                   z_vals=None if z is None else z.to(gpu))
    m, hit = hip.hull_mask(P, torch.from_numpy(c.verts).to(gpu), c.thresh)
    assert m.shape == ref.shape
    print(f"{name} ({form}): hit rays {int(hit.sum())} (reference {int(ref.any(1).sum())}), valid samples {int(m.sum())}")
    _same(name, form, m, ref, c.verts, Hc.ray_pts(name).reshape(-1, 3).numpy(), c.thresh)
    assert torch.equal(hit.cpu(), torch.from_numpy(ref.any(1))), (name, form)


# ---- what the workspace held does not matter -------------------------------------------------------------------------------
def _abi_mask(hip, gpu, name, ws):
    c = Hc.case(name)
    lib = hip.load_library()
    pts, verts = torch.from_numpy(np.array(c.pts)).to(gpu), torch.from_numpy(np.array(c.verts)).to(gpu)
    P = hip.Points(pts=pts)
    mask = torch.full((P.R,), 7, dtype=torch.uint8, device=gpu)
    hit = torch.full((P.R,), 7, dtype=torch.int32, device=gpu)
    assert ws.numel() >= lib.th_hull_workspace_bytes(verts.shape[0])
    rc = lib.th_hull_mask(hip.ctx(gpu), C.byref(P.c), hip._p(verts), verts.shape[0], c.thresh, hip._p(mask), hip._p(hit), hip._p(ws),
                          ws.numel(), hip._stream())
    assert rc == 0
    assert int(mask.max()) <= 1 and int(hit.max()) <= 1
    return mask.bool(), hit.bool()


@pytest.mark.parametrize("form", FORMS)
def test_workspace_contents_do_not_matter(hip, gpu, monkeypatch, form):
    """th_hull_mask through the C ABI in a workspace of 0x00 bytes and one of 0xFF bytes, a small grid (5^3 cells) and the 63^3
    one; then the small grid right behind the large one in the SAME workspace (which then holds the large grid's tables)"""
    _form(monkeypatch, form)
    lib = hip.load_library()
    small, large = "pop65", "cube20"
    nbytes = max(lib.th_hull_workspace_bytes(Hc.case(n).verts.shape[0]) for n in (small, large))
    for name in (small, large):
        c = Hc.case(name)
        got = []
        for fill in (0x00, 0xFF):
            ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=gpu)
            got.append(_abi_mask(hip, gpu, name, ws))
        assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1]), name
        _same(name, form, got[0][0], Hc.ref_of(name), c.verts, c.pts, c.thresh)
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=gpu)
    m_large, _ = _abi_mask(hip, gpu, large, ws)
    m_small, h_small = _abi_mask(hip, gpu, small, ws)
    c = Hc.case(small)
    _same(large, form, m_large, Hc.ref_of(large), Hc.case(large).verts, Hc.case(large).pts, 0.1)
    _same(small, form, m_small, Hc.ref_of(small), c.verts, c.pts, c.thresh)
    _same(small, form, h_small, Hc.ref_of(small), c.verts, c.pts, c.thresh)


# ---- the small-frame rule at its boundary ----------------------------------------------------------------------------------
def _prepass_counts(hip, gpu, name, thr):
    """render_prepass -> the three counts -> workspaces dropped: no prepass is pending when the next one is queued"""
    c = Hc.ray_case(name)
    P = hip.Points(c.ray_o.to(gpu), c.ray_d.to(gpu), c.near.to(gpu), c.far.to(gpu), n_samples=c.S)
    try:
        hip.render_prepass(P, torch.from_numpy(c.verts).to(gpu), 3, c.thresh, thr)
        return hip._prepass_counts(P._prepass_keep[1], gpu)
    finally:
        hip.drop_workspaces(gpu)


@pytest.mark.parametrize("name", Hc.RULE_SETS)
def test_small_frame_rule_switches_at_its_boundary(hip, gpu, name):
    """counts = (hit rays, the rule fired, listed samples): the rule fires for hit <= small_frame_rays and lists every sample of
    the hit rays; otherwise the samples of the mask.  small_frame_rays = -1 pins the masked branch."""
    m = Hc.ray_ref_of(name)
    S = m.shape[1]
    hit, valid = int(m.any(1).sum()), int(m.sum())
    assert hit >= 1 and valid < hit * S                                    # (the two branches give different counts)
    for thr in (-1, hit - 1, hit, hit + 1):
        want = (hit, int(hit <= thr), hit * S if hit <= thr else valid)
        got = _prepass_counts(hip, gpu, name, thr)
        print(f"{name}: small_frame_rays {thr}: counts {got}, expected {want}")
        assert got == want, (name, thr, got, want)


def test_small_frame_rule_on_rays_that_miss(hip, gpu):
    """no hit ray and small_frame_rays = 0: 0 <= 0, the rule fires over nothing"""
    assert not Hc.ray_ref_of("rays_miss").any()
    assert _prepass_counts(hip, gpu, "rays_miss", 0) == (0, 1, 0)
    assert _prepass_counts(hip, gpu, "rays_miss", -1) == (0, 0, 0)
