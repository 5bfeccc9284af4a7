"""CPU: the C-ABI shared library loads (no GPU needed) and exports every symbol
include/transhuman_hip.h declares; the ctypes binding table matches the header."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "transhuman_hip.h")


def header_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = re.findall(r"\b(th_[a-z0-9_]+)\s*\(", src)
    return sorted(set(names))


@pytest.fixture(scope="module")
def lib():
    from transhuman_amd import build, hip
    build.build(force=False, verbose=False)
    return hip.load_library()


def test_header_declares_the_expected_surface():
    names = header_functions()
    for must in ("th_ctx_create", "th_ctx_destroy", "th_last_error", "th_set_mlp_weights", "th_set_vit_weights",
                 "th_hull_mask", "th_paint_group", "th_vit_forward", "th_dparf_encode", "th_pixel_gather",
                 "th_network_forward", "th_composite", "th_render_rays", "th_eval_sigma_grid"):
        assert must in names


def test_library_exports_every_declared_symbol(lib):
    raw = ctypes.CDLL(os.path.join(ROOT, "transhuman_amd", "libtranshuman_hip.so"))
    missing = [n for n in header_functions() if not hasattr(raw, n)]
    assert not missing, f"declared in the header but not exported: {missing}"


def test_binding_table_matches_header(lib):
    from transhuman_amd import hip
    assert sorted(hip.SYMBOLS) == header_functions()
    assert lib.th_abi_version() == 12


def test_workspace_queries_are_pure_host_calls(lib):
    # no device needed for sizing
    assert lib.th_linear_workspace_bytes(256, 255) >= 256 * 256 * 4
    assert lib.th_hull_workspace_bytes(6890) > 6890 * 12
    assert lib.th_vit_workspace_bytes(3, 500, 192, 3) >= 3 * 500 * 192 * 4 * 6
    assert lib.th_network_workspace_bytes(3, 1000) > 3 * 1000 * (256 + 384) * 4


def test_no_fallback_without_a_device(lib):
    """the product path must fail loudly when there is no GPU / library, never compute on the CPU"""
    import torch
    from transhuman_amd import hip
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(hip.HipError):
        hip.ctx()
    from util import make_net
    net = make_net(2)
    with pytest.raises((hip.HipError, AssertionError)):
        net.ViT(torch.zeros(1, 8, 192), torch.zeros(1, 8, 3))


def test_errors_are_reported_not_crashed(lib):
    bad = lib.th_set_chunk_samples(3)
    assert bad != 0 and b"chunk" in lib.th_last_error()
    assert lib.th_set_chunk_samples(524288) == 0


def _integration_snippet_structs():
    """The ctypes Structure classes of INTEGRATION.md's python stub, executed as written."""
    import ctypes as C
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    blocks = re.findall(r"```python\n(.*?)```", text, flags=re.S)
    assert blocks, "INTEGRATION.md lost its ctypes stub"
    out = {}
    for blk in blocks:
        for m in re.finditer(r"^class (\w+)\(C\.Structure\):.*?\n(?:[ \t]+.*\n)+", blk, flags=re.M):
            ns = {"C": C}
            exec(m.group(0), ns)                      # (documentation of this repository, not reference content)
            out[m.group(1)] = ns[m.group(1)]
    return out


def test_integration_md_structs_match_the_library(lib):
    """the document's ThPoints once had 9 fields against the ABI's 11 -- a maintainer who copied it
    handed th_composite a struct 16 bytes short.  The snippet is now executed and held to th_sizeof()."""
    import ctypes as C
    from transhuman_amd import hip
    structs = _integration_snippet_structs()
    assert "ThPoints" in structs
    cname = {"ThPoints": b"th_points", "ThFrame": b"th_frame", "ThMapSource": b"th_map_source"}
    for name, cls in structs.items():
        want = lib.th_sizeof(cname[name])
        assert want > 0 and C.sizeof(cls) == want, (name, C.sizeof(cls), want)
        ours = getattr(hip, name)
        assert [f[0] for f in cls._fields_] == [f[0] for f in ours._fields_], name
    # the binding's own structs against the library as compiled
    assert C.sizeof(hip.ThPoints) == lib.th_sizeof(b"th_points")
    assert C.sizeof(hip.ThFrame) == lib.th_sizeof(b"th_frame")
    assert C.sizeof(hip.ThMapSource) == lib.th_sizeof(b"th_map_source")
    assert lib.th_sizeof(b"no_such_struct") == 0


# ---- the binding is derived from the header (transhuman_amd/cheader.py) ----
# every form the real header uses, once
SMALL_HEADER = """\
#ifndef SMALL_H
#define SMALL_H
#define TH_LIMIT 0x7B53u   /* 6.0e4 */
enum { TH_A = 1, TH_B = 2 /* a note */, TH_C = 8 };
typedef struct th_ctx th_ctx;
typedef void* th_stream;
typedef struct { const float* w; int out_f; } th_lin;
typedef struct {
    int a, b;                  /* two in one declaration */
    const float *p, *q;
    int32_t dims[6];
    th_lin first, second;
    const th_lin* next;
} th_box;
typedef struct th_rec { void* p; float lr; uint32_t flags; } th_rec;
int         th_version(void);
const char* th_error(void);
void th_free(th_ctx* ctx);
size_t th_bytes(const th_box* b, long long n, unsigned long long* count_out);
int th_run(th_ctx* ctx, const float* x /* [3] */, float scale, double* out,
           const void* const* tables, const th_lin* lin, th_rec* recs,
           th_ctx** made, double ratio, th_stream stream);
#endif
"""


def test_header_reader_on_every_declaration_form():
    import ctypes as C
    from transhuman_amd import cheader
    h = cheader.parse(SMALL_HEADER, records=("th_rec",))
    assert h.constants == {"TH_LIMIT": 0x7B53, "TH_A": 1, "TH_B": 2, "TH_C": 8}
    assert list(h.structs) == ["th_lin", "th_box"]
    lin, box = h.structs["th_lin"], h.structs["th_box"]
    assert (lin.__name__, box.__name__) == ("ThLin", "ThBox") and issubclass(box, C.Structure)
    assert lin._fields_ == [("w", C.c_void_p), ("out_f", C.c_int)]
    assert box._fields_ == [("a", C.c_int), ("b", C.c_int), ("p", C.c_void_p), ("q", C.c_void_p), ("dims", C.c_int32 * 6),
                            ("first", lin), ("second", lin), ("next", C.c_void_p)]
    assert h.records == {"th_rec": [("p", "<u8"), ("lr", "<f4"), ("flags", "<u4")]}
    vp = C.c_void_p
    assert h.prototypes == {
        "th_version": (C.c_int, []),
        "th_error": (C.c_char_p, []),
        "th_free": (None, [vp]),
        "th_bytes": (C.c_size_t, [C.POINTER(box), C.c_longlong, vp]),
        "th_run": (C.c_int, [vp, vp, C.c_float, vp, vp, C.POINTER(lin), vp, vp, C.c_double, vp]),
    }


@pytest.mark.parametrize("bad, line", [
    ("int th_ok(void);\nint th_bad(unsigned x);\n", 2),                        # a scalar type outside the rules
    ("int th_ok(void);\n\ntypedef struct { flaot x; } th_s;\n", 3),           # an unknown field type
    ("/* two\n lines */\nint th_bad(int a) int th_more(int b);\n", 3),         # a lost semicolon
    ("int th_ok(void);\nint th_ok(void);\n", 2),                               # declared twice
    ("enum { TH_A = 1, TH_B };\n", 1),                                         # an enumerator without a value
    ("#define TH_N twelve\n", 1),
    ("int th_ok(void);\nint th_unfinished(int a\n", 2),
    ("typedef struct th_rec { double d; } th_rec;\n", 1),                      # a record field numpy has no code for here
])
def test_header_reader_refuses_what_it_cannot_parse(bad, line):
    from transhuman_amd import cheader
    with pytest.raises(cheader.HeaderError, match=rf"^small\.h:{line}: "):
        cheader.parse(bad, records=("th_rec",), where="small.h")


def test_header_reader_is_complete_on_the_real_header(lib):
    import ctypes as C
    import numpy as np
    from transhuman_amd import cheader, hip
    h = cheader.load()
    assert hip.SYMBOLS is h.prototypes and len(h.prototypes) == len(header_functions())
    assert h.constants["TH_ABI_VERSION"] == lib.th_abi_version()
    assert (hip.RANGE_FP16_LIMIT, hip.RANGE_FP16_FLOOR) == (0x7B53, 0x2400)
    assert (hip.ADAM_CLIP, hip.ADAM_ZERO_GRAD, hip.ADAM_COUNT_NONFINITE, hip.ADAM_CHECK_POINTERS, hip.ADAM_T_DECOUPLED) == \
        (1, 2, 4, 8, 1)
    # every struct th_sizeof knows has a class or a record here, of the library's size
    api = open(os.path.join(ROOT, "transhuman_amd", "csrc", "th_api.hip")).read()
    sized = re.findall(r"TH_SZ\((th_\w+)\)", api)
    assert len(sized) == 8 and set(sized) == set(h.structs) | set(h.records)
    for name in sized:
        want = lib.th_sizeof(name.encode())
        have = C.sizeof(h.structs[name]) if name in h.structs else np.dtype(h.records[name]).itemsize
        assert want > 0 and have == want, (name, have, want)
    for name in ("ThLinear", "ThMlpWeights", "ThVitBlock", "ThPoints", "ThSmplModel", "ThMapSource", "ThFrame"):
        assert getattr(hip, name) in h.structs.values() and getattr(hip, name).__name__ == name
    assert hip.ADAM_TENSOR_FIELDS is h.records["th_adam_tensor"]


def test_derived_signatures_against_hand_written_ones():
    """The only signatures typed twice: five that between them use every rule of the reader."""
    import ctypes as C
    from transhuman_amd import hip
    vp, i, f, sz, ll = C.c_void_p, C.c_int, C.c_float, C.c_size_t, C.c_longlong
    frame, points, linear = C.POINTER(hip.ThFrame), C.POINTER(hip.ThPoints), C.POINTER(hip.ThLinear)
    assert hip.SYMBOLS["th_render_rays"] == (i, [vp, frame, points, vp, vp, vp, i, vp, sz, vp, sz, vp, vp])
    assert hip.SYMBOLS["th_patch_rays"] == (i, [vp, vp, vp, vp, vp, vp, vp, vp, vp, ll, ll, i, i, vp, C.c_double, i, i,
                                                vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp])
    assert hip.SYMBOLS["th_linear_bwd"] == (i, [vp, vp, i, i, i, vp, vp, f, linear, vp, i, vp, i, vp, vp, vp, vp, vp, sz, vp])
    assert hip.SYMBOLS["th_adam_step"] == (i, [vp, vp, vp, i, f, i, vp, vp])
    assert hip.SYMBOLS["th_shade_pool_bytes"] == (sz, [vp, frame, ll, i])


def test_struct_field_offsets():
    """th_sizeof cannot see two same-sized fields in the wrong order (H / W, centres / rot): offsets by hand from the header"""
    import ctypes as C
    from transhuman_amd import hip
    F, P = hip.ThFrame, hip.ThPoints
    assert [getattr(F, n).offset for n in ("verts_world", "H", "W", "centres", "rot", "map_fold")] == [0, 60, 64, 80, 88, 120]
    assert C.sizeof(F) == 128
    assert [getattr(P, n).offset for n in ("pts", "R", "S", "sigma_noise")] == [0, 56, 60, 72]
    assert C.sizeof(P) == 80
