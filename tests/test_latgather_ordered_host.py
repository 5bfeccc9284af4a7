"""The ordered form of K19's backward on the host: the switch cfg.train_gather_bwd (defaults to "atomic", a bad value raises,
"latents" + "ordered" refuses a CPU batch), the two C ABI entries th_latent_gather_bwd_ordered / _ws (declared, exported, bound
with the header's argument counts; the size query is a host computation; null pointers are refused before any device is
touched), the nine-argument LatentGatherFn.apply, and the sizes hip.py restates from k_latgather_ord.hip."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest
import torch

from transhuman_amd.config import _defaults, get_cfg, override
from transhuman_amd.networks import autograd_path, train_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("th_latent_gather_bwd_ordered", "th_latent_gather_bwd_ordered_ws")


def test_switch_defaults_to_atomic_refuses_a_bad_value_and_a_cpu_batch():
    from transhuman_amd import hip
    assert _defaults().train_gather_bwd == "atomic" and get_cfg().train_gather_bwd == "atomic"
    assert all(autograd_path._switch("train_gather_bwd", v, True) == v for v in ("atomic", "ordered"))
    batch = {"ray_o": torch.zeros(1, 4, 3), "ray_d": torch.ones(1, 4, 3)}
    with override(train_maps="latents", train_gather_bwd="ordered"), pytest.raises(hip.HipError, match="MI355X"):
        autograd_path.render(SimpleNamespace(net=None), batch)
    with override(train_maps="latents", train_gather_bwd="sorted"), pytest.raises(ValueError, match="train_gather_bwd"):
        autograd_path.render(SimpleNamespace(net=None), batch)
    with override(train_maps="full", train_gather_bwd="sorted"):   # the key is read with "latents" only
        with pytest.raises(Exception) as e:
            autograd_path.render(SimpleNamespace(net=None), batch)
    assert "train_gather_bwd" not in str(e.value)


def test_function_still_refuses_host_tensors_with_nine_and_with_ten_arguments():
    from transhuman_amd import hip
    V, dims = 2, ((10, 14), (5, 7), (3, 4))
    args = [torch.zeros((V, h, w, C)) for (h, w), C in zip(dims, (64, 64, 128))]
    args += [torch.zeros(128, 3), torch.zeros(128), torch.zeros(V, 3, 20, 28), torch.zeros(5, 3), torch.zeros(V, 21), torch.ones(2)]
    with pytest.raises(hip.HipError, match="MI355X"):
        train_ops.LatentGatherFn.apply(*args)
    with pytest.raises(hip.HipError, match="MI355X"):
        train_ops.LatentGatherFn.apply(*args, "ordered")
    with pytest.raises(ValueError, match="gather_bwd"):
        train_ops.LatentGatherFn.apply(*args, "sorted")


@pytest.fixture(scope="module")
def lib():
    from transhuman_amd import build, hip
    build.build(force=False, verbose=False)
    return hip.load_library()


def test_entry_points_declared_exported_bound(lib):
    from transhuman_amd import hip
    header = open(os.path.join(ROOT, "include", "transhuman_hip.h")).read()
    raw = ctypes.CDLL(os.path.join(ROOT, "transhuman_amd", "libtranshuman_hip.so"))
    for name, ret, res in zip(NAMES, ("int", "size_t"), (ctypes.c_int, ctypes.c_size_t)):
        assert hasattr(raw, name) and name in hip.SYMBOLS
        got_res, args = hip.SYMBOLS[name]
        decl = header[header.index(f"{ret} {name}("):]
        decl = decl[:decl.index(";")]
        assert got_res is res and decl.count(",") + 1 == len(args)
    assert len(hip.SYMBOLS[NAMES[0]][1]) == 20 and len(hip.SYMBOLS[NAMES[1]][1]) == 4
    assert callable(hip.latent_gather_bwd_ordered)
    assert lib.th_abi_version() == 12
    # the atomic entry keeps its signature
    assert len(hip.SYMBOLS["th_latent_gather_bwd"][1]) == 15


def test_size_query_is_a_host_call_positive_and_non_decreasing_in_P(lib):
    last = 0
    for P in (0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 3000, 153600):
        n = lib.th_latent_gather_bwd_ordered_ws(3, 512, 512, P)
        assert n > 0 and n >= last, (P, n, last)
        last = n
    # the index over the map pixels, four sort arrays of P V entries, the partials of the lift
    assert last >= 4 * (3 * 512 * 512 + 1) + 16 * 3 * 153600
    assert last < 32 << 20                                         # (the training shape: well under one latent gradient's 50 MB)
    assert lib.th_latent_gather_bwd_ordered_ws(0, 8, 8, 4) == 0 and lib.th_latent_gather_bwd_ordered_ws(1, 8, 8, -1) == 0


def test_null_pointers_are_refused_without_a_device(lib):
    dims = (ctypes.c_int32 * 6)(2, 2, 2, 2, 2, 2)
    assert lib.th_latent_gather_bwd_ordered(None, dims, 1, 4, 4, None, 0, None, None, None, 384, None, None, None, None, None,
                                            None, None, 0, None) < 0
    assert b"null" in lib.th_last_error()


def test_the_sizes_restated_in_python_are_the_kernels(lib):
    from transhuman_amd import hip
    src = open(os.path.join(ROOT, "transhuman_amd", "csrc", "k_latgather_ord.hip")).read()
    define = lambda name: int(re.search(rf"^#define {name} (\d+)", src, flags=re.M).group(1))
    assert hip.LATENT_GATHER_ORDERED_SIZES == dict(batch=define("LGO_B"), sort_round=define("LGO_ROUND"),
                                                   sort_tile=define("LGO_TILE"), lift_rows=define("LGO_LIFT_ROWS"))
    assert "atomicAdd(" not in src.replace("atomicAdd(&h[", "")    # one LDS integer count; no float atomic anywhere
