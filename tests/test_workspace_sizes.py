"""CPU: every size function of the C ABI answers what tests/golden/workspace_sizes.json pins (written by
tools/gen_workspace_sizes.py from the library BEFORE the workspaces moved onto layout functions, never since), and the arena
behind those layouts measures exactly what it carves (tests/arena_check.cpp, compiled with the host compiler)."""
import ctypes as C
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "workspace_sizes.json")
ROWS = json.load(open(GOLDEN))


@pytest.fixture(scope="module")
def lib():
    from transhuman_amd import build, hip
    build.build(force=False, verbose=False)
    return hip.load_library()


def test_every_size_function_is_pinned():
    from transhuman_amd import hip
    sized = {n for n, (res, _) in hip.SYMBOLS.items() if res is C.c_size_t}
    # th_shade_pool_bytes needs a context (its plan is one function already); th_sizeof sizes structs, not workspaces
    assert {r["fn"] for r in ROWS} == sized - {"th_shade_pool_bytes", "th_sizeof"}


def _call(lib, row):
    from transhuman_amd import hip
    if "frame" not in row:
        return int(getattr(lib, row["fn"])(*row["args"]))
    f = hip.ThFrame()
    f.V, f.H, f.W, f.map_channels, f.n_verts, f.n_clusters = row["frame"]
    return int(getattr(lib, row["fn"])(C.byref(f), *row["args"]))


def test_sizes_are_the_pinned_ones(lib):
    bad = [(r, got) for r in ROWS for got in [_call(lib, r)] if got != r["bytes"]]
    assert not bad, f"{len(bad)} of {len(ROWS)} sizes moved, first: {bad[:5]}"


def test_arena_measures_what_it_carves(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "arena_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "transhuman_amd", "csrc"),
                    os.path.join(ROOT, "tests", "arena_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "48 take sequences, 0 failures" in r.stdout
