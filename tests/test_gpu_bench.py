"""GPU: bench.py's two kinds of run on a small frame -- a plain run prints the headline line and nothing that needs runs of
its own; --full adds them after the same timed steps, and both runs return the same image from their last timed step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "fused_kernel_inside", "dropin_ms_per_step", "render_fast_ms_per_step", "cpu_baseline")


def _bench(tmp_path, name, extra=()):
    out = tmp_path / name
    r = subprocess.run([sys.executable, "bench.py", "--res", "128", "--steps", "2", "--warmup", "1", "--dump-outputs", str(out)]
                       + list(extra), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    return line, {k: np.load(out / f"{k}.npy") for k in ("rgb_map", "acc_map", "depth_map")}


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_full_adds_the_rest(tmp_path, gpu):
    plain, img_plain = _bench(tmp_path, "plain")
    full, img_full = _bench(tmp_path, "full", ("--full", "--no-extras"))
    for line in (plain, full):
        assert all(k in line for k in HEADLINE) and line["value"] > 0 and line["steps"] == 2 and line["warmup"] == 1
    assert not any(k in plain for k in FULL_ONLY) and "extra" not in plain
    assert all(k in full for k in FULL_ONLY) and "extra" not in full
    assert "sigma_pos_samples_rank0" in full["config"] and full["cpu_baseline"]["gpu_vs_oracle"]["max_abs_rgb_acc"] < 1e-4
    for k in img_plain:
        assert np.array_equal(img_plain[k], img_full[k]), k
