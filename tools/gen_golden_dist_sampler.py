"""Write tests/golden/g25_dist_sampler.npz: index lists recorded from the reference's own DistributedSampler.

    python tools/gen_golden_dist_sampler.py --reference <reference checkout>

CPU only, where the reference checkout exists.  lib/datasets/samplers.py is loaded by file path under its own module name; the
two project modules it imports at the top (lib.config, lib.datasets.get_human_info) are stood in for by empty modules -- the
sampler class reads neither.  For every case (n, world, epoch, shuffle) the sampler of EVERY rank is built on a stand-in data
set of length n, given the epoch through set_epoch, and iterated once.

Stored, as plain integer arrays only: ``cases`` [K, 4] = (n, world, epoch, shuffle) and per case k ``idx_k`` [world, ceil(n /
world)] (row r: rank r's indices in the order the sampler yields them).  ``iters`` [M, 3] = (max_iter, world, int(max_iter /
world)) is NOT a recording: make_data_loader needs the data set, so the expression of make_dataset.py:77-78 is evaluated here.
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# n not divisible by world (10/3, 7/2, 101/8, 5/4), divisible (12/3), a world larger than n (3/5), one rank, unshuffled
CASES = [(10, 3, 0, 1), (10, 3, 1, 1), (10, 3, 7, 1), (12, 3, 0, 1), (7, 2, 3, 1), (101, 8, 0, 1), (101, 8, 2999, 1),
         (5, 4, 2, 1), (3, 5, 1, 1), (9, 1, 4, 1), (10, 3, 5, 0), (7, 2, 0, 0)]
ITERS = [(500, 1), (500, 2), (500, 3), (500, 8), (7, 8), (1000, 6)]


def _load_sampler_module(reference):
    for pkg in ("lib", "lib.datasets"):
        m = types.ModuleType(pkg)
        m.__path__ = []
        sys.modules[pkg] = m
    conf = types.ModuleType("lib.config")
    conf.cfg = types.SimpleNamespace()
    sys.modules["lib.config"] = conf
    sys.modules["lib.datasets"].get_human_info = types.ModuleType("lib.datasets.get_human_info")
    sys.modules["lib.datasets.get_human_info"] = sys.modules["lib.datasets"].get_human_info
    spec = importlib.util.spec_from_file_location("lib.datasets.samplers", os.path.join(reference, "lib/datasets/samplers.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["lib.datasets.samplers"] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference checkout (holds lib/datasets/samplers.py)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "g25_dist_sampler.npz"))
    args = ap.parse_args()
    samplers = _load_sampler_module(args.reference)
    out = {"cases": np.array(CASES, dtype=np.int64)}
    for k, (n, world, epoch, shuffle) in enumerate(CASES):
        rows = []
        for rank in range(world):
            s = samplers.DistributedSampler(range(n), num_replicas=world, rank=rank, shuffle=bool(shuffle))
            s.set_epoch(epoch)
            rows.append(list(iter(s)))
            assert len(rows[-1]) == len(s)
        out[f"idx_{k}"] = np.array(rows, dtype=np.int64)
    out["iters"] = np.array([(m, w, int(m / w)) for m, w in ITERS], dtype=np.int64)
    np.savez_compressed(args.out, **out)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes, {len(CASES)} cases")


if __name__ == "__main__":
    main()
