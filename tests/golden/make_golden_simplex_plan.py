#!/usr/bin/env python3
"""Record what sd_simplex_sampled_workspace_bytes returns.

The fixture pins the numbers of the library as it was BEFORE the sampled workspace of K4 got its one plan behind sizing,
routing and launch: it is recorded from a build of that parent commit and never from the code under test,

    python3 tests/golden/make_golden_simplex_plan.py --lib <parent checkout>/statdepth_amd/lib/libstatdepth_hip.so

and tests/test_simplex_plan_host.py asks the library under test the same questions through table() below.  No GPU: the
size function is host code.

Sizes (simplex_plan_sizes.json, kind "simplex_plan_sizes"): the grid in the order of itertools.product over the axes n, T,
d and samples -- d = 0 and 9 and samples = 0 are outside what the function covers and give 0; samples = 256 is the
routing floor of every larger call; 2^20 pairs is the cap of a batch -- and the shapes that bench.py sizes, in the order of
BENCH.
"""
import argparse
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from statdepth_amd import _native  # noqa: E402

AXES = {"n": [1, 5, 40, 500, 10 ** 5, 2 ** 31 - 1], "T": [0, 1, 3, 50, 5000], "d": [0, 1, 3, 5, 8, 9],
        "samples": [0, 1, 16, 255, 256, 257, 4096, 2 ** 20, 2 ** 20 + 1, 10 ** 7]}
# (n, T, d, samples): the two sampled workloads, config 4 (i) and config 5 (iii)
BENCH = [[100000, 0, 3, 256], [500, 50, 8, 256], [5000, 500, 8, 4096], [1000000, 0, 3, 4096]]


def grid():
    return itertools.product(*(AXES[k] for k in ("n", "T", "d", "samples")))


def table(lib):
    size = lib.sd_simplex_sampled_workspace_bytes
    return {"grid": [size(*shape) for shape in grid()], "bench": [size(*shape) for shape in BENCH]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True, help="libstatdepth_hip.so of the parent commit")
    lib = _native.open_library(ap.parse_args().lib)
    out = {"name": "simplex_plan_sizes", "kind": "simplex_plan_sizes", "axes": AXES, "bench_shapes": BENCH, **table(lib)}
    path = os.path.join(HERE, "simplex_plan_sizes.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"), allow_nan=False)
        f.write("\n")
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out['grid'])} grid points, {sum(1 for v in out['grid'] if v)} not zero")


if __name__ == "__main__":
    main()
