#!/usr/bin/env python3
"""Oja depth (K7) timings, every point a target: (n, d) = (2 000, 2), (400, 3), (120, 5), (60, 8), and the K=2 sampled
estimator at n = 200, d = 2.  Per case: ms per call and simplex volumes (subsets) per second, with the host's Qhull
time and the GPU's volume sums reported separately.  One JSON line per case.

    python tools/time_oja.py [--reps 3] [--only NAME ...] [--once]

--once runs each selected case's GPU call once without timing (for rocprofv3 --kernel-trace --stats, or a separate
counter run: fp64 VALU instructions per subset = the counters' sum / the JSON's `subsets`)."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from statdepth_amd import PointcloudDepth, engine  # noqa: E402
from statdepth_amd.depth.calculations._pointcloud import _hull_volume  # noqa: E402

CASES = [("n2000_d2", 2000, 2, None), ("n400_d3", 400, 3, None), ("n120_d5", 120, 5, None), ("n60_d8", 60, 8, None),
         ("k2_n200_d2", 200, 2, 2)]


def _sync():
    torch.cuda.synchronize()


def _timed(fn, reps):
    fn()
    _sync()
    t = time.perf_counter()
    for _ in range(reps):
        r = fn()
    _sync()
    return (time.perf_counter() - t) / reps * 1e3, r


def _blocks(n, K, seed):
    """_samplepointwisedepth's blocks for every target (same draw rule), for the split timing."""
    np.random.seed(seed)
    ss = n // K
    rows = pd.Series(np.arange(n))
    blocks = []
    for tp in range(n):
        for _ in range(ss):
            drawn = rows.sample(n=ss).to_numpy()
            blocks.append(np.append(drawn[drawn != tp], tp))
    width = max(len(b) for b in blocks)
    mem = np.full((len(blocks), width), -1, dtype=np.int32)
    for i, b in enumerate(blocks):
        mem[i, :len(b)] = b
    return blocks, mem


def run(name, n, d, K, reps, once):
    P = np.random.default_rng(n * 10 + d).normal(size=(n, d))
    df = pd.DataFrame(P)
    res = {"case": name, "n": n, "d": d, "K": K}
    if K is None:
        res["subsets"] = n * math.comb(n - 1, d)
        if once:
            engine.oja_volume_sums(P)
            _sync()
            return res
        res["host_hull_ms"], _ = _timed(lambda: _hull_volume(P), reps)
        res["gpu_ms"], _ = _timed(lambda: engine.oja_volume_sums(P), reps)
        res["call_ms"], _ = _timed(lambda: PointcloudDepth(df, containment='oja'), reps)
    else:
        blocks, mem = _blocks(n, K, 1)
        res["blocks"] = len(blocks)
        res["subsets"] = sum(math.comb(len(b) - 1, d) for b in blocks)
        if once:
            engine.oja_subset_volume_sums(P, mem)
            _sync()
            return res
        res["host_hull_ms"], _ = _timed(lambda: [_hull_volume(P[b]) for b in blocks], reps)
        res["gpu_ms"], _ = _timed(lambda: engine.oja_subset_volume_sums(P, mem), reps)

        def call():
            np.random.seed(1)
            return PointcloudDepth(df, K=K, containment='oja')
        res["call_ms"], _ = _timed(call, reps)
    res["gpu_subsets_per_s"] = res["subsets"] / (res["gpu_ms"] * 1e-3)
    res["call_subsets_per_s"] = res["subsets"] / (res["call_ms"] * 1e-3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    torch.cuda.init()
    for name, n, d, K in CASES:
        if a.only and name not in a.only:
            continue
        print(json.dumps(run(name, n, d, K, a.reps, a.once)), flush=True)


if __name__ == "__main__":
    main()
