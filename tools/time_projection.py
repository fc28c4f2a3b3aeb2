#!/usr/bin/env python3
"""Projection depth (K12) timings next to halfspace depth (K10) in the same run.  Rows form, every point a target, k = 1 000
directions: (n, d) = (10^6, 3), (10^5, 8), (10^4, 3), each followed by engine.halfspace_counts at the same shape (the two
share projection and sort; K12 replaces the rank pass by a selection per direction and an evaluation per target); the
external form with 100 points against 10^6 in R^3; and one blocks shape, the K-sampled estimator's launch at n = 400,
K = 2, 64 directions: 400 x 200 blocks of 200 or 201 rows.  Per case: the median over --reps calls after one warm-up call,
each call ending in a device synchronise, data resident on the device.  One JSON line per case.

    python tools/time_projection.py [--reps 5] [--only NAME ...] [--once]

--once runs each selected case once without timing (for rocprofv3 --kernel-trace --stats: the split between the shared
projection / sort / merge kernels and pd_locscale_kernel, pd_outlyingness_kernel, pd_external_kernel, pd_blocks_kernel)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from statdepth_amd import engine  # noqa: E402
from statdepth_amd.depth.calculations._pointcloud import _halfspace_directions  # noqa: E402

CASES = [("projection_n1e6_d3", "projection", 10**6, 3, 1000, None), ("halfspace_n1e6_d3", "halfspace", 10**6, 3, 1000, None),
         ("projection_n1e5_d8", "projection", 10**5, 8, 1000, None), ("halfspace_n1e5_d8", "halfspace", 10**5, 8, 1000, None),
         ("projection_n1e4_d3", "projection", 10**4, 3, 1000, None), ("halfspace_n1e4_d3", "halfspace", 10**4, 3, 1000, None),
         ("external_m100_n1e6_d3", "external", 10**6, 3, 1000, 100),
         ("blocks_n400_K2_d3_k64", "blocks", 400, 3, 64, None)]


def _median_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t) * 1e3)
    return statistics.median(times), min(times), max(times)


def _k_blocks(n, K, rng):
    """The blocks of _samplepointwisedepth for every point: n // K draws of n // K rows, the point appended last."""
    ss = n // K
    mem = np.full((n * ss, ss + 1), -1, dtype=np.int32)
    for tp in range(n):
        for b in range(ss):
            drawn = rng.permutation(n)[:ss]
            blk = np.append(drawn[drawn != tp], tp)
            mem[tp * ss + b, :len(blk)] = blk
    return mem


def run(name, route, n, d, k, m, reps, once):
    rng = np.random.default_rng(n + d)
    dev = torch.device("cuda", torch.cuda.current_device())
    P = torch.from_numpy(rng.normal(size=(n, d))).to(dev)
    U = torch.from_numpy(_halfspace_directions(k, 0, d)).to(dev)
    res = {"case": name, "route": route, "n": n, "d": d, "k": k, "targets": m if m else n}
    if route == "external":
        Q = torch.from_numpy(rng.normal(size=(m, d))).to(dev)
        fn = lambda: engine.projection_external_outlyingness(P, Q, U)   # noqa: E731
    elif route == "blocks":
        mem = _k_blocks(n, 2, rng)
        res["blocks"], res["block_width"] = int(mem.shape[0]), int(mem.shape[1])
        fn = lambda: engine.projection_subset_outlyingness(P, mem, U)   # noqa: E731
    elif route == "halfspace":
        fn = lambda: engine.halfspace_counts(P, U)                      # noqa: E731
    else:
        fn = lambda: engine.projection_outlyingness(P, U)               # noqa: E731
    if once:
        fn()
        torch.cuda.synchronize()
        return res
    res["ms_median"], res["ms_min"], res["ms_max"] = _median_ms(fn, reps)
    res["reps"] = reps
    if route == "blocks":
        res["blocks_per_s"] = res["blocks"] / (res["ms_median"] * 1e-3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    torch.cuda.init()
    for name, route, n, d, k, m in CASES:
        if a.only and name not in a.only:
            continue
        print(json.dumps(run(name, route, n, d, k, m, a.reps, a.once)), flush=True)


if __name__ == "__main__":
    main()
