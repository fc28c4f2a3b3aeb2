#!/usr/bin/env python3
"""Halfspace depth (K10) timings, every point a target, k = 1 000 directions: (n, d) = (10^6, 3), (10^5, 8), (10^4, 3); the
external route with 100 targets against 10^6 points in R^3; and, at n = 20 000, d = 3, k = 256, the ranking route against
the pairwise kernel over the same targets (the reason for having two kernels).  Per case: the median over --reps calls
after one warm-up call, each call ending in a device synchronise, data resident on the device.  One JSON line per case.

    python tools/time_halfspace.py [--reps 5] [--only NAME ...] [--once]

--once runs each selected case once without timing (for rocprofv3 --kernel-trace --stats: the split between
hs_project_kernel and the sort / merge / rank kernels)."""
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

CASES = [("rank_n1e6_d3", "rank", 10**6, 3, 1000, None), ("rank_n1e5_d8", "rank", 10**5, 8, 1000, None),
         ("rank_n1e4_d3", "rank", 10**4, 3, 1000, None), ("external_m100_n1e6_d3", "external", 10**6, 3, 1000, 100),
         ("rank_n20000_d3_k256", "rank", 20000, 3, 256, None), ("pairwise_n20000_d3_k256", "pairwise", 20000, 3, 256, None)]


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


def run(name, route, n, d, k, m, reps, once):
    rng = np.random.default_rng(n + d)
    dev = torch.device("cuda", torch.cuda.current_device())
    P = torch.from_numpy(rng.normal(size=(n, d))).to(dev)
    U = torch.from_numpy(_halfspace_directions(k, 0, d)).to(dev)
    res = {"case": name, "route": route, "n": n, "d": d, "k": k, "targets": m if m else n}
    if route == "external":
        Q = torch.from_numpy(rng.normal(size=(m, d))).to(dev)
        fn = lambda: engine.halfspace_external_counts(P, Q, U)          # noqa: E731
        res["projections"] = m * n * k
    else:
        fn = lambda: engine.halfspace_counts(P, U, algo=route)          # noqa: E731
        res["projections"] = n * k if route == "rank" else n * n * k
    if once:
        fn()
        torch.cuda.synchronize()
        return res
    res["ms_median"], res["ms_min"], res["ms_max"] = _median_ms(fn, reps)
    res["reps"] = reps
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
