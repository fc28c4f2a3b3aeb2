#!/usr/bin/env python3
"""Halfspace and projection depth of multivariate curves over time (K18) timings, every curve a target:

  sd_multi_halfspace_sums / sd_multi_projection_sums   algo 1 (LDS route) and algo 2 (global route) at n x T x d =
                       5 000 x 500 x 8 (benchmark config 4), 1 000 x 1 000 x 3 and 200 x 100 x 2; algo 2 alone at
                       10 000 x 100 x 3, above the LDS capacity; k = 1 000 and k = 64 directions
  loop                 what a user had before: engine.halfspace_counts / engine.projection_outlyingness on P[:, t, :] once per
                       timepoint from Python (one upload and one launch chain per timepoint), summed on the host

Within one case the routes alternate: --reps rounds of (lds, global, loop), so a drift of the device shows in all three.
"lds" and "global" are device time of the C entry point alone, between two HIP events on the current stream: data, result
and workspace resident on the device, no copy inside the window.  "loop" is wall time of the Python loop from host arrays to
host results, synchronised at both ends: uploads, launches and downloads are what that user pays.  Per route: --warmup
calls first, then the rounds; median, minimum and maximum in ms per call.  One JSON line per case.

    python tools/time_multi_cloud.py [--reps 3] [--warmup 1] [--only NAME ...] [--limit 300]

Every case runs in a child process of its own under --limit seconds; the first case that fails or runs out of time ends
the run, and nothing more is started on the device."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (case, family, n, T, d, k)
SHAPES = [(5000, 500, 8), (1000, 1000, 3), (200, 100, 2), (10000, 100, 3)]
CASES = [(f"{fam}_n{n}_T{T}_d{d}_k{k}", fam, n, T, d, k)
         for (n, T, d) in SHAPES for k in (1000, 64) for fam in ("halfspace", "projection")]


def _directions(k, d, seed=0):
    U = np.random.default_rng(seed).standard_normal((k, d))
    return U / np.linalg.norm(U, axis=1, keepdims=True)


def run(name, fam, n, T, d, k, reps, warmup):
    import torch
    from statdepth_amd import engine
    from statdepth_amd._native import check
    torch.cuda.init()
    dev = torch.device("cuda", torch.cuda.current_device())
    lib = engine._lib()
    P = np.random.default_rng(n + T + d).normal(size=(n, T, d))
    U = _directions(k, d)
    Pd, Ud = torch.from_numpy(P).to(dev), torch.from_numpy(U).to(dev)
    out = torch.empty((n, 2), dtype=torch.int64 if fam == "halfspace" else torch.float64, device=dev)
    size, sums = getattr(lib, f"sd_multi_{fam}_workspace_bytes"), getattr(lib, f"sd_multi_{fam}_sums")
    routes = {}
    for route, algo in (("lds", 1), ("global", 2)):
        nbytes = int(size(n, T, d, k, n, algo))
        if nbytes == 0:                                              # the LDS route above its capacity
            continue
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

        def call(algo=algo, ws=ws, nbytes=nbytes):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            check(sums(Pd.data_ptr(), n, T, d, Ud.data_ptr(), k, None, n, algo, out.data_ptr(), ws.data_ptr(), nbytes,
                       engine._stream_ptr(dev)))
            b.record()
            b.synchronize()
            return a.elapsed_time(b)
        routes[route] = call
    point = engine.halfspace_counts if fam == "halfspace" else engine.projection_outlyingness

    def loop():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        acc = np.zeros(n)
        for t in range(T):
            v = point(P[:, t, :], U)
            acc = acc + (v if fam == "halfspace" else 1.0 / (1.0 + v))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    routes["loop"] = loop
    for fn in routes.values():
        for _ in range(warmup):
            fn()
    times = {r: [] for r in routes}
    for _ in range(reps):
        for r, fn in routes.items():
            times[r].append(fn())
    res = {"case": name, "entry": f"sd_multi_{fam}_sums", "n": n, "T": T, "d": d, "k": k, "reps": reps, "warmup": warmup}
    for r, ts in times.items():
        res[r] = {"ms_median": round(statistics.median(ts), 3), "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--limit", type=float, default=300.0, help="seconds a case may take")
    ap.add_argument("--case", default=None, help="run this one case in this process (what the parent starts)")
    a = ap.parse_args()
    if a.case:
        name, fam, n, T, d, k = next(c for c in CASES if c[0] == a.case)
        print(json.dumps(run(name, fam, n, T, d, k, a.reps, a.warmup)), flush=True)
        return 0
    for name, *_ in CASES:
        if a.only and name not in a.only:
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(a.reps), "--warmup", str(a.warmup)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(json.dumps({"case": name, "error": f"no result within {a.limit:g} s"}), flush=True)
            return 1
        if p.returncode != 0:
            print(json.dumps({"case": name, "error": f"exit status {p.returncode}", "stderr": p.stderr[-400:]}), flush=True)
            return 1
        print(p.stdout.strip().splitlines()[-1], flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
