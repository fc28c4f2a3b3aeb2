#!/usr/bin/env python3
"""Probabilistic depth (K8, K9) timings, every curve or distribution a target: normal n = 10^4 and 10^5, Poisson
10^3 timepoints x 10^4 curves at lim = 1 000 (and a 10^2 x 10^4 case), and ProbabilisticDepth's band sums (K9) in both
modes at 100 timepoints x 1 000 curves, 1 000 x 100, and K = 10 blocks at 2 000 x 200 (through the public API).  Per
case: ms per call and the evaluations per second (pairs for the normal depth, (timepoint, curve, z) triples for the
Poisson depth, (target, pair, timepoint) triples for the band depth).  One JSON
line per case, appended to profiles/prob_times.jsonl unless --out says otherwise.

    python tools/time_probabilistic.py [--reps 2] [--only NAME ...] [--once] [--out PATH]
    rocprofv3 --kernel-trace --stats -d DIR -o prob -- python tools/time_probabilistic.py --once --only normal_n1e5 \
        poisson_T1e2_n1e4_lim1e3
    python tools/time_probabilistic.py --summarize DIR/prob_results.db     # -> profiles/prob_kernel_stats.json
    rocprofv3 --kernel-trace --stats -d DIR -o band -- python tools/time_probabilistic.py --once --only \
        band_relax_T1e2_n1e3 band_strict_T1e2_n1e3
    python tools/time_probabilistic.py --summarize DIR/band_results.db --band   # -> profiles/prob_band_kernel_stats.json

--once runs each selected case once without timing (for the kernel trace); --summarize folds the trace's database into
per-kernel call counts and durations."""
import argparse
import json
import os
import re
import sqlite3
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name, kind, shape
CASES = [("normal_n1e4", "normal", (10_000,)), ("normal_n1e5", "normal", (100_000,)),
         ("poisson_T1e2_n1e4_lim1e3", "poisson", (100, 10_000, 1000)),
         ("poisson_T1e3_n1e4_lim1e3", "poisson", (1000, 10_000, 1000))]
for _mode in ("relax", "strict"):
    CASES += [(f"band_{_mode}_T1e2_n1e3", "band_" + _mode, (100, 1000, None)),
              (f"band_{_mode}_T1e3_n1e2", "band_" + _mode, (1000, 100, None)),
              (f"band_{_mode}_K10_T2e3_n2e2", "band_" + _mode, (2000, 200, 10))]


def _inputs(kind, shape, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "normal":
        n, = shape
        return rng.normal(0, 2, n), np.exp(rng.uniform(np.log(0.1), np.log(10), n))
    if kind.startswith("band"):
        T, n, K = shape
        import pandas as pd
        cols = [f"c{i}" for i in range(n)]
        mu = pd.DataFrame(rng.normal(0, 1, (T, n)) + rng.normal(0, 0.5, n), columns=cols)
        var = pd.DataFrame(np.exp(rng.uniform(np.log(0.01), np.log(4.0), (T, n))), columns=cols)
        return mu, var, K, kind == "band_relax"
    T, n, lim = shape
    return np.exp(rng.uniform(np.log(0.1), np.log(100), size=(T, n))), lim


def _call(kind, args):
    from statdepth_amd import engine
    if kind.startswith("band"):
        from statdepth_amd import ProbabilisticDepth
        mu, var, K, relax = args
        np.random.seed(0)
        return ProbabilisticDepth(mu, var, K=K, relax=relax).to_numpy()
    return engine.prob_normal_sums(*args) if kind == "normal" else engine.prob_poisson_sums(*args)


def _evaluations(kind, shape):
    if kind == "normal":
        return shape[0] * (shape[0] - 1)
    if kind == "poisson":
        return shape[0] * shape[1] * (shape[2] - 1)
    T, n, K = shape
    if K is None:
        return n * ((n - 1) * (n - 2) // 2) * T
    bs = n // K + 1                                   # a block with its target forced in
    return n * K * (bs * (bs - 1) // 2) * T


def summarize(db_path, out_path, band=False):
    db = sqlite3.connect(db_path)
    rows = db.execute("select name, count(*), sum(duration), avg(duration), min(duration), max(duration), max(vgpr_count) "
                      "from kernels group by name order by sum(duration) desc").fetchall()
    out = {"source": "rocprofv3 --kernel-trace --stats -- python tools/time_probabilistic.py --once --only normal_n1e5 "
                     "poisson_T1e2_n1e4_lim1e3 (one MI355X)",
           "note": "durations in microseconds; one call of each case (the normal n = 1e5 case is the pn_kernel launches, "
                   "the Poisson 100 x 10^4 x lim 1 000 case the pp_* launches)",
           "kernels": [{"kernel": re.sub(r"\(.*", "", name), "calls": cnt, "total_us": round(tot / 1e3, 1),
                        "avg_us": round(avg / 1e3, 1), "min_us": round(mn / 1e3, 1), "max_us": round(mx / 1e3, 1),
                        "vgprs": vg} for name, cnt, tot, avg, mn, mx, vg in rows]}
    if band:
        out["source"] = ("rocprofv3 --kernel-trace --stats -- python tools/time_probabilistic.py --once --only "
                         "band_relax_T1e2_n1e3 band_strict_T1e2_n1e3 (one MI355X)")
        out["note"] = ("durations in microseconds; one call of each case (pb_kernel<true> is the relax case, "
                       "pb_kernel<false> the strict one, pn_fold_kernel the tile folds of both)")
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--only", nargs="*")
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prob_times.jsonl"))
    ap.add_argument("--summarize", metavar="DB")
    ap.add_argument("--band", action="store_true", help="with --summarize: a trace of the band cases "
                    "(-> profiles/prob_band_kernel_stats.json)")
    a = ap.parse_args()
    if a.summarize:
        name = "prob_band_kernel_stats.json" if a.band else "prob_kernel_stats.json"
        summarize(a.summarize, os.path.join(ROOT, "profiles", name), a.band)
        return
    for name, kind, shape in CASES:
        if a.only and name not in a.only:
            continue
        import torch
        args = _inputs(kind, shape)
        if a.once:
            _call(kind, args)
            torch.cuda.synchronize()
            print(name, "ran once", flush=True)
            continue
        _call(kind, args)                                   # warm-up: code objects, allocator
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(a.reps):
            r = _call(kind, args)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t) / a.reps * 1e3
        evals = _evaluations(kind, shape)
        line = {"case": name, "kind": kind, "shape": list(shape), "ms_per_call": round(ms, 3), "reps": a.reps,
                "evaluations": evals, "evaluations_per_s": evals / (ms * 1e-3), "finite": bool(np.isfinite(r).all()),
                "device": torch.cuda.get_device_name(0)}
        print(json.dumps(line), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(a.out), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
