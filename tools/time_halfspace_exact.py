#!/usr/bin/env python3
"""Exact halfspace depth in the plane (K11) timings: the sweep against the pairwise kernel with every point a target at
n = 64, 256, 1 024, 4 096, 8 192; the tie-heavy 64 x 32 integer grid (n = 2 048, every point a target, where the
predicate's equal-products branch is hot); 100 external targets against 8 192 points; the K = 10 estimator at
n = 2 000 -- its 400 000 blocks in one sd_halfspace2_subset_counts call, and the whole PointcloudDepth(K=10) call with
its draws on the host.  Per case: the median over --reps calls after one warm-up call, each call ending in a device
synchronise, data resident on the device.  The PointcloudDepth case is timed once after a one-target warm-up: the
host's 400 000 `Series.sample` draws take tens of seconds.

    python tools/time_halfspace_exact.py [--reps 5] [--only NAME ...] [--out profiles/halfspace_exact_times.txt]

The parent process never touches the GPU: every case runs in a child of its own (`--case NAME`) under a time limit of its
own, and the first case that fails, dies or runs out of time ends the run.  The table goes to --out, one JSON line per
case to stdout."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (64, 256, 1024, 4096, 8192)
# name -> (kind, n, algo, time limit of the child in seconds)
CASES = {}
for _n in SIZES:
    CASES[f"all_n{_n}_sweep"] = ("all", _n, "sweep", 120)
    CASES[f"all_n{_n}_pairwise"] = ("all", _n, "pairwise", 240)
CASES["ties_n2048_sweep"] = ("ties", 2048, "sweep", 120)
CASES["ties_n2048_pairwise"] = ("ties", 2048, "pairwise", 120)
CASES["external_m100_n8192_sweep"] = ("external", 8192, "sweep", 120)
CASES["external_m100_n8192_pairwise"] = ("external", 8192, "pairwise", 120)
CASES["blocks_K10_n2000"] = ("blocks", 2000, "auto", 120)
CASES["sampled_K10_n2000"] = ("sampled", 2000, "auto", 300)


def _median_ms(fn, sync, reps):
    fn()
    sync()
    times = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        sync()
        times.append((time.perf_counter() - t) * 1e3)
    return statistics.median(times), min(times), max(times)


def run_case(name, reps):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from statdepth_amd import engine
    kind, n, algo, _ = CASES[name]
    torch.cuda.init()
    dev = torch.device("cuda", torch.cuda.current_device())
    rng = np.random.default_rng(n)
    Ph = rng.normal(size=(n, 2))
    P = torch.from_numpy(Ph).to(dev)
    res = {"case": name, "kind": kind, "n": n, "algo": algo}
    if kind == "all":
        fn = lambda: engine.halfspace_exact_counts(P, algo=algo)            # noqa: E731
        res["targets"] = n
    elif kind == "ties":                        # the 64 x 32 integer grid: collinear pairs and zero products throughout
        G = torch.from_numpy(np.stack(np.meshgrid(np.arange(64.0), np.arange(32.0)), axis=-1).reshape(n, 2)).to(dev)
        fn = lambda: engine.halfspace_exact_counts(G, algo=algo)            # noqa: E731
        res["targets"] = n
    elif kind == "external":
        Q = torch.from_numpy(rng.normal(size=(100, 2))).to(dev)
        fn = lambda: engine.halfspace_exact_external_counts(P, Q, algo=algo)   # noqa: E731
        res["targets"] = 100
    elif kind == "blocks":                      # the estimator's shape: per target n // K blocks of n // K draws + the target
        ss = n // 10
        mem = rng.integers(0, n, size=(n * ss, ss + 1)).astype(np.int32)     # (drawn with replacement: timing only)
        mem[:, -1] = np.repeat(np.arange(n), ss)
        fn = lambda: engine.halfspace_exact_subset_counts(P, mem, algo=algo)   # noqa: E731
        res["targets"], res["blocks"], res["block_size"] = n, n * ss, ss + 1
    else:
        import pandas as pd
        from statdepth_amd import PointcloudDepth
        df = pd.DataFrame(Ph)
        np.random.seed(0)
        PointcloudDepth(df, to_compute=[0], K=10, containment='halfspace', directions='exact')
        t = time.perf_counter()
        PointcloudDepth(df, K=10, containment='halfspace', directions='exact')
        torch.cuda.synchronize()
        res["ms_median"] = res["ms_min"] = res["ms_max"] = (time.perf_counter() - t) * 1e3
        res["targets"], res["blocks"], res["reps"] = n, n * (n // 10), 1
        print(json.dumps(res), flush=True)
        return
    res["ms_median"], res["ms_min"], res["ms_max"] = _median_ms(fn, torch.cuda.synchronize, reps)
    res["reps"] = reps
    print(json.dumps(res), flush=True)


def table(rows):
    by = {r["case"]: r for r in rows}
    ms = lambda name: f"{by[name]['ms_median']:.3f}" if name in by else "-"     # noqa: E731
    lines = ["exact halfspace depth in the plane (K11), one MI355X, median ms per call (tools/time_halfspace_exact.py)",
             "", "every point a target", f"{'n':>6} {'sweep':>12} {'pairwise':>12} {'pairwise/sweep':>15}"]
    for n in SIZES:
        s, p = by.get(f"all_n{n}_sweep"), by.get(f"all_n{n}_pairwise")
        ratio = f"{p['ms_median'] / s['ms_median']:.2f}" if s and p else "-"
        lines.append(f"{n:>6} {ms(f'all_n{n}_sweep'):>12} {ms(f'all_n{n}_pairwise'):>12} {ratio:>15}")
    lines += ["", f"tie-heavy: the 64 x 32 integer grid, every point a target: sweep {ms('ties_n2048_sweep')}, "
                  f"pairwise {ms('ties_n2048_pairwise')}"]
    lines += ["", f"100 external targets against 8192 points: sweep {ms('external_m100_n8192_sweep')}, "
                  f"pairwise {ms('external_m100_n8192_pairwise')}",
              f"K = 10 estimator at n = 2000: its 400 000 blocks of 201 points in one subset call {ms('blocks_K10_n2000')}; "
              f"PointcloudDepth(K=10), host draws included, one call {ms('sampled_K10_n2000')}", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "halfspace_exact_times.txt"))
    ap.add_argument("--case", default=None, help="(internal) run one case in this process")
    a = ap.parse_args()
    if a.case:
        run_case(a.case, a.reps)
        return 0
    rows = []
    for name, (_, _, _, limit) in CASES.items():
        if a.only and name not in a.only:
            continue
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--case", name,
               "--reps", str(a.reps)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if p.returncode != 0:                                         # a fault, an abort or the time limit: nothing more runs
            print(f"{name}: exit status {p.returncode}; stopping", file=sys.stderr)
            return p.returncode
        rows.append(json.loads(p.stdout.strip().splitlines()[-1]))
    text = table(rows)
    print(text)
    if not a.only:
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
