#!/usr/bin/env python3
"""Exact simplicial depth in the plane (K13) timings: the sweep and the pairwise kernel with every point a target at
n = 1 024, 4 096, 8 192, and K11's sweep (exact halfspace depth: the same compaction, sort and flag prefix) at the same
shapes in the same run; the tie-heavy 64 x 32 integer grid (n = 2 048, every point a target, where the predicate's
equal-products branch is hot); 100 external targets against 8 192 points; K4's enumeration of all C(n - 1, 3) triangles per
target at n = 256 (or the largest of 256, 128, 64 it finishes within a second).  Per case: the median over --reps calls
after one warm-up call, each call ending in a device synchronise, data resident on the device.

    python tools/time_simplicial_exact.py [--reps 5] [--only NAME ...] [--out profiles/simplicial_exact_times.txt]

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
SIZES = (1024, 4096, 8192)
K4_SIZES = (256, 128, 64)
# name -> (kind, n, algo, time limit of the child in seconds)
CASES = {}
for _n in SIZES:
    CASES[f"all_n{_n}_sweep"] = ("all", _n, "sweep", 120)
    CASES[f"all_n{_n}_pairwise"] = ("all", _n, "pairwise", 240)
    CASES[f"all_n{_n}_k11sweep"] = ("k11", _n, "sweep", 120)
CASES["ties_n2048_sweep"] = ("ties", 2048, "sweep", 120)
CASES["ties_n2048_pairwise"] = ("ties", 2048, "pairwise", 120)
CASES["external_m100_n8192_sweep"] = ("external", 8192, "sweep", 120)
CASES["external_m100_n8192_pairwise"] = ("external", 8192, "pairwise", 120)
CASES["external_m100_n8192_k11sweep"] = ("k11external", 8192, "sweep", 120)
CASES["k4_enumeration"] = ("k4", K4_SIZES[0], "enumeration", 240)


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
    res = {"case": name, "kind": kind, "algo": algo}
    if kind == "k4":                            # the largest size whose call stays within a second
        for n in K4_SIZES:
            P = torch.from_numpy(np.random.default_rng(n).normal(size=(n, 2))).to(dev)
            ms = _median_ms(lambda: engine.pointcloud_simplex_counts(P), torch.cuda.synchronize, reps)
            if ms[0] <= 1000.0 or n == K4_SIZES[-1]:
                break
        res.update(n=n, targets=n, ms_median=ms[0], ms_min=ms[1], ms_max=ms[2], reps=reps)
        print(json.dumps(res), flush=True)
        return
    rng = np.random.default_rng(n)
    P = torch.from_numpy(rng.normal(size=(n, 2))).to(dev)
    Q = torch.from_numpy(rng.normal(size=(100, 2))).to(dev)
    res["n"] = n
    if kind == "all":
        fn = lambda: engine.simplicial_exact_counts(P, algo=algo)           # noqa: E731
        res["targets"] = n
    elif kind == "ties":                        # the 64 x 32 integer grid: collinear pairs and zero products throughout
        G = torch.from_numpy(np.stack(np.meshgrid(np.arange(64.0), np.arange(32.0)), axis=-1).reshape(n, 2)).to(dev)
        fn = lambda: engine.simplicial_exact_counts(G, algo=algo)           # noqa: E731
        res["targets"] = n
    elif kind == "k11":
        fn = lambda: engine.halfspace_exact_counts(P, algo=algo)            # noqa: E731
        res["targets"] = n
    elif kind == "external":
        fn = lambda: engine.simplicial_exact_external_counts(P, Q, algo=algo)   # noqa: E731
        res["targets"] = 100
    else:
        fn = lambda: engine.halfspace_exact_external_counts(P, Q, algo=algo)    # noqa: E731
        res["targets"] = 100
    res["ms_median"], res["ms_min"], res["ms_max"] = _median_ms(fn, torch.cuda.synchronize, reps)
    res["reps"] = reps
    print(json.dumps(res), flush=True)


def table(rows):
    by = {r["case"]: r for r in rows}
    ms = lambda name: f"{by[name]['ms_median']:.3f}" if name in by else "-"     # noqa: E731
    lines = ["exact simplicial depth in the plane (K13), one MI355X, median ms per call (tools/time_simplicial_exact.py)",
             "", "every point a target; K11 sweep = exact halfspace depth at the same shape in the same run",
             f"{'n':>6} {'sweep':>12} {'pairwise':>12} {'pairwise/sweep':>15} {'K11 sweep':>12} {'sweep/K11':>10}"]
    for n in SIZES:
        s, p, h = by.get(f"all_n{n}_sweep"), by.get(f"all_n{n}_pairwise"), by.get(f"all_n{n}_k11sweep")
        ps = f"{p['ms_median'] / s['ms_median']:.2f}" if s and p else "-"
        sh = f"{s['ms_median'] / h['ms_median']:.2f}" if s and h else "-"
        lines.append(f"{n:>6} {ms(f'all_n{n}_sweep'):>12} {ms(f'all_n{n}_pairwise'):>12} {ps:>15} "
                     f"{ms(f'all_n{n}_k11sweep'):>12} {sh:>10}")
    lines += ["", f"tie-heavy: the 64 x 32 integer grid, every point a target: sweep {ms('ties_n2048_sweep')}, "
                  f"pairwise {ms('ties_n2048_pairwise')}"]
    lines += ["", f"100 external targets against 8192 points: sweep {ms('external_m100_n8192_sweep')}, "
                  f"pairwise {ms('external_m100_n8192_pairwise')}, K11 sweep {ms('external_m100_n8192_k11sweep')}"]
    k4 = by.get("k4_enumeration")
    if k4:
        lines.append(f"K4 enumeration (containment='simplex'), every point a target at n = {k4['n']}: "
                     f"{k4['ms_median']:.3f}")
    lines.append("")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simplicial_exact_times.txt"))
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
