#!/usr/bin/env python3
"""Directional outlyingness of multivariate curves (K19) timings, every curve a target, algo 0 (auto: the LDS route up to
8 192 curves, the global route above):

  projection           sd_multi_projection_sums, the yardstick: K18's call on the same inputs (the project-sort-select stage
                       that both calls share, plus K18's fold)
  moments              sd_multi_outlyingness_moments, records only (centres and curves NULL)
  curves               sd_multi_outlyingness_moments with the centres and the m x T x d curves written as well
  loop                 a host baseline at the smallest shape (--loop-shape): engine.projection_outlyingness on P[:, t, :]
                       once per timepoint from Python, the centre and the Welford step in numpy over all curves

at n x T x d = 5 000 x 500 x 8, 1 000 x 1 000 x 3 and 10 000 x 100 x 3, k = 1 000 and k = 64 directions.

Within one case the variants alternate: --reps rounds of (projection, moments, curves[, loop]), so a drift of the device
shows in all of them.  The three entry points are device time of the C call alone, between two HIP events on the current
stream: data, result and workspace (recommended size) resident on the device, no copy inside the window.  "loop" is wall time
from host arrays to host results, synchronised at both ends.  Per variant: --warmup calls first, then the rounds; median,
minimum and maximum in ms per call, and extra = moments - projection of the medians.  One JSON line per case.

    python tools/time_directional.py [--reps 5] [--warmup 2] [--only NAME ...] [--limit 300]

Every case runs in a child process of its own, in a process group of its own, under --limit seconds; the first case that
fails or runs out of time ends the run: the whole group is killed (under --kernels the child is the tracer and the case
runs below it), and nothing more is started on the device.

    python tools/time_directional.py --kernels DIR [--only NAME ...]

runs each case once more under `rocprofv3 --kernel-trace --stats` (a run of its own: tracing slows the host, its numbers
are kernel times and nothing else), KERNEL_WARMUP = 1 warm-up and KERNEL_REPS = 3 calls of projection and of moments, and prints per case the kernels of
the two calls from the statistics file: launches, total and mean time.  The centre kernel and the moments fold on their own
are do_centre_kernel and do_moments_kernel there; the copy and K18's fold are to_time_major_kernel and mc_fold_kernel."""
import argparse
import csv
import glob
import json
import os
import signal
import statistics
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(5000, 500, 8), (1000, 1000, 3), (10000, 100, 3)]
LOOP_SHAPE = (10000, 100, 3)                                         # the fewest timepoints: the loop pays per timepoint
CASES = [(f"n{n}_T{T}_d{d}_k{k}", n, T, d, k) for (n, T, d) in SHAPES for k in (1000, 64)]
KERNEL_REPS, KERNEL_WARMUP = 3, 1                                   # --kernels: calls of each entry point under the tracer
KERNELS = ("do_centre", "do_moments", "mc_fold", "mc_lds", "mc_gather", "time_major", "pd_", "hs_")


def _directions(k, d, seed=0):
    U = np.random.default_rng(seed).standard_normal((k, d))
    return U / np.linalg.norm(U, axis=1, keepdims=True)


def host_loop(engine, P, U):
    """What a user could do before: K12 per timepoint on the device, the centre and the Welford step in numpy."""
    n, T, d = P.shape
    M, Q = np.zeros((n, d)), np.zeros(n)
    with np.errstate(divide="ignore", invalid="ignore"):
        for t in range(T):
            o = engine.projection_outlyingness(P[:, t, :], U)
            diff = P[:, t, :] - P[int(np.argmin(o)), t, :]
            r = np.sqrt((diff * diff).sum(axis=1))
            O = np.where(r[:, None] == 0.0, 0.0, o[:, None] * (diff / r[:, None]))
            delta = O - M
            M = M + delta / (t + 1.0)
            Q = Q + (delta * (O - M)).sum(axis=1)
    return M, Q


def run(name, n, T, d, k, reps, warmup, kernels_only=False):
    import torch
    from statdepth_amd import engine
    from statdepth_amd._native import check
    torch.cuda.init()
    dev = torch.device("cuda", torch.cuda.current_device())
    lib = engine._lib()
    P = np.random.default_rng(n + T + d).normal(size=(n, T, d))
    U = _directions(k, d)
    Pd, Ud = torch.from_numpy(P).to(dev), torch.from_numpy(U).to(dev)
    out2 = torch.empty((n, 2), dtype=torch.float64, device=dev)
    out = torch.empty((n, d + 1), dtype=torch.float64, device=dev)
    cen = torch.empty(T, dtype=torch.int64, device=dev)
    nbytes = max(int(lib.sd_multi_outlyingness_workspace_bytes(n, T, d, k, n, 0)),
                 int(lib.sd_multi_projection_workspace_bytes(n, T, d, k, n, 0)))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    stream = engine._stream_ptr(dev)

    def timed(launch):
        def call():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            check(launch())
            b.record()
            b.synchronize()
            return a.elapsed_time(b)
        return call

    def moments(centres, curves):
        return lambda: lib.sd_multi_outlyingness_moments(Pd.data_ptr(), n, T, d, Ud.data_ptr(), k, None, n, 0, out.data_ptr(),
                                                         centres, curves, ws.data_ptr(), nbytes, stream)
    variants = {"projection": timed(lambda: lib.sd_multi_projection_sums(Pd.data_ptr(), n, T, d, Ud.data_ptr(), k, None, n, 0,
                                                                          out2.data_ptr(), ws.data_ptr(), nbytes, stream)),
                "moments": timed(moments(None, None))}
    if not kernels_only:
        cur = torch.empty((n, T, d), dtype=torch.float64, device=dev)
        variants["curves"] = timed(moments(cen.data_ptr(), cur.data_ptr()))
        if (n, T, d) == LOOP_SHAPE:
            def loop():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                host_loop(engine, P, U)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3
            variants["loop"] = loop
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    times = {v: [] for v in variants}
    for _ in range(reps):
        for v, fn in variants.items():
            times[v].append(fn())
    res = {"case": name, "n": n, "T": T, "d": d, "k": k, "reps": reps, "warmup": warmup}
    for v, ts in times.items():
        res[v] = {"ms_median": round(statistics.median(ts), 3), "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3)}
    res["extra_ms"] = round(res["moments"]["ms_median"] - res["projection"]["ms_median"], 3)
    return res


def kernel_stats(directory, name, calls):
    """The kernels of the two calls from rocprofv3's statistics file under `directory`: launches, total ms, mean us, and
    ms per call of an entry point (a kernel of the shared stage runs in both calls: 2 * calls entry calls)."""
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                kn = r.get("Name") or r.get("KernelName") or ""
                if any(s in kn for s in KERNELS):
                    total = float(r.get("TotalDurationNs") or r.get("TotalDuration(ns)") or 0.0)
                    launches = int(float(r.get("Calls") or 0))
                    own = any(s in kn for s in ("do_centre", "do_moments", "mc_fold"))
                    rows.append({"kernel": kn[:60], "launches": launches, "total_ms": round(total / 1e6, 3),
                                 "mean_us": round(total / 1e3 / max(launches, 1), 2),
                                 "ms_per_call": round(total / 1e6 / (calls if own else 2 * calls), 3)})
    return {"case": name, "entry_calls_each": calls, "kernels": sorted(rows, key=lambda r: -r["total_ms"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--limit", type=float, default=300.0, help="seconds a case may take")
    ap.add_argument("--kernels", default=None, metavar="DIR", help="kernel times under rocprofv3, its files kept in DIR")
    ap.add_argument("--case", default=None, help="run this one case in this process (what the parent starts)")
    ap.add_argument("--kernels-only", action="store_true", help="with --case: projection and moments alone")
    a = ap.parse_args()
    if a.case:
        name, n, T, d, k = next(c for c in CASES if c[0] == a.case)
        print(json.dumps(run(name, n, T, d, k, a.reps, a.warmup, a.kernels_only)), flush=True)
        return 0
    for name, *_ in CASES:
        if a.only and name not in a.only:
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(a.reps), "--warmup", str(a.warmup)]
        if a.kernels:
            out = os.path.join(a.kernels, name)
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--"] + cmd[:3] + \
                  [name, "--reps", str(KERNEL_REPS), "--warmup", str(KERNEL_WARMUP), "--kernels-only"]
        p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True)
        try:
            stdout, stderr = p.communicate(timeout=a.limit)
        except subprocess.TimeoutExpired:
            os.killpg(p.pid, signal.SIGKILL)                        # the child and whatever it started
            p.communicate()
            print(json.dumps({"case": name, "error": f"no result within {a.limit:g} s"}), flush=True)
            return 1
        if p.returncode != 0:
            print(json.dumps({"case": name, "error": f"exit status {p.returncode}", "stderr": stderr[-400:]}), flush=True)
            return 1
        if a.kernels:
            print(json.dumps(kernel_stats(os.path.join(a.kernels, name), name, KERNEL_REPS + KERNEL_WARMUP)), flush=True)
        else:
            print(stdout.strip().splitlines()[-1], flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
