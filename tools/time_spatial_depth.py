#!/usr/bin/env python3
"""Functional spatial depth (K21) timings, every curve a target, next to its yardstick on the same tensor in the same
process:

  sd_spatial_sums          weights (pass 1), sums (pass 2) and fold, without the field
  sd_curve_sqdist          all n x n squared distances: the yardstick -- pass 2 executes the same operation count
  sd_hmodal_sums           at 100 000 x 256, where no n x n matrix is stored: the fused distance pass
  FunctionalDepth          the whole containment='spatial' call on a host DataFrame (upload, sums, host formula; wall clock)

at n x T = 4 096 x 256, 10 000 x 1 000, 14 000 x 1 000 and 100 000 x 256.  "peak_share" counts 2 vector operations per
pair-timepoint and pass (sd_spatial_sums: two passes) against 39.3e12 fp64 vector operations a second (256 CUs x 4 SIMDs x
16 lanes a cycle x 2.4 GHz).

Device time of the C entry point alone: data, result and workspace resident on the device, no copy inside the window.  A
window is `inner` calls enqueued back to back between two HIP events on the current stream; the figure is the window over
`inner`.  `inner` follows from one timed call: as many as fit a quarter of a second, at most --inner.  Per line: --warmup
calls, then --reps windows; median, minimum and maximum in ms per call.  One JSON line per measurement.

    python tools/time_spatial_depth.py [--reps 7] [--inner 20] [--warmup 2] [--only SHAPE ...] [--limit 300] [--kernels DIR]

--kernels DIR gives the split per kernel instead: every shape runs once more under `rocprofv3 --kernel-trace --stats` (a
run of its own: tracing slows the host, its numbers are kernel times only), sd_spatial_sums and its yardstick alone, and
the statistics are read back: pass 1 (cd_tile_kernel<3>), pass 2 (sp_sum_kernel), the fold (sp_fold_kernel) and the
yardstick's kernel in ms per call, and pass 2 as a multiple of the yardstick.

Every shape runs in a child process of its own under --limit seconds; the first that fails or runs out of time ends the run,
and nothing more is started on the device."""
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

SHAPES = {"n4096_T256": (4096, 256, True), "n10000_T1000": (10000, 1000, True), "n14000_T1000": (14000, 1000, True),
          "n100000_T256": (100000, 256, False)}                      # (n, T, the yardstick is sd_curve_sqdist; else sd_hmodal_sums)
PEAK_OPS = 39.3e12
KERNEL_CALLS = 3                                                     # calls of each entry point under the profiler
KERNELS = {"pass1_weights": "cd_tile_kernel<3>", "pass2_sums": "sp_sum_kernel", "fold": "sp_fold_kernel",
           "yardstick_sqdist": "cd_tile_kernel<0>", "yardstick_hmodal": "cd_tile_kernel<1>"}


def timed(fn, reps, inner, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    inner = max(1, min(inner, int(250.0 / max(a.elapsed_time(b), 1e-3))))
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / inner)
    return dict(ms_median=round(statistics.median(times), 4), ms_min=round(min(times), 4), ms_max=round(max(times), 4),
                reps=reps, inner=inner, warmup=warmup)


def run(shape, reps, inner, warmup, kernels_only):
    import pandas as pd
    import torch
    from statdepth_amd import FunctionalDepth, engine
    from statdepth_amd._native import check
    n, T, square = SHAPES[shape]
    torch.cuda.init()
    dev = torch.device("cuda", torch.cuda.current_device())
    lib = engine._lib()
    stream = lambda: engine._stream_ptr(dev)                         # noqa: E731
    Xh = np.random.default_rng(n + T).normal(size=(T, n))
    X = torch.from_numpy(Xh).to(dev)                                 # time-major, continuous

    def emit(case, entry, res, **more):
        print(json.dumps({"case": f"{case}_{shape}", "entry": entry, "n": n, "T": T, **res, **more}), flush=True)

    def share(res, passes):
        return {"peak_share": round(passes * 2.0 * n * n * T / (res["ms_median"] * 1e-3) / PEAK_OPS, 3)}

    def measure(fn):
        if not kernels_only:
            return timed(fn, reps, inner, warmup)
        for _ in range(KERNEL_CALLS):
            fn()
        torch.cuda.synchronize()
        return None

    S = torch.empty(n, dtype=torch.float64, device=dev)
    nbytes = int(lib.sd_spatial_workspace_bytes(T, n, n, 1, n))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    res = measure(lambda: check(lib.sd_spatial_sums(X.data_ptr(), T, n, n, 1, 0, n, S.data_ptr(), None, ws.data_ptr(), nbytes, stream())))
    if res:
        emit("spatial", "sd_spatial_sums", res, **share(res, 2), workspace_bytes=nbytes,
             targets_per_batch=int(lib.sd_spatial_targets_per_batch(T, n, n, 1, n, nbytes)))
    spatial_ms = res["ms_median"] if res else None
    del ws
    torch.cuda.empty_cache()
    if square:
        out = torch.empty((n, n), dtype=torch.float64, device=dev)
        res = measure(lambda: check(lib.sd_curve_sqdist(X.data_ptr(), T, n, n, 1, 0, n, out.data_ptr(), None, 0, stream())))
        entry = "sd_curve_sqdist"
        del out
    else:
        nbytes = int(lib.sd_curve_sqdist_workspace_bytes(T, n, n, 1, n, 1))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        g = 1.0 / (2.0 * T)
        res = measure(lambda: check(lib.sd_hmodal_sums(X.data_ptr(), T, n, n, 1, 0, n, g, S.data_ptr(), ws.data_ptr(), nbytes, stream())))
        entry = "sd_hmodal_sums"
        del ws
    if res:
        emit("yardstick", entry, res, **share(res, 1), spatial_over_yardstick=round(spatial_ms / res["ms_median"], 3))
    if kernels_only:
        return
    torch.cuda.empty_cache()
    df = pd.DataFrame(Xh)
    walls = []
    for _ in range(3):
        t0 = time.perf_counter()
        d = FunctionalDepth([df], containment="spatial")
        walls.append((time.perf_counter() - t0) * 1e3)
    emit("functional_depth", "FunctionalDepth(containment='spatial')", {"wall_ms_min": round(min(walls), 2),
                                                                       "wall_ms_first": round(walls[0], 2)},
         depth_min=float(d.min()), depth_max=float(d.max()))


def kernel_stats(directory, shape):
    """The kernels of the calls from rocprofv3's statistics file under `directory`: launches and ms per call of the entry
    point, and pass 2 as a multiple of the yardstick's kernel."""
    found = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                kn = r.get("Name") or r.get("KernelName") or ""
                for key, sub in KERNELS.items():
                    if sub in kn:
                        total = float(r.get("TotalDurationNs") or r.get("TotalDuration(ns)") or 0.0)
                        found[key] = {"kernel": kn[:48], "launches": int(float(r.get("Calls") or 0)),
                                      "ms_per_call": round(total / 1e6 / KERNEL_CALLS, 4)}
    out = {"case": f"kernels_{shape}", "entry_calls_each": KERNEL_CALLS, **found}
    yard = found.get("yardstick_sqdist") or found.get("yardstick_hmodal")
    if yard and "pass2_sums" in found:
        out["pass2_over_yardstick"] = round(found["pass2_sums"]["ms_per_call"] / yard["ms_per_call"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--limit", type=float, default=300.0, help="seconds a shape may take")
    ap.add_argument("--kernels", default=None, metavar="DIR", help="kernel times under rocprofv3, its files kept in DIR")
    ap.add_argument("--shape", default=None, help="run this one shape in this process (what the parent starts)")
    ap.add_argument("--kernels-only", action="store_true", help="with --shape: a few calls of each entry point, untimed")
    a = ap.parse_args()
    if a.shape:
        run(a.shape, a.reps, a.inner, a.warmup, a.kernels_only)
        return 0
    for shape in SHAPES:
        if a.only and shape not in a.only:
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--shape", shape, "--reps", str(a.reps), "--inner", str(a.inner),
               "--warmup", str(a.warmup)]
        if a.kernels:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.join(a.kernels, shape), "--"] + \
                  cmd + ["--kernels-only"]
        p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True)
        try:
            stdout, stderr = p.communicate(timeout=a.limit)
        except subprocess.TimeoutExpired:
            os.killpg(p.pid, signal.SIGKILL)                        # the child and whatever it started
            p.communicate()
            print(json.dumps({"shape": shape, "error": f"no result within {a.limit:g} s"}), flush=True)
            return 1
        if p.returncode != 0:
            print(json.dumps({"shape": shape, "error": f"exit status {p.returncode}", "stderr": stderr[-400:]}), flush=True)
            return 1
        if a.kernels:
            print(json.dumps(kernel_stats(os.path.join(a.kernels, shape), shape)), flush=True)
        else:
            sys.stdout.write(stdout)
            sys.stdout.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
