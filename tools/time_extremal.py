#!/usr/bin/env python3
"""Extremal depth (K15) timings, every curve a target, next to the K14 call that shares its first stage, in the same run:

  sd_extremal_counts   n x T = 10 000 x 1 000 (image route), 14 000 x 1 000 (image and sort route), 100 000 x 256 (sort route),
                       continuous normal data; and 10 000 x 1 000 (image route) with 1 % of the curves duplicated and with the
                       values rounded to 0.1 -- the inputs on which heads tie and the tails are walked
  sd_rank_depth_sums   the same shapes and routes on the continuous data (stage 1 and a fold: what stages 2 - 4 add to)

Device time of the C entry point alone: data, result and workspace resident on the device, no copy inside the window.
A window is --inner calls enqueued back to back between two HIP events on the current stream (tools/time_rank_depths.py
says why); the figure is the window over --inner.  Per case: --warmup calls, then --reps windows; median, minimum and
maximum in ms per call.  A case whose warm-up call takes more than 1 / --inner of a quarter second gets shorter windows,
and says so in its line ("inner").  One JSON line per case.

    python tools/time_extremal.py [--reps 9] [--inner 20] [--warmup 2] [--only NAME ...] [--once]

--once runs each selected case --warmup + 1 times without timing (for a kernel trace: the split between stage 1's kernels,
ex_transform_kernel, ex_sort_kernel and ex_rank_kernel)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from statdepth_amd import engine  # noqa: E402
from statdepth_amd._native import check  # noqa: E402

# (case, entry point, n, T, algo, data)
CASES = [("extremal_image_n10000_T1000", "extremal", 10000, 1000, 1, "normal"),
         ("rank_depth_image_n10000_T1000", "rank_depth", 10000, 1000, 1, "normal"),
         ("extremal_image_n14000_T1000", "extremal", 14000, 1000, 1, "normal"),
         ("rank_depth_image_n14000_T1000", "rank_depth", 14000, 1000, 1, "normal"),
         ("extremal_sort_n14000_T1000", "extremal", 14000, 1000, 2, "normal"),
         ("rank_depth_sort_n14000_T1000", "rank_depth", 14000, 1000, 2, "normal"),
         ("extremal_sort_n100000_T256", "extremal", 100000, 256, 2, "normal"),
         ("rank_depth_sort_n100000_T256", "rank_depth", 100000, 256, 2, "normal"),
         ("extremal_image_n10000_T1000_duplicated", "extremal", 10000, 1000, 1, "duplicated"),
         ("extremal_image_n10000_T1000_tenths", "extremal", 10000, 1000, 1, "tenths")]


def _data(n, T, kind):
    rng = np.random.default_rng(n + T)
    X = rng.normal(size=(T, n))                                       # time-major
    if kind == "duplicated":                                          # 1 % of the curves are copies of others
        k = n // 100
        X[:, n - k:] = X[:, :k]
    elif kind == "tenths":
        X = np.round(X, 1)
    return X


def _call(kind, n, T, algo, data, dev):
    """A function of no arguments that enqueues the entry point once, everything it touches already on the device."""
    lib = engine._lib()
    stream = lambda: engine._stream_ptr(dev)                         # noqa: E731
    X = torch.from_numpy(_data(n, T, data)).to(dev)
    size, fn, width = {"extremal": (lib.sd_extremal_workspace_bytes, lib.sd_extremal_counts, 1),
                       "rank_depth": (lib.sd_rank_depth_workspace_bytes, lib.sd_rank_depth_sums, 5)}[kind]
    out = torch.empty((n, width), dtype=torch.int64, device=dev)
    nbytes = int(size(T, n, n, 1, n, algo))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    return lambda: check(fn(X.data_ptr(), T, n, n, 1, 0, n, algo, out.data_ptr(), ws.data_ptr(), nbytes, stream())), (X, out, ws)


def _window(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def run(name, kind, n, T, algo, data, reps, inner, warmup, once):
    dev = torch.device("cuda", torch.cuda.current_device())
    fn, keep = _call(kind, n, T, algo, data, dev)
    res = {"case": name, "entry": {"extremal": "sd_extremal_counts", "rank_depth": "sd_rank_depth_sums"}[kind], "n": n, "T": T,
           "route": {1: "image", 2: "sort"}[algo], "data": data}
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    if once:
        fn()
        torch.cuda.synchronize()
        return res
    inner = max(1, min(inner, int(250.0 / max(_window(fn, 1), 1e-3))))
    times = [_window(fn, inner) for _ in range(reps)]
    res.update(ms_median=round(statistics.median(times), 4), ms_min=round(min(times), 4), ms_max=round(max(times), 4),
               reps=reps, inner=inner, warmup=warmup)
    del keep
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    torch.cuda.init()
    for name, kind, n, T, algo, data in CASES:
        if a.only and name not in a.only:
            continue
        print(json.dumps(run(name, kind, n, T, algo, data, a.reps, a.inner, a.warmup, a.once)), flush=True)


if __name__ == "__main__":
    main()
