#!/usr/bin/env python3
"""Integrated rank depths (K14) timings, every curve a target, next to their yardsticks in the same run:

  sd_rank_depth_sums   n x T = 10 000 x 1 000 (image route), 14 000 x 1 000 (image and sort route), 100 000 x 256 (sort route)
  sd_mbd_counts        J = 2, the same three shapes (the image route's yardstick: the same rank kernel, folded in registers)
  sd_halfspace_counts  10^5 points in R^3, k = 256 directions (the sort route's yardstick: the same sort of 256 rows of 10^5)

Device time of the C entry point alone: data, result and workspace resident on the device, no copy inside the window.
A window is --inner calls enqueued back to back between two HIP events on the current stream, so that the host's enqueue
latency in front of the first kernel (the stream is idle when a window opens) is spread over the window instead of
sitting inside one call of 0.05 - 0.1 ms; the figure is the window over --inner.  Per case: --warmup calls, then --reps
windows; median, minimum and maximum in ms per call.  One JSON line per case.

    python tools/time_rank_depths.py [--reps 9] [--inner 20] [--warmup 2] [--only NAME ...] [--once]

--once runs each selected case once without timing (for a kernel trace: the split between the rank or sort kernels and
rank_depth_fold_kernel)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from statdepth_amd import engine, _native  # noqa: E402
from statdepth_amd._native import check  # noqa: E402
if os.environ.get("SD_LIB"):                     # experiments: another build of the library (this tool only; the cross-check
    _native.LIB_PATH = os.path.abspath(os.environ["SD_LIB"])      # build too, which the package itself refuses to load)
    _native._LIB = _native.open_library(_native.LIB_PATH)
from statdepth_amd.depth.calculations._pointcloud import _halfspace_directions  # noqa: E402

# (case, entry point, n, T or k, algo)
CASES = [("rank_depth_image_n10000_T1000", "rank_depth", 10000, 1000, 1), ("mbd_n10000_T1000", "mbd", 10000, 1000, 0),
         ("rank_depth_image_n14000_T1000", "rank_depth", 14000, 1000, 1), ("rank_depth_sort_n14000_T1000", "rank_depth", 14000, 1000, 2),
         ("mbd_n14000_T1000", "mbd", 14000, 1000, 0),
         ("rank_depth_sort_n100000_T256", "rank_depth", 100000, 256, 2), ("mbd_n100000_T256", "mbd", 100000, 256, 0),
         ("halfspace_n100000_d3_k256", "halfspace", 100000, 256, 0)]


def _call(kind, n, T, algo, dev):
    """A function of no arguments that enqueues the entry point once, everything it touches already on the device."""
    lib = engine._lib()
    rng = np.random.default_rng(n + T)
    stream = lambda: engine._stream_ptr(dev)                         # noqa: E731
    if kind == "halfspace":
        P = torch.from_numpy(rng.normal(size=(n, 3))).to(dev)
        U = torch.from_numpy(_halfspace_directions(T, 0, 3)).to(dev)
        out = torch.empty(n, dtype=torch.int64, device=dev)
        nbytes = int(lib.sd_halfspace_workspace_bytes(n, 3, T))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        return lambda: check(lib.sd_halfspace_counts(P.data_ptr(), n, 3, U.data_ptr(), T, 0, n, out.data_ptr(), ws.data_ptr(),
                                                     nbytes, stream())), (P, U, out, ws)
    X = torch.from_numpy(rng.normal(size=(T, n))).to(dev)            # time-major, continuous
    if kind == "mbd":
        out = torch.empty((n, 1), dtype=torch.int64, device=dev)
        nbytes = int(lib.sd_mbd_workspace_bytes(T, n, n, 1, n, 2, algo))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        return lambda: check(lib.sd_mbd_counts(X.data_ptr(), T, n, n, 1, 0, n, 2, algo, out.data_ptr(), ws.data_ptr(), nbytes,
                                               stream())), (X, out, ws)
    out = torch.empty((n, 5), dtype=torch.int64, device=dev)
    nbytes = int(lib.sd_rank_depth_workspace_bytes(T, n, n, 1, n, algo))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    return lambda: check(lib.sd_rank_depth_sums(X.data_ptr(), T, n, n, 1, 0, n, algo, out.data_ptr(), ws.data_ptr(), nbytes,
                                                stream())), (X, out, ws)


def run(name, kind, n, T, algo, reps, inner, warmup, once):
    dev = torch.device("cuda", torch.cuda.current_device())
    fn, keep = _call(kind, n, T, algo, dev)
    res = {"case": name, "entry": {"rank_depth": "sd_rank_depth_sums", "mbd": "sd_mbd_counts",
                                   "halfspace": "sd_halfspace_counts"}[kind], "n": n}
    res["k" if kind == "halfspace" else "T"] = T
    if kind == "rank_depth":
        res["route"] = {1: "image", 2: "sort"}[algo]
    if once:
        fn()
        torch.cuda.synchronize()
        return res
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / inner)
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
    for name, kind, n, T, algo in CASES:
        if a.only and name not in a.only:
            continue
        print(json.dumps(run(name, kind, n, T, algo, a.reps, a.inner, a.warmup, a.once)), flush=True)


if __name__ == "__main__":
    main()
