#!/usr/bin/env python3
"""Functional boxplot (K16, sd_central_regions) timings next to three yardsticks on the same device tensor, in the same run:

  shapes n x T         10 000 x 1 000 and 14 000 x 1 000 (row-resident route), 100 000 x 256 (column blocks); time-major
                       random walks, three curves scaled by 8, levels from a random depth, fractions 0.25 / 0.5 / 0.75, box = 1
  regions              sd_central_regions with box = -1: the envelopes of the three regions
  fence_counts         ... with the fence and the outside counts
  full                 ... and the whiskers (a second pass over X behind the counts)
  aminmax              torch.aminmax(X, dim=1): a general reduction that reads the same bytes once and does less (one
                       region, no levels, no fence, no counts)
  clone                X.clone(): reads and writes the bytes once
  rank_depth           sd_rank_depth_sums, the K14 call over the same matrix

Device time alone: data, results and workspace resident on the device, no copy inside the window.  A window is --inner calls
enqueued back to back between two HIP events on the current stream; the figure is the window over --inner.  Per case:
--warmup calls, then --reps windows; minimum and median in ms per call (the maximum shows the run-to-run spread).  One JSON
line per case, and per shape one line with the ratios to aminmax.

    python tools/time_boxplot.py [--reps 9] [--inner 20] [--warmup 2] [--only NAME ...]"""
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

SHAPES = [(10000, 1000), (14000, 1000), (100000, 256)]            # (n, T)
ALPHAS = (0.25, 0.5, 0.75)
KINDS = ("regions", "fence_counts", "full", "aminmax", "clone", "rank_depth")


def _data(n, T):
    rng = np.random.default_rng(n + T)
    X = rng.normal(size=(T, n)).cumsum(axis=0)                        # time-major
    X[:, rng.permutation(n)[:3]] *= 8
    depth = rng.random(n)
    rank = np.empty(n, dtype=np.int64)
    rank[np.argsort(-depth, kind="stable")] = np.arange(n)
    level = np.full(n, len(ALPHAS), dtype=np.uint8)
    for l in range(len(ALPHAS) - 1, -1, -1):
        level[rank < int(np.ceil(ALPHAS[l] * n))] = l
    return X, level


def _calls(n, T, dev):
    """{kind: function of no arguments that enqueues the call once}, everything it touches already on the device."""
    lib = engine._lib()
    stream = lambda: engine._stream_ptr(dev)                         # noqa: E731
    Xh, lh = _data(n, T)
    X, level = torch.from_numpy(Xh).to(dev), torch.from_numpy(lh).to(dev)
    L = len(ALPHAS)
    env = torch.empty((L, 2, T), dtype=torch.float64, device=dev)
    fence, whisker = (torch.empty((2, T), dtype=torch.float64, device=dev) for _ in range(2))
    outside = torch.empty((n, 2), dtype=torch.int32, device=dev)
    nbytes = int(lib.sd_central_regions_workspace_bytes(T, n, n, 1, L))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def regions(box, f, o, w):
        return lambda: check(lib.sd_central_regions(X.data_ptr(), T, n, n, 1, level.data_ptr(), L, box, 1.5, env.data_ptr(), f, o, w,
                                                    ws.data_ptr(), nbytes, stream()))
    rd = torch.empty((n, 5), dtype=torch.int64, device=dev)
    rbytes = int(lib.sd_rank_depth_workspace_bytes(T, n, n, 1, n, 0))
    rws = torch.empty(rbytes, dtype=torch.uint8, device=dev)
    keep = (X, level, env, fence, whisker, outside, ws, rd, rws)
    return {"regions": regions(-1, None, None, None),
            "fence_counts": regions(1, fence.data_ptr(), outside.data_ptr(), None),
            "full": regions(1, fence.data_ptr(), outside.data_ptr(), whisker.data_ptr()),
            "aminmax": lambda: torch.aminmax(X, dim=1),
            "clone": lambda: X.clone(),
            "rank_depth": lambda: check(lib.sd_rank_depth_sums(X.data_ptr(), T, n, n, 1, 0, n, 0, rd.data_ptr(), rws.data_ptr(),
                                                               rbytes, stream()))}, keep


def _window(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", nargs="*", default=None)
    a = ap.parse_args()
    torch.cuda.init()
    dev = torch.device("cuda", torch.cuda.current_device())
    for n, T in SHAPES:
        calls, keep = _calls(n, T, dev)
        med = {}
        for kind in KINDS:
            name = f"{kind}_n{n}_T{T}"
            if a.only and name not in a.only and kind not in a.only:
                continue
            fn = calls[kind]
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            inner = max(1, min(a.inner, int(250.0 / max(_window(fn, 1), 1e-3))))
            times = [_window(fn, inner) for _ in range(a.reps)]
            med[kind] = statistics.median(times)
            print(json.dumps({"case": name, "n": n, "T": T, "route": "row-resident" if n <= engine.central_regions_row_capacity()
                              else "column blocks", "mbytes": round(8e-6 * n * T, 1), "ms_min": round(min(times), 4),
                              "ms_median": round(med[kind], 4), "ms_max": round(max(times), 4), "reps": a.reps, "inner": inner,
                              "warmup": a.warmup}), flush=True)
        if "aminmax" in med:
            print(json.dumps({"case": f"ratios_n{n}_T{T}", "to": "aminmax (medians)",
                              **{k: round(v / med["aminmax"], 2) for k, v in med.items() if k != "aminmax"}}), flush=True)
        del calls, keep


if __name__ == "__main__":
    main()
