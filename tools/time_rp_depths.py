#!/usr/bin/env python3
"""Random projection depths of curves (K23) timings, every curve a target, with the stages and the yardstick in the same run:

  sd_rp_depth_sums      the whole call: projection, K14's pair image and fold over the k rows of Z
  sd_rp_outlyingness    the whole call: projection, K10's row sort, K12's selection, the maximum per target
  sd_curve_projections  the projection kernel alone (Z = U X in the specified order, two rounded operations a term)
  sd_rank_depth_sums    on a k x n matrix alone: the stage that sd_rp_depth_sums feeds
  torch.matmul(U, X)    fp64, the comparison and not a target: FMA and a free summation order

at n x T = 10 000 x 1 000 and 14 000 x 1 000 with k = 1 000 and k = 64, and 100 000 x 256 with k = 256.

Device time of the call alone: data, result and workspace resident on the device, no copy inside the window.  A window is
--inner calls enqueued back to back between two HIP events on the current stream; the figure is the window over --inner.
Per case: --warmup calls, then --reps windows; median, minimum and maximum in ms per call.  peak_share of the projection:
2 T n k operations (a multiplication and an addition a term, by definition) over the time, against the fp64 vector issue
peak of 39.3e12 operations a second (256 CUs x 4 SIMDs x 16 lanes a cycle x 2.4 GHz), as K20 reports it.  One JSON line per
case, printed and written to --out.

    python tools/time_rp_depths.py [--reps 7] [--inner 10] [--warmup 2] [--only SHAPE ...] [--out profiles/rp_depth_times.txt]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from statdepth_amd import engine  # noqa: E402
from statdepth_amd._native import check  # noqa: E402
from statdepth_amd.depth.calculations._pointcloud import _halfspace_directions  # noqa: E402

FP64_VECTOR_PEAK = 256 * 4 * 16 * 2.4e9
# (n, T, k)
SHAPES = [(10000, 1000, 1000), (10000, 1000, 64), (14000, 1000, 1000), (14000, 1000, 64), (100000, 256, 256)]


def _calls(n, T, k, dev):
    """{case: function of no arguments that enqueues it once}, everything it touches already on the device."""
    lib = engine._lib()
    rng = np.random.default_rng(n + T + k)
    stream = lambda: engine._stream_ptr(dev)                          # noqa: E731
    X = torch.from_numpy(rng.normal(size=(T, n))).to(dev)             # time-major, continuous
    U = torch.from_numpy(_halfspace_directions(k, 0, T)).to(dev)
    Z = torch.empty((k, n), dtype=torch.float64, device=dev)
    rec = torch.empty((n, 5), dtype=torch.int64, device=dev)
    out = torch.empty(n, dtype=torch.float64, device=dev)
    sizes = {"rp_depth": int(lib.sd_rp_depth_workspace_bytes(T, n, n, 1, k, n, 0)),
             "rp_outlyingness": int(lib.sd_rp_outlyingness_workspace_bytes(T, n, n, 1, k, n)),
             "rank_depth": int(lib.sd_rank_depth_workspace_bytes(k, n, n, 1, n, 0))}
    ws = torch.empty(max(sizes.values()), dtype=torch.uint8, device=dev)
    head = (X.data_ptr(), T, n, n, 1, U.data_ptr(), k)
    check(lib.sd_curve_projections(*head, Z.data_ptr(), None, 0, stream()))      # the rank stage's input
    calls = {
        "sd_rp_depth_sums": lambda: check(lib.sd_rp_depth_sums(*head, 0, n, 0, rec.data_ptr(), ws.data_ptr(), sizes["rp_depth"],
                                                               stream())),
        "sd_rp_outlyingness": lambda: check(lib.sd_rp_outlyingness(*head, 0, n, out.data_ptr(), ws.data_ptr(),
                                                                   sizes["rp_outlyingness"], stream())),
        "sd_curve_projections": lambda: check(lib.sd_curve_projections(*head, Z.data_ptr(), None, 0, stream())),
        "sd_rank_depth_sums": lambda: check(lib.sd_rank_depth_sums(Z.data_ptr(), k, n, n, 1, 0, n, 0, rec.data_ptr(), ws.data_ptr(),
                                                                   sizes["rank_depth"], stream())),
        "torch.matmul fp64": lambda: torch.matmul(U, X, out=Z),
    }
    return calls, sizes, (X, U, Z, rec, out, ws)


def _time(fn, reps, inner, warmup):
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
    return {"ms_median": round(statistics.median(times), 4), "ms_min": round(min(times), 4), "ms_max": round(max(times), 4)}


def run(n, T, k, reps, inner, warmup):
    dev = torch.device("cuda", torch.cuda.current_device())
    calls, sizes, keep = _calls(n, T, k, dev)
    route = "image" if n <= 16384 else "sort"
    for entry, fn in calls.items():
        res = {"shape": f"n{n}_T{T}_k{k}", "entry": entry, "n": n, "T": T, "k": k}
        if entry in ("sd_rp_depth_sums", "sd_rank_depth_sums"):
            res["route"] = route
        res.update(_time(fn, reps, inner, warmup), reps=reps, inner=inner, warmup=warmup)
        if entry == "sd_curve_projections":
            res["peak_share"] = round(2.0 * T * n * k / (res["ms_median"] * 1e-3) / FP64_VECTOR_PEAK, 3)
        if entry == "sd_rp_depth_sums":
            res["ws_bytes"] = sizes["rp_depth"]
        if entry == "sd_rp_outlyingness":
            res["ws_bytes"] = sizes["rp_outlyingness"]
        yield res
    del keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rp_depth_times.txt"))
    a = ap.parse_args()
    torch.cuda.init()
    with open(a.out, "w") as f:
        for n, T, k in SHAPES:
            if a.only and f"n{n}_T{T}_k{k}" not in a.only:
                continue
            for res in run(n, T, k, a.reps, a.inner, a.warmup):
                line = json.dumps(res)
                print(line, flush=True)
                f.write(line + "\n")
                f.flush()


if __name__ == "__main__":
    main()
