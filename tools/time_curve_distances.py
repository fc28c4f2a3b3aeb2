#!/usr/bin/env python3
"""Squared L2 distances, their selection and the h-modal sums (K20) timings, every curve a target, next to two yardsticks
on the same tensor in the same process:

  sd_curve_sqdist          all n x n squared distances
  sd_hmodal_sums           the fused pass, g = 1 / (2 T)
  sd_curve_sqdist_select   k = ceil(0.15 N), with the matrix stored (where it is at most 1 GiB) and recomputed per pass
  FunctionalDepth          the whole containment='hmodal' call on a host DataFrame (upload, selection, sums; wall clock)
  torch.cdist              fp64, on the n x T transpose: the library yardstick
  sd_tvd_sums, algo 2      the pairwise route of K17: this project's own O(n^2 T) curve kernel

at n x T = 4 096 x 256, 10 000 x 1 000 and 14 000 x 1 000; at 100 000 x 256 only sd_hmodal_sums (no matrix is stored) and
the tvd yardstick.  "peak_share" of the two tile-kernel lines counts 2 vector operations per pair-timepoint (the subtraction
and the fma) against 39.3e12 fp64 vector operations a second (256 CUs x 4 SIMDs x 16 lanes a cycle x 2.4 GHz; an fma counted
as two flops gives the published 78.6 TFLOP/s).

Device time of the C entry point alone: data, result and workspace resident on the device, no copy inside the window.  A
window is `inner` calls enqueued back to back between two HIP events on the current stream; the figure is the window over
`inner`.  `inner` follows from one timed call: as many as fit a quarter of a second, at most --inner.  Per line: --warmup
calls, then --reps windows; median, minimum and maximum in ms per call.  One JSON line per measurement.

    python tools/time_curve_distances.py [--reps 7] [--inner 20] [--warmup 2] [--only SHAPE ...] [--limit 300]

Every shape runs in a child process of its own under --limit seconds; the first that fails or runs out of time ends the run,
and nothing more is started on the device."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"n4096_T256": (4096, 256, True), "n10000_T1000": (10000, 1000, True), "n14000_T1000": (14000, 1000, True),
          "n100000_T256": (100000, 256, False)}                      # (n, T, the lines that hold an n x n matrix)
PEAK_OPS = 39.3e12


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


def run(shape, reps, inner, warmup):
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

    def share(res):
        return {"peak_share": round(2.0 * n * n * T / (res["ms_median"] * 1e-3) / PEAK_OPS, 3)}

    def workspace(what, floor=False):
        size = lib.sd_curve_sqdist_min_workspace_bytes if floor else lib.sd_curve_sqdist_workspace_bytes
        nbytes = int(size(T, n, n, 1, n, what))
        return torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev), nbytes

    if square:
        out = torch.empty((n, n), dtype=torch.float64, device=dev)
        ws, nbytes = workspace(0)
        res = timed(lambda: check(lib.sd_curve_sqdist(X.data_ptr(), T, n, n, 1, 0, n, out.data_ptr(), ws.data_ptr(), nbytes,
                                                      stream())), reps, inner, warmup)
        emit("sqdist", "sd_curve_sqdist", res, **share(res))
        del out
    S = torch.empty(n, dtype=torch.float64, device=dev)
    ws, nbytes = workspace(1)
    g = 1.0 / (2.0 * T)
    res = timed(lambda: check(lib.sd_hmodal_sums(X.data_ptr(), T, n, n, 1, 0, n, g, S.data_ptr(), ws.data_ptr(), nbytes, stream())),
                reps, inner, warmup)
    emit("hmodal", "sd_hmodal_sums", res, **share(res), targets_per_batch=int(lib.sd_curve_sqdist_targets_per_batch(T, n, n, 1, n, 1, nbytes)))
    if square:
        k = math.ceil(0.15 * (n * (n - 1) // 2))
        h2 = torch.empty(1, dtype=torch.float64, device=dev)
        for mode, floor in (("stored", False), ("recompute", True)):
            ws, nbytes = workspace(2, floor)
            if mode == "stored" and nbytes < 8 * n * n:
                emit("select_stored", "sd_curve_sqdist_select", {"skipped": "the matrix exceeds 1 GiB: every size recomputes"})
                continue
            res = timed(lambda: check(lib.sd_curve_sqdist_select(X.data_ptr(), T, n, n, 1, k, h2.data_ptr(), ws.data_ptr(), nbytes,
                                                                 stream())), reps, inner, warmup)
            emit(f"select_{mode}", "sd_curve_sqdist_select", res, k=k, h2=float(h2.cpu()[0]))
        del ws
        df = pd.DataFrame(Xh)
        walls = []
        for _ in range(3):
            t0 = time.perf_counter()
            d = FunctionalDepth([df], containment="hmodal")
            walls.append((time.perf_counter() - t0) * 1e3)
        emit("functional_depth", "FunctionalDepth(containment='hmodal')", {"wall_ms_min": round(min(walls), 2),
                                                                          "wall_ms_first": round(walls[0], 2)}, bandwidth=d.bandwidth)
        engine.release_workspace()
        torch.cuda.empty_cache()
        Xt = X.t().contiguous()
        emit("cdist", "torch.cdist fp64", timed(lambda: torch.cdist(Xt, Xt), reps, inner, warmup))
        del Xt
        torch.cuda.empty_cache()
    sd = torch.empty(n, dtype=torch.int64, device=dev)
    shp = torch.empty((n, 3), dtype=torch.float64, device=dev)
    nbytes = int(lib.sd_tvd_workspace_bytes(T, n, n, 1, n, 2))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    emit("tvd_pairwise", "sd_tvd_sums algo 2", timed(lambda: check(lib.sd_tvd_sums(X.data_ptr(), T, n, n, 1, 0, n, 2, sd.data_ptr(),
                                                                                 shp.data_ptr(), None, ws.data_ptr(), nbytes, stream())),
                                                    reps, inner, warmup))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--limit", type=float, default=300.0, help="seconds a shape may take")
    ap.add_argument("--shape", default=None, help="run this one shape in this process (what the parent starts)")
    a = ap.parse_args()
    if a.shape:
        run(a.shape, a.reps, a.inner, a.warmup)
        return 0
    for shape in SHAPES:
        if a.only and shape not in a.only:
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--shape", shape, "--reps", str(a.reps), "--inner", str(a.inner),
               "--warmup", str(a.warmup)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired as e:
            sys.stdout.write((e.stdout or b"").decode() if isinstance(e.stdout, bytes) else (e.stdout or ""))
            print(json.dumps({"shape": shape, "error": f"no result within {a.limit:g} s"}), flush=True)
            return 1
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if p.returncode != 0:
            print(json.dumps({"shape": shape, "error": f"exit status {p.returncode}", "stderr": p.stderr[-400:]}), flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
