#!/usr/bin/env python3
"""Lens, spherical and beta-skeleton depth (K22) timings, every curve a target, next to stage 1 alone and to the torch
expression a user had before, on the same tensor in the same process:

  sd_lens_counts           kappa = 0 (the lens form), kappa = 1 (the sphere form), kappa = 0.5 (the general form): the matrix
                           (stage 1), then the count over all triples (stage 2)
  sd_curve_sqdist          all n x n squared distances: stage 1 alone
  torch                    (torch.maximum(a[:, None], a[None, :]) <= D).triu(1).sum() per target, a = D[q], over 64 targets of
                           the same D: the lens count in eager torch, reported per target and scaled to n targets

at n x T = 1 024 x 256, 4 096 x 256, 10 000 x 1 000 and 14 000 x 1 000.  "triples_per_s" counts the n C(n, 2) triples of a
call against the time of the whole call; "lane_ops_share" counts 3 vector instructions per triple (5 in the general form)
against 39.3e12 lane-operations a second (256 CUs x 4 SIMDs x 16 lanes a cycle x 2.4 GHz).

Device time of the C entry point alone: data, result and workspace resident on the device, no copy inside the window.  A
window is `inner` calls enqueued back to back between two HIP events on the current stream; the figure is the window over
`inner`.  `inner` follows from one timed call: as many as fit a quarter of a second, at most --inner.  Per line: --warmup
calls, then --reps windows; median, minimum and maximum in ms per call.  One JSON line per measurement.

    python tools/time_lens_depth.py [--reps 5] [--inner 20] [--warmup 1] [--only SHAPE ...] [--limit 300] [--kernels DIR]

--kernels DIR gives the stage split instead: every shape runs once more under `rocprofv3 --kernel-trace --stats` (a run of
its own: tracing slows the host, its numbers are kernel times only), the three forms alone, and the statistics are read back:
stage 1 (cd_tile_kernel<0>) and the count kernel of each form in ms per call.

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

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"n1024_T256": (1024, 256), "n4096_T256": (4096, 256), "n10000_T1000": (10000, 1000), "n14000_T1000": (14000, 1000)}
FORMS = (("lens", 0.0, 3), ("sphere", 1.0, 3), ("general", 0.5, 5))  # (name, kappa, vector instructions per triple)
PEAK_OPS = 39.3e12
KERNEL_CALLS = 2                                                     # calls of each form under the profiler
YARD_TARGETS = 64
KERNELS = {"stage1_matrix": "cd_tile_kernel<0>", "count_lens": "lens_count_kernel<0>", "count_sphere": "lens_count_kernel<1>",
           "count_general": "lens_count_kernel<2>"}


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
    import torch
    from statdepth_amd import engine
    from statdepth_amd._native import check
    n, T = SHAPES[shape]
    torch.cuda.init()
    dev = torch.device("cuda", torch.cuda.current_device())
    lib = engine._lib()
    stream = lambda: engine._stream_ptr(dev)                         # noqa: E731
    X = torch.from_numpy(np.random.default_rng(n + T).normal(size=(T, n))).to(dev)   # time-major, continuous
    triples = n * (n * (n - 1) // 2)

    def emit(case, entry, res, **more):
        print(json.dumps({"case": f"{case}_{shape}", "entry": entry, "n": n, "T": T, **res, **more}), flush=True)

    G = torch.empty(n, dtype=torch.int64, device=dev)
    nbytes = int(lib.sd_lens_workspace_bytes(T, n, n, 1, n))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    lens_ms = None
    for name, kappa, per_triple in FORMS:
        call = lambda: check(lib.sd_lens_counts(X.data_ptr(), T, n, n, 1, 0, n, kappa, 0, G.data_ptr(), ws.data_ptr(), nbytes,  # noqa: E731
                                                stream()))
        if kernels_only:
            for _ in range(KERNEL_CALLS):
                call()
            torch.cuda.synchronize()
            continue
        res = timed(call, reps, inner, warmup)
        sec = res["ms_median"] * 1e-3
        emit(name, "sd_lens_counts", res, kappa=kappa, triples_per_s=float(f"{triples / sec:.4g}"),
             lane_ops_share=round(per_triple * triples / sec / PEAK_OPS, 3), workspace_bytes=nbytes,
             count_min=int(G.min()), count_max=int(G.max()))
        if name == "lens":
            lens_ms = res["ms_median"]
            lens_counts = G[:YARD_TARGETS].clone()
    if kernels_only:
        return
    del ws
    torch.cuda.empty_cache()
    D = torch.empty((n, n), dtype=torch.float64, device=dev)
    res = timed(lambda: check(lib.sd_curve_sqdist(X.data_ptr(), T, n, n, 1, 0, n, D.data_ptr(), None, 0, stream())), reps, inner, warmup)
    emit("stage1", "sd_curve_sqdist", res, lens_over_stage1=round(lens_ms / res["ms_median"], 3))

    got = torch.empty(YARD_TARGETS, dtype=torch.int64, device=dev)

    def yardstick():
        for q in range(YARD_TARGETS):
            a = D[q]
            got[q] = (torch.maximum(a[:, None], a[None, :]) <= D).triu(1).sum()

    res = timed(yardstick, max(2, reps // 2), 1, 1)
    per_target = {k: round(v / YARD_TARGETS, 4) for k, v in res.items() if k.startswith("ms_")}
    emit("yardstick", "torch: (maximum(a[:, None], a[None, :]) <= D).triu(1).sum(), per target", per_target, targets=YARD_TARGETS,
         equals_the_lens_counts=bool(torch.equal(got, lens_counts)),
         ms_for_n_targets=round(per_target["ms_median"] * n, 1), yardstick_over_lens=round(per_target["ms_median"] * n / lens_ms, 1))


def kernel_stats(directory, shape):
    """The kernels of the calls from rocprofv3's statistics file under `directory`: launches and ms per call of the entry
    point (stage 1 runs once in each of the 3 x KERNEL_CALLS calls)."""
    found = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                kn = r.get("Name") or r.get("KernelName") or ""
                for key, sub in KERNELS.items():
                    if sub in kn:
                        total = float(r.get("TotalDurationNs") or r.get("TotalDuration(ns)") or 0.0)
                        calls = KERNEL_CALLS * (len(FORMS) if key == "stage1_matrix" else 1)
                        found[key] = {"kernel": kn[:48], "launches": int(float(r.get("Calls") or 0)),
                                      "ms_per_call": round(total / 1e6 / calls, 4)}
    return {"case": f"kernels_{shape}", "entry_calls_each_form": KERNEL_CALLS, **found}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--limit", type=float, default=300.0, help="seconds a shape may take")
    ap.add_argument("--kernels", default=None, metavar="DIR", help="kernel times under rocprofv3, its files kept in DIR")
    ap.add_argument("--shape", default=None, help="run this one shape in this process (what the parent starts)")
    ap.add_argument("--kernels-only", action="store_true", help="with --shape: a few calls of each form, untimed")
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
