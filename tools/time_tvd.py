#!/usr/bin/env python3
"""Total variation depth and shape similarity (K17) timings, every curve a target, next to stage 1 alone in the same run:

  sd_tvd_sums          algo 1 (LDS route) and algo 2 (pairwise) at n x T = 4 096 x 256, 10 000 x 1 000 and 14 000 x 1 000;
                       algo 2 at 100 000 x 256
  sd_rank_depth_sums   the image route at the three shapes of algo 1: K14's pair image and its fold, which is stage 1 of the
                       LDS route.  "over_stage1_ms" of an algo 1 line is its median minus this one: what the dominance
                       kernel and the wider fold cost.

Device time of the C entry point alone: data, result and workspace resident on the device, no copy inside the window.
A window is `inner` calls enqueued back to back between two HIP events on the current stream (the host's enqueue latency in
front of the first kernel is spread over the window); the figure is the window over `inner`.  `inner` follows from one
timed call: as many as fit a quarter of a second, at most --inner.  Per case: --warmup calls, then --reps windows; median,
minimum and maximum in ms per call.  One JSON line per case.

    python tools/time_tvd.py [--reps 9] [--inner 20] [--warmup 2] [--only NAME ...] [--limit 180]

Every case runs in a child process of its own under --limit seconds; the first case that fails or runs out of time ends
the run, and nothing more is started on the device."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (case, entry point, n, T, algo)
SHAPES = [(4096, 256), (10000, 1000), (14000, 1000)]
CASES = []
for _n, _T in SHAPES:
    CASES += [(f"rank_depth_image_n{_n}_T{_T}", "rank_depth", _n, _T, 1), (f"tvd_lds_n{_n}_T{_T}", "tvd", _n, _T, 1),
              (f"tvd_pairwise_n{_n}_T{_T}", "tvd", _n, _T, 2)]
CASES.append(("tvd_pairwise_n100000_T256", "tvd", 100000, 256, 2))


def _call(kind, n, T, algo, dev):
    """A function of no arguments that enqueues the entry point once, everything it touches already on the device."""
    import torch
    from statdepth_amd import engine
    from statdepth_amd._native import check
    lib = engine._lib()
    rng = np.random.default_rng(n + T)
    stream = lambda: engine._stream_ptr(dev)                         # noqa: E731
    X = torch.from_numpy(rng.normal(size=(T, n))).to(dev)            # time-major, continuous
    if kind == "rank_depth":
        out = torch.empty((n, 5), dtype=torch.int64, device=dev)
        nbytes = int(lib.sd_rank_depth_workspace_bytes(T, n, n, 1, n, algo))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        return lambda: check(lib.sd_rank_depth_sums(X.data_ptr(), T, n, n, 1, 0, n, algo, out.data_ptr(), ws.data_ptr(), nbytes,
                                                    stream())), (X, out, ws)
    sd = torch.empty(n, dtype=torch.int64, device=dev)
    shape = torch.empty((n, 3), dtype=torch.float64, device=dev)
    nbytes = int(lib.sd_tvd_workspace_bytes(T, n, n, 1, n, algo))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    return lambda: check(lib.sd_tvd_sums(X.data_ptr(), T, n, n, 1, 0, n, algo, sd.data_ptr(), shape.data_ptr(), None,
                                         ws.data_ptr(), nbytes, stream())), (X, sd, shape, ws)


def run(name, kind, n, T, algo, reps, inner, warmup):
    import torch
    torch.cuda.init()
    dev = torch.device("cuda", torch.cuda.current_device())
    fn, keep = _call(kind, n, T, algo, dev)
    res = {"case": name, "entry": {"rank_depth": "sd_rank_depth_sums", "tvd": "sd_tvd_sums"}[kind], "n": n, "T": T,
           "route": {("rank_depth", 1): "image", ("tvd", 1): "lds", ("tvd", 2): "pairwise"}[(kind, algo)]}
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
    ap.add_argument("--limit", type=float, default=180.0, help="seconds a case may take")
    ap.add_argument("--case", default=None, help="run this one case in this process (what the parent starts)")
    a = ap.parse_args()
    if a.case:
        name, kind, n, T, algo = next(c for c in CASES if c[0] == a.case)
        print(json.dumps(run(name, kind, n, T, algo, a.reps, a.inner, a.warmup)), flush=True)
        return 0
    stage1 = {}
    for name, kind, n, T, algo in CASES:
        if a.only and name not in a.only:
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(a.reps), "--inner", str(a.inner),
               "--warmup", str(a.warmup)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(json.dumps({"case": name, "error": f"no result within {a.limit:g} s"}), flush=True)
            return 1
        if p.returncode != 0:
            print(json.dumps({"case": name, "error": f"exit status {p.returncode}", "stderr": p.stderr[-400:]}), flush=True)
            return 1
        res = json.loads(p.stdout.strip().splitlines()[-1])
        if kind == "rank_depth":
            stage1[(n, T)] = res["ms_median"]
        elif algo == 1 and (n, T) in stage1:
            res["over_stage1_ms"] = round(res["ms_median"] - stage1[(n, T)], 4)
        print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
