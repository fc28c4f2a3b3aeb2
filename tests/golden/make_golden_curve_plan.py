#!/usr/bin/env python3
"""Record what the size and rows functions of the curve rank depths return, and what their entry points refuse.

The fixture pins the numbers of the library as it was BEFORE the pair-image plan went behind sizing and launch: it is
recorded from a build of that parent commit and never from the code under test,

    python3 tests/golden/make_golden_curve_plan.py --lib <parent checkout>/statdepth_amd/lib/libstatdepth_hip.so

and tests/test_curve_plan_host.py asks the library under test the same questions through table() and refused() below.
No GPU: the size functions are host code and every recorded call returns before anything touches a device.

Sizes (curve_plan_sizes.json, kind "curve_plan_sizes"), in the order of itertools.product over the axes T, n, m, algo and
layout: sd_rank_depth_*, sd_extremal_* and sd_tvd_* give (recommended, floor), and the first and the last of them the rows
per batch at the seven workspace sizes of ws_points(); sd_central_regions_workspace_bytes over T, n, L and layout.
Refusals: the return code and the message of each call of CALLS.
"""
import argparse
import ctypes
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from statdepth_amd import _native  # noqa: E402

AXES = {"T": [1, 2, 7, 70, 1000, 16384, 16385, 65537],
        "n": [1, 2, 5, 63, 65, 300, 2500, 10000, 16384, 16385, 100000],
        "m": ["n", 10], "algo": [0, 1, 2], "curve_major": [0, 1]}
LEVELS = [0, 1, 3, 8, 9]


def ws_points(rec, floor):
    """floor - 1, floor, two points in between, recommended - 1, recommended, twice recommended"""
    return [max(floor - 1, 0), floor, floor + (rec - floor) // 3, floor + 2 * (rec - floor) // 3, max(rec - 1, 0), rec, 2 * rec]


def strides(T, n, curve_major):
    return (1, T) if curve_major else (n, 1)


def grid():
    for T, n, m, algo, cm in itertools.product(*(AXES[k] for k in ("T", "n", "m", "algo", "curve_major"))):
        yield T, n, *strides(T, n, cm), (n if m == "n" else m), algo


def table(lib):
    out = {"rank_depth": [], "extremal": [], "tvd": [], "central_regions": []}
    for shape in grid():
        for fam in ("rank_depth", "extremal", "tvd"):
            rec = getattr(lib, f"sd_{fam}_workspace_bytes")(*shape)
            floor = getattr(lib, f"sd_{fam}_min_workspace_bytes")(*shape)
            rows = getattr(lib, f"sd_{fam}_rows_per_batch", None)
            out[fam].append([rec, floor] + ([rows(*shape, ws) for ws in ws_points(rec, floor)] if rows else []))
    for T, n, L, cm in itertools.product(AXES["T"], AXES["n"], LEVELS, AXES["curve_major"]):
        out["central_regions"].append(lib.sd_central_regions_workspace_bytes(T, n, *strides(T, n, cm), L))
    return out


# ---- refused calls: (entry point, changes to the valid call below).  P stands for a pointer that is not null; no call gets a
# workspace (the last thing an entry point checks), so that none could reach a device whatever else it accepted. ----
P = 4096
BIG = 2 ** 31
VALID = {
    "sd_rank_depth_sums": dict(X=P, T=7, n=65, st=65, sn=1, targets=None, m=65, algo=0, out=P, ws=None, ws_bytes=0, stream=None),
    "sd_extremal_counts": dict(X=P, T=7, n=65, st=65, sn=1, targets=None, m=65, algo=0, out=P, ws=None, ws_bytes=0, stream=None),
    "sd_tvd_sums": dict(X=P, T=7, n=65, st=65, sn=1, targets=None, m=65, algo=0, sd_sum=P, shape=P, counts=None, ws=None,
                        ws_bytes=0, stream=None),
    "sd_central_regions": dict(X=P, T=7, n=65, st=65, sn=1, level=P, L=2, box=0, factor=1.5, env=P, fence=P, outside=P,
                               whisker=P, ws=None, ws_bytes=0, stream=None),
}
CURVES = ("sd_rank_depth_sums", "sd_extremal_counts", "sd_tvd_sums")
MILLION = dict(T=1000, n=10 ** 6, st=10 ** 6, m=10 ** 6, algo=2)            # 10^15 comparisons: above the work cap of K15 and K17
CALLS = [(fn, ch) for fn in CURVES for ch in (
    {},                                                                     # no workspace
    dict(ws=P, ws_bytes=255),                                               # ... and one below the floor
    dict(st=1, sn=7), dict(st=1, sn=7, ws=P, ws_bytes=255),                 # the same behind a time-major copy
    dict(X=None), dict(X=None, algo=3), dict(T=0), dict(n=0, st=1, m=0), dict(n=1, st=1, m=1), dict(n=1, st=1, m=1, algo=-1),
    dict(algo=3), dict(algo=-1, st=3, sn=7),
    dict(n=BIG, st=BIG, m=BIG), dict(n=BIG, st=BIG, m=BIG, algo=1), dict(n=BIG, st=BIG, m=BIG, algo=2), dict(T=BIG),
    dict(n=16385, st=16385, m=16385, algo=1), dict(n=16385, st=3, sn=7, m=16385, algo=1),
    dict(T=16385), dict(T=16385, algo=3), dict(T=16385, n=BIG, st=BIG, m=BIG), dict(T=16385, n=16385, st=16385, m=16385, algo=1),
    dict(st=3, sn=7), dict(st=0), dict(st=64), dict(m=-1, targets=P), dict(m=10),
    MILLION, dict(MILLION, st=3, sn=7), dict(MILLION, algo=1), dict(MILLION, m=10, targets=P), dict(MILLION, algo=0))]
CALLS += [("sd_rank_depth_sums", dict(out=None)), ("sd_rank_depth_sums", dict(out=None, algo=3)),
          ("sd_extremal_counts", dict(out=None)), ("sd_extremal_counts", dict(out=None, algo=3)),
          ("sd_tvd_sums", dict(sd_sum=None)), ("sd_tvd_sums", dict(shape=None, algo=3)), ("sd_tvd_sums", dict(counts=P))]
CALLS += [("sd_central_regions", ch) for ch in (
    {}, dict(ws=P, ws_bytes=8), dict(st=1, sn=7), dict(level=None), dict(env=None, L=9), dict(n=0, st=1), dict(T=0),
    dict(L=0), dict(L=9), dict(box=2), dict(box=-2), dict(factor=-1.0), dict(factor="nan"), dict(factor="inf"),
    dict(box=-1), dict(box=-1, fence=None, outside=None, whisker=None), dict(st=3, sn=7), dict(st=3, sn=7, L=0), dict(n=BIG, st=BIG))]


def refused(lib):
    out = []
    for fn, changes in CALLS:
        args = dict(VALID[fn], **changes)
        values = [float(v) if isinstance(v, str) else v for v in args.values()]
        code = getattr(lib, fn)(*values)
        out.append({"fn": fn, "changes": changes, "code": code, "message": lib.sd_last_error().decode()})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True, help="libstatdepth_hip.so of the parent commit")
    lib = _native.open_library(ap.parse_args().lib)
    out = {"name": "curve_plan_sizes", "kind": "curve_plan_sizes", "axes": AXES, "levels": LEVELS, **table(lib),
           "refusals": refused(lib)}
    assert all(r["code"] != 0 for r in out["refusals"]), [r for r in out["refusals"] if r["code"] == 0]
    path = os.path.join(HERE, "curve_plan_sizes.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"), allow_nan=False)
        f.write("\n")
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out['tvd'])} shapes, {len(out['refusals'])} refused calls")


if __name__ == "__main__":
    main()
