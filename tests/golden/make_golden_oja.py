#!/usr/bin/env python3
"""Generate the Oja-depth fixtures by running the REFERENCE itself (_oja_depth, _pointcloud.py:175-205).

Same rules as make_golden.py, whose reference loader and pandas-2 `DataFrame.append` shim are reused by import:
inputs are seeded recipes, outputs are what the reference returns (or the exception it raises).  New `kind` values
only (pointcloud_oja, pointcloud_oja_record, pointcloud_oja_error), so the existing parametrised tests never see
these files.

    PYTHONPATH=<statdepth checkout> PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_golden_oja.py
"""
import json
import os
import sys
import time

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _enc, _frame_json, _pandas2_append_shim, _ref, _series_json  # noqa: E402


def _run(name, kind, df, ref, **kw):
    R = _ref()
    _pandas2_append_shim()
    t0 = time.time()
    out = {"name": name, "kind": kind, "ref": ref,
           "call": {"containment": "oja", "to_compute": kw.get("to_compute"), "K": kw.get("K"),
                    "np_random_seed": kw.pop("seed", None)},
           "input": _frame_json(df)}
    if out["call"]["np_random_seed"] is not None:
        np.random.seed(out["call"]["np_random_seed"])
    try:
        s = R["PointcloudDepth"](df, containment="oja", **kw)
        out.update(_series_json(s))
    except Exception as e:                      # noqa: BLE001 -- the exception is the recorded behaviour
        out["raises"] = type(e).__name__
        out["message"] = str(e)
    out["elapsed_s"] = time.time() - t0
    return out


def build():
    gp = _ref()["gp"]
    cases = []
    # full depth, every point (:175-205)
    for (n, d, seed) in ((15, 2, 41), (12, 3, 42), (10, 4, 43), (9, 5, 44), (10, 8, 45)):
        cases.append(_run(f"oja_n{n}_d{d}", "pointcloud_oja", gp(n=n, d=d, seed=seed), "_pointcloud.py:175-205"))
    lab = gp(n=11, d=2, seed=46)
    lab.index = [f"pt{i}" for i in range(len(lab))]
    cases.append(_run("oja_labels", "pointcloud_oja", lab, "_pointcloud.py:175-205 (index=to_compute=None)"))
    # for the record: what the reference does where this project departs from it
    grid = pd.DataFrame(np.array([[x, y] for x in range(3) for y in range(3)] + [[1, 1], [2, 0]], dtype=float))
    cases.append(_run("oja_rec_grid", "pointcloud_oja_record", grid, "_pointcloud.py:197-199 (flat simplex raises)"))
    cases.append(_run("oja_rec_to_compute", "pointcloud_oja_record", gp(n=12, d=2, seed=47),
                      "_pointcloud.py:191-193 (subsets among to_compute only)", to_compute=[7, 2, 11, 4]))
    # K=2 on the reference test's input: generate_noisy_pointcloud(n=20, d=2) (tests/test_statdepth.py:59, unseeded there;
    # seeded here so that the frame is a fixture)
    cases.append(_run("oja_rec_k2", "pointcloud_oja_record", gp(n=20, d=2, seed=48),
                      "_pointcloud.py:68-123 -> :191-193 (one point: no subsets)", K=2, seed=7))
    # the sample's hull fails: DepthDegeneracy (:187-189)
    flat = pd.DataFrame({"x": np.arange(8.0), "y": 2.0 * np.arange(8.0) + 1.0})
    cases.append(_run("oja_err_flat", "pointcloud_oja_error", flat, "_pointcloud.py:187-189"))
    nan = gp(n=10, d=2, seed=49)
    nan.iloc[3, 1] = np.nan
    cases.append(_run("oja_err_nan", "pointcloud_oja_error", nan, "_pointcloud.py:187-189"))
    cases.append(_run("oja_err_d1", "pointcloud_oja_error", gp(n=10, d=1, seed=50), "_pointcloud.py:187-189"))
    return cases


def main():
    for out in build():
        with open(os.path.join(HERE, out["name"] + ".json"), "w") as f:
            json.dump(out, f, indent=None, separators=(",", ":"), allow_nan=False)
            f.write("\n")
        print(f"wrote {out['name']}: {out.get('raises', 'ok')} {out['elapsed_s']:.1f}s", flush=True)


if __name__ == "__main__":
    main()
