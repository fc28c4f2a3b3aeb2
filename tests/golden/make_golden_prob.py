#!/usr/bin/env python3
"""Generate the probabilistic-depth fixtures by running the REFERENCE itself (_uncertainty.py:63-70 and :123-139).

Same rules as make_golden.py, whose reference loader and JSON encoders are reused by import: inputs are seeded
recipes, outputs are what the reference returns (or the exception it raises).  New `kind` values only (prob_normal,
prob_poisson, prob_record), so the existing parametrised tests never see these files.  The reference's normal depth
runs one scipy `quad` per (target, pair): n = 8 takes about a minute, so the normal cases stay at n <= 9.

    PYTHONPATH=<statdepth checkout> PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_golden_prob.py
"""
import json
import os
import sys
import time
import warnings
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _enc, _frame_json, _ref, _series_json  # noqa: E402


def _unc():
    _ref()
    from statdepth.depth.calculations import _uncertainty
    return _uncertainty


def _normal(name, kind, means, stds, ref):
    U = _unc()
    out = {"name": name, "kind": kind, "ref": ref,
           "input": {"means": [_enc(v) for v in means], "stds": [_enc(v) for v in stds]}}
    t0 = time.time()
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            r = U.probabilistic_normal_depth(np.asarray(means, dtype=float), np.asarray(stds, dtype=float))
        out["columns"] = list(r.columns)
        out["depths"] = [_enc(v) for v in r["depths"].to_numpy(dtype=float)]
    except Exception as e:                      # noqa: BLE001 -- the exception is the recorded behaviour
        out["raises"] = type(e).__name__
        out["message"] = str(e)
    out["elapsed_s"] = time.time() - t0
    return out


def _poisson(name, kind, df, ref, **kw):
    U = _unc()
    out = {"name": name, "kind": kind, "ref": ref, "call": {"lim": kw.get("lim", 1000), "to_compute": kw.get("to_compute")},
           "input": _frame_json(df)}
    t0 = time.time()
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            s = U.probabilistic_poisson_depth(df, **kw)
        out.update(_series_json(s))
    except Exception as e:                      # noqa: BLE001
        out["raises"] = type(e).__name__
        out["message"] = str(e)
    out["elapsed_s"] = time.time() - t0
    return out


def _rates(T, n, seed, lo=0.1, hi=30.0):
    rng = np.random.default_rng(seed)
    return pd.DataFrame(np.exp(rng.uniform(np.log(lo), np.log(hi), size=(T, n))))


def jobs():
    rng = np.random.default_rng(900)
    J = []
    # normal (:123-139): one quad per (target, pair)
    for n, seed in ((3, 901), (5, 902), (7, 903)):
        r = np.random.default_rng(seed)
        J.append((_normal, (f"prob_normal_n{n}", "prob_normal", r.normal(0, 2, n).tolist(), r.uniform(0.3, 2.5, n).tolist(),
                            "_uncertainty.py:96-139")))
    r = np.random.default_rng(904)                 # means over three decades, stds from 0.05 to 20
    # a record: quad over (-inf, inf) misses the narrow integrand of target 2 (3.8e-5 returned as 1.7e-16)
    J.append((_normal, ("prob_rec_normal_quad_spread_n8", "prob_record",
                        (r.normal(0, 1, 8) * np.array([1, 10, 100, 1, 10, 100, 1, 5])).tolist(),
                        [0.05, 20.0, 1.0, 3.0, 0.5, 7.0, 0.2, 1.5], "_uncertainty.py:116 (quad of a narrow integrand)")))
    J.append((_normal, ("prob_normal_ties_n6", "prob_normal", [0.0, 0.0, 1.0, 1.0, -2.0, 0.0], [1.0, 1.0, 1.0, 2.0, 0.5, 1.0],
                        "_uncertainty.py:96-139 (equal distributions)")))
    # degenerate shapes: n = 1 is 0/0, n = 2 has no pairs
    J.append((_normal, ("prob_normal_n1", "prob_normal", [0.5], [1.0], "_uncertainty.py:121 (C(1,2) = 0)")))
    J.append((_normal, ("prob_normal_n2", "prob_normal", [0.5, -1.0], [1.0, 2.0], "_uncertainty.py:108 (no pairs)")))
    # records: what the reference does with input this project refuses
    J.append((_normal, ("prob_rec_normal_len", "prob_record", [0.0, 1.0, 2.0], [1.0, 1.0], "_uncertainty.py:124-125")))
    J.append((_normal, ("prob_rec_normal_nan_mean", "prob_record", [0.0, float("nan"), 2.0, 1.0], [1.0, 1.0, 0.5, 2.0],
                        "_uncertainty.py:116 (quad of a NaN integrand)")))
    J.append((_normal, ("prob_rec_normal_zero_std", "prob_record", [0.0, 1.0, 2.0, 1.5], [1.0, 0.0, 0.5, 2.0],
                        "_uncertainty.py:96-99 (norm(scale=0))")))
    # Poisson (:34-70)
    J.append((_poisson, ("prob_poisson_T6_n5", "prob_poisson", _rates(6, 5, 910), "_uncertainty.py:34-70"), {"lim": 100}))
    # the reference's terms are inf / inf (NaN) once lam^z z! leaves the fp64 range and 0 once z!^3 does: rates and lim
    # are chosen so that neither happens where a term is not negligible
    spread = _rates(4, 8, 911, lo=0.001, hi=1.0)
    spread.iloc[1, 2] = 0.0
    spread.iloc[3, 6] = 0.0
    spread.iloc[:, 0] = [0.0, 0.0, 0.0, 0.0]
    J.append((_poisson, ("prob_poisson_spread_T4_n8", "prob_poisson", spread, "_uncertainty.py:34-70 (lambda = 0, three decades)"),
              {"lim": 150}))
    wide = _rates(5, 7, 924, lo=0.01, hi=10.0)
    wide.iloc[2, 4] = 0.0
    J.append((_poisson, ("prob_poisson_wide_T5_n7", "prob_poisson", wide, "_uncertainty.py:34-70 (three decades)"), {"lim": 80}))
    perm = spread[[5, 2, 7, 0, 3, 6, 1, 4]]        # the same curves in another column order: the pair orientation
    J.append((_poisson, ("prob_poisson_spread_T4_n8_perm", "prob_poisson", perm, "_uncertainty.py:51 (i before j)"), {"lim": 150}))
    J.append((_poisson, ("prob_poisson_wide_T5_n7_perm", "prob_poisson", wide[[6, 3, 0, 5, 1, 4, 2]], "_uncertainty.py:51 (i before j)"),
              {"lim": 80}))
    lab = _rates(3, 6, 912, lo=0.5, hi=8.0)
    lab.columns = [f"c{i}" for i in range(6)]
    lab.index = [f"t{i}" for i in range(3)]
    J.append((_poisson, ("prob_poisson_labels_T3_n6", "prob_poisson", lab, "_uncertainty.py:63-70 (labels)"), {"lim": 40}))
    J.append((_poisson, ("prob_poisson_T8_n4", "prob_poisson", _rates(8, 4, 913, lo=1.0, hi=8.0), "_uncertainty.py:34-70"),
              {"lim": 80}))
    # degenerate shapes
    J.append((_poisson, ("prob_poisson_n2", "prob_poisson", _rates(5, 2, 914), "_uncertainty.py:50 (no pairs)"), {"lim": 50}))
    J.append((_poisson, ("prob_poisson_T1", "prob_poisson", _rates(1, 4, 915), "_uncertainty.py:67 (1 / C(1,2) = inf)"),
              {"lim": 50}))
    J.append((_poisson, ("prob_poisson_lim1", "prob_poisson", _rates(4, 4, 916), "_uncertainty.py:41 (empty z range)"),
              {"lim": 1}))
    J.append((_poisson, ("prob_poisson_lim0_T1", "prob_poisson", _rates(1, 3, 917), "_uncertainty.py:41,67 (inf * 0)"),
              {"lim": 0}))
    # records
    J.append((_poisson, ("prob_rec_poisson_default_lim", "prob_record", _rates(3, 3, 918, lo=1.0, hi=5.0),
                         "_uncertainty.py:41-42 (factorial(z), gamma(z) overflow at z >= 171: inf / inf)"), {}))
    J.append((_poisson, ("prob_rec_poisson_lim172", "prob_record", _rates(3, 3, 919, lo=1.0, hi=5.0),
                         "_uncertainty.py:41-42 (the first lim with z = 171)"), {"lim": 172}))
    J.append((_poisson, ("prob_rec_poisson_lim171", "prob_record", _rates(3, 3, 919, lo=1.0, hi=5.0),
                         "_uncertainty.py:41-42 (the last finite lim)"), {"lim": 171}))
    big = _rates(3, 4, 920, lo=1.0, hi=5.0)
    big.iloc[1, 2] = 40.0
    J.append((_poisson, ("prob_rec_poisson_big_rate", "prob_record", big,
                         "_uncertainty.py:41-42 (lambda^z z! beyond the fp64 range)"), {"lim": 150}))
    neg = _rates(3, 4, 921)
    neg.iloc[2, 1] = -0.5
    J.append((_poisson, ("prob_rec_poisson_negative", "prob_record", neg, "_uncertainty.py:41-42 (negative rate)"), {"lim": 50}))
    nanf = _rates(3, 4, 922)
    nanf.iloc[0, 3] = np.nan
    J.append((_poisson, ("prob_rec_poisson_nan", "prob_record", nanf, "_uncertainty.py:41-42 (NaN rate)"), {"lim": 50}))
    J.append((_poisson, ("prob_rec_poisson_to_compute", "prob_record", _rates(4, 5, 923),
                         "_uncertainty.py:63-70 (to_compute is ignored)"), {"lim": 60, "to_compute": [1, 3]}))
    del rng
    return J


def _run(job):
    fn, args = job[0], job[1]
    kw = job[2] if len(job) > 2 else {}
    return fn(*args, **kw)


def main():
    with ProcessPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        for out in ex.map(_run, jobs()):
            with open(os.path.join(HERE, out["name"] + ".json"), "w") as f:
                json.dump(out, f, indent=None, separators=(",", ":"), allow_nan=False)
                f.write("\n")
            print(f"wrote {out['name']}: {out.get('raises', 'ok')} {out['elapsed_s']:.1f}s", flush=True)


if __name__ == "__main__":
    main()
