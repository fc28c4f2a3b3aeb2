"""The single-pair fixtures of the probabilistic kernels (tests/golden/pairs_*.json) without a GPU: a sample of each file
recomputed by the generator's own functions, the two mpmath routes to K9's p against each other, and the fp64 oracles
that the other GPU tests lean on (`band_p`, `normal_sums`, `poisson_sums`) measured against the 40-digit values.

The loaders and error measures here are imported by tests/test_prob_pairs_gpu.py.
"""
import json
import os
import sys

import mpmath as mp
import numpy as np
import pytest

from conftest import GOLDEN
from test_probabilistic_band_host import band_p
from test_probabilistic_host import normal_sums, poisson_sums

sys.path.insert(0, GOLDEN)
import make_golden_prob_pairs as gen  # noqa: E402


def _load(name, kind):
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        fx = json.load(f)
    assert fx["kind"] == kind and fx["digits"] == gen.DIGITS
    return fx


@pytest.fixture(scope="module")
def band_fx():
    return _load("pairs_band", "pairs_band")


@pytest.fixture(scope="module")
def normal_fx():
    return _load("pairs_normal", "pairs_normal")


@pytest.fixture(scope="module")
def poisson_fx():
    return _load("pairs_poisson", "pairs_poisson")


def unhex(values):
    return [float.fromhex(v) for v in values]


def ref_and_error(got, want_str):
    """(float(want), |got - want|, |got - want| / |want|) with the difference formed at 50 digits."""
    with mp.workdps(50):
        w = mp.mpf(want_str)
        d = abs(mp.mpf(float(got)) - w)
        return float(w), float(d), float(d / abs(w)) if w != 0 else (0.0 if d == 0 else float("inf"))


def _sample(entries, count):
    step = max(1, len(entries) // count)
    return entries[::step][:count]


# ---------------------------------------------------------------- the files regenerate from the committed script
def test_band_entries_recompute(band_fx):
    names = dict(gen.band_triples() + gen.strict_items())
    assert [e["name"] for e in band_fx["entries"]] == [n for n, _ in gen.band_triples()]
    assert [e["name"] for e in band_fx["strict"]["factors"]] == [n for n, _ in gen.strict_items()]
    for e in _sample(band_fx["entries"], 10) + _sample(band_fx["strict"]["factors"], 2):
        assert tuple(unhex(e["in"])) == names[e["name"]]
        assert gen._band_entry((e["name"], tuple(unhex(e["in"])))) == e


def test_normal_entries_recompute(normal_fx):
    cases = gen.normal_cases()
    assert [e["name"] for e in normal_fx["entries"]] == [c[0] for c in cases]
    step = max(1, len(cases) // 12)
    for c, e in list(zip(cases, normal_fx["entries"]))[::step]:
        assert gen._normal_entry(c) == e


def test_poisson_entries_recompute(poisson_fx):
    cases = gen.poisson_cases()
    assert [e["name"] for e in poisson_fx["entries"]] == [c[0] for c in cases]
    quick = [(c, e) for c, e in zip(cases, poisson_fx["entries"]) if e["lim"] <= 600]
    for c, e in quick[::max(1, len(quick) // 12)]:
        assert gen._poisson_entry(c) == e


def test_fixture_shape(band_fx, normal_fx, poisson_fx):
    """The cases the tests sort by are all there, and each file stays small."""
    for name in ("pairs_band", "pairs_normal", "pairs_poisson"):
        assert os.path.getsize(os.path.join(GOLDEN, name + ".json")) < 200 * 1024
    by = {}
    for e in band_fx["entries"]:
        by.setdefault((e["branch"], e["regime"]), []).append(e)
    for branch in ("gl6", "gl12", "gl20", "near1", "point_i", "point_jk"):
        assert len(by.get((branch, "A"), [])) >= 2, branch
    assert len(by[("near1", "B")]) >= 8 and len(by[("gl12", "B")]) >= 6
    for e in band_fx["entries"] + band_fx["strict"]["factors"]:
        a = max(abs(e["hj"]), abs(e["hk"])) <= gen.H_REGIME_A and mp.mpf(e["p"]) >= gen.P_REGIME_A
        assert e["regime"] == ("A" if a else "B")
    assert all(e["regime"] == "A" for e in band_fx["strict"]["factors"]) and len(band_fx["strict"]["factors"]) == 72
    assert len(band_fx["entries"]) >= 230 and len(normal_fx["entries"]) >= 150 and len(poisson_fx["entries"]) >= 50
    assert {e["seam"] for e in poisson_fx["entries"]} == {"stirlerr15", "stirlerr35", "stirlerr80", "stirlerr500", "bd0", "tail",
                                                         "chunk", "tiny", "random"}


# ---------------------------------------------------------------- K9: the two routes
def test_band_routes_agree(band_fx):
    """The angle form against the 1-D integral over X_i on entries with |h| <= 12, four of each quadrature branch:
    1e-25 relative.  mp.quad stops at an absolute error of 10^-dps, so the digits follow p."""
    pick = [e for e in band_fx["entries"] if e["regime"] == "A" and 1e-9 < e["rho"] < 1 - 1e-9 and float(e["p"]) >= 1e-40]
    chosen = [e for b in ("gl6", "gl12", "gl20", "near1") for e in _sample([e for e in pick if e["branch"] == b], 4)]
    assert len(chosen) == 16
    worst = 0.0
    for e in chosen:
        dps = 32 - int(np.floor(np.log10(float(e["p"]))))
        with mp.workdps(dps):
            a, b = mp.mpf(e["p"]), gen.band_p_line(tuple(unhex(e["in"])), dps=dps)
            rel = float(abs(a - b) / a)
        worst = max(worst, rel)
        assert rel <= 1e-25, (e["name"], rel)
    print(f"angle form vs 1-D integral: worst relative difference {worst:.2e} (bound 1e-25)")


# ---------------------------------------------------------------- the fp64 oracles against the fixtures
def test_band_p_oracle(band_fx):
    """`band_p` (Owen's T from scipy) holds its 5e-15 absolute on every entry; its relative error is printed, not
    asserted: ndtr + ndtr - 2 Phi2 cancels, so it has none where p is small."""
    worst_abs, worst_rel = 0.0, 0.0
    for e in band_fx["entries"] + band_fx["strict"]["factors"]:
        got = float(band_p(*unhex(e["in"])))
        w, d, r = ref_and_error(got, e["p"])
        worst_abs = max(worst_abs, d)
        if e["regime"] == "A":
            worst_rel = max(worst_rel, r)
        assert np.isfinite(got) and d <= 5e-15, (e["name"], got, e["p"])
    print(f"band_p: worst absolute error {worst_abs:.2e} (bound 5e-15), worst relative error in regime A {worst_rel:.2e}")


def test_normal_sums_oracle(normal_fx):
    """`normal_sums` (Genz's angle form, 20 points) within 1e-12 of every pair term, finite everywhere."""
    worst = 0.0
    for e in normal_fx["entries"]:
        with np.errstate(over='ignore'):                 # h = +-inf where the means differ by more than the fp64 range
            got = float(normal_sums(unhex(e["mu"]), unhex(e["sigma"]), [0])[0])
        w, d, _ = ref_and_error(got, e["value"])
        assert np.isfinite(got), (e["name"], got)
        worst = max(worst, d)
        assert d <= 1e-12, (e["name"], got, e["value"])
    print(f"normal_sums: worst absolute error of a pair term {worst:.2e} (bound 1e-12)")


def test_poisson_sums_oracle(poisson_fx):
    """`poisson_sums` (scipy's pmf, cdf and sf) within rtol 1e-12 where the value is at least 1e-290, 0 where it is 0."""
    worst = 0.0
    for e in poisson_fx["entries"]:
        got = poisson_sums(np.array([unhex(e["lam"])]), e["lim"])
        for f in range(3):
            w, d, r = ref_and_error(got[f], e["values"][f])
            if mp.mpf(e["values"][f]) == 0:
                assert got[f] == 0.0, (e["name"], f)
            elif w >= 1e-290:
                worst = max(worst, r)
                assert r <= 1e-12, (e["name"], f, got[f], e["values"][f])
            else:
                assert np.isfinite(got[f]) and got[f] <= 1e-289, (e["name"], f, got[f])
    print(f"poisson_sums: worst relative error {worst:.2e} (bound 1e-12)")
