"""Probabilistic depths on the GPU (K8, sd_prob_*): the reference's fixtures through the public API, the engine against
the numpy restatements of tests/test_probabilistic_host.py at moderate and adversarial sizes, scale cases on sampled
targets, and bitwise determinism across calls, target subsets and forced launch splits."""
import math

import numpy as np
import pandas as pd
import pytest

from conftest import golden_names, load_golden
from test_probabilistic_host import _close, _frame, _mu_sigma, _want, normal_sums, poisson_sums

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from statdepth_amd import engine
    return engine


def _rel_close(got, want, rtol):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and np.isfinite(got).all()
    assert np.all(np.abs(got - want) <= rtol * np.abs(want) + 1e-300), np.max(np.abs(got - want) / np.abs(want))


# ---------------------------------------------------------------- the reference's values through the public API
@pytest.mark.parametrize("name", golden_names(kind="prob_normal"))
def test_golden_normal_api(name):
    from statdepth_amd import probabilistic_normal_depth
    fx = load_golden(name)
    mu, sg = _mu_sigma(fx)
    got = probabilistic_normal_depth(mu, sg)
    assert list(got.columns) == fx["columns"] == ["means", "stds", "depths"]
    assert np.array_equal(got["means"].to_numpy(), mu) and np.array_equal(got["stds"].to_numpy(), sg)
    _close(got["depths"].to_numpy(dtype=float), _want(fx), atol=1e-10)


@pytest.mark.parametrize("name", golden_names(kind="prob_poisson"))
def test_golden_poisson_api(name):
    from statdepth_amd import probabilistic_poisson_depth
    fx = load_golden(name)
    df = _frame(fx)
    got = probabilistic_poisson_depth(df, lim=fx["call"]["lim"])
    assert isinstance(got, pd.Series) and list(got.index) == fx["index"]
    _close(got.to_numpy(), _want(fx), atol=1e-300, rtol=1e-12)


def test_normal_custom_integrand_runs_on_the_host():
    """A custom f is integrated with quad as the reference does; the reference's own integrand given explicitly as a
    plain function reproduces the GPU's depths."""
    from scipy.stats import norm
    from statdepth_amd import probabilistic_normal_depth
    fx = load_golden("prob_normal_n5")
    mu, sg = _mu_sigma(fx)

    def f(z, p):
        return (norm.cdf(z, p[0], p[1]) - norm.cdf(z, p[4], p[5]) * norm.cdf(z, p[2], p[3])) * norm.pdf(z, p[4], p[5])
    got = probabilistic_normal_depth(mu, sg, f=f)
    _close(got["depths"].to_numpy(dtype=float), _want(fx), atol=1e-10)


def test_poisson_finite_where_the_reference_overflows():
    """The reference returns NaN for lim >= 172 (its default 1000 included) and where lam^z z! overflows; here the
    finite sum its formula denotes."""
    from statdepth_amd import probabilistic_poisson_depth
    for name, lim in (("prob_rec_poisson_default_lim", 1000), ("prob_rec_poisson_lim172", 172),
                      ("prob_rec_poisson_big_rate", 150)):
        fx = load_golden(name)
        assert np.isnan(_want(fx)).any()
        df = _frame(fx)
        got = probabilistic_poisson_depth(df, lim=lim) if name != "prob_rec_poisson_default_lim" else probabilistic_poisson_depth(df)
        _rel_close(got.to_numpy(), poisson_sums(df.to_numpy(), lim) / math.comb(df.shape[0], 2), 1e-12)


def test_poisson_to_compute_selects_targets():
    from statdepth_amd import probabilistic_poisson_depth
    fx = load_golden("prob_rec_poisson_to_compute")
    df = _frame(fx)
    full = probabilistic_poisson_depth(df, lim=60)
    _close(full.to_numpy(), _want(fx), rtol=1e-12)
    part = probabilistic_poisson_depth(df, to_compute=[3, 1], lim=60)
    assert list(part.index) == [3, 1]
    assert np.array_equal(part.to_numpy(), full.loc[[3, 1]].to_numpy())


# ---------------------------------------------------------------- engine vs the restatements
@pytest.mark.parametrize("n,seed", [(3, 1), (17, 2), (300, 3), (2500, 4)])
def test_normal_engine_moderate(eng, n, seed):
    rng = np.random.default_rng(seed)
    mu = rng.normal(0, 5, n)
    sg = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), n))     # six decades of scales
    if n > 3:
        mu[:3] = mu[3]                                          # ties
        sg[:3] = sg[3]
    got = eng.prob_normal_sums(mu, sg) / math.comb(n, 2)
    want = normal_sums(mu, sg) / math.comb(n, 2)
    assert np.max(np.abs(got - want)) <= 1e-12


@pytest.mark.parametrize("T,n,lim,lo,hi,seed", [
    (3, 3, 2, 0.1, 5, 1),            # one z
    (4, 9, 40, 1e-3, 1e1, 2),
    (2, 40, 300, 1e-3, 1e4, 3),      # rates far beyond lim
    (3, 300, 120, 0.5, 60, 4),       # two column blocks
    (2, 12, 5000, 1e-3, 1e4, 5),     # the whole bulk of lam = 1e4 inside lim
    (5, 7, 1, 0.1, 5, 6),            # lim = 1: empty z range
])
def test_poisson_engine_adversarial(eng, T, n, lim, lo, hi, seed):
    rng = np.random.default_rng(seed)
    lam = np.exp(rng.uniform(np.log(lo), np.log(hi), size=(T, n)))
    lam[0, min(2, n - 1)] = 0.0
    got = eng.prob_poisson_sums(lam, lim)
    want = poisson_sums(lam, lim)
    if lim <= 1:
        assert (got == 0).all()
        return
    pos = want > 0
    assert (got[~pos] == 0).all()
    _rel_close(got[pos], want[pos], 1e-12)


# ---------------------------------------------------------------- scale: many launches / many column blocks
def test_normal_scale_n50000(eng):
    rng = np.random.default_rng(11)
    n = 50_000
    mu = rng.normal(0, 1, n) * np.exp(rng.uniform(0, 3, n))
    sg = np.exp(rng.uniform(np.log(0.05), np.log(20), n))
    got = eng.prob_normal_sums(mu, sg)                          # every target
    tg = np.random.default_rng(12).choice(n, 64, replace=False)
    c = math.comb(n, 2)
    assert np.max(np.abs(got[tg] / c - normal_sums(mu, sg, tg) / c)) <= 1e-12
    assert np.array_equal(eng.prob_normal_sums(mu, sg, tg), got[tg])


def test_poisson_scale_64x4096(eng):
    rng = np.random.default_rng(13)
    T, n, lim = 64, 4096, 600
    lam = np.exp(rng.uniform(np.log(0.05), np.log(400), size=(T, n)))
    tg = np.sort(np.random.default_rng(14).choice(n, 64, replace=False))
    got = eng.prob_poisson_sums(lam, lim, tg)
    _rel_close(got, poisson_sums(lam, lim, tg), 1e-12)


# ---------------------------------------------------------------- determinism, bitwise
def test_normal_bitwise_determinism(eng, xcheck):
    rng = np.random.default_rng(21)
    n = 5000
    mu, sg = rng.normal(0, 2, n), np.exp(rng.uniform(-2, 2, n))
    a = eng.prob_normal_sums(mu, sg)
    assert np.array_equal(a, eng.prob_normal_sums(mu, sg))
    perm = np.random.default_rng(22).permutation(n)[:700]
    assert np.array_equal(eng.prob_normal_sums(mu, sg, perm), a[perm])
    for units in (1, 3, 7):                                     # launches of 1, 3, 7 workgroups: split inside targets
        with xcheck(SD_PROB_LAUNCH_UNITS=units):
            assert np.array_equal(eng.prob_normal_sums(mu, sg, perm[:40]), a[perm[:40]])


def test_poisson_bitwise_determinism(eng, xcheck):
    rng = np.random.default_rng(23)
    T, n, lim = 9, 700, 90
    lam = np.exp(rng.uniform(np.log(0.01), np.log(80), size=(T, n)))
    a = eng.prob_poisson_sums(lam, lim)
    assert np.array_equal(a, eng.prob_poisson_sums(lam, lim))
    perm = np.random.default_rng(24).permutation(n)[:100]
    assert np.array_equal(eng.prob_poisson_sums(lam, lim, perm), a[perm])
    for rows in (1, 2, 4):                                      # one, two, four rows per launch
        with xcheck(SD_PROB_LAUNCH_UNITS=rows):
            assert np.array_equal(eng.prob_poisson_sums(lam, lim, perm), a[perm])


def test_public_api_to_compute_equals_full():
    from statdepth_amd import probabilistic_poisson_depth
    rng = np.random.default_rng(25)
    df = pd.DataFrame(np.exp(rng.uniform(-1, 3, size=(6, 30))), columns=[f"c{i}" for i in range(30)])
    full = probabilistic_poisson_depth(df, lim=200)
    s = ["c29", "c0", "c7", "c7"]
    part = probabilistic_poisson_depth(df, to_compute=s, lim=200)
    assert list(part.index) == s
    assert np.array_equal(part.to_numpy(), full.loc[s].to_numpy())
