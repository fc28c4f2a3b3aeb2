"""ProbabilisticDepth on the GPU (K9, sd_prob_band_sums): single containment probabilities against the numpy oracle of
tests/test_probabilistic_band_host.py, closed values, bitwise agreement with FunctionalDepth at zero variance (plain and
K-block), whole depths against the oracle at moderate sizes and at scale, and bitwise determinism across calls, target
subsets and forced launch splits."""
import numpy as np
import pandas as pd
import pytest

from test_probabilistic_band_host import band_p, band_sums, random_triples, special_triples

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from statdepth_amd import engine
    return engine


def _rel_close(got, want, rtol, atol=1e-300):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and np.isfinite(got).all()
    err = np.abs(got - want)
    assert np.all(err <= rtol * np.abs(want) + atol), np.max(err / np.maximum(np.abs(want), atol))


def _frames(mu, var):
    cols = [f"c{i}" for i in range(mu.shape[1])]
    return pd.DataFrame(mu, columns=cols), pd.DataFrame(var, columns=cols)


def _noisy(T, n, seed, zero_frac=0.1):
    rng = np.random.default_rng(seed)
    mu = rng.normal(0, 1, (T, n))
    sd = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), (T, n)))
    sd[rng.random((T, n)) < zero_frac] = 0.0
    return mu, sd * sd


# ---------------------------------------------------------------- 1. single probabilities (n = 3, T = 1)
def test_single_probabilities(eng):
    """Absolute 5e-15 against `band_p`, whose own relative accuracy ends where p is small.  The relative bound of the
    kernel (|h| <= 12, against 40-digit values) is in tests/test_prob_pairs_gpu.py::test_band_regime_a."""
    triples = special_triples() + random_triples(2, 180) + random_triples(3, 20, zero_frac=0.5)
    worst = 0.0
    for tr in triples:
        mi, vi, mj, vj, mk, vk = tr
        mu, var = np.array([[mi, mj, mk]]), np.array([[vi, vj, vk]])
        want = band_p([mi, mj, mk], [vi, vj, vk], [mj, mi, mi], [vj, vi, vi], [mk, mk, mj], [vk, vk, vj])
        for relax in (True, False):
            got = eng.prob_band_sums(mu, var, relax)
            assert np.isfinite(got).all() and (got >= 0).all() and (got <= 1).all()
            worst = max(worst, float(np.max(np.abs(got - want))))
            assert np.all(np.abs(got - want) <= 5e-15), (tr, got, want)
    assert worst <= 5e-15


# ---------------------------------------------------------------- 2. closed value: equal means, equal variances
@pytest.mark.parametrize("n", [3, 5, 12])
def test_closed_value(n):
    from statdepth_amd import ProbabilisticDepth
    for T in (1, 4, 16, 50):
        df, s2 = _frames(np.full((max(T, 3), n), 0.7), np.full((max(T, 3), n), 2.5))
        T = df.shape[0]
        r = ProbabilisticDepth(df, s2, relax=True).to_numpy()
        _rel_close(r, np.full(n, (n - 2) / (3 * n)), 1e-15)
        s = ProbabilisticDepth(df, s2, relax=False).to_numpy()
        _rel_close(s, np.full(n, (n - 2) / n * 3.0 ** -T), T * 1e-15)
    df, s2 = _frames(np.zeros((2000, n)), np.ones((2000, n)))
    s = ProbabilisticDepth(df, s2, relax=False).to_numpy()
    assert np.all(s == 0.0)
    r = ProbabilisticDepth(df, s2, relax=True).to_numpy()
    assert np.isfinite(r).all()
    _rel_close(r, np.full(n, (n - 2) / (3 * n)), 1e-13)


# ---------------------------------------------------------------- 3. zero variance: FunctionalDepth's bits
@pytest.mark.parametrize("relax", [True, False])
def test_zero_variance_equals_functional_depth(relax):
    from statdepth_amd import FunctionalDepth, ProbabilisticDepth
    rng = np.random.default_rng(31)
    for T, n in ((8, 30), (40, 70)):
        mu = np.round(rng.normal(0, 0.3, (T, n)), 1)    # many ties
        df, s2 = _frames(mu, np.zeros((T, n)))
        want = FunctionalDepth([df], relax=relax)
        got = ProbabilisticDepth(df, s2, relax=relax)
        assert list(got.index) == list(want.index)
        assert np.array_equal(got.to_numpy(), want.to_numpy())
        sub = ["c5", "c0", "c29"]
        got = ProbabilisticDepth(df, s2, to_compute=sub, relax=relax)
        assert list(got.index) == sub
        assert np.array_equal(got.to_numpy(), FunctionalDepth([df], to_compute=sub, relax=relax).to_numpy())
        for K in (2, 3):
            np.random.seed(7)
            want = FunctionalDepth([df], K=K, relax=relax)
            np.random.seed(7)
            got = ProbabilisticDepth(df, s2, K=K, relax=relax)
            assert list(got.index) == list(want.index)
            assert np.array_equal(got.to_numpy(), want.to_numpy())
            # the pool shrinks to to_compute after the first target (the reference's draw rule): a reordered full set
            order = list(df.columns[::-1])
            np.random.seed(8)
            want = FunctionalDepth([df], to_compute=order, K=K, relax=relax)
            np.random.seed(8)
            got = ProbabilisticDepth(df, s2, to_compute=order, K=K, relax=relax)
            assert list(got.index) == order
            assert np.array_equal(got.to_numpy(), want.to_numpy())


# ---------------------------------------------------------------- 4. against the oracle
@pytest.mark.parametrize("n", [5, 17, 64])
@pytest.mark.parametrize("T", [3, 7, 33])
def test_against_oracle(eng, n, T):
    mu, var = _noisy(T, n, seed=100 * n + T)
    _rel_close(eng.prob_band_sums(mu, var, True), band_sums(mu, var, True), 1e-13)
    _rel_close(eng.prob_band_sums(mu, var, False), band_sums(mu, var, False), 1e-10)


def test_public_api_against_oracle():
    from scipy.special import binom
    from statdepth_amd import ProbabilisticDepth
    mu, var = _noisy(9, 20, seed=41)
    df, s2 = _frames(mu, var)
    got = ProbabilisticDepth(df, s2, relax=True)
    _rel_close(got.to_numpy(), band_sums(mu, var, True) / 9 / binom(20, 2), 1e-13)
    got = ProbabilisticDepth(df, s2)
    _rel_close(got.to_numpy(), band_sums(mu, var, False) / binom(20, 2), 1e-10)
    assert got.deepest(n=1).index[0] == got.ordered().index[0]
    assert got.get_data() is df


def test_members_against_oracle(eng):
    mu, var = _noisy(6, 150, seed=43)
    rng = np.random.default_rng(44)
    targets = np.array([3, 17, 17, 149, 0])
    mem = np.full((5, 90), -1, dtype=np.int32)
    for q, i in enumerate(targets):
        blk = rng.choice(150, 80 + q, replace=False)
        mem[q, :len(blk)] = blk                          # the target itself may be listed: skipped
    for relax, tol in ((True, 1e-13), (False, 1e-10)):
        _rel_close(eng.prob_band_sums(mu, var, relax, targets, mem), band_sums(mu, var, relax, targets, mem), tol)


# ---------------------------------------------------------------- 5. scale
@pytest.mark.parametrize("relax", [True, False])
def test_scale(eng, relax):
    T, n = 128, 600
    rng = np.random.default_rng(51)
    mu = rng.normal(0, 1, (T, n)) + rng.normal(0, 0.5, n)
    var = np.exp(rng.uniform(np.log(0.05), np.log(2.0), (T, n)))
    full = eng.prob_band_sums(mu, var, relax)
    tg = np.array([0, 77, 301, 455, 599])
    sub = eng.prob_band_sums(mu, var, relax, tg)
    assert np.array_equal(sub, full[tg])
    _rel_close(sub, band_sums(mu, var, relax, tg), 1e-13 if relax else 1e-10)


# ---------------------------------------------------------------- 6. determinism, bitwise
@pytest.mark.parametrize("relax", [True, False])
def test_bitwise_determinism(eng, xcheck, relax):
    mu, var = _noisy(37, 150, seed=61, zero_frac=0.05)
    var = var * 1e-2 + 1.0                               # products stay away from 0 over the 37 timepoints
    a = eng.prob_band_sums(mu, var, relax)
    assert np.array_equal(a, eng.prob_band_sums(mu, var, relax))
    perm = np.random.default_rng(62).permutation(150)[:40]
    assert np.array_equal(eng.prob_band_sums(mu, var, relax, perm), a[perm])
    for units in (1, 3, 7):                              # units and timepoints per launch: splits inside targets and t
        with xcheck(SD_PROB_LAUNCH_UNITS=units):
            assert np.array_equal(eng.prob_band_sums(mu, var, relax, perm[:12]), a[perm[:12]])
