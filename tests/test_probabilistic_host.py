"""Probabilistic depths (K8, _uncertainty.py) without a GPU: two independent restatements of each closed form -- numpy /
scipy and mpmath -- against the reference's fixtures, the records of where this project departs from the reference,
the host's argument checks and the C ABI's refusals before any device work.

The numpy restatements (`normal_sums`, `poisson_sums`) are imported by tests/test_probabilistic_gpu.py as its oracle.
The GPU kernel evaluates Owen's T by Gauss-Legendre in x; the oracle here uses Genz's form, Gauss-Legendre in the angle
theta = asin(r) of Phi2's derivative in r, and the mpmath form integrates Owen's T adaptively.
"""
import ctypes
import json
import math
import os
from itertools import combinations

import mpmath as mp
import numpy as np
import pandas as pd
import pytest
from scipy.special import ndtr
from scipy.stats import poisson

from conftest import GOLDEN, golden_names, load_golden

_GL_T, _GL_W = np.polynomial.legendre.leggauss(20)


# ---------------------------------------------------------------- normal: numpy / scipy (Genz's angle form)
def _phi2_zero(h, rho):
    """Phi2(0, h; rho) = Phi(0) Phi(h) + (1 / 2 pi) int_0^asin(rho) exp(-h^2 / (2 cos^2 theta)) d theta.
    Measured against tests/golden/pairs_normal.json (test_prob_pairs_host.py): a pair term of `normal_sums` is within
    1.1e-16 absolute."""
    h = np.asarray(h, dtype=np.float64)
    th0 = np.arcsin(rho)
    th = 0.5 * th0[..., None] * (1.0 + _GL_T)
    f = np.exp(-0.5 * h[..., None] ** 2 / np.cos(th) ** 2)
    return 0.5 * ndtr(h) + (0.5 * th0 * (f * _GL_W).sum(-1)) / (2 * np.pi)


def normal_sums(mu, sigma, targets=None):
    mu = np.asarray(mu, dtype=np.float64)
    sg = np.asarray(sigma, dtype=np.float64)
    n = len(mu)
    # h and rho in extended precision (x87 long double: 64-bit mantissa, 15-bit exponent), so that neither a difference
    # of means nor a sum of squares leaves the range and subnormal stds keep their bits -- another route than the
    # kernel's power-of-two scaling.  Where long double is double, the mpmath fixture (pairs_normal.json) alone covers
    # the ends of the range.
    mul, sgl = mu.astype(np.longdouble), sg.astype(np.longdouble)
    idx = np.arange(n)
    out = []
    for k in (range(n) if targets is None else targets):
        o = idx != k
        m = idx[o]
        with np.errstate(over='ignore'):                                # h beyond the fp64 range is +-inf
            s = np.sqrt(sgl[o] ** 2 + sgl[k] ** 2)
            h = ((mul[k] - mul[o]) / s).astype(np.float64)
            rho = (sgl[k] / (np.sqrt(np.longdouble(2.0)) * s)).astype(np.float64)
        wa = (n - 1 - m) - (k > m)
        wb = m - (k < m)
        out.append(float(np.sum(ndtr(h) * wa) - np.sum(_phi2_zero(h, rho) * wb)))
    return np.array(out)


def normal_depths(mu, sigma):
    n = len(mu)
    with np.errstate(divide='ignore', invalid='ignore'):
        return normal_sums(mu, sigma) / np.float64(math.comb(n, 2))


# ---------------------------------------------------------------- normal: mpmath (Owen's T, explicit pairs)
def normal_depths_mp(mu, sigma, dps=30):
    mp.mp.dps = dps
    n = len(mu)
    out = []
    for k in range(n):
        s = mp.mpf(0)
        others = [c for c in range(n) if c != k]
        for i, j in combinations(others, 2):
            def AB(m):
                sm, sk = mp.mpf(sigma[m]), mp.mpf(sigma[k])
                sq = mp.sqrt(sm ** 2 + sk ** 2)
                h = (mp.mpf(mu[k]) - mp.mpf(mu[m])) / sq
                a = sk / mp.sqrt(2 * sm ** 2 + sk ** 2)
                T = mp.quad(lambda x: mp.exp(-h ** 2 * (1 + x ** 2) / 2) / (1 + x ** 2), [0, a]) / (2 * mp.pi)
                return mp.ncdf(h), mp.ncdf(h) / 2 + T
            s += AB(i)[0] - AB(j)[1]
        out.append(float(s / math.comb(n, 2)) if n > 1 else float('nan'))
    return np.array(out)


# ---------------------------------------------------------------- Poisson: numpy / scipy (column scans)
def poisson_sums(lam, lim, targets=None):
    """sum_t sum_{z=1}^{lim-1} p_f(z) S_f(t, z), S_f = A.P + B.P + A.L B.U (columns before / after f)."""
    lam = np.asarray(lam, dtype=np.float64)
    T, n = lam.shape
    tg = np.arange(n) if targets is None else np.asarray(targets)
    out = np.zeros(len(tg))
    if lim <= 1:
        return out
    z = np.arange(1, lim)[:, None]
    for t in range(T):
        l = lam[t][None, :]
        p = poisson.pmf(z, l)
        L = poisson.cdf(z, l)
        U = poisson.sf(z - 1, l)
        zero = np.zeros((len(z), 1))
        PL = np.concatenate([zero, np.cumsum(L, axis=1)[:, :-1]], axis=1)          # sum of L before the column
        SU = np.concatenate([np.cumsum(U[:, ::-1], axis=1)[:, ::-1][:, 1:], zero], axis=1)   # sum of U after it
        F = np.concatenate([zero, np.cumsum(U * PL, axis=1)[:, :-1]], axis=1)      # pairs entirely before
        G = np.concatenate([np.cumsum((L * SU)[:, ::-1], axis=1)[:, ::-1][:, 1:], zero], axis=1)  # entirely after
        S = F + PL * SU + G
        out += (p * S).sum(axis=0)[tg]
    return out


# ---------------------------------------------------------------- Poisson: mpmath (explicit pairs, exact tails)
def poisson_depths_mp(lam, lim, dps=30):
    mp.mp.dps = dps
    lam = np.asarray(lam, dtype=np.float64)
    T, n = lam.shape
    out = []
    for f in range(n):
        s = mp.mpf(0)
        for t in range(T):
            lm = [mp.mpf(v) for v in lam[t]]
            for z in range(1, lim):
                pf = mp.exp(-lm[f]) * lm[f] ** z / mp.factorial(z) if lm[f] else mp.mpf(0)
                if pf == 0:
                    continue
                Lz = [mp.gammainc(z + 1, v, regularized=True) if v else mp.mpf(1) for v in lm]   # P(X <= z), upper
                Uz = [mp.gammainc(z, 0, v, regularized=True) if v else mp.mpf(0) for v in lm]    # P(X >= z), lower
                cols = [c for c in range(n) if c != f]
                s += pf * mp.fsum(Lz[i] * Uz[j] for i, j in combinations(cols, 2))
        c2 = math.comb(T, 2)
        out.append(float(s / c2) if c2 else (float('nan') if s == 0 else float('inf')))
    return np.array(out)


def _dec(v):
    return float(v) if isinstance(v, str) else v


def _frame(fx):
    from conftest import frame_df
    return frame_df(fx["input"])


def _mu_sigma(fx):
    return (np.array([_dec(v) for v in fx["input"]["means"]]), np.array([_dec(v) for v in fx["input"]["stds"]]))


def _want(fx):
    return np.array([_dec(v) for v in fx["depths"]], dtype=np.float64)


def _close(got, want, atol=0.0, rtol=0.0):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    assert (np.isnan(got) == np.isnan(want)).all() and (np.isinf(got) == np.isinf(want)).all(), (got, want)
    ok = np.isfinite(want)
    assert np.all(np.abs(got[ok] - want[ok]) <= atol + rtol * np.abs(want[ok])), (got, want)


# ---------------------------------------------------------------- oracles against the reference
@pytest.mark.parametrize("name", golden_names(kind="prob_normal"))
def test_normal_oracles_match_reference(name):
    fx = load_golden(name)
    mu, sg = _mu_sigma(fx)
    _close(normal_depths(mu, sg), _want(fx), atol=1e-10)
    if len(mu) <= 7:
        _close(normal_depths_mp(mu, sg), _want(fx), atol=1e-10)


def test_normal_oracles_agree_with_each_other():
    rng = np.random.default_rng(5)
    mu = rng.normal(0, 3, 6)
    sg = np.exp(rng.uniform(np.log(0.01), np.log(30), 6))
    _close(normal_depths(mu, sg), normal_depths_mp(mu, sg), atol=1e-14)


@pytest.mark.parametrize("name", golden_names(kind="prob_poisson"))
def test_poisson_oracles_match_reference(name):
    fx = load_golden(name)
    df = _frame(fx)
    lim = fx["call"]["lim"]
    T = df.shape[0]
    with np.errstate(divide='ignore', invalid='ignore'):
        got = np.float64(1.0) / np.float64(math.comb(T, 2)) * poisson_sums(df.to_numpy(), lim)
    _close(got, _want(fx), atol=1e-300, rtol=1e-12)
    if df.size <= 24 and lim <= 100:
        _close(poisson_depths_mp(df.to_numpy(), lim), _want(fx), atol=1e-300, rtol=1e-12)


def test_poisson_fixtures_pin_the_pair_orientation():
    """A column permutation changes the depths beyond a relabelling: i is the earlier column of each pair."""
    for a, b, order in (("prob_poisson_spread_T4_n8", "prob_poisson_spread_T4_n8_perm", [5, 2, 7, 0, 3, 6, 1, 4]),
                        ("prob_poisson_wide_T5_n7", "prob_poisson_wide_T5_n7_perm", [6, 3, 0, 5, 1, 4, 2])):
        A, B = _want(load_golden(a)), _want(load_golden(b))
        assert not np.allclose(A[order], B, rtol=1e-6)


# ---------------------------------------------------------------- records of the departures
def test_record_default_lim_is_nan_in_the_reference():
    """lim >= 172 (the default is 1000): factorial(171) and gamma(172) are inf, every term inf / inf.  Here the finite
    sum the formula denotes, which for these rates equals the sum at lim = 171 to the last bits."""
    for name in ("prob_rec_poisson_default_lim", "prob_rec_poisson_lim172"):
        fx = load_golden(name)
        assert np.isnan(_want(fx)).all()
    fx = load_golden("prob_rec_poisson_lim171")
    assert np.isfinite(_want(fx)).all()
    df = _frame(fx)
    full = poisson_sums(df.to_numpy(), 1000) / math.comb(3, 2)
    _close(full, _want(fx), rtol=1e-12)


def test_record_overflowing_rate_is_nan_in_the_reference():
    fx = load_golden("prob_rec_poisson_big_rate")
    assert np.isnan(_want(fx)).any()
    got = poisson_sums(_frame(fx).to_numpy(), 150)
    assert np.isfinite(got).all() and (got > 0).all()


def test_record_to_compute_is_ignored_by_the_reference():
    fx = load_golden("prob_rec_poisson_to_compute")
    assert fx["call"]["to_compute"] == [1, 3] and fx["index"] == fx["input"]["columns"]


@pytest.mark.parametrize("name", ["prob_rec_normal_nan_mean", "prob_rec_normal_zero_std", "prob_rec_poisson_negative",
                                  "prob_rec_poisson_nan"])
def test_record_invalid_parameters_give_nan_in_the_reference(name):
    assert np.isnan(_want(load_golden(name))).any()


# ---------------------------------------------------------------- refusals, no device needed
def test_invalid_parameters_are_refused_before_any_device_work():
    from statdepth_amd import probabilistic_normal_depth, probabilistic_poisson_depth
    fx = load_golden("prob_rec_normal_len")
    assert fx["raises"] == "ValueError"
    with pytest.raises(ValueError) as e:
        probabilistic_normal_depth([0.0, 1.0, 2.0], [1.0, 1.0])
    assert str(e.value) == fx["message"]
    for name, match in (("prob_rec_normal_nan_mean", "means must be finite"),
                        ("prob_rec_normal_zero_std", "stds must be finite and positive")):
        mu, sg = _mu_sigma(load_golden(name))
        with pytest.raises(ValueError, match=match):
            probabilistic_normal_depth(mu, sg)
    with pytest.raises(ValueError, match="stds must be finite and positive"):
        probabilistic_normal_depth([0.0, 1.0, 2.0], [1.0, np.inf, 1.0])
    with pytest.raises(ValueError, match="stds must be finite and positive"):
        probabilistic_normal_depth([0.0, 1.0, 2.0], [1.0, -1.0, 1.0])
    for name in ("prob_rec_poisson_negative", "prob_rec_poisson_nan"):
        with pytest.raises(ValueError, match="finite and non-negative"):
            probabilistic_poisson_depth(_frame(load_golden(name)), lim=50)
    df = pd.DataFrame(np.ones((3, 4)))
    df.iloc[1, 1] = np.inf
    with pytest.raises(ValueError, match="finite and non-negative"):
        probabilistic_poisson_depth(df, lim=50)
    with pytest.raises(KeyError):
        probabilistic_poisson_depth(pd.DataFrame(np.ones((3, 4))), to_compute=[7], lim=5)


def test_abi_refusals_before_device_work():
    from statdepth_amd import _native
    lib = _native.load()
    fake = ctypes.c_void_p(256)                  # never dereferenced: every refusal happens before device work
    out = ctypes.c_void_p(512)
    E = _native
    assert lib.sd_prob_normal_sums(None, fake, 10, None, 10, out, None) == E.SD_ERR_INVALID
    assert lib.sd_prob_normal_sums(fake, None, 10, None, 10, out, None) == E.SD_ERR_INVALID
    assert lib.sd_prob_normal_sums(fake, fake, 10, None, 10, None, None) == E.SD_ERR_INVALID
    assert b"null" in lib.sd_last_error()
    assert lib.sd_prob_normal_sums(fake, fake, -1, None, -1, out, None) == E.SD_ERR_INVALID
    assert lib.sd_prob_normal_sums(fake, fake, 10, fake, -2, out, None) == E.SD_ERR_INVALID
    assert lib.sd_prob_normal_sums(fake, fake, 10, None, 9, out, None) == E.SD_ERR_INVALID
    assert lib.sd_prob_normal_sums(fake, fake, 2**62, fake, 4, out, None) == E.SD_ERR_OVERFLOW
    assert lib.sd_prob_normal_sums(fake, fake, 10**8, None, 10**8, out, None) == E.SD_ERR_UNSUPPORTED
    assert b"cap" in lib.sd_last_error()
    assert lib.sd_prob_poisson_sums(None, 4, 5, 10, None, 5, out, None) == E.SD_ERR_INVALID
    assert lib.sd_prob_poisson_sums(fake, 4, 5, 10, None, 5, None, None) == E.SD_ERR_INVALID
    assert lib.sd_prob_poisson_sums(fake, -4, 5, 10, None, 5, out, None) == E.SD_ERR_INVALID
    assert lib.sd_prob_poisson_sums(fake, 4, -5, 10, None, -5, out, None) == E.SD_ERR_INVALID
    assert lib.sd_prob_poisson_sums(fake, 4, 5, 10, None, 4, out, None) == E.SD_ERR_INVALID
    assert lib.sd_prob_poisson_sums(fake, 2**40, 2**20, 2**10, fake, 1, out, None) == E.SD_ERR_OVERFLOW
    assert lib.sd_prob_poisson_sums(fake, 10**4, 10**4, 2**62, fake, 1, out, None) == E.SD_ERR_OVERFLOW
    assert b"overflows int64" in lib.sd_last_error()
    assert lib.sd_prob_poisson_sums(fake, 10**4, 10**4, 10**7, fake, 1, out, None) == E.SD_ERR_UNSUPPORTED


def test_engine_refuses_out_of_range_targets_on_the_host(monkeypatch):
    """The targets' range is checked on the host, before anything reaches the device."""
    from statdepth_amd import engine
    monkeypatch.setattr(engine, "_device", lambda device=None: "cpu")
    monkeypatch.setattr(engine._native, "require_device", lambda: None)
    with pytest.raises(IndexError):
        engine.prob_normal_sums(np.zeros(5), np.ones(5), [0, 5])
    with pytest.raises(IndexError):
        engine.prob_poisson_sums(np.ones((3, 5)), 10, [-1])


def test_fixture_kinds_are_new():
    """The existing parametrised tests select by kind; none of theirs appears here."""
    kinds = set()
    for fn in os.listdir(GOLDEN):
        if fn.startswith("prob_") and fn.endswith(".json"):
            with open(os.path.join(GOLDEN, fn)) as f:
                kinds.add(json.load(f)["kind"])
    assert kinds == {"prob_normal", "prob_poisson", "prob_record"}


def test_record_reference_quad_misses_a_narrow_integrand():
    """Means over three decades and stds from 0.05 to 20: the reference's quad returns 1.7e-16 for target 2, whose
    depth is 3.8e-5 by both closed-form oracles; every other target agrees within 1e-12."""
    fx = load_golden("prob_rec_normal_quad_spread_n8")
    mu, sg = _mu_sigma(fx)
    want = _want(fx)
    got = normal_depths(mu, sg)
    _close(np.delete(got, 2), np.delete(want, 2), atol=1e-12)
    assert want[2] < 1e-15 and abs(got[2] - 3.833e-5) < 1e-8
    _close(got[[2]], normal_depths_mp(mu, sg)[[2]], atol=1e-14)
