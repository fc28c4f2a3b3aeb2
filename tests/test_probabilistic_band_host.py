"""ProbabilisticDepth (K9, sd_prob_band_sums) without a GPU: a numpy oracle of the containment probability against mpmath,
the factory's argument checks (all before any device call), its import paths and signature, and the C ABI's refusals.

The numpy oracle (`band_p`, `band_sums`) is imported by tests/test_probabilistic_band_gpu.py.  It takes Phi2 from Owen's T
(scipy.special.owens_t), an algorithm independent of the kernel's BVND; the mpmath form integrates
int phi_i [F_j (1 - F_k) + F_k (1 - F_j)] adaptively, split at the means.
"""
import ctypes
import inspect

import mpmath as mp
import numpy as np
import pandas as pd
import pytest
from scipy.special import ndtr, owens_t


# ---------------------------------------------------------------- numpy oracle (Owen's T)
def _phi2_owen(x, y, rho, c, omr):
    """Phi2(x, y; rho) = Phi(x)/2 + Phi(y)/2 - T(x, ax) - T(y, ay) - beta, with c = sqrt(1 - rho^2) and omr = 1 - rho
    given to full accuracy; a zero argument is the limit from above."""
    x, y = np.broadcast_arrays(x, y)
    with np.errstate(divide='ignore', invalid='ignore'):
        ax = ((y - x) + omr * x) / (x * c)
        ay = ((x - y) + omr * y) / (y * c)
        tx = np.where(x == 0, np.sign(y) * 0.25, owens_t(x, np.where(x == 0, 0.0, ax)))
        ty = np.where(y == 0, np.sign(x) * 0.25, owens_t(y, np.where(y == 0, 0.0, ay)))
    beta = np.where((x * y < 0) | ((x * y == 0) & (x + y < 0)), 0.5, 0.0)
    both0 = (x == 0) & (y == 0)
    v = 0.5 * ndtr(x) + 0.5 * ndtr(y) - tx - ty - beta
    # x = y = 0: 1/4 + asin(rho) / 2 pi, with acos(rho) = atan2(c, rho) from the accurate c (asin(rho) loses it as rho -> 1)
    return np.where(both0, 0.5 - np.arctan2(c, rho) / (2 * np.pi), v)


def band_p(mi, vi, mj, vj, mk, vk):
    """P(min(X_j, X_k) <= X_i <= max(X_j, X_k)), X_c ~ N(m_c, v_c) independent (v_c = 0: a point mass); broadcasts.
    Measured against tests/golden/pairs_band.json (test_prob_pairs_host.py): 4.8e-16 absolute at worst, but up to 9e-11
    relative for |h| <= 12, since ndtr + ndtr - 2 Phi2 cancels where p is small."""
    mi, vi, mj, vj, mk, vk = np.broadcast_arrays(*[np.asarray(a, dtype=np.float64) for a in (mi, vi, mj, vj, mk, vk)])
    si, sj, sk = np.sqrt(vi), np.sqrt(vj), np.sqrt(vk)
    out = np.empty(mi.shape)
    with np.errstate(divide='ignore', invalid='ignore'):
        # sigma_i = 0: 1 - a_j a_k - b_j b_k, written as a_j b_k + b_j a_k + e_j + e_k - e_j e_k
        def abe(m, s):
            z = (m - mi) / s
            a = np.where(s > 0, ndtr(z), (m > mi).astype(float))
            b = np.where(s > 0, ndtr(-z), (m < mi).astype(float))
            e = np.where(s > 0, 0.0, (m == mi).astype(float))
            return a, b, e
        aj, bj, ej = abe(mj, sj)
        ak, bk, ek = abe(mk, sk)
        p0 = aj * bk + bj * ak + ej + ek - ej * ek
        # general: D_c = (X_i - X_c) / s_c ~ N(h_c, 1), corr rho; p = P(D_j, D_k differ in sign)
        s_j, s_k = np.hypot(si, sj), np.hypot(si, sk)
        hj, hk = (mi - mj) / s_j, (mi - mk) / s_k
        gj, gk = si / s_j, si / s_k
        uj, uk = (sj / s_j) ** 2, (sk / s_k) ** 2
        rho = gj * gk
        c2 = uj + gj * gj * uk                           # 1 - rho^2 without cancellation
        c = np.sqrt(c2)
        omr = c2 / (1 + rho)
        flip = hj + hk > 0                               # reflect so that the Phi terms are the small tails
        x, y = np.where(flip, -hj, hj), np.where(flip, -hk, hk)
        pg = ndtr(x) + ndtr(y) - 2 * _phi2_owen(x, y, rho, np.where(c > 0, c, 1.0), omr)
        # sigma_j = sigma_k = 0 < sigma_i: Phi(hmax) - Phi(hmin) from the tail that keeps digits
        lo, hi = np.minimum(hj, hk), np.maximum(hj, hk)
        pd_ = np.where(hi > 0, ndtr(-lo) - ndtr(-hi), ndtr(hi) - ndtr(lo))
    out = np.where(si == 0, p0, np.where((sj == 0) & (sk == 0), pd_, pg))
    return out


def band_sums(mu, var, relax, targets=None, members=None):
    """Unnormalised sums of sd_prob_band_sums: per target, over pairs j < k of its others, sum_t p or prod_t p."""
    mu, var = np.asarray(mu, dtype=np.float64), np.asarray(var, dtype=np.float64)
    T, n = mu.shape
    tg = range(n) if targets is None else targets
    out = []
    for q, i in enumerate(tg):
        others = [c for c in range(n) if c != i] if members is None else [c for c in members[q] if c >= 0 and c != i]
        others = np.asarray(others, dtype=np.int64)
        if len(others) < 2:
            out.append(0.0)
            continue
        a, b = np.triu_indices(len(others), 1)
        j, k = others[a], others[b]
        acc = np.zeros(len(j)) if relax else np.ones(len(j))
        for t in range(T):
            p = band_p(mu[t, i], var[t, i], mu[t, j], var[t, j], mu[t, k], var[t, k])
            acc = acc + p if relax else acc * p
        out.append(float(acc.sum()))
    return np.array(out)


# ---------------------------------------------------------------- mpmath: the 1-D integral
def mp_band_p(mi, vi, mj, vj, mk, vk):
    mp.mp.dps = 30
    mi, vi, mj, vj, mk, vk = (mp.mpf(float(v)) for v in (mi, vi, mj, vj, mk, vk))

    def F(m, v, x):
        if v == 0:
            return mp.mpf(1) if x >= m else mp.mpf(0)
        return mp.ncdf(x, m, mp.sqrt(v))

    if vi == 0:
        def ab(m, v):
            if v == 0:
                return mp.mpf(m > mi), mp.mpf(m < mi)
            b = mp.ncdf(mi, m, mp.sqrt(v))
            return 1 - b, b
        (aj, bj), (ak, bk) = ab(mj, vj), ab(mk, vk)
        return 1 - aj * ak - bj * bk
    si = mp.sqrt(vi)
    f = lambda x: mp.npdf(x, mi, si) * (F(mj, vj, x) * (1 - F(mk, vk, x)) + F(mk, vk, x) * (1 - F(mj, vj, x)))
    scales = [si] + [mp.sqrt(v) for v in (vj, vk) if v > 0]
    pts = {mi, mj, mk}
    for c0 in (mi, mj, mk):
        for s in scales:
            for z in (-8, -2, 2, 8):
                pts.add(c0 + z * s)
    return mp.quad(f, [-mp.inf] + sorted(pts) + [mp.inf])


def special_triples():
    """(mi, vi, mj, vj, mk, vk): rho -> 1, |h| up to 35, h = 0, every zero-variance case, ties."""
    return [
        (0, 1, 0, 1, 0, 1),                              # p = 1/3
        (0, 1e4, 0.3, 1e-4, -0.2, 1e-4),                 # rho -> 1: sigma_i = 100, sigma_j = sigma_k = 0.01
        (0, 1e4, 0.3, 1e-4, 0.3, 1e-4),
        (0, 1e4, 250.0, 1e-4, -40.0, 1e-4),
        (35, 1, 0, 0, 0, 0),                             # |h| = 35, point masses
        (35 * np.sqrt(2), 1, 0, 1, 0, 1),                # h = 35
        (-35 * np.sqrt(2), 1, 0, 1, 1, 1),
        (10, 1, 0, 1, 0.5, 1),
        (-8, 1, 0, 1, 0.5, 1),
        (5, 1, 0, 0.01, 0, 0.01),
        (0.5, 2, 0.5, 3, 0.5, 0.1),                      # h = 0 for both
        (0.5, 2, 0.5, 3, 1.5, 0.1),                      # h_j = 0
        (0, 0, 1, 1, -1, 1),                             # sigma_i = 0
        (0, 0, 1, 0, 0, 1),                              # sigma_i = sigma_j = 0
        (0, 0, 0, 0, 0, 0),                              # every variance zero, ties
        (0, 0, 1, 0, -1, 0),
        (0, 0, 1, 0, 2, 0),
        (0, 0, 0, 0, 2, 0),
        (0, 1, 1, 0, 2, 0),                              # sigma_j = sigma_k = 0 < sigma_i
        (0, 1, 1, 0, -2, 0),
        (0, 1, 0, 0, 0, 0),
        (0, 1, 30, 0, 31, 0),
        (0, 1, -30, 0, -29.5, 0),
        (3, 2, 0, 1e-6, 0.1, 3),                         # one near point mass
        (0, 1, 0.5, 0, 0.7, 1e-20),
        (0, 1e-6, 1, 1e6, -1, 1e6),                      # rho -> 0
    ]


def random_triples(seed, count, zero_frac=0.1):
    rng = np.random.default_rng(seed)
    m = rng.normal(0, 3, (count, 3))
    v = np.exp(rng.uniform(np.log(1e-6), np.log(1e6), (count, 3)))
    v[rng.random((count, 3)) < zero_frac] = 0.0
    return [(m[r, 0], v[r, 0], m[r, 1], v[r, 1], m[r, 2], v[r, 2]) for r in range(count)]


def test_oracle_matches_mpmath():
    triples = special_triples() + random_triples(1, 14)
    assert len(triples) >= 40
    A = np.array(triples, dtype=np.float64)
    got = band_p(*A.T)
    for g, tr in zip(got, triples):
        want = mp_band_p(*tr)
        assert abs(g - float(want)) <= 1e-15, (tr, g, want)
        assert 0.0 <= g <= 1.0


def test_oracle_closed_values():
    assert band_p(0, 1, 0, 1, 0, 1) == pytest.approx(1 / 3, rel=1e-15, abs=0)
    assert band_p(0, 0, 0, 0, 0, 0) == 1.0 and band_p(0, 0, 1, 0, 2, 0) == 0.0 and band_p(1, 0, 1, 0, 2, 0) == 1.0
    mu = np.zeros((3, 5))
    assert band_sums(mu, np.ones((3, 5)), True)[0] == pytest.approx(6 * 3 / 3, rel=1e-15)


# ---------------------------------------------------------------- the factory: checks before any device call
def _frames(T=6, n=5, seed=0):
    rng = np.random.default_rng(seed)
    cols = [f"c{i}" for i in range(n)]
    return (pd.DataFrame(rng.normal(size=(T, n)), columns=cols),
            pd.DataFrame(rng.uniform(0.1, 1.0, size=(T, n)), columns=cols))


@pytest.fixture
def no_device(monkeypatch):
    from statdepth_amd import engine

    def refuse(*a, **k):
        raise AssertionError("device call before validation")
    monkeypatch.setattr(engine, "prob_band_sums", refuse)


def test_validation_before_device(no_device):
    from statdepth_amd import ProbabilisticDepth
    df, s2 = _frames()
    bad = [
        (s2.iloc[:, :4], ValueError),                    # shape
        (s2.set_axis([f"d{i}" for i in range(5)], axis=1), ValueError),   # column labels
        (s2.set_axis(list(range(10, 16)), axis=0), ValueError),           # index
        (s2.to_numpy(), ValueError),                     # not a frame
        (s2 * -1.0, ValueError),                         # negative variances
    ]
    for sig, exc in bad:
        with pytest.raises(exc):
            ProbabilisticDepth(df, sig)
    for v, frame in ((np.nan, 's2'), (np.inf, 's2'), (np.nan, 'df'), (-np.inf, 'df')):
        d, s = df.copy(), s2.copy()
        (s if frame == 's2' else d).iloc[2, 3] = v
        with pytest.raises(ValueError):
            ProbabilisticDepth(d, s)
    with pytest.raises(NotImplementedError):
        ProbabilisticDepth(df, s2, J=3)
    dup = df.set_axis(["a", "b", "a", "c", "d"], axis=1)
    with pytest.raises(ValueError, match="unique"):
        ProbabilisticDepth(dup, s2.set_axis(["a", "b", "a", "c", "d"], axis=1))
    with pytest.raises(ValueError):                      # FunctionalDepth's checks: J < number of timepoints
        ProbabilisticDepth(df.iloc[:2], s2.iloc[:2])
    with pytest.raises(ValueError):
        ProbabilisticDepth(df, s2, relax=1)


def test_import_paths_and_signature():
    import statdepth_amd
    from statdepth_amd.depth import ProbabilisticDepth as a
    from statdepth_amd.depth.depth import ProbabilisticDepth as b
    assert statdepth_amd.ProbabilisticDepth is a is b
    assert "ProbabilisticDepth" in statdepth_amd.__all__
    sig = inspect.signature(a)
    assert list(sig.parameters)[:6] == ["data", "sigma2", "to_compute", "K", "J", "relax"]
    assert sig.parameters["K"].default is None and sig.parameters["J"].default == 2
    assert sig.parameters["relax"].default is False
    assert sig.parameters["device"].kind is inspect.Parameter.KEYWORD_ONLY


def test_abi_refusals_before_device_work():
    from statdepth_amd import _native
    lib = _native.load()
    fake = ctypes.c_void_p(256)                  # never dereferenced: every refusal happens before device work
    out = ctypes.c_void_p(512)
    E = _native
    f = lib.sd_prob_band_sums
    assert f(None, fake, 4, 5, None, 5, None, 0, 1, out, None) == E.SD_ERR_INVALID
    assert f(fake, None, 4, 5, None, 5, None, 0, 1, out, None) == E.SD_ERR_INVALID
    assert f(fake, fake, 4, 5, None, 5, None, 0, 1, None, None) == E.SD_ERR_INVALID
    assert b"null" in lib.sd_last_error()
    assert f(fake, fake, -4, 5, None, 5, None, 0, 1, out, None) == E.SD_ERR_INVALID
    assert f(fake, fake, 4, -5, None, -5, None, 0, 1, out, None) == E.SD_ERR_INVALID
    assert f(fake, fake, 4, 5, fake, -1, None, 0, 1, out, None) == E.SD_ERR_INVALID
    assert f(fake, fake, 4, 5, fake, 2, fake, -3, 0, out, None) == E.SD_ERR_INVALID
    assert f(fake, fake, 4, 5, None, 4, None, 0, 0, out, None) == E.SD_ERR_INVALID
    assert f(fake, fake, 2**40, 2**20, fake, 2**20, None, 0, 1, out, None) == E.SD_ERR_OVERFLOW
    assert f(fake, fake, 10**4, 10**4, fake, 10**4, None, 0, 0, out, None) == E.SD_ERR_UNSUPPORTED
    assert b"cap" in lib.sd_last_error()
    assert f(fake, fake, 4, 5, fake, 0, None, 0, 1, out, None) == E.SD_OK      # nothing to do
