"""Directional outlyingness of multivariate curves and the MS-plot's outlier rule (DirectionalOutlyingness, MSPlotOutliers;
K19), the part that needs no GPU: the numpy restatement of the device's records against a hand-computed case, Welford's
recurrence against the two-pass definition in 50-digit arithmetic, every refusal of the host layer with the engine never
reached, the indexing of the two forms, the outlier rule on restated records, the MCD alone, the cutoff's known answers and
the C ABI's declarations, sizes and refusals.

The restatement (`multi_outlyingness_records`) is a loop over the timepoints around K12's restatement
(tests/test_projection_host.py); tests/test_directional_gpu.py imports it as its oracle.  Every operation in it is one numpy
fp64 operation, i.e. one correctly rounded IEEE operation, in the order DESIGN §3 K19 states.
"""
import os
import re

import mpmath as mp
import numpy as np
import pandas as pd
import pytest
from scipy import stats

from statdepth_amd import DirectionalOutlyingness, MSPlotOutliers, engine
from statdepth_amd.depth.calculations import _containment, _directional
from statdepth_amd.depth.calculations._directional import (DirectionalOutlyingnessResult, MSPlotOutlierResult, _fast_mcd,
                                                            _hardin_rocke, _mcd_support_size, _ms_cutoff)

from test_halfspace_host import make_directions
from test_multi_cloud_host import KNOWN_P, KNOWN_U
from test_projection_host import projection_outlyingness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U53 = 2.0 ** -53


# ---------------------------------------------------------------- numpy restatement of the definition
def multi_outlyingness_records(P, U, targets=None, centres=False, curves=False):
    """fp64 [m, d + 1] = (M_0 .. M_(d-1), Q), the Welford record of the directional outlyingness over ascending t; with
    centres / curves the int64 [T] centres c_t and the fp64 [m, T, d] array O_t as well (a tuple in that order)."""
    P = np.asarray(P, dtype=np.float64)
    n, T, d = P.shape
    tg = np.arange(n) if targets is None else np.asarray(targets, dtype=np.int64)
    m = len(tg)
    M, Q = np.zeros((m, d), dtype=np.float64), np.zeros(m, dtype=np.float64)
    cen, cur = np.zeros(T, dtype=np.int64), np.zeros((m, T, d), dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore', under='ignore'):
        for t in range(T):
            o = projection_outlyingness(P[:, t, :], U)                     # every curve: never NaN
            c = int(np.argmin(o))                                          # the first minimum: the lowest index
            diff = P[tg, t, :] - P[c, t, :]
            s = np.zeros(m, dtype=np.float64)
            for e in range(d):
                s = s + diff[:, e] * diff[:, e]
            r = np.sqrt(s)
            cnt = np.float64(t + 1)
            for e in range(d):
                O = np.where(r == 0.0, 0.0, o[tg] * (diff[:, e] / r))
                delta = O - M[:, e]
                M[:, e] = M[:, e] + delta / cnt
                Q = Q + delta * (O - M[:, e])
                cur[:, t, e] = O
            cen[t] = c
    rec = np.concatenate([M, Q[:, None]], axis=1)
    if not centres and not curves:
        return rec
    return (rec,) + ((cen,) if centres else ()) + ((cur,) if curves else ())


def restated_engine(P, U, targets=None, device=None, algo='auto', ws_bytes=None, centres=False, curves=False):
    """engine.multi_outlyingness_moments, restated."""
    return multi_outlyingness_records(P, U, targets, centres=centres, curves=curves)


def _frames(P):
    return [pd.DataFrame(P[i]) for i in range(P.shape[0])]


def _curves(n=6, T=5, d=3, seed=1):
    return np.random.default_rng(seed).normal(size=(n, T, d))


def planted_design():
    """n = 100 curves, T = 50, d = 2: Gaussian processes with covariance exp(-|s - t| / 0.3) on [0, 1], default_rng(1), and
    four planted outliers: curve 0 shifted by +8 in feature 0, curve 1 by -8 in feature 1, curve 2 with 6 sin(40 t) added
    to both features, curve 3 shifted by +10 in feature 0 on the second half."""
    n, T, d = 100, 50, 2
    t = np.linspace(0.0, 1.0, T)
    L = np.linalg.cholesky(np.exp(-np.abs(t[:, None] - t[None, :]) / 0.3))
    P = np.einsum('ts,nsd->ntd', L, np.random.default_rng(1).normal(size=(n, T, d)))
    P[0, :, 0] += 8.0
    P[1, :, 1] -= 8.0
    P[2] += 6.0 * np.sin(40.0 * t)[:, None]
    P[3, T // 2:, 0] += 10.0
    return np.ascontiguousarray(P)


PLANTED = {0, 1, 2, 3}


@pytest.fixture
def restated(monkeypatch):
    calls = []

    def fake(P, U, targets=None, **kw):
        calls.append((np.array(P), np.array(U), None if targets is None else np.array(targets), kw))
        return restated_engine(P, U, targets, **kw)
    monkeypatch.setattr(engine, 'multi_outlyingness_moments', fake)
    return calls


@pytest.fixture
def no_engine(monkeypatch):
    def boom(*a, **k):
        raise AssertionError('the engine was reached')
    monkeypatch.setattr(engine, 'multi_outlyingness_moments', boom)
    monkeypatch.setattr(engine, '_upload', boom)


# ---------------------------------------------------------------- the restatement, by hand
def test_known_answer_records_restated():
    """KNOWN_P, axes as directions.  t0: A (0,0) B (1,2) C (2,1): med = MAD = 1 on both axes, o = 1 for all three, so
    c_0 = 0 (A, the lowest index).  O_0(A) = 0 (r = 0), O_0(B) = (1, 2) / sqrt 5, O_0(C) = (2, 1) / sqrt 5.
    t1: A = B = (1,1), C (5,0): MAD = 0 on both axes, o = (0, 0, inf), c_1 = 0; A and B sit on the centre (r = 0: the zero
    vector), C: diff (4, -1), O_1(C) = inf * (4, -1) / sqrt 17 = (inf, -inf).
    Records over t = 0, 1: A: all 0.  B: after t0 M = (a, b), Q = 0 with a = 1 / sqrt 5, b = 2 / sqrt 5; at t1 O = 0,
    delta = -a, M_0 = a + (-a) / 2 = a / 2, Q += (-a) (0 - a / 2), likewise b: Q = a (a / 2) + b (b / 2) (= 1 / 2 exactly in
    real numbers).  C: M = (b, a) after t0; at t1 delta = inf, M_0 = inf, Q += inf * (inf - inf) = NaN, M_1 = -inf."""
    rec, cen, cur = multi_outlyingness_records(KNOWN_P, KNOWN_U, centres=True, curves=True)
    r5, r17 = np.sqrt(5.0), np.sqrt(17.0)
    a, b = 1.0 / r5, 2.0 / r5
    assert np.array_equal(cen, [0, 0])
    want = np.array([[[0.0, 0.0], [0.0, 0.0]], [[a, b], [0.0, 0.0]], [[b, a], [np.inf, -np.inf]]])
    assert np.array_equal(cur, want)
    qb = (-a) * (0.0 - a / 2.0) + (-b) * (0.0 - b / 2.0)
    assert abs(qb - 0.5) < 4 * U53
    assert np.array_equal(rec, np.array([[0.0, 0.0, 0.0], [a / 2.0, b / 2.0, qb], [np.inf, -np.inf, np.nan]]), equal_nan=True)
    assert 4.0 / r17 > 0.0 > -1.0 / r17                                  # the signs of C's infinities
    sub = multi_outlyingness_records(KNOWN_P, KNOWN_U, [2, 2, 1], centres=True)
    assert np.array_equal(sub[0], rec[[2, 2, 1]], equal_nan=True) and np.array_equal(sub[1], cen)   # the centres: all curves


def test_host_numbers_from_the_known_records(restated):
    res = DirectionalOutlyingness(_frames(KNOWN_P), directions=KNOWN_U)
    a, b = 1.0 / np.sqrt(5.0), 2.0 / np.sqrt(5.0)
    qb = (-a) * (0.0 - a / 2.0) + (-b) * (0.0 - b / 2.0)
    assert np.array_equal(res.mean.to_numpy()[:2], [[0.0, 0.0], [a / 2.0, b / 2.0]])
    assert np.array_equal(res.variation.to_numpy()[:2], [0.0, qb / 2.0])                # VO = Q / T
    assert np.array_equal(res.total.to_numpy()[:2], [0.0, (a / 2.0) ** 2 + (b / 2.0) ** 2 + qb / 2.0])
    assert not np.isfinite(res.mean.to_numpy()[2]).any() and np.isnan(res.variation.to_numpy()[2])
    assert np.array_equal(res.centres, [0, 0]) and res.centres.dtype == np.int64
    with pytest.raises(ValueError, match=r'1 of 3 curves.*MAD is 0'):
        MSPlotOutliers(_frames(KNOWN_P), directions=KNOWN_U)


def test_the_centre_is_the_lowest_index_of_the_minimum():
    P = _curves(7, 3, 2, seed=4)
    P[5, 1] = P[2, 1]                                                    # a duplicate of curve 2 at t = 1
    U = make_directions(9, 1, 2)
    rec, cen, cur = multi_outlyingness_records(P, U, centres=True, curves=True)
    for t in range(3):
        o = projection_outlyingness(P[:, t, :], U)
        assert cen[t] == min(i for i in range(7) if o[i] == o.min())
        assert np.array_equal(cur[cen[t], t], [0.0, 0.0])
        off = (P[:, t] != P[cen[t], t]).any(axis=1)                      # the centre (and a duplicate of it) has no direction
        norm = np.sqrt((cur[:, t] ** 2).sum(axis=1))
        np.testing.assert_allclose(norm[off], o[off], rtol=8 * U53)      # |O_t| = o_t: the unit vector
        assert not norm[~off].any()
    assert np.array_equal(cur[5, 1], cur[2, 1])


# ---------------------------------------------------------------- Welford against the two-pass definition
def test_welford_against_the_two_pass_definition_in_50_digits():
    """MO = mean_t O_t and Q = sum_t |O_t - MO|^2 in 50-digit arithmetic from the restatement's own fp64 O_t, on seeded
    curves with one curve shifted by 10^6 (|MO| ~ 10^6 in units of the MAD, VO ~ 0: the pure magnitude outlier, where
    sum |O|^2 - T |MO|^2 would lose every digit).

    The bounds are derived, not measured (u = 2^-53):
      M: the running mean is a convex combination formed with 3 rounded operations per step: |M - exact| <= 2 T u max|O|;
      Q: every term delta (O - M_new) carries 4 rounded operations and there are T terms per feature, each bounded by the
         exact sum S = sum |O - MO|^2 up to first order: |Q - exact| <= 8 T u S + O(u^2).
    Worst error / bound seen on this case: M 0.005, Q 0.022 -- the Q bound did not need widening, also not for the shifted
    curve (delta = O - M is an exact subtraction of close numbers there)."""
    mp.mp.dps = 50
    n, T, d = 12, 40, 3
    P = np.random.default_rng(7).normal(size=(n, T, d))
    P[4] += 1e6
    U = make_directions(15, 2, d)
    rec, cur = multi_outlyingness_records(P, U, curves=True)
    assert np.isfinite(rec).all() and np.abs(rec[4, :d]).max() > 1e5
    worst = {'M': 0.0, 'Q': 0.0}
    for i in range(n):
        O = [[mp.mpf(float(cur[i, t, e])) for e in range(d)] for t in range(T)]
        MO = [mp.fsum(O[t][e] for t in range(T)) / T for e in range(d)]
        S = mp.fsum((O[t][e] - MO[e]) ** 2 for t in range(T) for e in range(d))
        omax = float(np.abs(cur[i]).max())
        m_err = max(abs(mp.mpf(float(rec[i, e])) - MO[e]) for e in range(d))
        q_err = abs(mp.mpf(float(rec[i, d])) - S)
        m_bound = 2 * T * U53 * omax
        q_bound = 8 * T * U53 * float(S)
        worst['M'] = max(worst['M'], float(m_err / m_bound))
        worst['Q'] = max(worst['Q'], float(q_err / q_bound))
        assert m_err <= m_bound, (i, float(m_err), m_bound)
        assert q_err <= q_bound, (i, float(q_err), q_bound)
    print('worst error / bound:', worst)


# ---------------------------------------------------------------- refusals of the host layer
@pytest.mark.parametrize('bad', [np.nan, np.inf, -np.inf, 2.0 ** 501])
def test_refuses_nan_inf_and_huge_values(bad, no_engine):
    P = _curves()
    P[4, 2, 1] = bad
    for call in (DirectionalOutlyingness, MSPlotOutliers):
        with pytest.raises(ValueError):
            call(_frames(P))
    X = _curves()[:, :, 0].T.copy()
    X[1, 2] = bad
    with pytest.raises(ValueError):
        DirectionalOutlyingness([pd.DataFrame(X)])


def test_refuses_unequal_frames_too_many_features_and_too_few_curves(no_engine):
    fr = _frames(_curves())
    fr[3] = fr[3].iloc[:-1]
    with pytest.raises(ValueError, match='one shape'):
        DirectionalOutlyingness(fr)
    with pytest.raises(ValueError, match='at most 8 features'):
        DirectionalOutlyingness(_frames(_curves(d=9)))
    with pytest.raises(ValueError, match='at least 2 curves'):
        DirectionalOutlyingness([pd.DataFrame(np.arange(5.0)[:, None])])
    with pytest.raises(ValueError, match='at least one timepoint'):
        DirectionalOutlyingness([pd.DataFrame(np.zeros((0, 3))) for _ in range(4)])
    with pytest.raises(ValueError, match='list'):
        DirectionalOutlyingness(pd.DataFrame(np.zeros((3, 3))))
    with pytest.raises(ValueError):
        DirectionalOutlyingness([])
    df = pd.DataFrame(_curves()[:, :, 0].T)
    df.columns = ['a', 'b', 'a', 'c', 'd', 'e']
    with pytest.raises(ValueError, match='unique'):
        DirectionalOutlyingness([df])


def test_refuses_bad_directions(no_engine):
    fr = _frames(_curves())
    for bad in (0, -3, np.zeros((2, 3)), np.ones((2, 2)), [[np.nan, 1.0, 0.0]], 'all'):
        with pytest.raises(ValueError):
            DirectionalOutlyingness(fr, directions=bad)
        with pytest.raises(ValueError):
            MSPlotOutliers(fr, directions=bad)
    U = np.eye(3)
    U[0, 0] = 2.0 ** 501
    with pytest.raises(ValueError, match='2\\^500'):
        DirectionalOutlyingness(fr, directions=U)


@pytest.mark.parametrize('level', [0.0, 1.0, -0.1, 1.5, np.nan, 'high', None, True])
def test_refuses_a_level_outside_the_unit_interval(level, no_engine):
    with pytest.raises(ValueError, match='level'):
        MSPlotOutliers(_frames(_curves()), level=level)


def test_the_refusals_name_the_caller_and_containments_keep_their_names(no_engine):
    with pytest.raises(ValueError, match='DirectionalOutlyingness'):
        DirectionalOutlyingness(_frames(_curves(d=9)))
    assert _containment.CLOUD_DEPTHS == ('halfspace', 'projection')              # no new containment name


def test_engine_checks_values_and_algo_itself(monkeypatch):
    def boom(*a, **k):
        raise AssertionError('uploaded')
    monkeypatch.setattr(engine, '_upload', boom)
    monkeypatch.setattr(engine, '_lib', lambda: None)
    monkeypatch.setattr(engine, '_device', lambda device=None: None)
    P = _curves()
    with pytest.raises(ValueError, match='algo'):
        engine.multi_outlyingness_moments(P, np.eye(3), algo='sort')
    with pytest.raises(ValueError, match='3-D'):
        engine.multi_outlyingness_moments(P[0], np.eye(3))
    P[0, 0, 0] = 2.0 ** 501
    with pytest.raises(ValueError, match='coordinates'):
        engine.multi_outlyingness_moments(P, np.eye(3))
    U = np.eye(3)
    U[1, 1] = np.inf
    with pytest.raises(ValueError, match='direction entries'):
        engine.multi_outlyingness_moments(_curves(), U)
    with pytest.raises(ValueError, match='algo'):
        engine.multi_outlyingness_workspace_bytes(10, 3, 2, 5, algo='pairwise')


# ---------------------------------------------------------------- the two forms: types, indices, targets
def test_multivariate_form_is_indexed_by_list_position(restated):
    P = _curves(6, 5, 3)
    full = DirectionalOutlyingness(_frames(P), directions=9, seed=2, curves=True)
    assert type(full) is DirectionalOutlyingnessResult
    Pc, Uc, tg, kw = restated[-1]
    assert Pc.shape == (6, 5, 3) and np.array_equal(Uc, make_directions(9, 2, 3)) and list(tg) == list(range(6))
    assert kw['centres'] is True and kw['curves'] is True
    rec, cen, cur = multi_outlyingness_records(P, make_directions(9, 2, 3), centres=True, curves=True)
    assert type(full.mean) is pd.DataFrame and list(full.mean.index) == list(range(6))
    assert list(full.mean.columns) == ['MO0', 'MO1', 'MO2'] and np.array_equal(full.mean.to_numpy(), rec[:, :3])
    assert type(full.variation) is pd.Series and np.array_equal(full.variation.to_numpy(), rec[:, 3] / 5.0)
    assert type(full.total) is pd.Series
    assert np.array_equal(full.total.to_numpy(), (rec[:, :3] * rec[:, :3]).sum(axis=1) + rec[:, 3] / 5.0)
    assert np.array_equal(full.centres, cen) and np.array_equal(full.curves, cur) and full.curves.shape == (6, 5, 3)
    pts = full.points()
    assert list(pts.columns) == ['MO0', 'MO1', 'MO2', 'VO'] and np.array_equal(pts['VO'].to_numpy(), full.variation.to_numpy())
    part = DirectionalOutlyingness(_frames(P), to_compute=[4, 1, 1], directions=9, seed=2)
    assert list(part.mean.index) == [4, 1, 1] and list(restated[-1][2]) == [4, 1, 1] and part.curves is None
    assert np.array_equal(part.mean.to_numpy(), full.mean.to_numpy()[[4, 1, 1]])
    assert np.array_equal(part.centres, full.centres)                     # the centres do not depend on to_compute


def test_one_frame_form_takes_the_columns_as_curves(restated):
    X = np.round(np.random.default_rng(8).normal(size=(6, 5)), 1)          # T = 6 timepoints, n = 5 curves
    df = pd.DataFrame(X, columns=list('abcde'))
    full = DirectionalOutlyingness([df], directions=77)
    Pc, Uc, tg, _ = restated[-1]
    assert Pc.shape == (5, 6, 1) and np.array_equal(Pc[:, :, 0], X.T) and list(tg) == [0, 1, 2, 3, 4]
    assert np.array_equal(Uc, [[1.0]])                                   # one feature: the direction (1.0) is exact
    assert list(full.mean.index) == list('abcde') and list(full.mean.columns) == ['MO0']
    part = DirectionalOutlyingness([df], to_compute=['d', 'a'], directions=77)
    assert list(part.variation.index) == ['d', 'a'] and list(restated[-1][2]) == [3, 0]
    assert np.array_equal(part.total.to_numpy(), full.total.to_numpy()[[3, 0]])
    with pytest.raises(KeyError):
        DirectionalOutlyingness([df], to_compute=['z'])


# ---------------------------------------------------------------- the outlier rule on restated records
def test_the_rule_flags_the_planted_outliers(restated):
    """Dai & Genton's rule on the planted design, 200 directions: the four planted curves are flagged and at most 5 % of
    n more."""
    res = MSPlotOutliers(_frames(planted_design()), directions=200)
    assert type(res) is MSPlotOutlierResult
    flagged = set(res.outliers)
    print('flagged:', sorted(flagged), 'cutoff:', res.cutoff)
    assert PLANTED <= flagged and len(flagged) <= 4 + 5
    assert res.points.shape == (100, 3) and list(res.points.columns) == ['MO0', 'MO1', 'VO']
    assert list(res.distances.index) == list(range(100))
    assert flagged == set(res.distances.index[res.distances.to_numpy() > res.cutoff])
    assert res.cutoff == _ms_cutoff(100, 3, 0.993)
    assert len(res.support) == _mcd_support_size(100, 3) and not PLANTED & set(res.support)
    again = MSPlotOutliers(_frames(planted_design()), directions=200)
    assert list(again.outliers) == list(res.outliers) and np.array_equal(again.distances, res.distances)
    strict = MSPlotOutliers(_frames(planted_design()), directions=200, level=0.999999)
    assert set(strict.outliers) <= flagged and strict.cutoff > res.cutoff


def test_the_rule_on_univariate_curves(restated):
    """The one-frame form: feature 0 of the first 60 curves; the outliers are column labels, in column order.  (With n = 60,
    h = 31 and q = 2 Hardin & Rocke's m is 3.54 (m_asy = 2.39), so the F quantile has m - q + 1 = 2.5 degrees of freedom in
    its denominator and explodes: the cutoff is 171.5 where chi2_(2; 0.993) is 9.9.  The two shape outliers c2 and c3 lie
    far above it, the shifted curve c0 with a squared distance of 56 below.  Which curves a rule this wide flags is not
    asserted.)"""
    P = planted_design()[:60, :, 0]
    df = pd.DataFrame(P.T, columns=[f'c{i}' for i in range(60)])
    res = MSPlotOutliers([df])
    print('flagged:', list(res.outliers), 'cutoff:', res.cutoff)
    assert np.array_equal(restated[-1][1], [[1.0]])
    assert list(res.points.index) == list(df.columns) and list(res.points.columns) == ['MO0', 'VO']
    assert list(res.outliers) == [c for c in df.columns if res.distances[c] > res.cutoff]
    assert res.cutoff == _ms_cutoff(60, 2, 0.993)
    m_asy, m = _hardin_rocke(60, _mcd_support_size(60, 2), 2)
    assert m_asy == pytest.approx(2.39, abs=5e-3) and m == pytest.approx(3.54, abs=5e-3)
    assert res.cutoff == pytest.approx(171.5, abs=0.05)


@pytest.mark.parametrize('shift', [1e4, 1e6, 1e9])
def test_the_rule_flags_a_gross_magnitude_outlier(restated, shift):
    """Curve 0 of the planted design shifted by 10^4, 10^6 and 10^9 instead of 8 (a sentinel value, a unit mix-up): its
    |MO| and the covariance of all n points grow with the shift, the h most concentrated points stay where they were.
    The rule must not mistake them for a hyperplane: it flags the four planted curves as before."""
    P = planted_design()
    P[0, :, 0] += shift - 8.0
    res = MSPlotOutliers(_frames(P), directions=200)
    flagged = set(res.outliers)
    print('flagged:', sorted(flagged), 'RMD2 of curve 0:', res.distances[0])
    assert PLANTED <= flagged and len(flagged) <= 4 + 5
    assert not PLANTED & set(res.support) and res.distances[0] == res.distances.max()


# ---------------------------------------------------------------- the MCD alone
def test_mcd_support_avoids_a_far_cluster():
    rng = np.random.default_rng(3)
    far = rng.normal(size=(15, 3))
    far = 50.0 * far / np.linalg.norm(far, axis=1, keepdims=True)
    Y = np.vstack([rng.normal(size=(60, 3)), far])
    mu, C, support, det = _fast_mcd(Y, seed=0)
    assert len(support) == _mcd_support_size(75, 3) == 39 and support.max() < 60
    assert det == pytest.approx(np.linalg.det(C)) and np.abs(mu).max() < 1.0
    again = _fast_mcd(Y, seed=0)
    assert np.array_equal(again[2], support) and again[3] == det         # deterministic for a seed


@pytest.mark.parametrize('far', [1e3, 1e6, 1e12])
def test_mcd_is_not_moved_by_one_gross_outlier(far):
    """100 standard-normal points in R^3 and one point at `far`: the same support, location and covariance as with the
    point at 1000, and no hyperplane -- the scale that decides what is singular does not see the outlier."""
    Y = np.vstack([np.random.default_rng(11).normal(size=(100, 3)), [[far, -far, far]]])
    mu, C, support, det = _fast_mcd(Y, seed=0)
    assert len(support) == _mcd_support_size(101, 3) and 100 not in support
    assert np.abs(mu).max() < 1.0 and 0.0 < det < 1.0
    ref = _fast_mcd(np.vstack([Y[:100], [[1e3, -1e3, 1e3]]]), seed=0)
    assert np.array_equal(support, ref[2]) and det == ref[3]


def test_mcd_does_not_depend_on_the_units_of_a_coordinate():
    """One coordinate in units 10^-9 times the others': the same support (the MCD is affine equivariant, and what counts
    as singular is judged per coordinate on its own robust scale)."""
    Y = np.random.default_rng(12).normal(size=(60, 3))
    a, b = _fast_mcd(Y, seed=0), _fast_mcd(Y * [1.0, 1e-9, 1e6], seed=0)
    assert np.array_equal(a[2], b[2]) and b[3] == pytest.approx(a[3] * 1e-6, rel=1e-9)


def test_mcd_refuses_h_points_sharing_a_coordinate():
    Y = np.random.default_rng(13).normal(size=(20, 2))
    Y[:12, 1] = 0.25                                                 # h = 11 of 20
    with pytest.raises(ValueError, match='more than half of the points lie in a hyperplane'):
        _fast_mcd(Y, seed=0)


def test_mcd_refuses_more_than_half_of_the_points_on_a_line():
    rng = np.random.default_rng(5)
    s = np.arange(6.0)
    Y = np.vstack([np.stack([s, 2.0 * s + 1.0], axis=1), rng.normal(size=(4, 2)) * 10.0])
    with pytest.raises(ValueError, match='more than half of the points lie in a hyperplane'):
        _fast_mcd(Y, seed=0)


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_mcd_is_as_good_as_scikit_learns(seed):
    pytest.importorskip('sklearn')
    from sklearn.covariance import MinCovDet
    Y = np.random.default_rng(100 + seed).normal(size=(80, 3)) @ np.array([[2.0, 0.3, 0.0], [0.0, 1.0, 0.5], [0.0, 0.0, 0.7]])
    h = _mcd_support_size(80, 3)
    ours = _fast_mcd(Y, h, seed=seed)[3]
    theirs = np.linalg.det(MinCovDet(support_fraction=h / 80, random_state=seed).fit(Y).raw_covariance_)
    print('determinants (ours, scikit-learn):', ours, theirs)
    assert ours <= theirs * (1 + 1e-9)


# ---------------------------------------------------------------- the cutoff
def test_hardin_rocke_degrees_of_freedom_known_answers():
    for n, want in ((10 ** 3, 102.87), (10 ** 6, 59388.0)):
        assert _hardin_rocke(n, _mcd_support_size(n, 3), 3)[1] == pytest.approx(want, rel=1e-3)


def test_cutoff_approaches_the_chi_square_quantile():
    chi = stats.chi2.ppf(0.993, 3)
    small, large = _ms_cutoff(10 ** 3, 3, 0.993) / chi, _ms_cutoff(10 ** 6, 3, 0.993) / chi
    assert abs(large - 1.0) < 0.01 and abs(small - 1.0) > abs(large - 1.0)
    assert small == pytest.approx(1.0780, abs=5e-4) and large == pytest.approx(1.00013, abs=5e-5)


def test_asymptotic_degrees_of_freedom_are_linear_in_n():
    for q in (2, 3, 5):
        a = _hardin_rocke(1000, 520, q)[0]                               # the same alpha = 0.48
        b = _hardin_rocke(4000, 2080, q)[0]
        assert b / a == pytest.approx(4.0, rel=1e-9)


# ---------------------------------------------------------------- the C ABI is declared and bound
NEW = [('sd_multi_outlyingness_workspace_bytes', 'size_t', 6), ('sd_multi_outlyingness_min_workspace_bytes', 'size_t', 6),
       ('sd_multi_outlyingness_moments', 'int', 15)]


@pytest.mark.parametrize('fn,res,count', NEW)
def test_header_and_signatures_carry_the_entry_points(fn, res, count):
    from statdepth_amd import _native
    src = open(os.path.join(ROOT, 'include', 'statdepth_hip.h')).read()
    decl = re.search(r'\b%s\s+%s\s*\(([^;]*)\)\s*;' % (res, fn), src)
    assert decl, f'{fn} is not declared in statdepth_hip.h'
    params = [p for p in decl.group(1).split(',') if p.strip() != 'void']
    got_res, args = _native.SIGNATURES[fn]
    assert len(params) == count and len(args) == count
    assert got_res is {'size_t': _native._sz, 'int': _native._int}[res]
    if fn == 'sd_multi_outlyingness_moments':
        names = [p.split()[-1].lstrip('*') for p in params]
        assert names == ['P', 'n', 'T', 'd', 'U', 'k', 'targets', 'm', 'algo', 'out', 'centres', 'curves', 'ws', 'ws_bytes',
                         'stream']


def test_the_header_states_the_two_rules():
    src = open(os.path.join(ROOT, 'include', 'statdepth_hip.h')).read()
    k19 = src[src.index('K19'):]
    assert 'r == 0' in k19 and '+inf' in k19 and 'NOT special-cased' in k19


@pytest.fixture(scope='module')
def native():
    from statdepth_amd import _native
    return _native, _native.load()


def test_abi_refusals_come_before_any_device_work(native):
    nv, lib = native
    cap = lib.sd_multi_cloud_lds_capacity()
    order = ('P', 'n', 'T', 'd', 'U', 'k', 'targets', 'm', 'algo', 'out', 'centres', 'curves', 'ws', 'ws_bytes', 'stream')
    base = dict(P=1, n=10, T=4, d=3, U=1, k=5, targets=None, m=10, algo=0, out=1, centres=None, curves=None, ws=None,
                ws_bytes=0, stream=None)
    call = lambda **k: lib.sd_multi_outlyingness_moments(*[{**base, **k}[a] for a in order])          # noqa: E731
    assert call(P=None) == nv.SD_ERR_INVALID and call(U=None) == nv.SD_ERR_INVALID and call(out=None) == nv.SD_ERR_INVALID
    for zero in ('n', 'T', 'd', 'k'):
        assert call(**{zero: 0}) == nv.SD_ERR_INVALID, zero
    assert call(algo=3) == nv.SD_ERR_INVALID and call(algo=-1) == nv.SD_ERR_INVALID
    assert call(m=4) == nv.SD_ERR_INVALID and b'targets=NULL' in lib.sd_last_error()
    assert call(d=9) == nv.SD_ERR_UNSUPPORTED and b'[1,8]' in lib.sd_last_error()
    assert call(n=1 << 31, m=1 << 31) == nv.SD_ERR_UNSUPPORTED and b'2^31' in lib.sd_last_error()
    assert call(n=10 ** 6, m=10 ** 6, T=10 ** 4, k=10 ** 3) == nv.SD_ERR_UNSUPPORTED and b'cap' in lib.sd_last_error()
    assert call(n=cap + 1, m=cap + 1, algo=1) == nv.SD_ERR_UNSUPPORTED and str(cap).encode() in lib.sd_last_error()
    assert call() == nv.SD_ERR_WORKSPACE and b'sd_multi_outlyingness_min_workspace_bytes' in lib.sd_last_error()
    floor = lib.sd_multi_outlyingness_min_workspace_bytes(10, 4, 3, 5, 10, 0)
    assert call(ws=256, ws_bytes=floor - 1) == nv.SD_ERR_WORKSPACE


def test_workspace_sizes(native):
    size, proj = engine.multi_outlyingness_workspace_bytes, engine.multi_projection_workspace_bytes
    cap = engine.multi_cloud_lds_capacity()
    for n, T, d, k in [(2, 1, 1, 1), (65, 3, 3, 5), (1000, 1000, 3, 64), (5000, 500, 8, 1000), (cap, 2, 2, 3)]:
        for algo in ('lds', 'auto', 'global'):
            (rec, floor), (prec, pfloor) = size(n, T, d, k, algo=algo), proj(n, T, d, k, algo=algo)
            assert 0 < floor <= rec and rec >= prec and floor >= pfloor
        rec, floor = size(n, T, d, k, algo='lds')
        per = n * (8 * d + 8) + 8                                      # K18's projection layout and a centre per timepoint
        assert floor == 768 + per and rec == 768 + min(T, max(1, (1 << 25) // (n * d))) * per
        assert size(n, T, d, k, algo='global') == tuple(x + 256 for x in proj(n, T, d, k, algo='global'))
    assert size(cap + 1, 2, 2, 3, algo='lds') == (0, 0)
    assert size(cap + 1, 2, 2, 3, algo='auto') == size(cap + 1, 2, 2, 3, algo='global') != (0, 0)
    assert size(10, 0, 2, 3) == (0, 0) and size(10, 2, 9, 3) == (0, 0) and size(0, 2, 2, 3) == (0, 0)
    assert size(10, 2, 2, 0) == (0, 0) and size(10, 2, 2, 3, algo=3) == (0, 0)
