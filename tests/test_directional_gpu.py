"""Directional outlyingness of multivariate curves on the GPU (K19, sd_multi_outlyingness_moments): the records, the centres
and the curves EQUAL, bit for bit, the numpy restatement of tests/test_directional_host.py on both routes
(np.array_equal(..., equal_nan=True) on float64 and int64, no tolerance) -- n across the padding, the wave, the
points-per-thread and the route edges, every kind of d and k, the slices and the unit chunks in front of the centre kernel,
workspace independence, centre ties and degenerate timepoints, target lists, the optional outputs, the anchors to K12 and
K18, and the public API."""
import functools

import numpy as np
import pandas as pd
import pytest

from test_directional_host import PLANTED, multi_outlyingness_records, planted_design, restated_engine
from test_halfspace_host import make_directions

pytestmark = pytest.mark.gpu

ROUTES = ("lds", "global")
ALL = ROUTES + ("auto",)                                         # auto chooses one of the two: the same bits again
U53 = 2.0 ** -53


@pytest.fixture(scope="module")
def eng():
    from statdepth_amd import engine
    return engine


@functools.lru_cache(maxsize=None)
def _case(n, T, d, k, seed=0):
    """(P, U, (records, centres, curves)) of a continuous sample, computed once per shape and not modified."""
    P = np.random.default_rng(1000 * n + 10 * T + d + seed).normal(size=(n, T, d))
    U = make_directions(k, n + T, d)
    want = multi_outlyingness_records(P, U, centres=True, curves=True)
    for A in (P, U) + want:
        A.setflags(write=False)
    return P, U, want


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _check(eng, P, U, want=None, targets=None, algos=ALL, ws=None):
    """Records, centres and curves on every route of `algos` against the restatement (want: its results for ALL curves)."""
    if want is None:
        want = multi_outlyingness_records(P, U, centres=True, curves=True)
    rec, cen, cur = want
    if targets is not None:
        rec, cur = rec[np.asarray(targets)], cur[np.asarray(targets)]
    for algo in algos:
        got = eng.multi_outlyingness_moments(P, U, targets, algo=algo, ws_bytes=ws, centres=True, curves=True)
        assert _same(got[0], rec), (algo, "records")
        assert _same(got[1], cen), (algo, "centres")
        assert _same(got[2], cur), (algo, "curves")


# ---------------------------------------------------------------- n across padding, wave, per-thread and route edges
@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 1000, 1025, 2049, 5000])
def test_n_across_padding_wave_and_per_thread_edges(eng, n):
    _check(eng, *_case(n, 3, 3, 5))


def test_n_at_the_capacity_and_one_above(eng):
    from statdepth_amd._native import SD_ERR_UNSUPPORTED, StatdepthHipError
    cap = eng.multi_cloud_lds_capacity()
    _check(eng, *_case(cap, 2, 2, 3))
    P, U, want = _case(cap + 1, 2, 2, 3)
    _check(eng, P, U, want, algos=("auto", "global"))               # auto takes the global route above the capacity
    with pytest.raises(StatdepthHipError) as e:
        eng.multi_outlyingness_moments(P, U, algo="lds")
    assert e.value.code == SD_ERR_UNSUPPORTED and str(cap) in str(e.value)


# ---------------------------------------------------------------- dimensions, directions, slices, unit chunks
@pytest.mark.parametrize("k", [1, 7])
@pytest.mark.parametrize("d", [1, 2, 3, 8])
def test_dimensions_and_directions(eng, d, k):
    _check(eng, *_case(130, 2, d, k))


@pytest.mark.parametrize("k", [32, 33, 65])
def test_the_centre_is_taken_after_the_last_slice(eng, k):
    """One, two and three slices of 32 directions meet in V through atomicMax; the centre is the argmin of the final V."""
    _check(eng, *_case(70, 3, 3, k))


def test_more_units_than_a_launch_has_workgroups(eng):
    """T = 520, k = 1: 520 units, two slice launches in front of the one centre launch of the batch."""
    _check(eng, *_case(5, 520, 2, 1), algos=("lds", "auto"))
    P, U, _ = _case(5, 520, 2, 1)
    _check(eng, P[:, :30], U, algos=("global",))                    # the global route: one launch chain per timepoint


# ---------------------------------------------------------------- workspace independence
@pytest.mark.parametrize("algo", ALL)
def test_workspace_size_does_not_change_a_bit(eng, algo):
    """At the floor one timepoint per batch: the Welford record and the counter t + 1 cross every batch; then 3 timepoints
    per batch (batches of 3, 3, 1) and the recommended size (one batch)."""
    from statdepth_amd._native import SD_ERR_WORKSPACE, StatdepthHipError
    n, T, d, k = 40, 7, 3, 5
    P, U, want = _case(n, T, d, k)
    rec, floor = eng.multi_outlyingness_workspace_bytes(n, T, d, k, algo=algo)
    assert floor <= rec
    per = n * (8 * d + 8) + 8
    for ws in (floor, floor + 2 * per, rec):
        _check(eng, P, U, want, algos=(algo,), ws=ws)
    with pytest.raises(StatdepthHipError) as e:
        eng.multi_outlyingness_moments(P, U, algo=algo, ws_bytes=floor - 1)
    assert e.value.code == SD_ERR_WORKSPACE


# ---------------------------------------------------------------- centre ties and degenerate timepoints
def test_two_identical_deepest_curves_give_the_lower_index(eng):
    """At t = 1 curves 4 and 1 sit at one point and the other eight in four pairs mirrored at it: on every direction four
    projections lie below and four above the two equal ones, the median is their value and o = 0 for both."""
    n, T, d = 10, 3, 2
    rng = np.random.default_rng(21)
    P = rng.normal(size=(n, T, d)) * 3.0
    U = np.vstack([np.eye(2), make_directions(6, 3, 2)])
    A = rng.normal(size=(4, d))
    P[4, 1] = P[1, 1] = [0.75, -1.5]
    P[[0, 2, 3, 5], 1] = P[1, 1] + A
    P[[6, 7, 8, 9], 1] = P[1, 1] - A
    want = multi_outlyingness_records(P, U, centres=True, curves=True)
    assert want[1][1] == 1 and not want[2][4, 1].any() and not want[2][1, 1].any() and want[2][0, 1].all()
    _check(eng, P, U, want)


def test_all_curves_identical_at_one_timepoint(eng):
    P, U, _ = _case(70, 3, 3, 5)
    Q = P.copy()
    Q[:, 1, :] = [0.5, -2.0, 3.0]
    want = multi_outlyingness_records(Q, U, centres=True, curves=True)
    assert want[1][1] == 0 and not want[2][:, 1].any() and np.isfinite(want[0]).all()
    _check(eng, Q, U, want)
    _check(eng, Q[:, 1:2], U)


def test_a_constant_feature_with_its_axis_among_the_directions(eng):
    """MAD = 0 on the axis at t = 1: o = inf off the median, the products follow IEEE -- inf, -inf and NaN (diff_e = 0)."""
    n, T, d = 33, 3, 3
    P = np.random.default_rng(9).normal(size=(n, T, d))
    P[:, 1, 2] = 1.25
    P[7, 1, 2] = 4.0                                                 # one curve off the constant: o = inf
    P[8, 1] = [P[0, 1, 0], P[0, 1, 1], -1.0]                         # off it too, sharing two coordinates with another curve
    U = np.vstack([np.eye(3), make_directions(4, 1, 3)])
    want = multi_outlyingness_records(P, U, centres=True, curves=True)
    assert np.isinf(want[2][7, 1]).any() and not np.isfinite(want[0][7]).all() and np.isfinite(want[0][0]).all()
    _check(eng, P, U, want)


def test_one_curve_at_a_million_times_the_scale(eng):
    P, U, _ = _case(50, 4, 3, 8)
    P = P.copy()
    P[17] *= 1e6
    _check(eng, P, U)


# ---------------------------------------------------------------- targets and the optional outputs
def test_subset_permutation_and_repeated_targets(eng):
    P, U, want = _case(65, 3, 3, 5)
    rng = np.random.default_rng(2)
    for tg in (np.array([64, 3, 17]), rng.permutation(65), np.array([5, 5, 0, 64, 5, 0]), np.array([7])):
        _check(eng, P, U, want, targets=tg)                         # (the centres: those of all targets)
    none = eng.multi_outlyingness_moments(P, U, np.array([], dtype=np.int64), centres=True, curves=True)
    assert none[0].shape == (0, 4) and none[2].shape == (0, 3, 3)
    assert none[1].shape == (0,) and none[1].dtype == np.int64        # nothing was launched: no centres, not T zeros
    with pytest.raises(IndexError):
        eng.multi_outlyingness_moments(P, U, [65])


@pytest.mark.parametrize("algo", ALL)
def test_optional_outputs_do_not_change_the_records(eng, algo):
    P, U, want = _case(65, 3, 3, 5)
    for centres in (False, True):
        for curves in (False, True):
            got = eng.multi_outlyingness_moments(P, U, algo=algo, centres=centres, curves=curves)
            got = got if isinstance(got, tuple) else (got,)
            assert len(got) == 1 + centres + curves and _same(got[0], want[0])
            if centres:
                assert _same(got[1], want[1])
            if curves:
                assert _same(got[-1], want[2])


# ---------------------------------------------------------------- anchors to shipped code
@pytest.mark.parametrize("algo", ALL)
def test_one_feature_is_the_signed_univariate_outlyingness(eng, algo):
    X = np.round(np.random.default_rng(14).normal(size=(41, 6)), 2)          # n = 41 curves, T = 6
    P = X[:, :, None]
    rec, cen, cur = eng.multi_outlyingness_moments(P, [[1.0]], algo=algo, centres=True, curves=True)
    for t in range(6):
        x = X[:, t]
        med = np.median(x)
        mad = np.median(np.abs(x - med))
        assert np.array_equal(cur[:, t, 0], np.sign(x - x[cen[t]]) * (np.abs(x - med) / mad))


@pytest.mark.parametrize("algo", ALL)
@pytest.mark.parametrize("d", [2, 3])
def test_the_norm_of_the_curves_is_the_outlyingness_of_k18(eng, d, algo):
    """max_t |O_t| against OM of multi_projection_sums, within 4 u relative (u = 2^-53).  O_t = o v with v = diff / r.
    The sum s of the d squares, added in ascending e from an exact first term: a square that passes through j additions
    carries (1 + j) u, the first two squares d u at most, every later one less, so s (1 + th) with |th| <= d u (all terms
    positive).  The square root halves that and adds u: r (1 + rho), |rho| <= (d / 2 + 1) u.  The division and the
    product add u each to every component, 2 u to the exact norm of the computed components.  Together
        |O_t| = o (1 + e),   |e| <= (d / 2 + 3) u to first order:   4 u for d = 2,   4.5 u for d = 3.
    For d = 2 the 4 u are this bound.  For d = 3 they are half a unit below it, and safe all the same: the 4.5 u need
    diff_2 = 0 (the last square carries 2 u, not 3 u, and th is the mean of the squares' errors weighted by the squares)
    and the seven roundings that remain (two products, two additions, the root, the quotient, the product with o) each
    at its extreme u, all in the one direction that adds up; a rounding error reaches u only for a result just above a
    power of two.  On a continuous sample none of this holds at the one timepoint that gives the maximum.
    The norm is recomputed in extended precision so that the test adds nothing of its own.  The curves that are a centre
    somewhere have no direction there and do not take part."""
    P, U, _ = _case(65, 3, d, 5)
    _, cen, cur = eng.multi_outlyingness_moments(P, U, algo=algo, centres=True, curves=True)
    om = eng.multi_projection_sums(P, U, algo=algo)[:, 1]
    wide = cur.astype(np.longdouble)
    norm = np.sqrt((wide * wide).sum(axis=2)).max(axis=1)
    take = np.ones(65, dtype=bool)
    take[cen] = False
    off = np.abs(norm[take] - om[take]) / om[take]
    print("max relative deviation / u:", float(off.max() / U53))
    assert (off <= 4 * U53).all()


# ---------------------------------------------------------------- the public API
def test_directional_outlyingness_and_ms_plot_on_the_planted_design(monkeypatch):
    from statdepth_amd import DirectionalOutlyingness, MSPlotOutliers, engine
    P = planted_design()
    frames = [pd.DataFrame(P[i]) for i in range(P.shape[0])]
    dev = MSPlotOutliers(frames, directions=200)
    res = DirectionalOutlyingness(frames, directions=200, curves=True)
    part = DirectionalOutlyingness(frames, to_compute=[3, 0], directions=200)
    U = make_directions(200, 0, 2)
    rec, cen, cur = multi_outlyingness_records(P, U, centres=True, curves=True)
    assert np.array_equal(res.mean.to_numpy(), rec[:, :2]) and np.array_equal(res.variation.to_numpy(), rec[:, 2] / 50.0)
    assert np.array_equal(res.centres, cen) and np.array_equal(res.curves, cur)
    assert list(part.mean.index) == [3, 0] and np.array_equal(part.total.to_numpy(), res.total.to_numpy()[[3, 0]])
    monkeypatch.setattr(engine, "multi_outlyingness_moments", restated_engine)
    host = MSPlotOutliers(frames, directions=200)
    assert list(dev.outliers) == list(host.outliers) and np.array_equal(dev.distances.to_numpy(), host.distances.to_numpy())
    assert PLANTED <= set(dev.outliers) and len(dev.outliers) <= 4 + 5
