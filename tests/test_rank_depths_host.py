"""Integrated rank depths (K14), the part that needs no GPU: the normalisation of the records, the definitions restated
twice in numpy, the tie to the C oracle's above/below counts, and every refusal of the host layer."""
from fractions import Fraction

import numpy as np
import pandas as pd
import pytest

from statdepth_amd import FunctionalDepth, engine
from statdepth_amd.depth.calculations._containment import RANK_DEPTHS
from statdepth_amd.depth.calculations._rank import _rank_depth_values
from statdepth_amd.homogeneity import FunctionalHomogeneity

NAMES = ('fm', 'mei', 'mhi', 'half_region', 'integrated_halfspace', 'infimal_halfspace')

# three curves over two timepoints: rows t0 = [1, 2, 3], t1 = [3, 1, 2]
KNOWN_X = np.array([[1.0, 2.0, 3.0], [3.0, 1.0, 2.0]])
KNOWN_RECORDS = np.array([[2, 2, 4, 4, 2], [3, 1, 2, 3, 2], [1, 3, 4, 3, 2]], dtype=np.int64)
F = Fraction
KNOWN_DEPTHS = {
    'fm': [F(2, 3), F(5, 6), F(2, 3)],
    'mei': [F(2, 3), F(5, 6), F(1, 2)],
    'mhi': [F(2, 3), F(1, 2), F(5, 6)],
    'half_region': [F(2, 3), F(1, 2), F(1, 2)],
    'integrated_halfspace': [F(1, 3), F(1, 2), F(1, 2)],
    'infimal_halfspace': [F(1, 3), F(1, 3), F(1, 3)],
}


def above_below_np(X):
    """A[t, i], B[t, i]: the other curves strictly above / strictly below curve i at timepoint t."""
    X = np.asarray(X, dtype=np.float64)
    A = np.array([[(X[t] > x).sum() for x in X[t]] for t in range(X.shape[0])], dtype=np.int64)
    B = np.array([[(X[t] < x).sum() for x in X[t]] for t in range(X.shape[0])], dtype=np.int64)
    return A, B


def records_np(X):
    """The record (SA, SB, SF, SM, MM) of every curve, from the integers A and B."""
    A, B = above_below_np(X)
    n = X.shape[1]
    M = np.maximum(A, B)
    return np.stack([A.sum(0), B.sum(0), np.abs(2 * A - n).sum(0), M.sum(0), M.max(0)], axis=1).astype(np.int64)


def depths_np(X):
    """The six depths of every curve straight from their definitions (proportions and empirical CDFs), no records."""
    X = np.asarray(X, dtype=np.float64)
    T, n = X.shape
    le = np.array([[np.mean(X[t] <= x) for x in X[t]] for t in range(T)])     # F_{n,t}(x(t)); the curve counts itself
    ge = np.array([[np.mean(X[t] >= x) for x in X[t]] for t in range(T)])
    tukey = np.minimum(le, ge)
    return {'fm': np.mean(1 - np.abs(0.5 - le), axis=0), 'mei': ge.mean(0), 'mhi': le.mean(0),
            'half_region': np.minimum(ge.mean(0), le.mean(0)), 'integrated_halfspace': tukey.mean(0),
            'infimal_halfspace': tukey.min(0)}


@pytest.fixture(scope='module')
def tied():
    rng = np.random.default_rng(14)
    return np.round(rng.normal(size=(7, 9)), 1)          # 63 values on a grid of tenths: ties in most rows


def test_names():
    assert tuple(RANK_DEPTHS) == NAMES


def test_known_answer_records_restated():
    assert np.array_equal(records_np(KNOWN_X), KNOWN_RECORDS)


@pytest.mark.parametrize('name', NAMES)
def test_known_answer_normalisation(name):
    got = _rank_depth_values(KNOWN_RECORDS, 3, 2, name)
    assert got.dtype == np.float64 and got.shape == (3,)
    want = np.array([float(f) for f in KNOWN_DEPTHS[name]])
    assert (got == want).all(), (name, got, want)


def test_normalisation_refuses_unknown_name():
    with pytest.raises(ValueError, match='band'):
        _rank_depth_values(KNOWN_RECORDS, 3, 2, 'band')


def test_records_agree_with_definitions(tied):
    assert any(len(np.unique(row)) < len(row) for row in tied)
    T, n = tied.shape
    R = records_np(tied)
    want = depths_np(tied)
    for name in NAMES:
        got = _rank_depth_values(R, n, T, name)
        assert np.max(np.abs(got - want[name])) <= 1e-15, name
    assert np.array_equal(_rank_depth_values(R, n, T, 'half_region'),
                          np.minimum(_rank_depth_values(R, n, T, 'mei'), _rank_depth_values(R, n, T, 'mhi')))


def test_oracle_counts_are_the_restatement(tied, oracle):
    A, B = above_below_np(tied)
    ab = oracle.above_below(tied)                        # [curve, t, (above, below)]
    assert np.array_equal(ab[:, :, 0], A.T)
    assert np.array_equal(ab[:, :, 1], B.T)
    assert np.array_equal(oracle.above_below(KNOWN_X)[:, :, 0], above_below_np(KNOWN_X)[0].T)


# ---- refusals: ValueError that names the containment, and the engine is never reached ----
@pytest.fixture
def no_engine(monkeypatch):
    def boom(*a, **k):
        raise AssertionError('engine.rank_depth_sums was reached')
    monkeypatch.setattr(engine, 'rank_depth_sums', boom)


def _frame(T=6, n=5, seed=3):
    return pd.DataFrame(np.random.default_rng(seed).normal(size=(T, n)), columns=[f'c{i}' for i in range(n)])


@pytest.mark.parametrize('name', NAMES)
def test_refuses_multivariate(name, no_engine):
    with pytest.raises(ValueError, match=name):
        FunctionalDepth([_frame(6, 2, s) for s in range(4)], containment=name)


@pytest.mark.parametrize('name', NAMES)
def test_refuses_K(name, no_engine):
    with pytest.raises(ValueError, match=name):
        FunctionalDepth([_frame()], K=2, containment=name)


@pytest.mark.parametrize('name', NAMES)
def test_refuses_nan(name, no_engine):
    df = _frame()
    df.iloc[4, 2] = np.nan
    with pytest.raises(ValueError, match=name):
        FunctionalDepth([df], containment=name)


@pytest.mark.parametrize('name', NAMES)
def test_refuses_single_curve(name, no_engine):
    with pytest.raises(ValueError, match=name):
        FunctionalDepth([_frame(6, 1)], containment=name)


@pytest.mark.parametrize('name', NAMES)
def test_refuses_other_J(name, no_engine):
    with pytest.raises(ValueError, match=name):
        FunctionalDepth([_frame()], J=3, containment=name)


@pytest.mark.parametrize('name', NAMES)
def test_refuses_homogeneity(name, no_engine):
    with pytest.raises(ValueError, match=name):
        FunctionalHomogeneity([_frame(6, 5, 1)], [_frame(6, 5, 2)], containment=name, relax=True)


def test_J_two_as_a_numpy_integer_is_accepted(monkeypatch):
    monkeypatch.setattr(engine, 'rank_depth_sums', lambda X, targets=None, **k: KNOWN_RECORDS[np.asarray(targets)])
    d = FunctionalDepth([pd.DataFrame(KNOWN_X)], J=np.int64(2), containment='mei')
    assert (d.to_numpy() == np.array([float(f) for f in KNOWN_DEPTHS['mei']])).all()
    for J in (np.int64(3), True, 2.0):
        with pytest.raises(ValueError, match='mei'):
            FunctionalDepth([pd.DataFrame(KNOWN_X)], J=J, containment='mei')


def test_refuses_duplicate_labels(no_engine):
    df = _frame()
    df.columns = ['a', 'b', 'a', 'c', 'd']
    with pytest.raises(ValueError, match='unique'):
        FunctionalDepth([df], containment='fm')


def test_unknown_containment_lists_the_new_names():
    with pytest.raises(ValueError) as e:
        FunctionalDepth([_frame()], containment='epigraph')
    for name in NAMES + ('r2',):
        assert f"'{name}'" in str(e.value)


def test_dispatch_reaches_the_engine_once_with_positions(monkeypatch):
    """Labels -> positions, one engine call, the series indexed by the labels asked for, in their order; relax ignored."""
    df = pd.DataFrame(KNOWN_X, columns=['a', 'b', 'c'])
    calls = []

    def fake(X, targets=None, device=None, algo='auto', ws_bytes=None):
        calls.append(np.asarray(targets))
        return KNOWN_RECORDS[np.asarray(targets)]
    monkeypatch.setattr(engine, 'rank_depth_sums', fake)
    for relax in (False, True):
        d = FunctionalDepth([df], to_compute=['c', 'a'], containment='mhi', relax=relax)
        assert list(d.index) == ['c', 'a']
        assert (d.to_numpy() == np.array([float(F(5, 6)), float(F(2, 3))])).all()
    assert len(calls) == 2 and all(list(c) == [2, 0] for c in calls)
    assert list(FunctionalDepth([df], containment='fm').deepest(1).index) == ['b']


# ---- workspace sizes and batches (the library's host-side arithmetic: no device) ----
IMAGE_CAP_ROWS, IMAGE_CAP_BYTES, SORT_REC_VALUES, SORT_CAP_VALUES = 1 << 16, 1 << 30, 1 << 23, 1 << 25


def _up(x):
    return -(-x // 256) * 256


def _image_rows_model(T, n, b):
    """The most rows r <= cap whose image (4 n r bytes) and NaN counts (4 r bytes), each padded to 256, fit b bytes."""
    cap = min(T, IMAGE_CAP_ROWS, IMAGE_CAP_BYTES // (4 * n))
    fits = [r for r in (range(1, cap + 1) if cap <= 4096 else
                        range(max(1, b // (4 * n + 4) - 200), min(cap, b // (4 * n + 4)) + 1))
            if _up(4 * n * r) + _up(4 * r) <= b]
    return (cap, max(fits)) if fits else (cap, 0)


@pytest.mark.parametrize('curve_major', [False, True])
@pytest.mark.parametrize('T,n', [(1, 2), (3, 5), (70, 300), (1000, 10000), (1000, 14000), (999, 16384), (2051, 130),
                                 (65536, 63), (65537, 64), (70000, 7), (20000, 16000)])
def test_image_route_recommended_size_is_one_batch(T, n, curve_major):
    """The recommended workspace holds the batch it is sized for: all T rows when T is within the route's caps (2^16
    rows, a 1 GiB image), the cap otherwise.  The floor holds at least one row and one byte less none; every size holds
    what a restatement of the layout says fits, and never more than the cap."""
    rec, floor = engine.rank_depth_workspace_bytes(T, n, algo='image', curve_major=curve_major)
    rows = lambda b: engine.rank_depth_rows_per_batch(T, n, b, algo='image', curve_major=curve_major)    # noqa: E731
    copy = _up(8 * T * n) if curve_major and T > 1 else 0          # the time-major copy of a curve-major matrix
    cap = min(T, IMAGE_CAP_ROWS, IMAGE_CAP_BYTES // (4 * n))
    assert rows(rec) == cap
    assert rows(floor) >= 1 and rows(floor - 1) == 0
    assert rows(rec + 12345) == cap and rows(10 * rec) == cap
    assert floor == copy + _up(4 * n) + 256
    for b in (floor, floor + 1, rec - 1, rec, floor + (rec - floor) // 2, floor + (rec - floor) // 7, rec + 511):
        assert (cap, rows(b)) == _image_rows_model(T, n, b - copy), b
    if n >= 64 and cap > 2:                                         # a row is at least a padding unit: one byte less, one row less
        assert rows(rec - 1) == cap - 1


@pytest.mark.parametrize('curve_major', [False, True])
@pytest.mark.parametrize('T,n', [(1, 2), (70, 2500), (256, 100000), (1000, 14000), (2, 16385), (5000, 2049), (3, 9000000)])
def test_sort_route_recommended_size_is_one_chunk_within_the_cap(T, n, curve_major):
    rec, floor = engine.rank_depth_workspace_bytes(T, n, algo='sort', curve_major=curve_major)
    rows = lambda b: engine.rank_depth_rows_per_batch(T, n, b, algo='sort', curve_major=curve_major)     # noqa: E731
    assert rows(rec) == min(T, max(1, SORT_REC_VALUES // n))
    assert rows(floor) == 1 and rows(floor - 1) == 0
    assert rows(100 * rec) == min(T, max(1, SORT_CAP_VALUES // n))
    if rows(rec) > 1:
        assert rows(rec - 1) == rows(rec) - 1


def test_rows_per_batch_of_a_refused_call_is_zero():
    assert engine.rank_depth_rows_per_batch(2, 16385, 1 << 30, algo='image') == 0
    assert engine.rank_depth_rows_per_batch(0, 5, 1 << 30) == 0
    assert engine.rank_depth_rows_per_batch(5, 1, 1 << 30) == 0
