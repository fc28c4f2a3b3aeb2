"""Extremal depth (K15), the part that needs no GPU: the definition restated twice in numpy -- the paper's depth-CDF form
and a sort + lexsort form for large n -- and their agreement, the worked example, the public API over a stand-in engine,
every refusal of the host layer, and the declaration of the C entry points."""
import os
import re

import numpy as np
import pandas as pd
import pytest

from conftest import ROOT
from statdepth_amd import FunctionalDepth, engine
from statdepth_amd.depth.calculations._containment import ORDER_DEPTHS, RANK_DEPTHS
from statdepth_amd.homogeneity import FunctionalHomogeneity

NAME = 'extremal'

# four curves over three timepoints (rows are timepoints)
KNOWN_X = np.array([[1.0, 2.0, 3.0, 4.0], [2.0, 1.0, 3.0, 3.0], [1.0, 3.0, 2.0, 4.0]])
KNOWN_E = np.array([[3, 1, 1, 3], [1, 3, 2, 2], [3, 1, 1, 3]], dtype=np.int64)
KNOWN_V = np.array([[3, 3, 1], [3, 1, 1], [2, 1, 1], [3, 3, 2]], dtype=np.int64)
KNOWN_G = np.array([2, 3, 4, 1], dtype=np.int64)
KNOWN_ED = np.array([0.5, 0.75, 1.0, 0.25])


def extremity_np(X):
    """e[t, i] = |A - B|: A, B the other curves strictly above / strictly below curve i at timepoint t (ties in neither)."""
    X = np.asarray(X, dtype=np.float64)
    T, n = X.shape
    e = np.empty((T, n), dtype=np.int64)
    for t in range(T):
        s = np.sort(X[t])
        B = np.searchsorted(s, X[t], 'left').astype(np.int64)
        A = n - np.searchsorted(s, X[t], 'right').astype(np.int64)
        e[t] = np.abs(A - B)
    return e


def extremal_counts_dcdf(X):
    """(a) The paper's form.  Phi_i(k) = #{t : e_i(t) >= k} is T times the depth CDF of curve i at the depth level
    1 - k / n; the levels are compared from the lowest depth (k = n - 1) upward and at the first difference the larger Phi
    is the more extreme curve.  G_q = #{i : i is more extreme than or equal to q}.  O(n^2) tuple comparisons: small n."""
    X = np.asarray(X, dtype=np.float64)
    T, n = X.shape
    A = np.array([[(X[t] > x).sum() for x in X[t]] for t in range(T)], dtype=np.int64)
    B = np.array([[(X[t] < x).sum() for x in X[t]] for t in range(T)], dtype=np.int64)
    e = np.abs(A - B)
    phi = []
    for i in range(n):
        hist = np.bincount(e[:, i], minlength=n)[:n]              # values 0 .. n - 1
        phi.append(tuple(int(v) for v in np.cumsum(hist[::-1])))  # from e = n - 1 downward
    return np.array([sum(1 for i in range(n) if phi[i] >= phi[q]) for q in range(n)], dtype=np.int64)


def extremal_counts_lexsort(X):
    """(b) v_i = e_i sorted descending; the curves in ascending lexicographic order of v by np.lexsort; a group of
    identical vectors that starts at sorted position s has G = n - s."""
    V = -np.sort(-extremity_np(X).T, axis=1)                      # n x T, rows descending
    n, T = V.shape
    order = np.lexsort(V.T[::-1])                                 # the last key is the primary one: column 0
    Vs = V[order]
    new = np.ones(n, dtype=bool)
    new[1:] = (Vs[1:] != Vs[:-1]).any(axis=1)
    start = np.maximum.accumulate(np.where(new, np.arange(n), 0))
    G = np.empty(n, dtype=np.int64)
    G[order] = n - start
    return G


def test_known_answer_restated():
    assert np.array_equal(extremity_np(KNOWN_X), KNOWN_E)
    assert np.array_equal(-np.sort(-KNOWN_E.T, axis=1), KNOWN_V)
    assert np.array_equal(extremal_counts_dcdf(KNOWN_X), KNOWN_G)
    assert np.array_equal(extremal_counts_lexsort(KNOWN_X), KNOWN_G)
    assert np.array_equal(KNOWN_G / 4, KNOWN_ED)


@pytest.mark.parametrize('seed', range(12))
def test_restatements_agree(seed):
    """(a) == (b) on small random shapes: continuous values, values on a coarse grid (ties in most rows), duplicated
    curves, a constant row."""
    rng = np.random.default_rng(seed)
    T, n = int(rng.integers(1, 9)), int(rng.integers(2, 14))
    X = rng.normal(size=(T, n))
    if seed % 3 == 1:
        X = np.round(X, 0)
    if seed % 3 == 2:
        X = np.round(X, 1)
        X[:, -1] = X[:, 0]
        if n > 4:
            X[:, -2] = X[:, 1]
    if seed % 4 == 3:
        X[T // 2] = 0.5
    a, b = extremal_counts_dcdf(X), extremal_counts_lexsort(X)
    assert np.array_equal(a, b), (T, n, a, b)
    assert a.min() >= 1 and a.max() == n                           # some curve is at most as extreme as every other


def test_names():
    assert tuple(ORDER_DEPTHS) == (NAME,)
    assert tuple(RANK_DEPTHS) == ('fm', 'mei', 'mhi', 'half_region', 'integrated_halfspace', 'infimal_halfspace')


# ---- the public API over a stand-in engine ----
def test_api_known_answer_labels_and_order(monkeypatch):
    df = pd.DataFrame(KNOWN_X, columns=['a', 'b', 'c', 'd'])
    calls = []

    def fake(X, targets=None, device=None, algo='auto', ws_bytes=None):
        assert np.array_equal(np.asarray(X), KNOWN_X)
        calls.append(np.asarray(targets))
        return KNOWN_G[np.asarray(targets)]
    monkeypatch.setattr(engine, 'extremal_counts', fake)
    d = FunctionalDepth([df], containment=NAME)
    assert list(d.index) == ['a', 'b', 'c', 'd']
    assert d.to_numpy().dtype == np.float64 and np.array_equal(d.to_numpy(), KNOWN_ED)
    assert list(d.deepest(1).index) == ['c'] and list(d.outlying(1).index) == ['d']
    for relax in (False, True):                                    # accepted and ignored
        sub = FunctionalDepth([df], to_compute=['d', 'a', 'd'], containment=NAME, relax=relax)
        assert list(sub.index) == ['d', 'a', 'd']
        assert np.array_equal(sub.to_numpy(), np.array([0.25, 0.5, 0.25]))
    assert [list(c) for c in calls] == [[0, 1, 2, 3], [3, 0, 3], [3, 0, 3]]
    with pytest.raises(KeyError):
        FunctionalDepth([df], to_compute=['a', 'zz'], containment=NAME)


# ---- refusals: raised before the engine is reached ----
@pytest.fixture
def no_engine(monkeypatch):
    def boom(*a, **k):
        raise AssertionError('engine.extremal_counts was reached')
    monkeypatch.setattr(engine, 'extremal_counts', boom)


def _frame(T=6, n=5, seed=3):
    return pd.DataFrame(np.random.default_rng(seed).normal(size=(T, n)), columns=[f'c{i}' for i in range(n)])


def test_refuses_multivariate(no_engine):
    with pytest.raises(ValueError, match=NAME):
        FunctionalDepth([_frame(6, 2, s) for s in range(4)], containment=NAME)


def test_refuses_K(no_engine):
    with pytest.raises(ValueError, match='has no K-block estimator'):
        FunctionalDepth([_frame()], K=2, containment=NAME)


def test_refuses_nan(no_engine):
    df = _frame()
    df.iloc[4, 2] = np.nan
    with pytest.raises(ValueError, match=NAME):
        FunctionalDepth([df], containment=NAME)


def test_refuses_single_curve(no_engine):
    with pytest.raises(ValueError, match=NAME):
        FunctionalDepth([_frame(6, 1)], containment=NAME)


def test_refuses_no_timepoint(no_engine):
    with pytest.raises(ValueError, match=NAME):
        FunctionalDepth([pd.DataFrame(np.zeros((0, 4)), columns=list('abcd'))], containment=NAME)


@pytest.mark.parametrize('J', [3, np.int64(3), True, 2.0])
def test_refuses_other_J(J, no_engine):
    with pytest.raises(ValueError, match=NAME):
        FunctionalDepth([_frame()], J=J, containment=NAME)


def test_refuses_duplicate_labels(no_engine):
    df = _frame()
    df.columns = ['a', 'b', 'a', 'c', 'd']
    with pytest.raises(ValueError, match='unique'):
        FunctionalDepth([df], containment=NAME)


def test_refuses_more_than_16384_timepoints(no_engine):
    df = pd.DataFrame(np.zeros((16385, 2)), columns=['a', 'b'])
    with pytest.raises(NotImplementedError, match=NAME):
        FunctionalDepth([df], containment=NAME)


def test_refuses_homogeneity(no_engine):
    with pytest.raises(ValueError, match=NAME):
        FunctionalHomogeneity([_frame(6, 5, 1)], [_frame(6, 5, 2)], containment=NAME, relax=True)


def test_unknown_containment_mentions_the_name():
    with pytest.raises(ValueError) as e:
        FunctionalDepth([_frame()], containment='extreme')
    assert f"'{NAME}'" in str(e.value) and "'fm'" in str(e.value)


# ---- the C ABI is declared and bound ----
@pytest.mark.parametrize('fn,res,count', [('sd_extremal_workspace_bytes', 'size_t', 6),
                                          ('sd_extremal_min_workspace_bytes', 'size_t', 6), ('sd_extremal_counts', 'int', 12)])
def test_header_and_signatures_carry_the_entry_points(fn, res, count):
    from statdepth_amd import _native
    src = open(os.path.join(ROOT, 'include', 'statdepth_hip.h')).read()
    decl = re.search(r'\b%s\s+%s\s*\(([^;]*)\)\s*;' % (res, fn), src)
    assert decl, f'{fn} is not declared in statdepth_hip.h'
    assert len(re.sub(r'/\*.*?\*/', '', decl.group(1), flags=re.S).split(',')) == count
    got_res, args = _native.SIGNATURES[fn]
    assert len(args) == count and got_res is {'size_t': _native._sz, 'int': _native._int}[res]


def test_workspace_sizes_follow_the_documented_layout():
    """Time-major copy (curve-major input only), E (4 T n) and H (8 n), each padded to 256 bytes, in front of K14's
    batch; nothing for what the call refuses."""
    up = lambda x: -(-x // 256) * 256                              # noqa: E731
    for T, n, algo in [(1, 2, 'image'), (70, 300, 'image'), (70, 2500, 'sort'), (3, 20000, 'auto'), (16384, 3, 'sort')]:
        for cm in (False, True):
            rec, floor = engine.extremal_workspace_bytes(T, n, algo=algo, curve_major=cm)
            krec, kfloor = engine.rank_depth_workspace_bytes(T, n, algo=algo, curve_major=cm)
            fixed = up(4 * T * n) + up(8 * n)
            assert (rec, floor) == (krec + fixed, kfloor + fixed), (T, n, algo, cm)
    assert engine.extremal_workspace_bytes(16385, 3) == (0, 0)
    assert engine.extremal_workspace_bytes(2, 16385, algo='image') == (0, 0)
    assert engine.extremal_workspace_bytes(5, 1) == (0, 0)
