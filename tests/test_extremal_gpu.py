"""Extremal depth on the GPU (K15, sd_extremal_counts): the int64 counts G EQUAL to the sort + lexsort restatement of
tests/test_extremal_host.py (which that file ties to the paper's depth-CDF form) -- smallest shapes, ties, duplicated and
identical curves, a constant row, infinities, both routes, both memory layouts, target lists, the sort's padding, heads
shorter than, equal to and longer than the packed prefix, vectors that differ only at their last entry, the widths at
which the head loses a field, workspace independence with ragged transpose tiles, invariances, and the public API."""
import functools

import numpy as np
import pandas as pd
import pytest

from test_extremal_host import (KNOWN_ED, KNOWN_G, KNOWN_X, extremal_counts_dcdf, extremal_counts_lexsort,
                                extremity_np)

pytestmark = pytest.mark.gpu

IMAGE, SORT = 1, 2
TILE = 64                                                         # rows and curves of the transform's transpose tile


@pytest.fixture(scope="module")
def eng():
    from statdepth_amd import engine
    return engine


KINDS = ("normal", "tenths", "duplicated", "constant_row", "infinities", "identical")


def _data(T, n, kind, seed):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(T, n))
    if kind == "tenths":
        X = np.round(X, 1)
    elif kind == "duplicated":                            # 10 % of the curves are copies of others
        k = max(1, n // 10)
        X[:, n - k:] = X[:, :k]
    elif kind == "constant_row":
        X[T // 2] = 1.5
    elif kind == "infinities":
        u = rng.random(size=(T, n))
        X[u < 0.03] = np.inf
        X[u > 0.97] = -np.inf
    elif kind == "identical":
        X[:, :] = X[:, :1]
    return X


@functools.lru_cache(maxsize=None)
def _case(T, n, kind):
    """(X, G of every curve by the restatement), computed once per case and not modified."""
    X = _data(T, n, kind, 100 * T + n)
    want = extremal_counts_lexsort(X)
    X.setflags(write=False)
    want.setflags(write=False)
    return X, want


def _subset(n, seed):
    """A shuffled subset of the curves with one index twice."""
    rng = np.random.default_rng(seed)
    tg = rng.permutation(n)[:max(2, (2 * n) // 3)]
    tg[-1] = tg[0]
    return tg.astype(np.int64)


def _family(n, T, L):
    """Curves in mirror pairs (i, n - 1 - i) whose vectors agree on the first T - L entries and differ from there on.
    The first T - L rows rank the curves 0 .. n - 1 (e_i = |n - 1 - 2 i| = c, the same for a curve and its mirror); the
    last L rows move the mirror of i < k one rank towards the centre (e = c - 2) and give what is left over the freed
    top rank.  So v_i = (c, .., c) and v_mirror = (c x (T - L), (c - 2) x L), except for the left-over curve."""
    k = n // 2
    rho = np.arange(n, dtype=np.float64)
    i = np.arange(k)
    rho[n - 1 - i] = n - 2 - i
    rho[k] = n - 1                                                 # odd n: the centre curve; even n: the mirror of k - 1
    assert len(np.unique(rho)) == n
    X = np.tile(np.arange(n, dtype=np.float64), (T, 1))
    X[T - L:] = rho
    return X


def test_restatement_and_family_construction():
    """The reference used here is the paper's form on small cases, and the family is what its docstring says."""
    for kind in KINDS:
        X = _data(6, 11, kind, 5)
        assert np.array_equal(extremal_counts_lexsort(X), extremal_counts_dcdf(X)), kind
    for n, T, L in [(21, 9, 1), (20, 9, 1), (21, 5, 2)]:
        X = _family(n, T, L)
        V = -np.sort(-extremity_np(X).T, axis=1)
        assert np.array_equal(extremal_counts_lexsort(X), extremal_counts_dcdf(X))
        for i in range(n // 2 - 1):
            assert np.array_equal(V[i, :T - L], V[n - 1 - i, :T - L]) and (V[i, T - L:] == V[n - 1 - i, T - L:] + 2).all()


# ---------------------------------------------------------------- small shapes, both routes, both layouts, target lists
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T,n", [(1, 2), (3, 4), (2, 3), (7, 64), (33, 257), (17, 1025), (5, 4097)])
def test_small_shapes(eng, T, n, kind):
    X, want = _case(T, n, kind)
    if kind == "identical":
        assert (want == n).all()
    tg = _subset(n, T + n)
    for algo in (IMAGE, SORT):
        for A in (np.array(X, order="C"), np.array(X, order="F")):            # writable copies in either layout
            assert np.array_equal(eng.extremal_counts(A, algo=algo), want), (algo, A.flags.f_contiguous)
            assert np.array_equal(eng.extremal_counts(A, tg, algo=algo), want[tg]), (algo, A.flags.f_contiguous, "subset")


def test_known_answer(eng):
    for algo in (0, IMAGE, SORT, "auto", "image", "sort"):
        got = eng.extremal_counts(KNOWN_X, algo=algo)
        assert got.dtype == np.int64 and np.array_equal(got, KNOWN_G), algo
        assert np.array_equal(got / 4, KNOWN_ED)


# ---------------------------------------------------------------- the boundary between the routes
@pytest.mark.parametrize("n", [16384, 16385])
def test_route_boundary(eng, n):
    X = np.random.default_rng(n).normal(size=(2, n))
    X[1, ::7] = np.round(X[1, ::7], 1)
    assert np.array_equal(eng.extremal_counts(X, algo=0), extremal_counts_lexsort(X))


def test_image_route_refuses_more_than_16384_curves(eng):
    from statdepth_amd._native import SD_ERR_UNSUPPORTED, StatdepthHipError
    with pytest.raises(StatdepthHipError) as e:
        eng.extremal_counts(np.zeros((2, 16385)), algo=IMAGE)
    assert e.value.code == SD_ERR_UNSUPPORTED


# ---------------------------------------------------------------- the sort's padding
@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 255, 257, 1023, 1025])
def test_sort_padding(eng, T):
    """n = 5: e takes five values, so from T = 63 on the heads are all equal and every pair is decided in the tail."""
    X, want = _case(T, 5, "tenths")
    for algo in (IMAGE, SORT):
        assert np.array_equal(eng.extremal_counts(X.copy(), algo=algo), want), algo


def test_sort_at_its_capacity(eng):
    X, want = _case(16384, 3, "normal")
    assert np.array_equal(eng.extremal_counts(X.copy()), want)


def test_refuses_more_than_16384_timepoints(eng):
    from statdepth_amd._native import SD_ERR_UNSUPPORTED, StatdepthHipError
    for algo in (0, IMAGE, SORT):
        with pytest.raises(StatdepthHipError) as e:
            eng.extremal_counts(np.zeros((16385, 3)), algo=algo)
        assert e.value.code == SD_ERR_UNSUPPORTED


# ---------------------------------------------------------------- head and tail
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5])
def test_vectors_around_the_head_length(eng, T):
    """P = 4 at this n: T < P leaves zero-filled fields, T = P fills the head, T = 5 has one tail entry."""
    X, want = _case(T, 37, "tenths")
    tg = _subset(37, T)
    for algo in (IMAGE, SORT):
        assert np.array_equal(eng.extremal_counts(X.copy(), algo=algo), want), algo
        assert np.array_equal(eng.extremal_counts(X.copy(), tg, algo=algo), want[tg]), algo


@pytest.mark.parametrize("n,T,L", [(21, 9, 1), (20, 9, 1), (301, 70, 1), (300, 5, 1), (301, 130, 2)])
def test_vectors_that_differ_only_at_the_end(eng, n, T, L):
    X = _family(n, T, L)
    want = extremal_counts_lexsort(X)
    assert len(np.unique(want)) >= n - 2                           # the pairs are told apart
    for algo in (IMAGE, SORT):
        assert np.array_equal(eng.extremal_counts(X, algo=algo), want), algo


@pytest.mark.parametrize("n,T", [(21, 9), (300, 70)])
def test_distinct_curves_with_equal_vectors(eng, n, T):
    """Every row ranks the curves 0 .. n - 1: a curve and its mirror have different values and the same vector."""
    X = np.tile(np.arange(n, dtype=np.float64), (T, 1))
    want = extremal_counts_lexsort(X)
    assert np.array_equal(want, want[::-1]) and want[0] == 2
    for algo in (IMAGE, SORT):
        assert np.array_equal(eng.extremal_counts(X, algo=algo), want), algo


def test_smooth_curves_share_long_prefixes(eng):
    T, n = 200, 300
    rng = np.random.default_rng(15)
    t = np.arange(T)[:, None] / T
    X = rng.normal(size=n) + rng.normal(size=n) * np.sin(2 * np.pi * (t + rng.random(size=n)))
    V = -np.sort(-extremity_np(X).T, axis=1)
    order = np.lexsort(V.T[::-1])
    shared = [int(np.argmax(np.append(V[a] != V[b], True))) for a, b in zip(order[:-1], order[1:])]
    assert max(shared) >= 10                                       # far beyond the 4 entries of the head
    want = extremal_counts_lexsort(X)
    for algo in (IMAGE, SORT):
        assert np.array_equal(eng.extremal_counts(X, algo=algo), want), algo


# ---------------------------------------------------------------- head packing boundaries
@pytest.mark.parametrize("n", [65536, 65537])
def test_head_loses_its_fourth_field(eng, n):
    """T = 5; P = 4 at 65 536 curves and 3 at 65 537.  The family's pairs differ from entry 3 on: the last field of the
    head at P = 4, the first entry of the tail at P = 3."""
    X = _family(n, 5, 2)
    assert np.array_equal(eng.extremal_counts(X), extremal_counts_lexsort(X))
    Y = np.round(np.random.default_rng(n).normal(size=(5, n)), 2)
    tg = _subset(n, 5)[:4096]
    assert np.array_equal(eng.extremal_counts(Y, tg), extremal_counts_lexsort(Y)[tg])


@pytest.mark.parametrize("n", [2 ** 21, 2 ** 21 + 1])
def test_head_loses_its_third_field(eng, n):
    """T = 3 on the sort route; P = 3 at 2^21 curves and 2 at 2^21 + 1.  The pairs differ at entry 2."""
    X = _family(n, 3, 1)
    rng = np.random.default_rng(n)
    i = rng.integers(0, n // 2 - 1, size=30)
    tg = np.concatenate([i, n - 1 - i, [0, n - 1, n // 2, n // 2 - 1]]).astype(np.int64)
    want = extremal_counts_lexsort(X)
    assert (want[i] != want[n - 1 - i]).all()
    assert np.array_equal(eng.extremal_counts(X, tg, algo=SORT), want[tg])


# ---------------------------------------------------------------- workspace independence
@pytest.mark.parametrize("T,n,algo", [(70, 300, IMAGE), (70, 2500, SORT)])
@pytest.mark.parametrize("order", ["C", "F"])
def test_workspace_independence(eng, T, n, algo, order):
    from statdepth_amd._native import SD_ERR_WORKSPACE, StatdepthHipError
    X, want = _case(T, n, "tenths")
    A = np.array(X, order=order)
    cm = order == "F"
    rec, floor = eng.extremal_workspace_bytes(T, n, algo=algo, curve_major=cm)
    assert 0 < floor < rec
    fixed = -(-4 * T * n // 256) * 256 + -(-8 * n // 256) * 256    # E and H in front of stage 1's batch
    sizes = [floor, floor + (rec - floor) // 9, floor + (rec - floor) // 2, rec]
    heights = [eng.rank_depth_rows_per_batch(T, n, b - fixed, algo=algo, curve_major=cm) for b in sizes]
    assert heights[0] == 1 and heights[-1] == T and len(set(heights)) == 4
    assert all(h % TILE for h in heights), heights                 # ragged tiles in the batch and in its last one
    assert any(T % h and h > 1 for h in heights), heights          # a last batch shorter than the others
    for b in sizes:
        assert np.array_equal(eng.extremal_counts(A, algo=algo, ws_bytes=b), want), b
    with pytest.raises(StatdepthHipError) as e:
        eng.extremal_counts(A, algo=algo, ws_bytes=floor - 1)
    assert e.value.code == SD_ERR_WORKSPACE


# ---------------------------------------------------------------- properties
@functools.lru_cache(maxsize=None)
def _property_case():
    X = np.random.default_rng(40500).normal(size=(40, 500))
    want = extremal_counts_lexsort(X)
    X.setflags(write=False)
    want.setflags(write=False)
    return X, want


@pytest.mark.parametrize("algo", [IMAGE, SORT])
def test_invariances(eng, algo):
    X, want = _property_case()
    got = eng.extremal_counts(X.copy(), algo=algo)
    assert np.array_equal(got, want)
    assert np.array_equal(eng.extremal_counts(-X, algo=algo), got)                          # A and B change places
    perm = np.random.default_rng(1).permutation(40)
    assert np.array_equal(eng.extremal_counts(X[perm].copy(), algo=algo), got)              # the vector is sorted anyway
    scale = np.linspace(0.5, 3.0, 40)[:, None]
    assert np.array_equal(eng.extremal_counts(np.exp(X * scale) - scale, algo=algo), got)   # ranks within a row stay
    V = -np.sort(-extremity_np(X).T, axis=1)
    assert len(np.unique(V, axis=0)) == 500                        # all vectors distinct: a strict order
    assert np.array_equal(np.sort(got), np.arange(1, 501))


# ---------------------------------------------------------------- public API
def test_api(eng):
    from statdepth_amd import FunctionalDepth
    X = np.round(np.random.default_rng(37).normal(size=(12, 9)).cumsum(axis=0), 1)
    frame = pd.DataFrame(X, index=[f"t{i}" for i in range(12)], columns=list("abcdefghi"))
    want = extremal_counts_lexsort(X) / 9
    d = FunctionalDepth([frame], containment="extremal")
    assert list(d.index) == list(frame.columns)
    assert np.array_equal(d.to_numpy(), want)
    sub = FunctionalDepth([frame], to_compute=["h", "b", "e"], containment="extremal", relax=True)
    assert list(sub.index) == ["h", "b", "e"]
    assert np.array_equal(sub.to_numpy(), want[[7, 1, 4]])
    assert np.array_equal(d.ordered().to_numpy(), np.sort(want)[::-1])
    known = FunctionalDepth([pd.DataFrame(KNOWN_X, columns=list("wxyz"))], containment="extremal")
    assert np.array_equal(known.to_numpy(), KNOWN_ED) and list(known.deepest(1).index) == ["y"]
