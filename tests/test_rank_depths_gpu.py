"""Integrated rank depths on the GPU (K14, sd_rank_depth_sums): the int64 records EQUAL to an O(n log n) numpy restatement
(np.sort per row + np.searchsorted) on both routes -- smallest shapes, ties, duplicated curves, a constant row, infinities,
both memory layouts, target lists, the sort route's tile and merge boundaries, the boundary between the routes, workspace
independence, the fold's row batching -- and the public API against the definitions of tests/test_rank_depths_host.py."""
import functools

import numpy as np
import pandas as pd
import pytest

from conftest import assert_depths_close
from test_rank_depths_host import KNOWN_DEPTHS, KNOWN_RECORDS, KNOWN_X, NAMES, depths_np, records_np

pytestmark = pytest.mark.gpu

IMAGE, SORT = 1, 2


@pytest.fixture(scope="module")
def eng():
    from statdepth_amd import engine
    return engine


def records_sorted(X):
    """The record (SA, SB, SF, SM, MM) of every curve: B = searchsorted left, A = n - searchsorted right, per sorted row."""
    X = np.asarray(X, dtype=np.float64)
    T, n = X.shape
    R = np.zeros((n, 5), dtype=np.int64)
    for t in range(T):
        s = np.sort(X[t])
        B = np.searchsorted(s, X[t], "left").astype(np.int64)
        A = n - np.searchsorted(s, X[t], "right").astype(np.int64)
        M = np.maximum(A, B)
        R[:, 0] += A
        R[:, 1] += B
        R[:, 2] += np.abs(2 * A - n)
        R[:, 3] += M
        R[:, 4] = np.maximum(R[:, 4], M)
    return R


KINDS = ("normal", "tenths", "duplicated", "constant_row", "infinities")


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
    return X


@functools.lru_cache(maxsize=None)
def _case(T, n, kind):
    """(X, records of every curve by the restatement), computed once per case and not modified."""
    X = _data(T, n, kind, 100 * T + n)
    want = records_sorted(X)
    X.setflags(write=False)
    want.setflags(write=False)
    return X, want


def _subset(n, seed):
    """A shuffled subset of the curves with one index twice."""
    rng = np.random.default_rng(seed)
    tg = rng.permutation(n)[:max(2, (2 * n) // 3)]
    tg[-1] = tg[0]
    return tg.astype(np.int64)


def test_restatements_agree():
    """The sorted restatement used here is the integer restatement of the host tests (which the C oracle pins)."""
    for kind in KINDS:
        X = _data(7, 9, kind, 5)
        assert np.array_equal(records_sorted(X), records_np(X)), kind
    assert np.array_equal(records_sorted(KNOWN_X), KNOWN_RECORDS)


# ---------------------------------------------------------------- small shapes, both routes, both layouts, target lists
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T,n", [(1, 2), (3, 5), (7, 64), (33, 257), (17, 1025), (5, 4097)])
def test_small_shapes(eng, T, n, kind):
    X, want = _case(T, n, kind)
    tg = _subset(n, T + n)
    for algo in (IMAGE, SORT):
        for A in (np.array(X, order="C"), np.array(X, order="F")):            # writable copies in either layout
            assert np.array_equal(eng.rank_depth_sums(A, algo=algo), want), (algo, A.flags.f_contiguous)
            assert np.array_equal(eng.rank_depth_sums(A, tg, algo=algo), want[tg]), (algo, A.flags.f_contiguous, "subset")


def test_known_answer_records(eng):
    for algo in (0, IMAGE, SORT, "auto", "image", "sort"):
        assert np.array_equal(eng.rank_depth_sums(KNOWN_X, algo=algo), KNOWN_RECORDS)


# ---------------------------------------------------------------- tile and merge boundaries of the sort route
@pytest.mark.parametrize("n", [2047, 2048, 2049, 4097, 6145])
def test_sort_route_tie_runs_cross_tiles(eng, n):
    """Values from 50 integers: runs of ties some n / 50 long cross the 2048-value tiles and the merge passes' borders."""
    X = np.random.default_rng(n).integers(0, 50, size=(3, n)).astype(np.float64)
    want = records_sorted(X)
    assert np.array_equal(eng.rank_depth_sums(X, algo=SORT), want)
    assert np.array_equal(eng.rank_depth_sums(X, algo=IMAGE), want)


# ---------------------------------------------------------------- the boundary between the routes
@pytest.mark.parametrize("n", [16384, 16385])
def test_route_boundary(eng, n):
    X = np.random.default_rng(n).normal(size=(2, n))
    X[1, ::7] = np.round(X[1, ::7], 1)
    assert np.array_equal(eng.rank_depth_sums(X, algo=0), records_sorted(X))


def test_image_route_refuses_more_than_16384_curves(eng):
    from statdepth_amd._native import SD_ERR_UNSUPPORTED, StatdepthHipError
    X = np.zeros((2, 16385))
    with pytest.raises(StatdepthHipError) as e:
        eng.rank_depth_sums(X, algo=IMAGE)
    assert e.value.code == SD_ERR_UNSUPPORTED


# ---------------------------------------------------------------- workspace independence
@pytest.mark.parametrize("T,n,algo", [(70, 300, IMAGE), (70, 2500, SORT)])
@pytest.mark.parametrize("order", ["C", "F"])
def test_workspace_independence(eng, T, n, algo, order):
    from statdepth_amd._native import SD_ERR_WORKSPACE, StatdepthHipError
    X, want = _case(T, n, "tenths")
    A = np.array(X, order=order)
    rec, floor = eng.rank_depth_workspace_bytes(T, n, algo=algo, curve_major=order == "F")
    assert 0 < floor < rec
    at_floor = eng.rank_depth_sums(A, algo=algo, ws_bytes=floor)       # one row per batch: 70 batches
    at_rec = eng.rank_depth_sums(A, algo=algo, ws_bytes=rec)
    between = eng.rank_depth_sums(A, algo=algo, ws_bytes=floor + (rec - floor) // 9)
    assert np.array_equal(at_floor, at_rec) and np.array_equal(at_floor, between)
    assert np.array_equal(at_floor, want)
    with pytest.raises(StatdepthHipError) as e:
        eng.rank_depth_sums(A, algo=algo, ws_bytes=floor - 1)
    assert e.value.code == SD_ERR_WORKSPACE


# ---------------------------------------------------------------- row batching of the fold
@pytest.mark.parametrize("algo", [IMAGE, SORT])
def test_fold_row_slices(eng, algo):
    """2051 rows over the fold's 16 slices: 16 unrolled steps of 8 rows and a ragged tail of 0 or 1 row per slice."""
    X, want = _case(2051, 130, "tenths")
    X = X.copy()
    assert np.array_equal(eng.rank_depth_sums(X, algo=algo), want)
    tg = _subset(130, 9)
    assert np.array_equal(eng.rank_depth_sums(X, tg, algo=algo), want[tg])


# ---------------------------------------------------------------- public API
@pytest.fixture(scope="module")
def frame():
    # seed 37: values tie inside rows, yet no two curves tie in depth for five of the six names (infimal_halfspace takes
    # multiples of 1/9 and must tie), so the order of the labels is determined there
    X = np.round(np.random.default_rng(37).normal(size=(12, 9)).cumsum(axis=0), 1)
    return pd.DataFrame(X, index=[f"t{i}" for i in range(12)], columns=list("abcdefghi"))


def test_api_all_names(frame):
    from statdepth_amd import FunctionalDepth
    r2_before = FunctionalDepth([frame], containment="r2", relax=True).to_numpy().copy()
    want = depths_np(frame.to_numpy())
    got, ties_free = {}, []
    for name in NAMES:
        d = FunctionalDepth([frame], containment=name)
        assert list(d.index) == list(frame.columns)
        assert_depths_close(d.to_numpy(), want[name])
        got[name] = d.to_numpy()
        sub = FunctionalDepth([frame], to_compute=["h", "b", "e"], containment=name, relax=True)
        assert list(sub.index) == ["h", "b", "e"]
        assert_depths_close(sub.to_numpy(), want[name][[7, 1, 4]])
        by_depth = sorted(range(9), key=lambda i: -want[name][i])     # the labels' order when no two depths tie
        if len(set(np.round(want[name], 12))) == 9:
            ties_free.append(name)
            assert list(d.ordered().index) == [frame.columns[i] for i in by_depth]
            assert list(d.deepest(2).index) == [frame.columns[i] for i in by_depth[:2]]
            assert list(d.outlying(1).index) == [frame.columns[by_depth[-1]]]
        assert sorted(d.ordered().index) == sorted(frame.columns)
        assert_depths_close(d.ordered().to_numpy(), np.sort(want[name])[::-1])
        assert_depths_close(d.deepest(2).to_numpy(), np.sort(want[name])[::-1][:2])
    assert ties_free == [name for name in NAMES if name != "infimal_halfspace"]
    assert np.array_equal(got["half_region"], np.minimum(got["mei"], got["mhi"]))
    r2_after = FunctionalDepth([frame], containment="r2", relax=True).to_numpy()
    assert np.array_equal(r2_before, r2_after)


def test_api_known_answer():
    from statdepth_amd import FunctionalDepth
    df = pd.DataFrame(KNOWN_X, columns=["x", "y", "z"])
    for name in NAMES:
        d = FunctionalDepth([df], containment=name)
        assert_depths_close(d.to_numpy(), np.array([float(f) for f in KNOWN_DEPTHS[name]]))
        assert list(d.index) == ["x", "y", "z"]
