"""Exact halfspace (Tukey) depth in the plane on the GPU (K11, sd_halfspace2_*): counts EQUAL to the numpy restatement of
tests/test_halfspace_exact_host.py, from the sweep and from the pairwise kernel -- smallest shapes, integer clouds with
duplicates and collinear triples, the nearly collinear cloud (which a rounded predicate fails), every capacity tier of the
sweep from below, at and above, target lists, external and block forms, and the public API (directions='exact')."""
import functools

import numpy as np
import pandas as pd
import pytest

from test_halfspace_exact_host import (exact_counts, exact_external, exact_sampled, integer_cloud,
                                       nearly_collinear_cloud)
from test_halfspace_host import make_directions

pytestmark = pytest.mark.gpu

ALGOS = ("sweep", "pairwise")
TIERS = (64, 512, 2048, 8192)                                          # sample points a sweep workgroup holds, per tier


@pytest.fixture(scope="module")
def eng():
    from statdepth_amd import engine
    return engine


def _continuous(n):
    return np.random.default_rng(2000 + n).normal(size=(n, 2))


@functools.lru_cache(maxsize=None)
def _checked(n):
    """(targets, their counts by the restatement) of _continuous(n): every target up to n = 257, 16 beyond, 2 from
    n = 8191 on; computed once per size and not modified."""
    P = _continuous(n)
    if n <= 257:
        tg = np.arange(n)
    else:
        tg = np.sort(np.random.default_rng(n).permutation(n)[:2 if n >= 8191 else 16])
    want = exact_counts(P, tg)
    for a in (tg, want):
        a.setflags(write=False)
    return tg, want


# ---------------------------------------------------------------- smallest shapes
@pytest.mark.parametrize("algo", ALGOS + ("auto",))
@pytest.mark.parametrize("n", [1, 2, 3])
def test_smallest_shapes(eng, n, algo):
    P = np.random.default_rng(10 + n).normal(size=(n, 2))
    assert np.array_equal(eng.halfspace_exact_counts(P, algo=algo), exact_counts(P))
    assert eng.halfspace_exact_counts(P, algo=algo).tolist() == [1] * n
    Q = np.vstack([P[:1] + 0.25, P[:1]])
    assert np.array_equal(eng.halfspace_exact_external_counts(P, Q, algo=algo), exact_external(P, Q))
    same = np.repeat(P[:1], n, axis=0)                                 # no nonzero vector at all
    assert eng.halfspace_exact_counts(same, algo=algo).tolist() == [n] * n


def test_hand_cases(eng):
    line = np.array([[i, 2.0 * i] for i in range(7)], dtype=np.float64)
    square = np.array([[1, 1], [1, -1], [-1, 1], [-1, -1], [0, 0]], dtype=np.float64)
    for algo in ALGOS:
        assert eng.halfspace_exact_counts(line, algo=algo).tolist() == [1, 2, 3, 4, 3, 2, 1]
        assert eng.halfspace_exact_counts(square, algo=algo).tolist() == [1, 1, 1, 1, 3]
        assert eng.halfspace_exact_counts(np.full((5, 2), 0.25), algo=algo).tolist() == [5] * 5


# ---------------------------------------------------------------- ties, duplicates, collinear triples
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("n", [40, 257])
def test_integer_clouds(eng, n, algo):
    P = integer_cloud(n, n)
    assert np.array_equal(eng.halfspace_exact_counts(P, algo=algo), exact_counts(P))


@pytest.mark.parametrize("algo", ALGOS)
def test_nearly_collinear_cloud_needs_the_exact_predicate(eng, algo):
    """tests/test_halfspace_exact_host.py::test_rounded_cross_product_is_not_a_substitute: counting with the sign of the
    rounded cross product changes counts on this cloud."""
    P = nearly_collinear_cloud()
    assert np.array_equal(eng.halfspace_exact_counts(P, algo=algo), exact_counts(P))


# ---------------------------------------------------------------- the sweep's capacity tiers
@pytest.mark.parametrize("n", [c + o for c in TIERS[:3] for o in (-1, 0, 1)])
def test_tier_boundaries(eng, n):
    P = _continuous(n)
    tg, want = _checked(n)
    tg = tg.copy()                                                     # (torch wants a writable array)
    for algo in ALGOS:
        assert np.array_equal(eng.halfspace_exact_counts(P, tg, algo=algo), want), algo
    if n > 257:                                                        # every target: the two kernels against each other
        assert np.array_equal(eng.halfspace_exact_counts(P), eng.halfspace_exact_counts(P, algo="pairwise"))


@pytest.mark.parametrize("n", [8191, 8192, 8193])
def test_capacity_limit(eng, n):
    """The largest tier: below and at the capacity the sweep (by name and as auto's choice), one point above it auto alone
    (the sweep is refused there), against the pairwise kernel on 64 targets and against numpy on 2."""
    from statdepth_amd._native import SD_ERR_UNSUPPORTED, StatdepthHipError
    P = _continuous(n)
    tg, want = _checked(n)
    tg = tg.copy()                                                     # (torch wants a writable array)
    t64 = np.sort(np.random.default_rng(1).permutation(n)[:64])
    pair = eng.halfspace_exact_counts(P, t64, algo="pairwise")
    assert np.array_equal(eng.halfspace_exact_counts(P, t64), pair)
    assert np.array_equal(eng.halfspace_exact_counts(P, tg), want)
    if n <= 8192:
        assert np.array_equal(eng.halfspace_exact_counts(P, t64, algo="sweep"), pair)
        assert np.array_equal(eng.halfspace_exact_counts(P, tg, algo="sweep"), want)
    else:
        with pytest.raises(StatdepthHipError) as e:
            eng.halfspace_exact_counts(P, tg, algo="sweep")
        assert e.value.code == SD_ERR_UNSUPPORTED


# ---------------------------------------------------------------- target lists
@pytest.mark.parametrize("algo", ALGOS)
def test_targets(eng, algo):
    P = _continuous(257)
    _, want = _checked(257)
    rng = np.random.default_rng(3)
    for tg in (np.array([5, 100, 256]), rng.permutation(257), np.array([7, 7, 0, 7, 256, 0])):
        assert np.array_equal(eng.halfspace_exact_counts(P, tg, algo=algo), want[tg])
    assert eng.halfspace_exact_counts(P, [], algo=algo).shape == (0,)
    for bad in ([257], [-1], [0, 300]):
        with pytest.raises(ValueError):
            eng.halfspace_exact_counts(P, bad, algo=algo)


# ---------------------------------------------------------------- external form
@pytest.mark.parametrize("algo", ALGOS)
def test_external_form(eng, algo):
    for P in (_continuous(65), integer_cloud(40, 9), nearly_collinear_cloud()):
        own = exact_counts(P)
        rng = np.random.default_rng(len(P))
        Q = np.vstack([P[[3, 0, len(P) - 1]],                          # sample points: their own count + 1
                       [[1e6, -1e6], [-1e9, 3.0]],                     # far away: alone in a halfplane
                       rng.normal(size=(6, 2)), np.round(rng.normal(size=(4, 2)))])
        got = eng.halfspace_exact_external_counts(P, Q, algo=algo)
        assert got[:3].tolist() == (own[[3, 0, len(P) - 1]] + 1).tolist()
        assert got[3:5].tolist() == [1, 1]
        assert np.array_equal(got, exact_external(P, Q))
        assert np.array_equal(got, [exact_counts(np.vstack([P, g]), [len(P)])[0] for g in Q])
    assert eng.halfspace_exact_external_counts(_continuous(65), np.empty((0, 2)), algo=algo).shape == (0,)


# ---------------------------------------------------------------- block form
@pytest.mark.parametrize("algo", ALGOS)
def test_block_form(eng, algo):
    P = integer_cloud(40, 11)
    C = _continuous(257)
    blocks = [[3, 9, 27, 5, 12], [12], [], [5, 5, 12, 5], list(range(39, -1, -1)), [0, 1], [7, 30, 7, 7]]
    width = max(len(b) for b in blocks)
    mem = np.full((len(blocks), width), -1, dtype=np.int32)
    for i, b in enumerate(blocks):
        mem[i, :len(b)] = b
    for X in (P, C):
        want = [exact_counts(X[b], [len(b) - 1])[0] if b else 0 for b in blocks]
        assert eng.halfspace_exact_subset_counts(X, mem, algo=algo).tolist() == want
    wide = np.full((3, 300), -1, dtype=np.int32)                       # a wider tier, blocks of 257, 1 and 70 rows
    wide[0, :257] = np.random.default_rng(0).permutation(257)
    wide[1, 0] = 4
    wide[2, :70] = np.arange(70)
    want = [exact_counts(C[r[r >= 0]], [int((r >= 0).sum()) - 1])[0] for r in wide]
    assert eng.halfspace_exact_subset_counts(C, wide, algo=algo).tolist() == want
    for bad in ([[0, 40]], [[-2, 1]]):
        with pytest.raises(ValueError):
            eng.halfspace_exact_subset_counts(P, bad, algo=algo)


# ---------------------------------------------------------------- public API
def test_public_api_exact(eng):
    from statdepth_amd import PointcloudDepth
    P = np.random.default_rng(5).normal(size=(200, 2))
    df = pd.DataFrame(P, index=[f"p{i}" for i in range(200)])
    want = exact_counts(P)
    exact = PointcloudDepth(df, containment='halfspace', directions='exact')
    assert np.array_equal(exact.to_numpy(), want / 200)
    assert np.array_equal(PointcloudDepth(df, containment='halfspace', directions='exact', seed=99).to_numpy(), want / 200)
    coarse = PointcloudDepth(df, containment='halfspace', directions=8).to_numpy()
    assert (exact.to_numpy() <= coarse).all()
    assert (exact.to_numpy() < coarse).sum() == 160
    some = ["p7", "p0", "p199"]
    part = PointcloudDepth(df, to_compute=some, containment='halfspace', directions='exact')
    assert list(part.index) == some
    assert np.array_equal(part.to_numpy(), want[[7, 0, 199]] / 200)
    assert np.array_equal(PointcloudDepth(df, K=1, containment='halfspace', directions='exact').to_numpy(), want / 200)


def test_public_api_sampled(eng):
    from statdepth_amd import PointcloudDepth
    P = np.random.default_rng(6).normal(size=(30, 2))
    P[4] = P[20]                                                       # a duplicated point among the draws
    df = pd.DataFrame(P)
    np.random.seed(12)
    got = PointcloudDepth(df, to_compute=[0, 4, 29], K=4, containment='halfspace', directions='exact').to_numpy()
    np.random.seed(12)
    assert np.array_equal(got, exact_sampled(P, [0, 4, 29], 4))


def test_public_api_other_dimensions(eng):
    from statdepth_amd import PointcloudDepth
    x = pd.DataFrame(np.random.default_rng(8).integers(-5, 6, size=(31, 1)).astype(np.float64))
    k10 = PointcloudDepth(x, containment='halfspace', directions=[[1.0]]).to_numpy()
    assert np.array_equal(PointcloudDepth(x, containment='halfspace', directions='exact').to_numpy(), k10)
    with pytest.raises(NotImplementedError, match='implemented for the plane'):
        PointcloudDepth(pd.DataFrame(np.random.default_rng(8).normal(size=(20, 3))), containment='halfspace',
                        directions='exact')
    with pytest.raises(ValueError, match="or 'exact'"):
        PointcloudDepth(pd.DataFrame(np.random.default_rng(8).normal(size=(20, 2))), containment='halfspace',
                        directions='tukey')


def test_engine_refuses_what_the_predicate_cannot_take(eng):
    P = _continuous(65).copy()
    with pytest.raises(ValueError, match="'auto', 'sweep' or 'pairwise'"):
        eng.halfspace_exact_counts(P, algo="rank")
    with pytest.raises(ValueError, match="n x 2"):
        eng.halfspace_exact_counts(np.zeros((5, 3)))
    for bad in (np.nan, np.inf, 2.0 ** 501):
        P[7, 1] = bad
        with pytest.raises(ValueError, match=r"2\^500"):
            eng.halfspace_exact_counts(P)
        with pytest.raises(ValueError, match=r"2\^500"):
            eng.halfspace_exact_external_counts(_continuous(65), P[6:8])
