"""Exact simplicial depth in the plane on the GPU (K13, sd_simplicial2_*): counts EQUAL to the numpy restatement of
tests/test_simplicial_exact_host.py, from the sweep and from the pairwise kernel -- smallest shapes, integer clouds with
duplicates and collinear triples, the nearly collinear cloud (which a rounded predicate fails), a cloud on one line (one
group holds everything), every capacity tier of the sweep from below, at and above, target lists, external and block
forms, K4's enumeration on the golden fixtures, and the public API (containment='simplex_exact')."""
import functools
from math import comb

import numpy as np
import pandas as pd
import pytest

from conftest import frame_df, load_golden
from test_halfspace_exact_host import integer_cloud, nearly_collinear_cloud
from test_simplicial_exact_host import (EQUAL, LINE, SQUARE, SQUARE_EXTERNAL, simplicial_counts, simplicial_external,
                                        simplicial_sampled)

pytestmark = pytest.mark.gpu

ALGOS = ("sweep", "pairwise")
TIERS = (64, 512, 2048, 8192)                                          # others a sweep workgroup holds, per tier


@pytest.fixture(scope="module")
def eng():
    from statdepth_amd import engine
    return engine


def _continuous(n):
    return np.random.default_rng(3000 + n).normal(size=(n, 2))


@functools.lru_cache(maxsize=None)
def _checked(n):
    """(targets, their counts by the restatement) of _continuous(n): every target up to n = 257, 16 beyond, 2 from
    n = 8192 on; computed once per size and not modified."""
    P = _continuous(n)
    if n <= 257:
        tg = np.arange(n)
    else:
        tg = np.sort(np.random.default_rng(n).permutation(n)[:2 if n >= 8192 else 16])
    want = simplicial_counts(P, tg)
    for a in (tg, want):
        a.setflags(write=False)
    return tg, want


# ---------------------------------------------------------------- smallest shapes
@pytest.mark.parametrize("algo", ALGOS + ("auto",))
@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_smallest_shapes(eng, n, algo):
    P = np.random.default_rng(10 + n).normal(size=(n, 2))
    got = eng.simplicial_exact_counts(P, algo=algo)
    assert np.array_equal(got, simplicial_counts(P))
    if n <= 3:
        assert got.tolist() == [0] * n                                 # fewer than 3 others: no triple
    else:
        assert set(got.tolist()) <= {0, 1} and got.dtype == np.int64   # one triangle per target
    Q = np.vstack([P[:1] + 0.25, P[:1]])
    assert np.array_equal(eng.simplicial_exact_external_counts(P, Q, algo=algo), simplicial_external(P, Q))
    same = np.repeat(P[:1], n, axis=0)                                 # no nonzero vector at all: every triple counts
    assert eng.simplicial_exact_counts(same, algo=algo).tolist() == [comb(n - 1, 3)] * n


@pytest.mark.parametrize("algo", ALGOS + ("auto",))
def test_hand_cases(eng, algo):
    assert eng.simplicial_exact_counts(LINE, algo=algo).tolist() == [0, 10, 16, 18, 16, 10, 0]
    assert eng.simplicial_exact_counts(SQUARE, algo=algo).tolist() == [0, 0, 0, 0, 4]
    assert eng.simplicial_exact_counts(EQUAL, algo=algo).tolist() == [4] * 5
    assert eng.simplicial_exact_external_counts(SQUARE, SQUARE_EXTERNAL, algo=algo).tolist() == [10, 6, 0, 3]
    same = np.full((70, 2), -3.5)                                      # all duplicates, two runs of 64 others
    assert eng.simplicial_exact_counts(same, algo=algo).tolist() == [comb(69, 3)] * 70


# ---------------------------------------------------------------- ties, duplicates, collinear triples
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("n", [40, 257])
def test_integer_clouds(eng, n, algo):
    P = integer_cloud(n, n)
    assert np.array_equal(eng.simplicial_exact_counts(P, algo=algo), simplicial_counts(P))


@pytest.mark.parametrize("algo", ALGOS)
def test_nearly_collinear_cloud_needs_the_exact_predicate(eng, algo):
    """tests/test_simplicial_exact_host.py::test_rounded_predicate_is_not_a_substitute: counting with rounded signs changes
    counts on this cloud."""
    P = nearly_collinear_cloud()
    assert np.array_equal(eng.simplicial_exact_counts(P, algo=algo), simplicial_counts(P))


def test_one_line(eng):
    """2 048 points on one line through the origin: two directions, so one group holds all 2 047 vectors -- the tie-heavy
    worst case of the group handling.  The target at position p has a = p points on one side and b = 2047 - p on the other."""
    P = np.outer(np.arange(-1024, 1024), [1.0, 2.0])
    tg = np.array([0, 1, 2, 63, 64, 65, 511, 1023, 1024, 1025, 1500, 1983, 1984, 2045, 2046, 2047])
    want = np.array([comb(2047, 3) - comb(int(p), 3) - comb(2047 - int(p), 3) for p in tg], dtype=np.int64)
    sweep = eng.simplicial_exact_counts(P, tg, algo="sweep")
    assert np.array_equal(sweep, eng.simplicial_exact_counts(P, tg, algo="pairwise"))
    assert np.array_equal(sweep, want)


# ---------------------------------------------------------------- the sweep's capacity tiers
@pytest.mark.parametrize("n", [c + 1 + o for c in TIERS[:3] for o in (-1, 0, 1)])
def test_tier_boundaries(eng, n):
    """CAP - 1, CAP, CAP + 1 OTHERS of a row target: samples of CAP, CAP + 1, CAP + 2 points."""
    P = _continuous(n)
    tg, want = _checked(n)
    tg = tg.copy()                                                     # (torch wants a writable array)
    for algo in ALGOS:
        assert np.array_equal(eng.simplicial_exact_counts(P, tg, algo=algo), want), algo
    if n > 257:                                                        # every target: the two kernels against each other
        assert np.array_equal(eng.simplicial_exact_counts(P), eng.simplicial_exact_counts(P, algo="pairwise"))


@pytest.mark.parametrize("n", [8192, 8193, 8194])
def test_capacity_limit(eng, n):
    """8 191 / 8 192 / 8 193 others.  Below and at the capacity the sweep (by name and as auto's choice), one above it auto
    alone (the sweep is refused there), against the pairwise kernel on 64 targets and against numpy on 2."""
    from statdepth_amd._native import SD_ERR_UNSUPPORTED, StatdepthHipError
    P = _continuous(n)
    tg, want = _checked(n)
    tg = tg.copy()                                                     # (torch wants a writable array)
    t64 = np.sort(np.random.default_rng(1).permutation(n)[:64])
    pair = eng.simplicial_exact_counts(P, t64, algo="pairwise")
    assert np.array_equal(eng.simplicial_exact_counts(P, t64), pair)
    assert np.array_equal(eng.simplicial_exact_counts(P, tg), want)
    if n - 1 <= 8192:
        assert np.array_equal(eng.simplicial_exact_counts(P, t64, algo="sweep"), pair)
        assert np.array_equal(eng.simplicial_exact_counts(P, tg, algo="sweep"), want)
    else:
        with pytest.raises(StatdepthHipError) as e:
            eng.simplicial_exact_counts(P, tg, algo="sweep")
        assert e.value.code == SD_ERR_UNSUPPORTED


# ---------------------------------------------------------------- target lists
@pytest.mark.parametrize("algo", ALGOS)
def test_targets(eng, algo):
    P = _continuous(257)
    _, want = _checked(257)
    rng = np.random.default_rng(3)
    for tg in (np.array([5, 100, 256]), rng.permutation(257), np.array([7, 7, 0, 7, 256, 0])):
        assert np.array_equal(eng.simplicial_exact_counts(P, tg, algo=algo), want[tg])
    assert eng.simplicial_exact_counts(P, [], algo=algo).shape == (0,)
    for bad in ([257], [-1], [0, 300]):
        with pytest.raises(ValueError):
            eng.simplicial_exact_counts(P, bad, algo=algo)


# ---------------------------------------------------------------- external form
@pytest.mark.parametrize("algo", ALGOS)
def test_external_form(eng, algo):
    for P in (_continuous(65), integer_cloud(40, 9), nearly_collinear_cloud()):
        rng = np.random.default_rng(len(P))
        Q = np.vstack([P[[3, 0, len(P) - 1]],                          # sample points: their own row is an other, a duplicate
                       [[1e6, -1e6], [-1e9, 3.0]],                     # far away: inside no triangle
                       rng.normal(size=(6, 2)), np.round(rng.normal(size=(4, 2)))])
        got = eng.simplicial_exact_external_counts(P, Q, algo=algo)
        assert got[3:5].tolist() == [0, 0]
        assert np.array_equal(got, simplicial_external(P, Q))
        assert np.array_equal(got, [simplicial_counts(np.vstack([P, g]), [len(P)])[0] for g in Q])
    assert eng.simplicial_exact_external_counts(_continuous(65), np.empty((0, 2)), algo=algo).shape == (0,)


# ---------------------------------------------------------------- block form
@pytest.mark.parametrize("algo", ALGOS)
def test_block_form(eng, algo):
    P = integer_cloud(40, 11)
    C = _continuous(257)
    blocks = [[3, 9, 27, 5, 12], [12], [], [5, 5, 12, 5], list(range(39, -1, -1)), [0, 1], [7, 30, 7, 7], [1, 2, 3],
              [8, 6, 4, 2, 0, 1, 3, 5, 7, 9, 11]]
    width = max(len(b) for b in blocks)
    mem = np.full((len(blocks), width), -1, dtype=np.int32)            # ragged, padded with -1
    for i, b in enumerate(blocks):
        mem[i, :len(b)] = b
    for X in (P, C):
        want = [simplicial_counts(X[b], [len(b) - 1])[0] if b else 0 for b in blocks]
        assert all(w == 0 for w, b in zip(want, blocks) if len(b) <= 3)
        assert eng.simplicial_exact_subset_counts(X, mem, algo=algo).tolist() == want
    wide = np.full((3, 300), -1, dtype=np.int32)                       # a wider tier, blocks of 257, 1 and 70 rows
    wide[0, :257] = np.random.default_rng(0).permutation(257)
    wide[1, 0] = 4
    wide[2, :70] = np.arange(70)
    want = [simplicial_counts(C[r[r >= 0]], [int((r >= 0).sum()) - 1])[0] for r in wide]
    assert eng.simplicial_exact_subset_counts(C, wide, algo=algo).tolist() == want
    for bad in ([[0, 40]], [[-2, 1]]):
        with pytest.raises(ValueError):
            eng.simplicial_exact_subset_counts(P, bad, algo=algo)


def test_block_across_a_tier(eng):
    """A block of 2 049 members (2 048 others: the 2048 tier at its capacity) beside one of 2 050 slots (2 049 others: the
    8192 tier) and short ones."""
    n = 2100
    P = _continuous(n)
    rng = np.random.default_rng(4)
    for bs in (2049, 2050):
        mem = np.full((3, bs), -1, dtype=np.int32)
        mem[0] = rng.permutation(n)[:bs]
        mem[1, :5] = [9, 8, 7, 6, 5]
        mem[2, :2049] = rng.permutation(n)[:2049]
        want = [simplicial_counts(P[r[r >= 0]], [int((r >= 0).sum()) - 1])[0] for r in mem]
        for algo in ALGOS:
            assert eng.simplicial_exact_subset_counts(P, mem, algo=algo).tolist() == want, (bs, algo)


# ---------------------------------------------------------------- K4's enumeration
@pytest.mark.parametrize("name", ["g5_pc_n30_d2", "g5_pc_n12_d2", "g5_pc_grid_d2"])
def test_agreement_with_the_enumeration(eng, name):
    fx = load_golden(name)
    df = frame_df(fx["input"])
    P = df.to_numpy(dtype=np.float64)
    k4 = eng.pointcloud_simplex_counts(P)
    pos = df.index.get_indexer(fx["index"])
    assert np.array_equal(k4[pos], np.array(fx["counts"], dtype=np.int64))
    for algo in ALGOS:
        assert np.array_equal(eng.simplicial_exact_counts(P, algo=algo), k4), algo


# ---------------------------------------------------------------- public API
def test_public_api(eng):
    from statdepth_amd import PointcloudDepth
    P = np.random.default_rng(5).normal(size=(200, 2))
    df = pd.DataFrame(P, index=[f"p{i}" for i in range(200)])
    want = simplicial_counts(P)
    exact = PointcloudDepth(df, containment='simplex_exact')
    assert list(exact.index) == list(df.index)
    assert np.array_equal(exact.to_numpy(), want / comb(200, 3))
    assert np.array_equal(PointcloudDepth(df, containment='simplex_exact', directions=3, seed=99).to_numpy(),
                          want / comb(200, 3))                         # directions and seed are ignored
    some = ["p7", "p0", "p199"]
    part = PointcloudDepth(df, to_compute=some, containment='simplex_exact')
    assert list(part.index) == some
    assert np.array_equal(part.to_numpy(), want[[7, 0, 199]] / comb(200, 3))
    assert np.array_equal(PointcloudDepth(df, K=1, containment='simplex_exact').to_numpy(), want / comb(200, 3))
    with pytest.raises(NotImplementedError, match="containment='simplex'"):
        PointcloudDepth(pd.DataFrame(np.random.default_rng(8).normal(size=(20, 3))), containment='simplex_exact')


def test_public_api_sampled(eng):
    from statdepth_amd import PointcloudDepth
    P = np.random.default_rng(6).normal(size=(30, 2))
    P[4] = P[20]                                                       # a duplicated point among the draws
    df = pd.DataFrame(P)
    np.random.seed(12)
    got = PointcloudDepth(df, to_compute=[0, 4, 29], K=3, containment='simplex_exact').to_numpy()
    after = np.random.random()
    np.random.seed(12)
    assert np.array_equal(got, simplicial_sampled(P, [0, 4, 29], 3))
    assert after == np.random.random()                                 # the draws and nothing else consumed the global RNG
    np.random.seed(12)
    PointcloudDepth(df, to_compute=[0, 4, 29], K=3, containment='l1')
    assert after == np.random.random()                                 # the same draws as any other containment


def _homogeneity_restated(Fx, Gx, method):
    Fd, Gd = simplicial_counts(Fx) / comb(len(Fx), 3), simplicial_counts(Gx) / comb(len(Gx), 3)
    ext = simplicial_external(Fx, Gx) / comb(len(Fx) + 1, 3)
    # median() = deepest(n=1): the first of the largest values in pandas' descending sort order
    g_star = pd.Series(Gd).sort_values(ascending=False).index[0]
    return ext[g_star] / Fd.max() if method == 'p1' else ext.max() / Gd.max()


@pytest.mark.parametrize("method", ["p1", "p3"])
def test_pointcloud_homogeneity(eng, method):
    """P1 and P3 as their host composition: depths of F and G, the points of G as external targets inside F u {g}.
    PointcloudHomogeneity takes samples of equal length only (the reference's check), so the coefficient is checked on
    30 + 30 points and the external depths it is made of on 30 + 20."""
    from statdepth_amd.homogeneity import PointcloudHomogeneity
    from statdepth_amd.homogeneity.homogeneity import _external_point_depths
    rng = np.random.default_rng(31)
    F = pd.DataFrame(rng.normal(size=(30, 2)), index=[f"f{i}" for i in range(30)])
    G = pd.DataFrame(rng.normal(size=(30, 2)) * 0.8 + 0.2, index=[f"g{i}" for i in range(30)])
    got = PointcloudHomogeneity(F, G, method=method, containment='simplex_exact').homogeneity()
    assert got == _homogeneity_restated(F.to_numpy(), G.to_numpy(), method)
    G20 = G.iloc[:20]
    assert np.array_equal(_external_point_depths(F, G20, None, 'simplex_exact'),
                          simplicial_external(F.to_numpy(), G20.to_numpy()) / comb(31, 3))


def test_engine_refuses_what_the_predicate_cannot_take(eng):
    P = _continuous(65).copy()
    with pytest.raises(ValueError, match="'auto', 'sweep' or 'pairwise'"):
        eng.simplicial_exact_counts(P, algo="rank")
    with pytest.raises(ValueError, match="n x 2"):
        eng.simplicial_exact_counts(np.zeros((5, 3)))
    for bad in (np.nan, np.inf, 2.0 ** 501):
        P[7, 1] = bad
        with pytest.raises(ValueError, match=r"2\^500"):
            eng.simplicial_exact_counts(P)
        with pytest.raises(ValueError, match=r"2\^500"):
            eng.simplicial_exact_external_counts(_continuous(65), P[6:8])
