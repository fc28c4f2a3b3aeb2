"""Exact simplicial depth in the plane (containment='simplex_exact', K13) without a GPU: the numpy restatement of the
definition (C(m, 3) - sum_j C(e_j, 2) over the vectors to the target's others, exact signs) against hand-computed cases,
against brute-force triangle enumeration in rational arithmetic and against the reference's golden counts; the rounded
predicate shown to be no substitute; invariances; the host-side validation, the C ABI's refusals, and the missing device
reported as such (no CPU fallback).

The restatement (`simplicial_counts`, `simplicial_external`, `simplicial_sampled`) is imported by
tests/test_simplicial_exact_gpu.py as its oracle.
"""
import ctypes
import itertools
from fractions import Fraction
from math import comb

import numpy as np
import pandas as pd
import pytest

from conftest import frame_df, load_golden
from test_halfspace_exact_host import integer_cloud, nearly_collinear_cloud, sign_diff


# ---------------------------------------------------------------- numpy restatement of the definition
def _rounded_sign_diff(a, b, c, d):
    """What the exact predicate is NOT: the sign of fl(fl(a b) - fl(c d))."""
    return np.sign(np.asarray(a) * np.asarray(b) - np.asarray(c) * np.asarray(d)).astype(np.int8)


def _count_one(V, sign=sign_diff):
    """V: the vectors from the target to its others, in sample order.  C(m, 3) - sum_j C(e_j, 2)."""
    m = len(V)
    nz = (V != 0.0).any(axis=1)
    x, y = V[nz, 0], V[nz, 1]
    missing = 0
    step = max(1, (1 << 20) // max(1, len(x)))                         # rows of the pair matrix at a time
    for j0 in range(0, len(x), step):
        xj, yj = x[j0:j0 + step], y[j0:j0 + step]
        C = sign(xj[:, None], y[None, :], yj[:, None], x[None, :])     # cross(v_j, v_k)
        e = (C > 0).sum(axis=1).astype(np.int64)
        j, k = np.nonzero(C == 0)
        later = k > j + j0                                             # same direction counts for the later ones only
        j, k = j[later], k[later]
        D = sign(xj[j], x[k], -yj[j], y[k])                            # dot(v_j, v_k)
        e += np.bincount(j[D > 0], minlength=len(xj))
        missing += int((e * (e - 1) // 2).sum())
    return comb(m, 3) - missing


def simplicial_counts(P, targets=None, sign=sign_diff):
    """Triples of the OTHER rows whose closed hull contains P[t]: the definition as it stands."""
    P = np.asarray(P, dtype=np.float64)
    targets = range(len(P)) if targets is None else targets
    return np.array([_count_one(np.delete(P, t, axis=0) - P[t], sign) for t in targets], dtype=np.int64)


def simplicial_external(P, Q, sign=sign_diff):
    """Triples of ALL rows of P whose closed hull contains the external point g."""
    P = np.asarray(P, dtype=np.float64)
    return np.array([_count_one(P - g, sign) for g in np.asarray(Q, dtype=np.float64)], dtype=np.int64)


def simplicial_sampled(P, targets, K):
    """The K-block estimator replaying _samplepointwisedepth's draws from the global numpy RNG (as
    test_halfspace_exact_host.exact_sampled does), counts / C(block size, 3) inside each block."""
    P = np.asarray(P, dtype=np.float64)
    n = len(P)
    ss = n // K
    rows = pd.Series(np.arange(n))
    out = []
    for tp in targets:
        vals = []
        for _ in range(ss):
            drawn = rows.sample(n=ss).to_numpy()
            blk = np.append(drawn[drawn != tp], tp)
            vals.append(simplicial_counts(P[blk], [len(blk) - 1])[0] / comb(len(blk), 3))
        out.append(np.mean(vals))
    return np.array(out)


def _sgn(v):
    return (v > 0) - (v < 0)


def _brute_one(V):
    """Every triple of the vectors V in rational arithmetic: does its closed hull contain the origin?"""
    F = [(Fraction(float(a)), Fraction(float(b))) for a, b in V]
    cross = lambda a, b: a[0] * b[1] - a[1] * b[0]                     # noqa: E731
    dot = lambda a, b: a[0] * b[0] + a[1] * b[1]                       # noqa: E731
    total = 0
    for a, b, c in itertools.combinations(F, 3):
        if any(v == (0, 0) for v in (a, b, c)):
            total += 1
            continue
        pairs = ((a, b), (b, c), (c, a))
        s = [_sgn(cross(u, v)) for u, v in pairs]
        disagree = (1 in s) and (-1 in s)
        if 0 not in s and not disagree:
            total += 1
        elif not disagree and any(si == 0 and dot(u, v) < 0 for si, (u, v) in zip(s, pairs)):
            total += 1
    return total


def simplicial_brute(P, targets=None):
    P = np.asarray(P, dtype=np.float64)
    targets = range(len(P)) if targets is None else targets
    return np.array([_brute_one(np.delete(P, t, axis=0) - P[t]) for t in targets], dtype=np.int64)


LINE = np.array([[i, 2.0 * i] for i in range(7)], dtype=np.float64)
SQUARE = np.array([[1, 1], [1, -1], [-1, 1], [-1, -1], [0, 0]], dtype=np.float64)
EQUAL = np.full((5, 2), 0.25)
SQUARE_EXTERNAL = np.array([[0.0, 0.0], [1.0, 1.0], [5.0, 5.0], [0.5, 0.0]])


# ---------------------------------------------------------------- hand cases
def test_hand_cases():
    for fn in (simplicial_counts, simplicial_brute):
        assert fn(LINE).tolist() == [0, 10, 16, 18, 16, 10, 0]
        assert fn(SQUARE).tolist() == [0, 0, 0, 0, 4]
        assert fn(EQUAL).tolist() == [4] * 5
    assert simplicial_external(SQUARE, SQUARE_EXTERNAL).tolist() == [10, 6, 0, 3]
    assert [_brute_one(SQUARE - g) for g in SQUARE_EXTERNAL] == [10, 6, 0, 3]
    for n in (1, 2, 3):
        assert simplicial_counts(np.random.default_rng(n).normal(size=(n, 2))).tolist() == [0] * n


# ---------------------------------------------------------------- against brute force in rational arithmetic
@pytest.mark.parametrize("seed", range(6))
def test_restatement_equals_brute_force_on_integer_clouds(seed):
    P = integer_cloud(14, seed)
    assert np.array_equal(simplicial_counts(P), simplicial_brute(P))
    Q = np.random.default_rng(100 + seed).integers(-3, 4, size=(5, 2)).astype(np.float64)
    assert np.array_equal(simplicial_external(P, Q), [_brute_one(P - g) for g in Q])


def test_restatement_equals_brute_force_on_a_normal_cloud():
    P = np.random.default_rng(3).normal(size=(20, 2))
    assert np.array_equal(simplicial_counts(P), simplicial_brute(P))


def test_restatement_equals_brute_force_on_the_nearly_collinear_cloud():
    P = nearly_collinear_cloud()[:16]
    assert np.array_equal(simplicial_counts(P), simplicial_brute(P))


# ---------------------------------------------------------------- the reference's own counts
@pytest.mark.parametrize("name", ["g5_pc_n30_d2", "g5_pc_n12_d2", "g5_pc_grid_d2"])
def test_golden_counts(name):
    fx = load_golden(name)
    df = frame_df(fx["input"])
    P = df.to_numpy(dtype=np.float64)
    assert P.shape[1] == 2 and fx["normaliser"] == comb(len(P), 3)
    pos = df.index.get_indexer(fx["index"])
    assert np.array_equal(simplicial_counts(P, pos), np.array(fx["counts"], dtype=np.int64))


# ---------------------------------------------------------------- the predicate
def test_rounded_predicate_is_not_a_substitute():
    """Counting with the signs of the rounded cross and dot products changes the counts on the nearly collinear cloud: the
    GPU test on this cloud cannot pass with a rounded predicate."""
    P = nearly_collinear_cloud()
    exact = simplicial_counts(P)
    rounded = simplicial_counts(P, sign=_rounded_sign_diff)
    assert (exact != rounded).sum() > 0


# ---------------------------------------------------------------- invariances
def test_invariances_exact_in_fp64():
    rng = np.random.default_rng(7)
    for P in (rng.normal(size=(40, 2)), nearly_collinear_cloud(), integer_cloud(30, 5)):
        want = simplicial_counts(P)
        perm = rng.permutation(len(P))
        assert np.array_equal(simplicial_counts(P[perm]), want[perm])  # the tie order inside a direction does not matter
        assert np.array_equal(simplicial_counts(P[:, ::-1]), want)     # the mirror (x, y) -> (y, x)
        for s in (2.0 ** -40, 2.0 ** 13, -4.0):
            assert np.array_equal(simplicial_counts(P * s), want)


# ---------------------------------------------------------------- host validation (no device needed)
def test_validation_errors_before_device_work():
    from statdepth_amd import PointcloudDepth
    from statdepth_amd.homogeneity import PointcloudHomogeneity
    rng = np.random.default_rng(2)
    good = pd.DataFrame(rng.normal(size=(10, 2)))
    for kw in ({}, {"K": 2}):
        for d in (1, 3):
            with pytest.raises(NotImplementedError, match="containment='simplex'"):
                PointcloudDepth(pd.DataFrame(rng.normal(size=(10, d))), containment='simplex_exact', **kw)
        for bad_value in (np.nan, np.inf, -np.inf):
            bad = good.copy()
            bad.iloc[3, 1] = bad_value
            with pytest.raises(ValueError, match='NaN or infinite'):
                PointcloudDepth(bad, containment='simplex_exact', **kw)
        big = good.copy()
        big.iloc[0, 0] = -2.0 ** 501
        with pytest.raises(ValueError, match=r'2\^500'):
            PointcloudDepth(big, containment='simplex_exact', **kw)
        with pytest.raises(KeyError, match='not in index'):
            PointcloudDepth(good, to_compute=[3, 77], containment='simplex_exact', **kw)
    with pytest.raises(NotImplementedError, match="containment='simplex'"):
        PointcloudHomogeneity(pd.DataFrame(rng.normal(size=(10, 3))), pd.DataFrame(rng.normal(size=(10, 3))),
                              containment='simplex_exact')


def test_engine_argument_checks_need_no_device_call():
    from statdepth_amd import engine
    P = np.zeros((4, 2))
    for call in (lambda: engine.simplicial_exact_counts(P, algo="rank"),
                 lambda: engine.simplicial_exact_external_counts(P, P, algo="enumerate"),
                 lambda: engine.simplicial_exact_subset_counts(P, [[0, 1]], algo=1)):
        with pytest.raises(ValueError, match="'auto', 'sweep' or 'pairwise'"):
            call()


# ---------------------------------------------------------------- C ABI, no device needed
def _lib():
    from statdepth_amd import _native
    return _native, _native.load()


def _most_others():
    """The most others whose C(others, 3) fits int64."""
    lo, hi = 3, 1 << 31
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if comb(mid, 3) <= 2 ** 63 - 1 else (lo, mid)
    return lo


def test_abi_refusals_before_device_work():
    _native, lib = _lib()
    fake = ctypes.c_void_p(256)                  # never dereferenced: every refusal happens before device work
    out = ctypes.c_void_p(512)
    INV, UNS = _native.SD_ERR_INVALID, _native.SD_ERR_UNSUPPORTED
    counts, external, subsets = lib.sd_simplicial2_counts, lib.sd_simplicial2_external_counts, lib.sd_simplicial2_subset_counts
    for algo in (0, 1, 2):
        assert counts(None, 10, None, 10, algo, out, None) == INV
        assert counts(fake, 10, None, 10, algo, None, None) == INV
        assert counts(fake, 0, None, 0, algo, out, None) == INV
        assert counts(fake, 10, None, 9, algo, out, None) == INV                  # NULL targets, m != n
        assert external(None, 10, fake, 3, algo, out, None) == INV
        assert external(fake, 10, None, 3, algo, out, None) == INV
        assert external(fake, 10, fake, 3, algo, None, None) == INV
        assert external(fake, 0, fake, 3, algo, out, None) == INV
        assert subsets(None, 10, fake, 3, 4, algo, out, None) == INV
        assert subsets(fake, 10, None, 3, 4, algo, out, None) == INV
        assert subsets(fake, 10, fake, 3, 4, algo, None, None) == INV
        assert subsets(fake, 10, fake, 3, 0, algo, out, None) == INV
        assert subsets(fake, 0, fake, 3, 4, algo, out, None) == INV
        assert counts(fake, 2**31, fake, 1, algo, out, None) == UNS               # 2^31 points
        assert b"2^31" in lib.sd_last_error()
        assert external(fake, 2**31, fake, 1, algo, out, None) == UNS
        assert subsets(fake, 2**31, fake, 1, 4, algo, out, None) == UNS
    assert counts(fake, 10, None, 10, 3, out, None) == INV                        # unknown algo
    assert counts(fake, 10, None, 10, -1, out, None) == INV
    # the sweep asked for by name above its capacity of 8192 OTHERS: n - 1, n, bs - 1 of them
    assert counts(fake, 8194, fake, 1, 1, out, None) == UNS
    assert b"8192" in lib.sd_last_error()
    assert external(fake, 8193, fake, 1, 1, out, None) == UNS
    assert subsets(fake, 10**5, fake, 1, 8194, 1, out, None) == UNS
    # beyond 1e14 predicate evaluations on the route that would run: pairwise m others^2, sweep per target by capacity tier
    assert counts(fake, 10**5, None, 10**5, 0, out, None) == UNS                  # auto above the capacity: pairwise
    assert b"cap" in lib.sd_last_error()
    assert counts(fake, 10**5, None, 10**5, 2, out, None) == UNS
    assert external(fake, 10**6, fake, 10**3, 0, out, None) == UNS
    assert subsets(fake, 10**6, fake, 10**7, 10**4, 0, out, None) == UNS
    assert subsets(fake, 10**6, fake, 2**30, 8192, 1, out, None) == UNS           # 2^30 blocks x 372 736 comparators
    assert external(fake, 8192, fake, 2**30, 0, out, None) == UNS
    # C(others, 3) beyond int64: one target keeps the pairwise work (1.5e13) under the cap, so this is what refuses
    most = _most_others()
    assert 3_800_000 < most < 3_900_000 and comb(most, 3) < 2 ** 63 <= comb(most + 1, 3)
    for algo in (0, 2):
        assert counts(fake, most + 2, fake, 1, algo, out, None) == UNS            # most + 1 others
        assert b"int64" in lib.sd_last_error() and str(most).encode() in lib.sd_last_error()
        assert external(fake, most + 1, fake, 1, algo, out, None) == UNS
        assert b"int64" in lib.sd_last_error()
        assert subsets(fake, 10**7, fake, 1, most + 2, algo, out, None) == UNS
        assert b"int64" in lib.sd_last_error()


def test_no_device_is_an_error_not_a_fallback():
    from statdepth_amd import PointcloudDepth, engine
    from statdepth_amd.homogeneity import PointcloudHomogeneity
    _native, lib = _lib()
    if lib.sd_device_count() > 0:
        pytest.skip("a HIP device is visible: tests/test_simplicial_exact_gpu.py covers this machine")
    rng = np.random.default_rng(1)
    P = rng.normal(size=(12, 2))
    df = pd.DataFrame(P)
    with pytest.raises(RuntimeError, match='no HIP device'):
        PointcloudDepth(df, containment='simplex_exact')
    with pytest.raises(RuntimeError, match='no HIP device'):
        PointcloudDepth(df, containment='simplex_exact', K=2)
    with pytest.raises(RuntimeError, match='no HIP device'):
        PointcloudHomogeneity(df, pd.DataFrame(rng.normal(size=(12, 2))), containment='simplex_exact')
    for call in (lambda: engine.simplicial_exact_counts(P), lambda: engine.simplicial_exact_external_counts(P, P[:2]),
                 lambda: engine.simplicial_exact_subset_counts(P, [[0, 1, 2]])):
        with pytest.raises(RuntimeError, match='no HIP device'):
            call()
