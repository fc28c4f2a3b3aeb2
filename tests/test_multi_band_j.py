"""Componentwise band depth of multivariate curves ('r2_enum', relax=True) for J = 3 and 4: sd_multi_band_j_counts
(j-subsets counted by inclusion-exclusion over the 3^d state classes) against the oracle's literal enumeration, the
pair kernel, the univariate kernels and closed forms, then through FunctionalDepth / FunctionalHomogeneity.
Counts are integers: every comparison of counts is exact."""
import functools
import math
import os
import re

import numpy as np
import pandas as pd
import pytest

from conftest import ROOT, assert_depths_close

gpu = pytest.mark.gpu
TOL = 1e-12
N, T = 23, 7
DIMS = [1, 2, 3, 5, 8]


@pytest.fixture(scope="module")
def eng():
    from statdepth_amd import engine
    return engine


@functools.lru_cache(maxsize=None)
def _case(d):
    """(P, want): the n = 23 recipe of test_componentwise_band_vs_literal_enumeration and the oracle's int64[n, 3] for
    J = 4, computed once per d and shared; no test writes to either."""
    import oracle
    oracle.build()
    rng = np.random.default_rng(300 + d)
    P = np.round(rng.normal(size=(N, T, d)).cumsum(axis=1), 1)          # rounded: ties in single components
    P[3] = P[4]                                                          # a duplicated curve
    P[5, :, 0] = P[6, :, 0]                                              # a shared component
    want = oracle.multi_band_enum(P, None, 4, True)
    want.setflags(write=False)                                           # (P stays writable: torch wraps it for the upload)
    return P, want


def _univariate_want(X, tg, J):
    """Exact Python-int totals of the univariate formula: sum_t C(n-1, j) - C(A, j) - C(B, j).  X: T x n."""
    n = X.shape[1]
    out = []
    for q in tg:
        A = (X > X[:, q:q + 1]).sum(axis=1)
        B = (X < X[:, q:q + 1]).sum(axis=1)
        out.append([sum(math.comb(n - 1, j) - math.comb(int(a), j) - math.comb(int(b), j) for a, b in zip(A, B))
                    for j in range(2, J + 1)])
    return out


# ---------------------------------------------------------------- CPU: the ABI is declared and bound
def test_header_and_signatures_carry_the_entry_point():
    from statdepth_amd import _native
    src = open(os.path.join(ROOT, "include", "statdepth_hip.h")).read()
    decl = re.search(r"\bint\s+sd_multi_band_j_counts\s*\(([^;]*)\)\s*;", src)
    assert decl, "sd_multi_band_j_counts is not declared in statdepth_hip.h"
    assert len(re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")) == 11
    res, args = _native.SIGNATURES["sd_multi_band_j_counts"]
    assert len(args) == 11 and res is _native._int
    # that the library exports every name of SIGNATURES is test_host_logic's check; the library is not opened here, so
    # that the GPU tests below still import torch before it


# ---------------------------------------------------------------- counts
@gpu
@pytest.mark.parametrize("d", DIMS)
def test_literal_enumeration(eng, d):
    """All three columns of J = 4 against the literal subset enumeration (ties, a duplicated curve, a shared component);
    odd d takes the lone last transform pass, d = 8 the full LDS layout; odd m takes the one-target tail of a sweep."""
    P, want = _case(d)
    assert (want.sum(axis=0) > 0).all(), want.sum(axis=0)
    got = eng.multi_band_j_counts(P, J=4)
    assert got.shape == (N, 3) and got.dtype == np.int64
    assert (got == want).all()
    for tg in ([22, 0, 4], [7]):
        assert (eng.multi_band_j_counts(P, np.array(tg), J=4) == want[tg]).all()
    # fewer columns are the same columns
    assert (eng.multi_band_j_counts(P, J=3) == want[:, :2]).all()
    assert (eng.multi_band_j_counts(P, J=2) == want[:, :1]).all()


@gpu
@pytest.mark.parametrize("d", DIMS)
def test_pair_column_equals_pair_kernel(eng, d):
    P, want = _case(d)
    assert (eng.multi_band_j_counts(P, J=4)[:, 0] == eng.multi_band_counts(P)).all()


@gpu
@pytest.mark.parametrize("n", [3, 2])
def test_too_few_curves(eng, oracle, n):
    rng = np.random.default_rng(41 + n)
    P = np.round(rng.normal(size=(n, 5, 3)), 0)
    P[0, :3] = P[1, :3]                                                  # ties, so that a pair can contain at n = 3
    want = oracle.multi_band_enum(P, None, 4, True)
    got = eng.multi_band_j_counts(P, J=4)
    for j in (2, 3, 4):
        if math.comb(n - 1, j) == 0:
            assert (got[:, j - 2] == 0).all()
    assert (got == want).all()
    if n == 3:
        assert want[:, 0].sum() > 0


@gpu
def test_all_ties(eng):
    """Every curve ties with the target everywhere: only the all-don't-care pattern counts, 3 timepoints x C(39, j)."""
    got = eng.multi_band_j_counts(np.zeros((40, 3, 4)), J=4)
    for j in (2, 3, 4):
        assert (got[:, j - 2] == 3 * math.comb(39, j)).all()


@gpu
def test_more_curves_than_threads(eng):
    """n = 1 100 > the 1 024 threads of a block.  A second feature that is an increasing or a decreasing image of the
    first constrains nothing new (above and below keep or swap their roles): the univariate totals, J = 4."""
    rng = np.random.default_rng(5)
    n, Tn = 1100, 3
    X = np.round(rng.normal(size=(n, Tn)).cumsum(axis=1), 1)             # n x T, ties
    want = eng.mbd_counts(np.ascontiguousarray(X.T), None, 4)
    assert want.shape == (n, 3) and (want.sum(axis=0) > 0).all()
    assert want[:5].tolist() == _univariate_want(X.T, range(5), 4)
    for second in (2.0 * X + 1.0, -X):
        P = np.stack([X, second], axis=2)
        assert (eng.multi_band_j_counts(P, J=4) == want).all()


@gpu
def test_large_n_image_route(eng):
    """n = 16 500 > 16 384: the ranks come from sd_above_below instead of the bucket kernel's image mode."""
    rng = np.random.default_rng(6)
    n = 16500
    x = np.round(rng.normal(size=n) * 50.0, 0)                           # ties
    P = np.stack([x, 0.5 * x - 3.0], axis=1)[:, None, :]                 # (n, 1, 2)
    tg = np.array([0, 1, 8000, 16383, n - 1])
    want = eng.mbd_counts(x[None, :], tg, 3)
    assert want.tolist() == _univariate_want(x[None, :], tg, 3)
    assert (eng.multi_band_j_counts(P, tg, J=3) == want).all()


@gpu
@pytest.mark.parametrize("d,n", [(8, 6911), (2, 40750)])
def test_largest_admitted_n(eng, d, n):
    """The largest n the LDS bound of sd_multi_band_counts admits (n*d*2 + 8*3^d + 768 <= 163 840 bytes) is served at
    J = 4 as well, and n + 1 is refused by both entries.  Every feature is an increasing or decreasing image of the
    first (exact: integers times powers of two), so the result is the univariate one."""
    from statdepth_amd._native import SD_ERR_UNSUPPORTED, StatdepthHipError
    assert n * d * 2 + 8 * 3 ** d + 768 <= 163840 < (n + 1) * d * 2 + 8 * 3 ** d + 768
    rng = np.random.default_rng(11 + d)
    Tn = 2
    X = rng.integers(-2000, 2001, size=(n + 1, Tn)).astype(np.float64)   # ties
    scale = np.array([(-1.0) ** f * 2.0 ** (f - 3) for f in range(d)])
    scale[0] = 1.0
    P = X[:, :, None] * scale + np.arange(d)
    tg = np.array([0, 1, n // 2, n - 2, n - 1])
    want = eng.mbd_counts(np.ascontiguousarray(X[:n].T), tg, 4)
    assert want.tolist() == _univariate_want(X[:n].T, tg, 4)
    assert (eng.multi_band_j_counts(P[:n], tg, J=4) == want).all()
    assert (eng.multi_band_counts(P[:n], tg) == want[:, 0]).all()
    for call in (lambda: eng.multi_band_j_counts(P, tg, J=4), lambda: eng.multi_band_counts(P, tg)):
        with pytest.raises(StatdepthHipError) as e:
            call()
        assert e.value.code == SD_ERR_UNSUPPORTED


# ---------------------------------------------------------------- refusals and the int64 limit
@gpu
def test_refusals(eng):
    from statdepth_amd._native import SD_ERR_OVERFLOW, SD_ERR_UNSUPPORTED, StatdepthHipError
    P, _ = _case(2)
    Pn = P.copy()
    Pn[1, 2, 0] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        eng.multi_band_j_counts(Pn, J=3)
    with pytest.raises(StatdepthHipError) as e:
        eng.multi_band_j_counts(P, J=5)
    assert e.value.code == SD_ERR_UNSUPPORTED
    # T * C(n-1, 4) >= 2^63 is refused before anything is launched.  n = 60 000 needs T = 18 for that: at T = 16 the
    # bound is 8.64e18 < 2^63 = 9.22e18 and the call is computable (test_totals_just_below_int64).
    n, Tn = 60000, 18
    assert Tn * math.comb(n - 1, 4) >= 2 ** 63 > (Tn - 1) * math.comb(n - 1, 4)
    with pytest.raises(StatdepthHipError) as e:
        eng.multi_band_j_counts(np.zeros((n, Tn, 1)), np.array([0]), J=4)
    assert e.value.code == SD_ERR_OVERFLOW


@gpu
def test_totals_just_below_int64(eng):
    """n = 60 000, T = 16, d = 1, J = 4: T * C(n-1, 4) = 8 638 560 083 998 000 016 < 2^63, so the call is served
    (a curve tied with all others everywhere would reach exactly that total); the alternating sums inside the kernel wrap
    on the way.  Values in {-1, 0, 1} with four all-tied timepoints, expected totals from exact integer arithmetic."""
    rng = np.random.default_rng(8)
    n, Tn = 60000, 16
    assert Tn * math.comb(n - 1, 4) < 2 ** 63
    X = rng.integers(-1, 2, size=(n, Tn)).astype(np.float64)
    X[:, :4] = 0.0                                                       # four timepoints where everything ties
    X[7] = 0.0
    tg = np.array([7, 0, n - 1])
    want = _univariate_want(X.T, tg, 4)
    assert max(max(r) for r in want) > 2 ** 61
    assert eng.multi_band_j_counts(X[:, :, None], tg, J=4).tolist() == want


# ---------------------------------------------------------------- public API
@gpu
@pytest.mark.parametrize("J", [3, 4])
@pytest.mark.parametrize("d", DIMS)
def test_functional_depth(d, J):
    from statdepth_amd import FunctionalDepth
    P, want = _case(d)
    frames = [pd.DataFrame(P[i]) for i in range(N)]
    wd = sum(want[:, j - 2] / T / math.comb(N, j) for j in range(2, J + 1))
    got = FunctionalDepth(frames, J=J, containment="r2_enum", relax=True)
    assert_depths_close(got.to_numpy(), wd, TOL)
    some = FunctionalDepth(frames, J=J, containment="r2_enum", relax=True, to_compute=[0, 3, 10])
    assert_depths_close(some.to_numpy(), wd[[0, 3, 10]], TOL)


@gpu
def test_functional_depth_one_feature_is_univariate_and_j5_is_refused():
    from statdepth_amd import FunctionalDepth
    P, _ = _case(1)
    frames = [pd.DataFrame(P[i]) for i in range(N)]
    multi = FunctionalDepth(frames, J=4, containment="r2_enum", relax=True)
    uni = FunctionalDepth([pd.DataFrame(P[:, :, 0].T)], J=4, relax=True)
    assert_depths_close(multi.to_numpy(), uni.to_numpy(), TOL)
    with pytest.raises(NotImplementedError, match="J <= 4"):
        FunctionalDepth(frames, J=5, containment="r2_enum", relax=True)


@gpu
def test_functional_homogeneity_reaches_it(oracle):
    """FunctionalHomogeneity on multivariate samples goes through FunctionalDepth: P1 = depth of G's first curve inside
    F u {it}, over the depth of G's median (its deepest curve).  The samples have 8 curves each: the coefficient refuses samples of different
    sizes (as the reference does), whatever the containment."""
    from statdepth_amd import FunctionalDepth
    from statdepth_amd.homogeneity import FunctionalHomogeneity
    rng = np.random.default_rng(9)
    Tn, d = 6, 2
    PF = np.round(rng.normal(size=(8, Tn, d)).cumsum(axis=1), 1)
    PG = np.round(rng.normal(size=(8, Tn, d)).cumsum(axis=1) * 0.8 + 0.1, 1)
    F = [pd.DataFrame(PF[i]) for i in range(8)]
    G = [pd.DataFrame(PG[i]) for i in range(8)]
    kw = dict(J=3, containment="r2_enum", relax=True)
    got = float(FunctionalHomogeneity(F, G, method="p1", **kw).homogeneity())
    assert np.isfinite(got)
    g_depths = FunctionalDepth(G, **kw)
    inside = FunctionalDepth(F + [G[0]], to_compute=[8], **kw)
    assert got == float(inside.iloc[0] / g_depths.median().iloc[0])
    # and from the literal enumeration
    wg = oracle.multi_band_enum(PG, None, 3, True)
    wf = oracle.multi_band_enum(np.concatenate([PF, PG[:1]]), [8], 3, True)
    dg = sum(wg[:, j - 2] / Tn / math.comb(8, j) for j in (2, 3))
    df = sum(wf[:, j - 2] / Tn / math.comb(9, j) for j in (2, 3))
    assert dg.max() > 0
    assert abs(got - df[0] / dg.max()) <= TOL * max(1.0, abs(got))
    with pytest.raises(ValueError, match="same length"):
        FunctionalHomogeneity(F, G[:6], method="p1", **kw)
