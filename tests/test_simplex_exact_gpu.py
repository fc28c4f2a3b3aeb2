"""Simplex containment counts on the GPU (K4, K4s: sd_pointcloud_simplex_*, sd_multi_simplex_*) against the exact rational
reference of tests/test_simplex_exact_host.py.  Every comparison is equality of integer counts; every case is exhaustive (or,
for the sampled estimators, exact on the very subsets drawn) at the smallest shape that reaches its code path; the reference
holds every (target, subset) it decides against the guards, so no input sits in the band where the kernels' tolerances and
an exact decision may differ; and every case has a target with a non-zero expected count.
(a) every instantiation, (b) scale and shift, (c) the three forms, (d) the work split, (e) curves, (f) the sampled estimators,
(g) the package."""
import math

import numpy as np
import pandas as pd
import pytest

from test_simplex_exact_host import (D_ALL, D_SHIFT, FAMILIES, SAMPLED_SEED, SAMPLED_VARIANTS, UTM_CENTRE, VARIANTS, Guard, cloud,
                                     cloud_counts, counts_exact, counts_int, counts_int_rows, curves_case, curves_counts,
                                     curves_targets, forms_case, int_cloud, sampled_case, sampled_counts, sampled_exact,
                                     utm_cloud)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from statdepth_amd import engine
    return engine


# ---------------------------------------------------------------- (a) every instantiation
@pytest.mark.parametrize("d", D_ALL)
@pytest.mark.parametrize("family", FAMILIES)
def test_every_instantiation(eng, xcheck, family, d):
    """simplex_kernel_fast<d> (product route) and simplex_kernel (SD_SIMPLEX_GENERIC) for d = 1 .. 8, rows form, every row a
    target.  n = 11, 10 or d + 4 (two rows more with the NaN and the infinite row): the smallest clouds that still give every
    target several subsets, at most C(d + 3, 2) of them at high d.  The lattice, flat and mixed families put targets on faces,
    edges and vertices and make rank-deficient simplices, which leave hull_full_rank<d> for point_in_hull."""
    P = cloud(family, d)
    want, g = cloud_counts(family, d)
    print(family, d, g)
    assert want.any()
    assert np.array_equal(eng.pointcloud_simplex_counts(P), want)
    with xcheck(SD_SIMPLEX_GENERIC="1"):
        assert np.array_equal(eng.pointcloud_simplex_counts(P), want)


# ---------------------------------------------------------------- (b) scale and shift
@pytest.mark.parametrize("d", D_SHIFT)
@pytest.mark.parametrize("family", ("dyadic", "lattice"))
def test_scale_and_shift(eng, xcheck, family, d):
    """The clouds of (a) multiplied by 2^-480, 2^-40, 2^40, 2^480, translated by 2^24 and 2^40, translated and then scaled; every map
    is exact on these inputs (asserted), so the counts are the exact counts of the original, and the kernel's bits on the
    original.  Same kernels and shapes as (a).  These variants FAIL on the parent commit: scale = max(1, max |entry|) of the
    raw data made the rank and consistency thresholds absolute below |P| = 1 and swamped them above (lattice, d = 2, scaled by
    2^-40: every subset counted for every target)."""
    P = cloud(family, d)
    want, _ = cloud_counts(family, d)
    base = eng.pointcloud_simplex_counts(P)
    assert want.any() and np.array_equal(base, want)
    for name, f in VARIANTS.items():
        Y = f(P)
        got = eng.pointcloud_simplex_counts(Y)
        assert np.array_equal(got, want) and np.array_equal(got, base), name
        with xcheck(SD_SIMPLEX_GENERIC="1"):
            assert np.array_equal(eng.pointcloud_simplex_counts(Y), want), name


def test_utm_like_cloud(eng, xcheck):
    """Integer metres around (5 10^5, 5 10^6), spread 10^3, n = 11, d = 2 (simplex_kernel_fast<2>, 120 subsets per target):
    the counts of the centred cloud (the centring is exact), which are the exact ones.  Fails on the parent commit."""
    P = utm_cloud()
    Z = P - UTM_CENTRE
    want = counts_exact(Z)
    assert want.any()
    base = eng.pointcloud_simplex_counts(Z)
    assert np.array_equal(base, want)
    assert np.array_equal(eng.pointcloud_simplex_counts(P), base)
    with xcheck(SD_SIMPLEX_GENERIC="1"):
        assert np.array_equal(eng.pointcloud_simplex_counts(P), want)


# ---------------------------------------------------------------- (c) the three forms and the target skip
@pytest.mark.parametrize("d", (1, 2, 3, 8))
def test_three_forms(eng, xcheck, d):
    """Rows form with the first, a middle (d + 1 of n >= d + 5) and the last row as targets (sx_src skips the target's own row before every other,
    in the middle, after every other).  External form: a vertex, an edge midpoint, a centroid, a point 2^-6 outside a face, a
    point 2^30 extents away (its scale makes every pivot fall below rank_eps: outside by every path).  Blocks of d + 1 members (no
    subset), d + 2 (one subset) and d + 5 in one call, each also alone.  n = max(n_of(d), d + 5): the smallest with such blocks."""
    P, Q, mem, ext, blk = forms_case(d)
    n = len(P)
    tg = [0, d + 1, n - 1]                                                 # row d + 1 is the centroid of rows 0 .. d
    want = counts_exact(P, tg)
    assert want.any() and ext[:3].all() and ext[4] == 0 and blk.tolist()[:2] == [0, 1] and blk[2] >= 1
    for generic in (False, True):
        with xcheck(SD_SIMPLEX_GENERIC="1" if generic else "0"):
            assert np.array_equal(eng.pointcloud_simplex_counts(P, tg), want)
            assert np.array_equal(eng.pointcloud_simplex_external_counts(P, Q), ext)
            assert np.array_equal(eng.pointcloud_simplex_subset_counts(P, mem), blk)
    assert np.array_equal(eng.pointcloud_simplex_counts(P, tg), want)           # the product library
    assert np.array_equal(eng.pointcloud_simplex_external_counts(P, Q), ext)
    assert np.array_equal(eng.pointcloud_simplex_subset_counts(P, mem), blk)
    for b in range(3):
        assert np.array_equal(eng.pointcloud_simplex_subset_counts(P, mem[b:b + 1]), blk[b:b + 1]), b


# ---------------------------------------------------------------- (d) the work split of launch_simplex_common
def _both_kernels(eng, xcheck, call, want):
    assert want.any()
    assert np.array_equal(call(), want)
    with xcheck(SD_SIMPLEX_GENERIC="1"):
        assert np.array_equal(call(), want)


def test_split_one_target_many_subsets(eng, xcheck):
    """n = 120, d = 2, one target: C(119, 3) = 273 819 > 2^18 subsets, so per_thread = 2: every thread but the first unranks a
    non-zero start and steps with next_comb, and the last thread's range is partial (273 819 is odd).  n = 119 is the smallest
    with per_thread > 1; 120 has some margin to it."""
    assert math.comb(117, 3) <= 2 ** 18 < math.comb(118, 3) < math.comb(119, 3) <= 2 ** 19
    P = int_cloud(120, 2, 120)
    P[7] = np.rint(P.mean(axis=0))
    want = counts_int_rows(P, [7])
    _both_kernels(eng, xcheck, lambda: eng.pointcloud_simplex_counts(P, [7]), want)


@pytest.mark.parametrize("d,n", ((2, 24), (3, 14)))
def test_split_many_targets(eng, xcheck, d, n):
    """External form, m = 2 048 targets: 2^18 / m = 128 < 256 wanted threads per target, and C(24, 3) = 2 024 (d = 3, n = 14:
    C(14, 4) = 1 001) subsets over them is per_thread = 8 (4) with a partial last thread."""
    F = int_cloud(n, d, 10 * n + d)
    Q = int_cloud(2048, d, 11 * n + d, lim=700)
    want = counts_int(F, Q)
    _both_kernels(eng, xcheck, lambda: eng.pointcloud_simplex_external_counts(F, Q), want)


def test_split_grid_y_fold(eng, xcheck):
    """External form, n = 6, d = 2, m = 65 539 targets: grid.y folds at 65 535 into a second launch of 4 rows (q0 = 65 535).
    Targets 65 534 .. 65 538, on either side of the fold, are checked one by one as well."""
    F = int_cloud(6, 2, 66)
    Q = int_cloud(65539, 2, 67, lim=700)
    Q[65534:] = np.rint(F.mean(axis=0)) + np.arange(5)[:, None]
    want = counts_int(F, Q)
    assert want[65534:].all()
    _both_kernels(eng, xcheck, lambda: eng.pointcloud_simplex_external_counts(F, Q), want)
    got = eng.pointcloud_simplex_external_counts(F, Q)
    for q in range(65534, 65539):
        assert got[q] == want[q] == eng.pointcloud_simplex_external_counts(F, Q[q:q + 1])[0], q


# ---------------------------------------------------------------- (e) curves
@pytest.mark.parametrize("d", (1, 2, 3, 8))
def test_curves(eng, xcheck, d):
    """multi_simplex_counts, T = 3, n = d + 5 (a duplicated curve, a tight core: strict containment occurs), relax and strict, on
    simplex_kernel_fast<d> and simplex_kernel.  In `moved`, timepoint 1 is translated by 2^24 and timepoint 2 scaled by 2^-40: the
    system of each timepoint is normalised on its own, so the counts are the same.  (moved fails on the parent commit.)"""
    C, M = curves_case(d)
    tg = curves_targets(d)
    for relax, want in zip((True, False), curves_counts(d)):
        assert want.any()
        for X in (C, M):
            assert np.array_equal(eng.multi_simplex_counts(X, tg, relax=relax), want), relax
            with xcheck(SD_SIMPLEX_GENERIC="1"):
                assert np.array_equal(eng.multi_simplex_counts(X, tg, relax=relax), want), relax


# ---------------------------------------------------------------- (f) the sampled estimators
@pytest.mark.parametrize("d", (1, 3, 8))
def test_sampled_point_cloud(eng, xcheck, d):
    """n = 40, 64 samples: the workspace route (sxw_factor / sxw_apply replay, sxw_spare for the targets that are members of
    shared subsets, sxw_special for the far row, whose own scale puts every pivot below rank_eps) and the per-target route
    (SD_SIMPLEX_PERTARGET: simplex_kernel_fast<d> on the same subsets), against exact membership on the subsets drawn; then
    the same call on the cloud scaled by 2^-480, and translated by 2^40 and scaled by 2^40."""
    P = sampled_case(d)
    tg, want, g = sampled_counts(d)
    seed = SAMPLED_SEED[d]
    print(d, tg, want.tolist(), g)
    assert want.any() and want[-1] == 0
    for X in [P] + [f(P) for f in SAMPLED_VARIANTS.values()]:
        assert np.array_equal(eng.pointcloud_simplex_counts(X, tg, samples=64, seed=seed), want)
        with xcheck(SD_SIMPLEX_PERTARGET="1"):
            assert np.array_equal(eng.pointcloud_simplex_counts(X, tg, samples=64, seed=seed), want)


@pytest.mark.parametrize("d", (1, 3, 8))
def test_sampled_curves(eng, xcheck, d):
    """T = 3: relax=True takes the replay (counts add over the timepoints), relax=False the per-target kernels."""
    P = sampled_case(d, T=3)
    tg, want, g = sampled_counts(d, 3)
    seed = SAMPLED_SEED[d]
    strict = sampled_exact(P, tg, False, 64, seed, Guard(strict=d != 8))
    assert want.any()
    for X in [P] + [f(P) for f in SAMPLED_VARIANTS.values()]:
        assert np.array_equal(eng.multi_simplex_counts(X, tg, relax=True, samples=64, seed=seed), want)
        assert np.array_equal(eng.multi_simplex_counts(X, tg, relax=False, samples=64, seed=seed), strict)
        with xcheck(SD_SIMPLEX_PERTARGET="1"):
            assert np.array_equal(eng.multi_simplex_counts(X, tg, relax=True, samples=64, seed=seed), want)


@pytest.mark.parametrize("d", (1, 3, 8))
def test_sampled_route_switch(eng, d):
    """n = d + 2 (per-target kernels: every target has exactly one subset of others) and n = d + 3 (the first n with the shared
    factorisation), 16 samples, the first rows of the lattice cloud of (a): row 0 is the midpoint of rows 1 and 2."""
    for n in (d + 2, d + 3):
        P = cloud("lattice", d)[:n]
        want = sampled_exact(P, None, True, 16, 5)
        assert want.any(), n
        assert np.array_equal(eng.pointcloud_simplex_counts(P, samples=16, seed=5), want), n
        assert np.array_equal(eng.pointcloud_simplex_counts(P * 2.0 ** -480, samples=16, seed=5), want), n


@pytest.mark.parametrize("d", (1, 3, 8))
def test_sampled_workspace_sizes_and_routes(eng, xcheck, oracle, d):
    """300 samples, relax=True, every row a target (members of shared subsets take sxw_spare_kernel), on the curves
    sampled_case(d, T=3) (900 pairs) and the point cloud sampled_case(d), with five workspace sizes: the recommended one (one
    batch), the routing floor -- the size for 256 samples, which at T = 3 holds 768 to 899 pairs: two batches --, a third
    of the way between them, one byte below the floor and none at all (both: the per-target route), and the retired generic
    kernel through its hook.  All equal the C oracle's counts on the same subsets, which are neither all zero nor saturated."""
    size = eng._lib().sd_simplex_sampled_workspace_bytes                 # (torch first: engine._lib)
    seed = SAMPLED_SEED[d]
    for P in (sampled_case(d, T=3), sampled_case(d)):
        n, T = (P.shape[0], P.shape[1]) if P.ndim == 3 else (P.shape[0], 0)
        call = (lambda **kw: eng.multi_simplex_counts(P, relax=True, samples=300, seed=seed, **kw)) if T else \
               (lambda **kw: eng.pointcloud_simplex_counts(P, samples=300, seed=seed, **kw))
        want = oracle.simplex_sampled(P, None, relax=True, samples=300, seed=seed)
        floor, rec = size(n, T, d, 256), size(n, T, d, 300)
        print(d, T, floor, rec, want.tolist())
        assert 0 < floor < rec and want.any() and want.min() < 300 * max(T, 1)
        for ws_bytes in (rec, floor, floor + (rec - floor) // 3, floor - 1, 0):
            assert np.array_equal(call(ws_bytes=ws_bytes), want), ws_bytes
        with xcheck(SD_SIMPLEX_GENERIC="1"):
            assert np.array_equal(call(), want)


# ---------------------------------------------------------------- (g) through the package
def test_package_utm_and_simplex_exact():
    """PointcloudDepth(containment='simplex') on the UTM-like frame == on the centred frame == the exact counts / C(n, 3), and
    == containment='simplex_exact' (K13) on a planar cloud in general position."""
    from statdepth_amd import PointcloudDepth
    P = utm_cloud()
    want = counts_exact(P - UTM_CENTRE) / math.comb(len(P), 3)
    assert want.any()
    for X in (P, P - UTM_CENTRE):
        assert np.array_equal(PointcloudDepth(pd.DataFrame(X), containment='simplex').to_numpy(), want)
    G = int_cloud(14, 2, 77) + UTM_CENTRE
    assert (counts_int_rows(G, range(14)) > 0).any()                        # asserts the general position too
    df = pd.DataFrame(G)
    assert np.array_equal(PointcloudDepth(df, containment='simplex').to_numpy(),
                          PointcloudDepth(df, containment='simplex_exact').to_numpy())


def test_package_functional_scaled():
    """The multivariate FunctionalDepth simplex route (d = 2, T = 3, 7 curves) on frames scaled by 2^-40 == unscaled == exact."""
    from statdepth_amd import FunctionalDepth
    C, _ = curves_case(2)
    want = curves_counts(2)[0]
    frames = [pd.DataFrame(c) for c in C]
    small = [pd.DataFrame(c * 2.0 ** -40) for c in C]
    a = FunctionalDepth(frames, containment="simplex", relax=True)
    b = FunctionalDepth(small, containment="simplex", relax=True)
    assert np.array_equal(a.to_numpy(), b.to_numpy())
    assert np.array_equal(a.to_numpy(), want.astype(np.float64) / 3 / math.comb(len(C) - 1, 3))
