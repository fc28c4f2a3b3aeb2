"""Oja volume sums on the GPU (K7, sd_oja_*) against the exact references of tests/test_oja_exact_host.py, within the
derived `oja_tolerance`: (a) slice and range boundaries for every d in all three forms, (b) mixed block sizes over
several slices, (c) the global-memory path in the external and block forms, (d) conditioning, (e) exact scaling and
translation, (f) values through PointcloudDepth.  Every comparison prints max |kernel - exact| / (u H) beside its
bound; DESIGN.md (K7, Numerics) records the worst per d."""
import math
from functools import lru_cache

import numpy as np
import pandas as pd
import pytest
from scipy.spatial import ConvexHull

from test_oja_exact_host import (BOUNDARY, D_COND, D_EQUI, FAMILIES, SLICE, ZERO_FAMILIES, boundary_cloud,
                                 conditioning_case, dyadic_cloud, int_cloud, normal_cloud, oja_exact, oja_exact_int,
                                 oja_k, oja_tolerance, outside, ratio, three_targets)
from test_oja_host import oja2_rowwise_targets

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from statdepth_amd import engine
    return engine


def _against_exact(label, got, want, H, d, subsets):
    got = np.asarray(got, dtype=np.float64)
    tol = oja_tolerance(d, subsets, H)
    r = ratio(got, want, H)
    worst = "not finite" if np.isnan(r).any() else f"{np.max(r):.3f}"
    slices = max(1, -(-subsets // SLICE))
    print(f"{label}: d={d} max |kernel - exact| / (u H) = {worst} (bound {oja_k(d) + 138 + slices:.0f})")
    assert np.isfinite(got).all(), got
    assert not outside(got, want, tol).any(), (label, worst)


# ---------------------------------------------------------------- (a) slice and range boundaries, every d
@lru_cache(maxsize=None)
def boundary_case(d, others):
    """(P, targets, exact, H): others + 1 integer rows; the first, a middle and the last row as targets."""
    P = boundary_cloud(d, others)
    tg = three_targets(others + 1)
    want, H = oja_exact_int(P, tg)
    return P, tg, want, H


BOUNDARY_CASES = [(d, o) for d in range(1, 9) for o in BOUNDARY[d]] + [(1, 127), (1, 128), (1, 129)]


@pytest.mark.parametrize("d,others", BOUNDARY_CASES)
def test_slice_and_range_boundaries(eng, d, others):
    """C(others, d) on either side of 32 768 (one slice, two slices), and of one range at d = 1; the skip of the
    target's own row falls before every other, in the middle and after every other."""
    P, tg, want, H = boundary_case(d, others)
    subsets = math.comb(others, d)
    assert (subsets <= SLICE) == (others == BOUNDARY[d][0]) or d == 1 and others < 200
    _against_exact(f"rows others={others}", eng.oja_volume_sums(P, tg), want, H, d, subsets)


def test_four_slices_d8(eng):
    """d = 8, 20 others: 125 970 subsets in 4 slices, the last one partial (27 666 subsets, 217 ranges)."""
    P = int_cloud(21, 8, 8020)
    want, H = oja_exact_int(P, [10])
    _against_exact("rows others=20", eng.oja_volume_sums(P, [10]), want, H, 8, math.comb(20, 8))


@pytest.mark.parametrize("d", range(1, 9))
def test_boundary_external_and_block(eng, d):
    """The two-slice case of each d as an external target, and as a block whose members are in shuffled row order."""
    others = BOUNDARY[d][1]
    subsets = math.comb(others, d)
    rng = np.random.default_rng(50 + d)
    F = int_cloud(others, d, 2000 * d)
    Q = int_cloud(1, d, 2000 * d + 1)
    want, H = oja_exact_int(F, ('external', Q))
    _against_exact("external", eng.oja_external_volume_sums(F, Q), want, H, d, subsets)
    P = int_cloud(others + 7, d, 2000 * d + 2)
    mem = rng.permutation(others + 7)[:others + 1].astype(np.int32)[None, :]
    assert (np.diff(mem[0]) < 0).any()
    want, H = oja_exact_int(P, ('blocks', mem))
    got = eng.oja_subset_volume_sums(P, mem)
    _against_exact("block", got, want, H, d, subsets)
    # the same others in the same order as rows of an array of their own: the same operations, the same bits
    assert np.array_equal(got, eng.oja_volume_sums(P[mem[0]], [others]))


# ---------------------------------------------------------------- (b) mixed block sizes, S > 1
def test_mixed_block_sizes_two_slices(eng):
    """d = 4, bs = 33: a full block (32 others, 35 960 subsets, 2 slices), a 20-member block (3 876 subsets: its second
    unit leaves early), a 4-member block (3 others: no subset) and an empty block, in one call."""
    d, bs = 4, 33
    rng = np.random.default_rng(4)
    P = int_cloud(48, d, 4033)
    mem = np.full((4, bs), -1, dtype=np.int32)
    mem[0] = rng.permutation(48)[:33]
    mem[1, :20] = rng.permutation(48)[:20]
    mem[2, :4] = rng.permutation(48)[:4]
    want, H = oja_exact_int(P, ('blocks', mem))
    assert want[2] == 0.0 and want[3] == 0.0 and H[2] == 0.0
    got = eng.oja_subset_volume_sums(P, mem)
    _against_exact("block of 33", got[:1], want[:1], H[:1], d, math.comb(32, 4))
    _against_exact("block of 20", got[1:2], want[1:2], H[1:2], d, math.comb(19, 4))
    assert got[2] == 0.0 and got[3] == 0.0
    for b in range(4):                                                     # alone, same padding
        assert np.array_equal(eng.oja_subset_volume_sums(P, mem[b:b + 1]), got[b:b + 1]), b
    for b, c in ((1, 20), (2, 4)):                                         # alone, no padding: one slice per block
        assert np.array_equal(eng.oja_subset_volume_sums(P, mem[b:b + 1, :c]), got[b:b + 1]), b
    assert np.array_equal(eng.oja_subset_volume_sums(P, mem[::-1].copy()), got[::-1])


# ---------------------------------------------------------------- (c) global-memory path, external and blocks
def test_global_memory_path_external_and_block(eng):
    """d = 2.  4 200 others are 67 200 bytes: above the 64 KB that LDS takes, read from global memory.
    External: Q over 4 200 rows, against the row-wise oracle; bit for bit the rows form of the same others with the
    point appended.  (No call has these 4 200 others in LDS, so the comparison across the two paths is the block's.)
    Blocks: bs = 4 200 puts the whole call on the global-memory path; its 4 097-member block has 4 096 others, which as
    the rows of an array of their own are exactly 64 KB in LDS: same operations, same bits."""
    rng = np.random.default_rng(42)
    F = rng.random((4200, 2))
    Q = rng.random((2, 2))
    got = eng.oja_external_volume_sums(F, Q)
    for k in range(2):
        both = np.vstack([F, Q[k]])
        want = oja2_rowwise_targets(both, [4200])
        assert np.all(np.abs(got[k] - want) <= 1e-11 * want)
        assert np.array_equal(eng.oja_volume_sums(both, [4200]), got[k:k + 1])
    P = rng.random((4300, 2))
    mem = np.full((2, 4200), -1, dtype=np.int32)
    mem[0] = rng.permutation(4300)[:4200]
    mem[1, :4097] = rng.permutation(4300)[:4097]
    got = eng.oja_subset_volume_sums(P, mem)
    want = np.concatenate([oja2_rowwise_targets(P[mem[0]], [4199]), oja2_rowwise_targets(P[mem[1, :4097]], [4096])])
    assert np.all(np.abs(got - want) <= 1e-11 * want)
    lds = eng.oja_volume_sums(P[mem[1, :4097]], [4096])                     # rows form, 4 097 rows: the LDS path
    assert np.array_equal(got[1:], lds)
    assert np.array_equal(eng.oja_subset_volume_sums(P, mem[1:, :4097].copy()), lds)   # bs = 4 097: blocks in LDS


# ---------------------------------------------------------------- (d) conditioning
@pytest.mark.parametrize("d", D_COND)
@pytest.mark.parametrize("family", FAMILIES)
def test_conditioning(eng, family, d):
    P, want, H = conditioning_case(family, d)
    got = eng.oja_volume_sums(P.copy())
    with np.errstate(all='ignore'):
        rel = np.max(np.abs(got - want) / want) if (want > 0).all() else float('nan')
    print(f"{family}: d={d} max relative error {rel:.2e}")
    _against_exact(family, got, want, H, d, math.comb(len(P) - 1, d))


@pytest.mark.parametrize("d", D_COND)
@pytest.mark.parametrize("family", ZERO_FAMILIES)
def test_exactly_flat_cloud_with_duplicates_is_zero(eng, family, d):
    P, want, H = conditioning_case(family, d)
    assert (want == 0.0).all()
    got = eng.oja_volume_sums(P.copy())
    assert (got == 0.0).all(), got


# ---------------------------------------------------------------- (e) exact equivariances
@pytest.mark.parametrize("d", D_EQUI)
def test_isotropic_scaling_is_exact(eng, d):
    """sums(P 2^k) == sums(P) 2^(k d), k = -60 and 60: every operation commutes with a power of two while nothing
    leaves the normal range; an absolute threshold anywhere would not."""
    P = normal_cloud(d)
    base = eng.oja_volume_sums(P)
    want, H = oja_exact(P)
    _against_exact("normal", base, want, H, d, math.comb(len(P) - 1, d))
    for k in (-60, 60):
        got = eng.oja_volume_sums(P * 2.0 ** k)
        assert np.array_equal(got, base * 2.0 ** (k * d)), k


@pytest.mark.parametrize("d", D_EQUI)
def test_exact_translation_is_bitwise(eng, d):
    """20-bit dyadic coordinates in [0, 1) moved by 2^13: the sum is exact in 33 bits, the differences are the same
    numbers, so are the results."""
    P = dyadic_cloud(d)
    Y = P + 2.0 ** 13
    assert np.array_equal(Y - 2.0 ** 13, P)
    base = eng.oja_volume_sums(P)
    assert np.array_equal(eng.oja_volume_sums(Y), base)
    want, H = oja_exact(P)
    _against_exact("dyadic", base, want, H, d, math.comb(len(P) - 1, d))


# ---------------------------------------------------------------- (f) values through the public API
def test_public_api_d5_integer_cloud():
    from statdepth_amd import PointcloudDepth
    d, others = 5, BOUNDARY[5][0]
    P = boundary_case(d, others)[0]
    df = pd.DataFrame(P, index=[f"p{i}" for i in range(len(P))])
    got = PointcloudDepth(df, containment='oja')
    assert list(got.index) == list(df.index)
    vol = ConvexHull(P).volume
    want, H = oja_exact_int(P)
    _against_exact("PointcloudDepth", got.to_numpy(), want / vol, H / vol, d, math.comb(others, d))
