"""Bucket-local key images of the two-launch rank path (rank_bucket32_kernel + rank_bucket_kernel's SEL form).

A key's bucket is the top 14 bits of its 31-bit image q, and LDS holds a 31-bit bucket-local image: q's low 17 bits followed by
14 more bits of the core's fraction, i.e. 45 bits of resolution in all (tail keys and NaN keep 31).  Keys closer than
range / 2^31 but farther apart than range / 2^45 are now ordered by their images; closer ones still share an image and are
settled by the tie list.  Every case is compared with the oracle's rank-sort totals and with the fp64 bucket kernel alone
(SD_RB_NO32=1).  Rows = 300 timepoints: every workgroup of the first launch ranks one row.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T = 300
CORE = float(0x7FFFFE00 - 256) - 64.0                                 # images of an unclipped row's core, as the kernel scales it


@pytest.fixture(scope="module")
def eng():
    from statdepth_amd import engine
    return engine


def _check(eng, oracle, xcheck, X):
    want = oracle.mbd_counts_ranksort(X, 2)
    got = eng.mbd_counts(X, None, 2, algo="rank")
    assert (got == want).all()
    with xcheck(SD_RB_NO32="1"):
        assert (eng.mbd_counts(X, None, 2, algo="rank") == want).all()


def _walks(n, seed):
    return np.random.default_rng(seed).normal(size=(T, n)).cumsum(axis=0)


def _plant_pairs(X, rng, k, rel):
    """k pairs per row: a curve moved to `rel` x the row's range above another one (away from the row's extremes)."""
    for row in X:
        span = row.max() - row.min()
        order = np.argsort(row)
        cur = rng.choice(order[10:-10], size=2 * k, replace=False)
        for i in range(k):
            a, b = cur[2 * i], cur[2 * i + 1]
            row[b] = row[a] + rel * span
            assert row[b] != row[a]


def test_bucket32_pairs_resolved_by_local_images(eng, oracle, xcheck):
    """Pairs 2^-38 x range apart: one image apart at 31 bits at most (they collided), 2^7 apart at 45 bits."""
    rng = np.random.default_rng(61)
    X = _walks(10000, 61)
    _plant_pairs(X, rng, 40, 2.0 ** -38)
    _check(eng, oracle, xcheck, X)


def test_bucket32_pairs_below_local_resolution(eng, oracle, xcheck):
    """Pairs 2^-46 x range apart: half a 45-bit image, so most share one and go to the tie list (8 pairs per row: 16 keys)."""
    rng = np.random.default_rng(62)
    X = _walks(10000, 62)
    _plant_pairs(X, rng, 8, 2.0 ** -46)
    _check(eng, oracle, xcheck, X)


def test_bucket32_pairs_across_bucket_edges(eng, oracle, xcheck):
    """Keys a hair either side of a bucket edge (image b << 17) and of a 45-bit image edge inside a bucket, at distances
    below one 31-bit image and below one 45-bit image, plus the edge value itself and the next double."""
    rng = np.random.default_rng(63)
    X = np.stack([rng.permutation(10000).astype(np.float64) - 5000 for _ in range(T)])   # distinct, no coincidences of their own
    for row in X:
        lo, hi = row.min(), row.max()
        scale = CORE / (hi - lo)
        free = rng.permutation(np.flatnonzero(np.abs(row) < 4000))
        i = 0
        for b in rng.choice(np.arange(200, 16000), size=4, replace=False):
            for u in (b * 2.0 ** 17, b * 2.0 ** 17 + 37.0 + 5.0 / 16384.0):   # a bucket edge; a 45-bit edge inside the bucket
                xe = lo + (u - 256.0) / scale
                for v in (xe - (hi - lo) * 2.0 ** -40, xe + (hi - lo) * 2.0 ** -40, xe - (hi - lo) * 2.0 ** -50,
                          xe + (hi - lo) * 2.0 ** -50, xe, np.nextafter(xe, np.inf)):
                    row[free[i]] = v
                    i += 1
    _check(eng, oracle, xcheck, X)


def test_bucket32_near_ties_in_cauchy_tails(eng, oracle, xcheck):
    """Cauchy rows take the three-piece map; near-ties among the tail keys (31-bit resolution there) at 2^-38 x their
    magnitude and a few ulps, on both sides, and core near-ties in the same rows."""
    rng = np.random.default_rng(64)
    X = rng.standard_cauchy(size=(T, 10000))
    for row in X:
        order = np.argsort(row)
        for side in (order[5:200], order[-200:-5]):                   # far outside the bulk, not the extremes
            cur = rng.choice(side, size=6, replace=False)
            row[cur[1]] = row[cur[0]] * (1.0 + 2.0 ** -38)
            row[cur[3]] = np.nextafter(np.nextafter(row[cur[2]], np.inf), np.inf)
            row[cur[5]] = row[cur[4]]
        mid = rng.choice(order[4000:6000], size=4, replace=False)
        row[mid[1]] = row[mid[0]] + 2.0 ** -38
        row[mid[3]] = np.nextafter(row[mid[2]], -np.inf)
    _check(eng, oracle, xcheck, X)


def test_bucket32_signed_zero_and_denormals_in_walks(eng, oracle, xcheck):
    """-0.0 and +0.0 (equal) next to the smallest denormals of either sign (distinct, but within one 45-bit image of 0) in
    continuous rows."""
    rng = np.random.default_rng(65)
    X = _walks(10000, 65)
    for row in X:
        z = rng.choice(np.argsort(row)[100:-100], size=5, replace=False)
        row[z] = [0.0, -0.0, 5e-324, -5e-324, 0.0]
    _check(eng, oracle, xcheck, X)


@pytest.mark.parametrize("n", [3500, 8192, 11264])
def test_bucket32_local_images_other_sizes(eng, oracle, xcheck, n):
    """Walks at E = 8, 16 and 22 keys per thread, with pairs resolved by the local images and pairs that still collide."""
    rng = np.random.default_rng(n)
    X = _walks(n, n)
    _plant_pairs(X, rng, 20, 2.0 ** -38)
    _plant_pairs(X, rng, 4, 2.0 ** -47)
    _check(eng, oracle, xcheck, X)
