"""The kernels that fold a pair image into the MBD totals (mbd_rank_fold.hip on the skeleton of rank_fold.h): every one
of them through its unrolled row loop and its ragged tail, with both image words, the half-word image and its markers, the
=| += store over several batches -- EQUAL to the oracle's integers.

Data: walks rounded to 0.01 (rows hold tied keys), one NaN-free untied row, one row with NaN in every 7th curve, one +inf
and one -inf entry.  T runs over the edges of slices x loads in flight of the kernels: 16 x 8 and 64 x 4 for the 16-bit
image, 16 x 8, 16 x 4 and 32 x 4 for the AB2 image.  Oracles: mbd_counts_ranksort(X, 2) for every curve, mbd_counts(X, tg, J)
on at most 200 targets for J = 3, 4."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from statdepth_amd import engine
    return engine


@functools.lru_cache(maxsize=None)
def _walk():
    X = np.round(np.random.default_rng(1313).normal(size=(300, 16392)).cumsum(axis=0), 2)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def _data(T, n):
    X = _walk()[:T, :n].copy()
    X[0] = np.random.default_rng(T * 100003 + n).normal(size=n)       # NaN-free, untied
    assert len(np.unique(X[0])) == n
    if T > 1:
        X[1, ::7] = np.nan
    X[T - 1, 3] = np.inf
    X[T // 2, n - 2] = -np.inf
    if T > 2:
        assert any(len(np.unique(row)) < n for row in X[2:])          # tied keys
    return X                                                          # (stays writable for the upload; nobody writes to it)


def _targets(n, k, seed):
    """k targets in shuffled order, the first one twice, the last curve among them"""
    tg = np.random.default_rng(seed).permutation(n)[:k].astype(np.int64)
    tg[-1] = tg[0]
    tg[1 % k] = n - 1
    return tg


@functools.lru_cache(maxsize=None)
def _want_all(T, n):
    """J = 2, every curve"""
    import oracle
    oracle.build()
    w = oracle.mbd_counts_ranksort(_data(T, n), 2)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def _want_some(T, n, J, k=200, lo=0, hi=None):
    """(tg, totals of tg): k targets (at most 200) among the curves [lo, hi)"""
    import oracle
    oracle.build()
    assert k <= 200
    hi = n if hi is None else hi
    tg = lo + _targets(hi - lo, min(k, hi - lo), 7 * T + n + J)
    w = oracle.mbd_counts(_data(T, n), tg, J)
    w.setflags(write=False)                                           # (tg stays writable for the upload)
    return tg, w


def _check_all_curves(eng, T, n, J, what):
    """every curve as a target: J = 2 against the rank-sort oracle, J >= 3 on the oracle's targets"""
    got = eng.mbd_counts(_data(T, n), None, J=J, algo="rank")
    if J == 2:
        assert np.array_equal(got, _want_all(T, n)), (what, T, n, J)
    else:
        tg, want = _want_some(T, n, J)
        assert np.array_equal(got[tg], want), (what, T, n, J)


def _check_list(eng, T, n, J, k, what):
    tg, want = _want_some(T, n, J, k)
    assert np.array_equal(eng.mbd_counts(_data(T, n), tg, J=J, algo="rank"), want), (what, T, n, J)


def _check_range(eng, T, n, J, begin, m, what):
    got = eng.mbd_counts_range(_data(T, n), begin, m, J=J, algo="rank")
    if J == 2:
        assert np.array_equal(got, _want_all(T, n)[begin:begin + m]), (what, T, n, J)
    else:
        tg, want = _want_some(T, n, J, 200, begin, begin + m)
        assert np.array_equal(got[tg - begin], want), (what, T, n, J)


# ---------------------------------------------------------------- 16-bit folds, tiny n
TINY_T = [1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300]


def _tiny(eng, xcheck, T, **more):
    for n in (66, 68):
        _check_all_curves(eng, T, n, 4, "rank_accumulate_kernel<4>")          # product: J >= 4 folds a pair image
        _check_list(eng, T, n, 4, 50, "rank_accumulate_kernel<4>, list")
        with xcheck(SD_RANK_IMPL=5, **more):                                  # image mode for J <= 3 as well
            for J in (2, 3):
                # n = 68: four curves per thread (rank_accumulate4_kernel); n = 66 or a list: rank_accumulate_kernel
                _check_all_curves(eng, T, n, J, "image mode")
                _check_list(eng, T, n, J, 50, "image mode, list")
            if more:
                _check_all_curves(eng, T, n, 4, "image mode, batches")


@pytest.mark.parametrize("T", TINY_T)
def test_pair16_folds_tiny_n(eng, xcheck, T):
    _tiny(eng, xcheck, T)


def test_pair16_folds_several_batches(eng, xcheck):
    """300 rows in batches of 130, 130 and 40: out = then out += twice"""
    _tiny(eng, xcheck, 300, SD_RANK_ROWS_PER_BATCH=130)


# ---------------------------------------------------------------- 16-bit folds behind the medium route
@pytest.mark.parametrize("J", [2, 3])
def test_pair16_folds_medium_route(eng, J):
    """n = 16 388, T = 257 on the product library: rank_medium_image_kernel writes the image; every curve goes through
    rank_accumulate4_kernel (four unrolled steps of its 64 slices and one more row), 50 listed targets through
    rank_accumulate_kernel (two unrolled steps of its 16 slices and one more row)."""
    _check_all_curves(eng, 257, 16388, J, "rank_accumulate4_kernel")
    _check_list(eng, 257, 16388, J, 50, "rank_accumulate_kernel")


# ---------------------------------------------------------------- AB2 folds (large-n route)
AB2_T = [1, 17, 33, 65, 129, 200]


def _ab2(eng, xcheck, T, **more):
    N8, N4, N1 = 16392, 16388, 16386
    with xcheck(SD_BIG_NOMEDIUM=1, **more):                                   # half-word image
        for J in (2, 3):
            _check_all_curves(eng, T, N8, J, "rank_accumulate_h8_kernel")
            _check_range(eng, T, N8, J, 4, 16384, "rank_accumulate2x4_kernel, half words")
            _check_range(eng, T, N8, J, 1, 16384, "rank_accumulate2_kernel, half words, begin 1")
            _check_list(eng, T, N8, J, 200, "rank_accumulate2_kernel, half words, list")
            _check_all_curves(eng, T, N4, J, "rank_accumulate2x4_kernel, n % 8 = 4")
            _check_all_curves(eng, T, N1, J, "rank_accumulate2_kernel, n % 4 = 2")
        _check_all_curves(eng, T, N8, 4, "rank_accumulate2_kernel<4>")
    with xcheck(SD_BIG_NOMEDIUM=1, SD_BIG_NOHALF=1, **more):                  # B words
        for J in (2, 3):
            _check_all_curves(eng, T, N8, J, "rank_accumulate2x4_kernel, B words")
            _check_all_curves(eng, T, N4, J, "rank_accumulate2x4_kernel, B words, n % 8 = 4")
            _check_all_curves(eng, T, N1, J, "rank_accumulate2_kernel, B words")
            _check_list(eng, T, N8, J, 200, "rank_accumulate2_kernel, B words, list")


@pytest.mark.parametrize("T", AB2_T)
def test_ab2_folds(eng, xcheck, T):
    _ab2(eng, xcheck, T)


def test_ab2_folds_several_batches(eng, xcheck):
    """200 rows in batches of 70, 70 and 60"""
    _ab2(eng, xcheck, 200, SD_RANK_ROWS_PER_BATCH=70)
