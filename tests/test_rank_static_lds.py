"""The first launch of the two-launch rank path (rank_bucket32_kernel) with a compile-time LDS block and buffer loads.

The kernel's LDS block is sized at compile time for the largest n of its class (E keys per thread, E * 512 curves); the
run-time n decides where the sentinels and the dummy word lie inside it.  A row is loaded through a buffer resource of the
row (32-bit lane offsets, the key's stride in the scalar offset), and a key slot at or beyond n must still read as NaN.
Every case compares sd_mbd_counts (engine.mbd_counts) with the oracle's rank-sort totals; the oracle alone decides.
T = 256 timepoints: the fewest rows the two-launch path takes on 256 CUs.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T = 256


@pytest.fixture(scope="module")
def eng():
    from statdepth_amd import engine
    return engine


def _walks(n, seed):
    return np.random.default_rng(seed).normal(size=(T, n)).cumsum(axis=0)


def _check(eng, oracle, X):
    want = oracle.mbd_counts_ranksort(X, 2)
    got = eng.mbd_counts(X, None, 2, algo="rank")
    assert got.shape == want.shape
    assert (got == want).all()


@pytest.mark.parametrize("n", [3073, 4096, 4097, 10240, 10241, 11261, 11264])
def test_class_boundaries(eng, oracle, n):
    """The edges of the classes of n.  A multiple of 1 024 puts the sentinels and the dummy at the end of the static block,
    n = 1 mod 1 024 leaves the last key slot to one curve, 11 261 is padded to a whole quad of keys (al4)."""
    _check(eng, oracle, _walks(n, n))


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_padding_slots_read_as_nan(eng, oracle, sign):
    """n = 10 000: the last key slot is empty from thread 272 on.  With data of one sign a padding slot read as 0 instead of
    NaN would be a key below (above) every curve and change the ranks."""
    X = sign * (np.abs(_walks(10000, 71)) + 1.0)
    assert (sign * X > 0).all()
    _check(eng, oracle, X)


def test_targets_in_the_last_slot_of_the_last_row(eng, oracle):
    """Targets among the curves of the last, partly empty key slot, the matrix's last curve included: their totals need
    every row, the matrix's last row too, whose empty slots lie past the end of the matrix (the row's resource ends at
    its n-th double)."""
    n = 10000
    X = _walks(n, 72)
    targets = np.array([n - 1, n - 2, 19 * 512, 19 * 512 + 271, 19 * 512 - 1, 0], dtype=np.int64)
    want = oracle.mbd_counts(X, targets, 2)
    got = eng.mbd_counts(X, targets, 2, algo="rank")
    assert (got == want).all()
    assert (want == oracle.mbd_counts_ranksort(X, 2)[targets]).all()


@pytest.mark.parametrize("n", [10000, 4097])
def test_ties_duplicates_and_a_nan_row(eng, oracle, n):
    """Values rounded to 0.1 with duplicated curves (closed form, tie list) and one row with a NaN (handed over to the
    second launch): the paths that keep their addressing still work beside the new one."""
    rng = np.random.default_rng(n + 5)
    X = np.round(_walks(n, n + 5), 1)
    dup = rng.choice(n, size=n // 100, replace=False)
    X[:, dup] = X[:, rng.choice(n, size=n // 100, replace=False)]
    X[T // 2, rng.integers(n)] = np.nan
    _check(eng, oracle, X)
