"""Projection depth (containment='projection', K12: 1 / (1 + Stahel-Donoho outlyingness) over a fixed direction set)
without a GPU: the numpy restatement of the definition against hand-computed cases, the MAD selected from two ascending
deviation sequences against the sorted-deviations median, the host-side validation, the C ABI's refusals, and the missing
device reported as such (no CPU fallback).

The restatement (`median_rule`, `locscale`, `outlyingness`, `projection_outlyingness`, `projection_external`,
`projection_sampled`) is imported by tests/test_projection_gpu.py as its oracle.  Every operation in it is one numpy fp64
operation, i.e. one correctly rounded IEEE operation, in the order DESIGN §3 K12 states.
"""
import ctypes

import numpy as np
import pandas as pd
import pytest

from test_halfspace_host import make_directions, projections


# ---------------------------------------------------------------- numpy restatement of the definition
def median_rule(s):
    """s sorted ascending, N >= 1: s[(N-1)/2] for N odd, (s[N/2-1] + s[N/2]) * 0.5 for N even (sum, then product)."""
    N = len(s)
    if N % 2:
        return s[(N - 1) // 2]
    return (s[N // 2 - 1] + s[N // 2]) * 0.5


def locscale(z):
    """(med, mad) of the projections z of a sample on one direction."""
    z = np.asarray(z, dtype=np.float64)
    med = median_rule(np.sort(z))
    return med, median_rule(np.sort(np.abs(z - med)))


def outlyingness(zq, med, mad):
    """|zq - med| / mad elementwise; a numerator of 0 gives 0 (also for mad = 0), above 0 with mad = 0 gives inf."""
    num = np.abs(np.asarray(zq, dtype=np.float64) - med)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        o = num / mad
    return np.where(num == 0.0, 0.0, o)


def projection_outlyingness(P, U, targets=None):
    """max over directions of |z_r(q) - med_r| / mad_r, q = P[t], the sample all rows of P."""
    Z = projections(P, U)
    tg = np.arange(Z.shape[1]) if targets is None else np.asarray(targets, dtype=np.int64)
    best = np.zeros(len(tg), dtype=np.float64)
    for z in Z:
        med, mad = locscale(z)
        best = np.maximum(best, outlyingness(z[tg], med, mad))
    return best


def projection_external(F, Q, U):
    """Outlyingness of each external point g inside F u {g}: n + 1 points, a median and a MAD per external point."""
    F = np.asarray(F, dtype=np.float64)
    return np.array([projection_outlyingness(np.vstack([F, g]), U, [len(F)])[0] for g in np.asarray(Q, dtype=np.float64)],
                    dtype=np.float64)


def depth_of(O):
    return 1.0 / (1.0 + np.asarray(O, dtype=np.float64))


def projection_sampled(P, targets, K, U):
    """The K-block estimator replaying _samplepointwisedepth's draws from the global numpy RNG: per target ss = n // K
    blocks of `rows.sample(n=ss)` with the target appended last; depth inside the block, mean over the blocks."""
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
            vals.append(depth_of(projection_outlyingness(P[blk], U, [len(blk) - 1]))[0])
        out.append(np.mean(vals))
    return np.array(out)


# ---------------------------------------------------------------- the selection the kernels use, as Python
def mad_by_selection(s):
    """(med, mad) from the sorted sequence s without sorting the deviations: a = lower_bound(s, med); med - s[a-1-j] and
    s[a+j] - med are two ascending sequences; the (N-1)//2-th smallest of their union by a merge-path binary search, the
    N//2-th is the next of the merge.  Counts the reads of s to show O(log N)."""
    N = len(s)
    reads = [0]

    def at(i):
        assert 0 <= i < N
        reads[0] += 1
        return s[i]

    k1, k2 = (N - 1) // 2, N // 2
    med = at(k1) if k1 == k2 else (at(k1) + at(k2)) * 0.5
    lo, hi = 0, N
    while lo < hi:
        mid = (lo + hi) // 2
        if at(mid) < med:
            lo = mid + 1
        else:
            hi = mid
    a = lo
    la, lb = a, N - a
    A = lambda j: med - at(a - 1 - j)                                   # noqa: E731
    B = lambda j: at(a + j) - med                                       # noqa: E731
    lo, hi = max(k1 - lb, 0), min(k1, la)
    while lo < hi:
        mid = (lo + hi) // 2
        if A(mid) <= B(k1 - 1 - mid):
            lo = mid + 1
        else:
            hi = mid
    i, j = lo, k1 - lo
    av = A(i) if i < la else np.inf
    bv = B(j) if j < lb else np.inf
    e1 = min(av, bv)
    if k1 == k2:
        return med, e1, reads[0]
    if av <= bv:
        i += 1
        av = A(i) if i < la else np.inf
    else:
        j += 1
        bv = B(j) if j < lb else np.inf
    return med, (e1 + min(av, bv)) * 0.5, reads[0]


def test_selection_equals_sorted_deviations():
    rng = np.random.default_rng(5)
    for N in range(1, 41):
        cases = [rng.normal(size=N), rng.integers(-3, 4, size=N).astype(np.float64),
                 np.repeat(rng.normal(size=(N + 2) // 3), 3)[:N],         # runs of ties
                 np.full(N, 2.5), np.arange(N, dtype=np.float64),
                 np.concatenate([np.zeros(N - N // 3), rng.normal(size=N // 3)]),
                 rng.normal(size=N) * 2.0 ** rng.integers(-40, 40, size=N)]
        for z in cases:
            s = np.sort(z)
            med, mad, reads = mad_by_selection(s)
            wmed, wmad = locscale(z)
            assert med == wmed and mad == wmad, (N, z)
    s = np.sort(rng.normal(size=100001))
    med, mad, reads = mad_by_selection(s)
    assert (med, mad) == locscale(s)
    assert reads <= 4 * 17 + 8                                          # two binary searches, two reads per merge-path step


def test_selection_with_an_inserted_value():
    """The external form's sample: F's sorted row with g's projection inserted at its lower_bound position."""
    rng = np.random.default_rng(6)
    for n in (1, 2, 5, 6, 31):
        row = np.sort(rng.integers(-4, 5, size=n).astype(np.float64))
        for v in (-9.0, 9.0, row[0], row[n // 2], 0.5):
            pos = int(np.searchsorted(row, v, side='left'))
            s = np.insert(row, pos, v)
            assert np.array_equal(s, np.sort(np.append(row, v)))
            med, mad, _ = mad_by_selection(s)
            assert (med, mad) == locscale(np.append(row, v))


# ---------------------------------------------------------------- the restatement against hand-computed cases
ONE = [[1.0]]


def test_hand_computed_odd():
    P = np.array([0.0, 1.0, 2.0, 3.0, 10.0])[:, None]                   # med 2, deviations 2 1 0 1 8, MAD 1
    O = projection_outlyingness(P, ONE)
    assert O.tolist() == [2.0, 1.0, 0.0, 1.0, 8.0]
    assert np.array_equal(depth_of(O), np.array([1 / 3, 1 / 2, 1.0, 1 / 2, 1 / 9]))


def test_hand_computed_even():
    P = np.array([0.0, 1.0, 3.0, 10.0])[:, None]                        # med 2, deviations 2 1 1 8, MAD 1.5
    assert locscale(P[:, 0]) == (2.0, 1.5)
    assert np.array_equal(projection_outlyingness(P, ONE), np.array([2.0 / 1.5, 1.0 / 1.5, 1.0 / 1.5, 8.0 / 1.5]))
    assert np.array_equal(projection_outlyingness(P, ONE), np.array([4 / 3, 2 / 3, 2 / 3, 16 / 3]))


def test_hand_computed_zero_mad():
    P = np.array([5.0, 5.0, 5.0, 5.0, 9.0])[:, None]
    O = projection_outlyingness(P, ONE)
    assert O.tolist() == [0.0, 0.0, 0.0, 0.0, np.inf]
    assert depth_of(O).tolist() == [1.0, 1.0, 1.0, 1.0, 0.0]


def test_hand_computed_single_point_and_external():
    assert projection_outlyingness(np.array([[7.0]]), ONE).tolist() == [0.0]
    assert projection_outlyingness(np.array([[7.0, -2.0]]), [[1.0, 0.0], [3.0, 4.0]]).tolist() == [0.0]
    # inside F u {g}: [0 1 2 3] u {10} is the odd case above; u {2} has med 2, deviations 2 1 0 1 0, MAD 1
    F = np.array([0.0, 1.0, 2.0, 3.0])[:, None]
    assert projection_external(F, [[10.0], [2.0], [-1.0]], ONE).tolist() == [8.0, 0.0, 2.0]


def test_targets_and_direction_maximum():
    P = np.array([[0.0, 0.0], [1.0, 5.0], [2.0, 1.0], [3.0, 2.0], [10.0, 3.0]])
    U = np.array([[1.0, 0.0], [0.0, 1.0]])
    ox, oy = projection_outlyingness(P[:, :1], ONE), projection_outlyingness(P[:, 1:], ONE)
    assert np.array_equal(projection_outlyingness(P, U), np.maximum(ox, oy))
    assert np.array_equal(projection_outlyingness(P, U, [4, 1, 1]), np.maximum(ox, oy)[[4, 1, 1]])


# ---------------------------------------------------------------- host validation
def test_validation_errors_before_device_work():
    from statdepth_amd import PointcloudDepth
    rng = np.random.default_rng(2)
    good = pd.DataFrame(rng.normal(size=(10, 2)))
    for kw in ({}, {"K": 2}):
        for bad_value in (np.nan, np.inf, -np.inf):
            bad = good.copy()
            bad.iloc[3, 1] = bad_value
            with pytest.raises(ValueError, match=r'finite coordinates of magnitude at most 2\^500'):
                PointcloudDepth(bad, containment='projection', **kw)
        big = good.copy()
        big.iloc[0, 0] = -2.0 ** 501
        with pytest.raises(ValueError, match=r'2\^500'):
            PointcloudDepth(big, containment='projection', **kw)
        with pytest.raises(ValueError, match='all-zero row'):
            PointcloudDepth(good, containment='projection', directions=[[1.0, 0.0], [0.0, 0.0]], **kw)
        with pytest.raises(ValueError, match='finite'):
            PointcloudDepth(good, containment='projection', directions=[[1.0, np.nan]], **kw)
        with pytest.raises(ValueError, match=r'2\^500'):
            PointcloudDepth(good, containment='projection', directions=[[1.0, 2.0 ** 501]], **kw)
        with pytest.raises(ValueError, match=r'\(k x 2\) array'):
            PointcloudDepth(good, containment='projection', directions=np.ones((4, 3)), **kw)
        with pytest.raises(ValueError, match='positive number'):
            PointcloudDepth(good, containment='projection', directions=0, **kw)
        with pytest.raises(NotImplementedError, match='d <= 8'):
            PointcloudDepth(pd.DataFrame(rng.normal(size=(12, 9))), containment='projection', **kw)
        with pytest.raises(NotImplementedError, match='projection depth'):
            PointcloudDepth(good, containment='projection', directions='exact', **kw)
        with pytest.raises(ValueError, match='directions must be'):
            PointcloudDepth(good, containment='projection', directions='all', **kw)


@pytest.mark.parametrize("n,K", [(4096, 2), (4097, 2), (2 * 2049, 2), (3 * 2048 + 2, 3)])
def test_k_blocks_above_one_sort_tile_are_refused_before_the_rng(n, K):
    """A block holds the n // K drawn rows and, where the draw missed it, the point: n // K = 2048 already reaches 2 049
    members.  NotImplementedError from the host, and nothing drawn from the global RNG."""
    from statdepth_amd import PointcloudDepth
    assert n // K + 1 > 2048
    wide = pd.DataFrame(np.random.default_rng(3).normal(size=(n, 2)))
    for tc in (None, [5]):
        np.random.seed(4)
        with pytest.raises(NotImplementedError, match='at most 2048 rows'):
            PointcloudDepth(wide, to_compute=tc, containment='projection', K=K, directions=4)
        after = np.random.random()
        np.random.seed(4)
        assert after == np.random.random()                              # nothing was drawn for the refused call


def test_widest_k_block_that_is_taken_passes_the_host_check():
    """n // K = 2047: blocks of at most 2 048 members.  The host check lets it through (it then needs a device; without
    one the call ends in the missing-device error, never in NotImplementedError)."""
    from statdepth_amd import PointcloudDepth, _native
    ok = pd.DataFrame(np.random.default_rng(3).normal(size=(2 * 2047, 2)))
    if _native.load().sd_device_count() > 0:
        got = PointcloudDepth(ok, to_compute=[7], containment='projection', K=2, directions=2)
        assert 0.0 <= got.to_numpy()[0] <= 1.0
    else:
        with pytest.raises(RuntimeError, match='no HIP device'):
            PointcloudDepth(ok, to_compute=[7], containment='projection', K=2, directions=2)


def test_the_value_check_has_one_definition():
    """engine.projection_check is what PointcloudDepth and PointcloudHomogeneity run; the engine's projection_* functions
    take their arrays as they are, like halfspace_counts."""
    from statdepth_amd import engine
    from statdepth_amd.depth.calculations import _pointcloud
    P = np.random.default_rng(0).normal(size=(6, 2))
    engine.projection_check('coordinates', P, P[:2], np.empty((0, 2)))
    for bad_value in (np.nan, np.inf, -np.inf, 2.0 ** 501, -2.0 ** 501):
        bad = P.copy()
        bad[2, 0] = bad_value
        with pytest.raises(ValueError, match=r'finite coordinates of magnitude at most 2\^500'):
            engine.projection_check('coordinates', P, bad)
        with pytest.raises(ValueError, match=r'finite coordinates of magnitude at most 2\^500'):
            _pointcloud._projection_check(bad)
    engine.projection_check('coordinates', P * 0 + 2.0 ** 500)
    assert not hasattr(_pointcloud, '_PROJECTION_MAX_ABS')


def test_unknown_containment_keeps_its_message():
    from statdepth_amd import PointcloudDepth
    from statdepth_amd.homogeneity import PointcloudHomogeneity
    df = pd.DataFrame(np.random.default_rng(0).normal(size=(6, 2)))
    for kw in ({}, {"K": 2}, {"directions": 5, "seed": 1}):
        with pytest.raises(ValueError) as e:
            PointcloudDepth(df, containment='nonsense', **kw)
        assert str(e.value) == 'nonsense is not a valid containment measure. '
    with pytest.raises(ValueError) as e:
        PointcloudDepth(df, containment='projections')
    assert str(e.value) == 'projections is not a valid containment measure. '
    G = pd.DataFrame(np.random.default_rng(1).normal(size=(6, 2)))
    with pytest.raises(ValueError) as e:
        PointcloudHomogeneity(df, G, containment='nonsense').homogeneity()
    assert str(e.value) == 'nonsense is not a valid containment measure. '


# ---------------------------------------------------------------- C ABI, no device needed
def _lib():
    from statdepth_amd import _native
    return _native, _native.load()


def test_abi_refusals_before_device_work():
    _native, lib = _lib()
    fake = ctypes.c_void_p(256)                  # never dereferenced: every refusal happens before device work
    out = ctypes.c_void_p(512)
    INV, UNS, WSP = _native.SD_ERR_INVALID, _native.SD_ERR_UNSUPPORTED, _native.SD_ERR_WORKSPACE

    def rows(P, n, d, U, k, tg, m, o):
        return lib.sd_projection_outlyingness(P, n, d, U, k, tg, m, o, fake, 1 << 40, None)

    def ext(P, n, d, U, k, Q, m, o):
        return lib.sd_projection_external_outlyingness(P, n, d, U, k, Q, m, o, fake, 1 << 40, None)

    def sub(P, n, d, U, k, mem, nb, bs, o):
        return lib.sd_projection_subset_outlyingness(P, n, d, U, k, mem, nb, bs, o, None)

    assert rows(None, 10, 2, fake, 4, None, 10, out) == INV
    assert rows(fake, 10, 2, None, 4, None, 10, out) == INV
    assert rows(fake, 10, 2, fake, 4, None, 10, None) == INV
    assert rows(fake, 10, 2, fake, 4, None, 9, out) == INV                    # NULL targets, m != n
    assert rows(fake, 0, 2, fake, 4, None, 0, out) == INV
    assert rows(fake, 10, 0, fake, 4, None, 10, out) == INV
    assert rows(fake, 10, 2, fake, 0, None, 10, out) == INV                   # k = 0
    assert rows(fake, 10, 9, fake, 4, None, 10, out) == UNS                   # d = 9
    assert b"d in [1,8]" in lib.sd_last_error()
    assert rows(fake, 2**31, 1, fake, 1, fake, 1, out) == UNS                 # n = 2^31
    assert b"2^31" in lib.sd_last_error()
    assert rows(fake, 2**30, 3, fake, 10**4, fake, 1, out) == UNS             # beyond 1e14 projections and comparisons
    assert b"cap" in lib.sd_last_error()
    assert ext(fake, 10, 2, fake, 4, None, 3, out) == INV
    assert ext(fake, 10, 2, fake, 0, fake, 3, out) == INV
    assert ext(fake, 10, 9, fake, 4, fake, 3, out) == UNS
    assert ext(fake, 2**31 - 1, 1, fake, 1, fake, 1, out) == UNS              # n + 1 points
    assert ext(fake, 10**6, 3, fake, 10**4, fake, 10**9, out) == UNS
    assert sub(fake, 10, 2, fake, 4, None, 3, 4, out) == INV
    assert sub(fake, 10, 2, fake, 4, fake, 3, 0, out) == INV
    assert sub(fake, 10, 2, fake, 0, fake, 3, 4, out) == INV
    assert sub(fake, 10, 9, fake, 4, fake, 3, 4, out) == UNS
    assert sub(fake, 10**4, 2, fake, 4, fake, 3, 2049, out) == UNS            # a block above one sort tile
    assert b"2048" in lib.sd_last_error()
    assert sub(fake, 10**7, 8, fake, 10**6, fake, 10**6, 2048, out) == UNS
    assert b"cap" in lib.sd_last_error()
    # a workspace below the floor is refused by the launcher's first check, before any launch
    floor = lib.sd_projection_min_workspace_bytes(1000, 3, 8)
    args = (fake, 1000, 3, fake, 8, None, 1000, out)
    assert lib.sd_projection_outlyingness(*args, fake, floor - 1, None) == WSP
    assert lib.sd_projection_outlyingness(*args, None, 0, None) == WSP
    assert lib.sd_projection_external_outlyingness(fake, 1000, 3, fake, 8, fake, 5, out, fake, floor - 1, None) == WSP


def test_workspace_sizes():
    _native, lib = _lib()
    for n, d, k in ((1, 1, 1), (1000, 3, 8), (10**6, 3, 1000), (2**31 - 1, 8, 5)):
        floor = lib.sd_projection_min_workspace_bytes(n, d, k)
        rec = lib.sd_projection_workspace_bytes(n, d, k)
        assert 24 * n <= floor <= rec
        assert floor <= 24 * n + 4 * (n // 2048 + 1) + 16 + 8 * 256     # one direction: about 24 bytes per point
    assert lib.sd_projection_workspace_bytes(10**6, 3, 1000) <= 256 << 20
    for bad in ((0, 3, 5), (10, 0, 5), (10, 3, 0), (2**31, 3, 5)):
        assert lib.sd_projection_workspace_bytes(*bad) == 0 and lib.sd_projection_min_workspace_bytes(*bad) == 0


def test_no_device_is_an_error_not_a_fallback():
    from statdepth_amd import PointcloudDepth
    from statdepth_amd.homogeneity import PointcloudHomogeneity
    _native, lib = _lib()
    if lib.sd_device_count() > 0:
        pytest.skip("a HIP device is visible: tests/test_projection_gpu.py covers this machine")
    rng = np.random.default_rng(1)
    df = pd.DataFrame(rng.normal(size=(12, 2)))
    with pytest.raises(RuntimeError, match='no HIP device'):
        PointcloudDepth(df, containment='projection')
    with pytest.raises(RuntimeError, match='no HIP device'):
        PointcloudDepth(df, containment='projection', K=2, directions=8)
    with pytest.raises(RuntimeError, match='no HIP device'):
        PointcloudHomogeneity(df, pd.DataFrame(rng.normal(size=(12, 2))), containment='projection').homogeneity()
