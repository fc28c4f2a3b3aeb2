"""Squared L2 distances between curves, their k-th smallest and the h-modal sums (K20) on the GPU: the distances equal the
specified recurrence in rational arithmetic bit for bit (tests/test_curve_dist_host.py), the matrix is bitwise symmetric
with a +0.0 diagonal, the selection equals np.partition of the device's own matrix in both of its modes, the h-modal sums
lie within their derived rounding bound of the 50-digit reference, nothing depends on the memory layout, the target list or
the workspace size, and the public API returns what the engine calls give."""
import functools
import math

import numpy as np
import pandas as pd
import pytest

from test_curve_dist_host import (CASES, TILE, UNDERFLOW, curves, far_curve, g_of, hmodal_bound, hmodal_reference, pairs_of,
                                  rank_of, select_np, sqdist_exact)
from test_tvd_host import two_outlier_example
from statdepth_amd import CurveDistances, FunctionalDepth, engine
from statdepth_amd._native import SD_ERR_WORKSPACE, StatdepthHipError

pytestmark = pytest.mark.gpu

WHOLE = 65                                                         # up to here the whole matrix is compared in rational arithmetic
DRAWN = 16                                                         # targets drawn above


@functools.lru_cache(maxsize=None)
def case(n, T, kind):
    """(X, the targets compared exactly, their exact rows, the device's whole matrix), computed once per case."""
    X = curves(T, n, kind)
    if n <= WHOLE:
        pick = np.arange(n)
    else:                                                           # drawn targets, the last curve (the far one) among them
        pick = np.unique(np.append(np.random.default_rng(n).choice(n - 1, DRAWN - 1, replace=False), n - 1))
    exact = sqdist_exact(X, pick)
    dev = engine.curve_sqdist(X)
    for a in (exact, dev):
        a.setflags(write=False)
    return X, pick, exact, dev


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize('n,T,kind', CASES)
def test_squared_distances(n, T, kind):
    X, pick, exact, dev = case(n, T, kind)
    assert dev.shape == (n, n) and dev.dtype == np.float64
    assert same_bits(dev[pick], exact), np.argwhere(bits(dev[pick]) != bits(exact))[:5]
    assert same_bits(dev, dev.T)                                    # bitwise symmetric
    assert not bits(dev).diagonal().any()                           # +0.0
    if kind == 'identical':
        assert not bits(dev).any()
    if kind == 'subnormal':
        assert 0 < dev.max() < 2.0 ** -1022                         # subnormal products are kept


FORMS = [(65, 5, 'rounded'), (129, 17, 'duplicated'), (129, 17, 'far'), (257, 33, 'up470'), (257, 2, 'rounded'), (1025, 3, 'down470')]


@pytest.mark.parametrize('n,T,kind', FORMS)
def test_forms_of_the_distances(n, T, kind):
    """C- and F-contiguous X, a shuffled target list with one index twice, external targets, and the workspace floor."""
    assert (n, T, kind) in CASES
    X, pick, exact, dev = case(n, T, kind)
    rng = np.random.default_rng(n + T)
    tg = rng.permutation(n)[:max(2, n // 3)]
    tg[-1] = tg[0]
    for M in (np.ascontiguousarray(X), np.asfortranarray(X)):
        cm = M.flags.f_contiguous and not M.flags.c_contiguous
        assert same_bits(engine.curve_sqdist(M, targets=tg), dev[tg])   # a target's row does not depend on the target list
        assert same_bits(engine.curve_sqdist(M), dev)
        rec, floor = engine.curve_sqdist_workspace_bytes(T, n, 'sqdist', curve_major=cm, m=len(tg))
        assert engine.curve_sqdist_targets_per_batch(T, n, floor, 'sqdist', curve_major=cm, m=len(tg)) == len(tg)
        assert same_bits(engine.curve_sqdist(M, targets=tg, ws_bytes=floor), dev[tg]) and rec == floor
        if cm:                                                      # (a time-major X needs no workspace: there is no "below")
            with pytest.raises(StatdepthHipError) as e:
                engine.curve_sqdist(M, targets=tg, ws_bytes=floor - 1)
            assert e.value.code == SD_ERR_WORKSPACE
    assert same_bits(engine.curve_sqdist_external(X, X[:, tg]), dev[tg])
    assert same_bits(engine.curve_sqdist_external(X, X[:, :1]), dev[:1])
    assert engine.curve_sqdist(X, targets=np.zeros(0, dtype=np.int64)).shape == (0, n)


def ranks_to_try(n):
    N = pairs_of(n)
    drawn = np.random.default_rng(N).integers(1, N + 1, size=5)
    return sorted({k for k in [1, 2, rank_of(0.15, n), N - 1, N, *map(int, drawn)] if 1 <= k <= N})


@pytest.mark.parametrize('n,T,kind', CASES)
def test_selection(n, T, kind):
    """The k-th smallest squared distance with the matrix stored (the recommended workspace) and recomputed in every pass
    (the floor): both equal np.partition of the device's own matrix, which test_squared_distances verifies and which no
    histogram kernel has touched; up to 65 curves also that of the exact matrix.  'rounded', 'duplicated' and 'identical'
    carry heavy ties."""
    X, pick, exact, dev = case(n, T, kind)
    rec, floor = engine.curve_sqdist_workspace_bytes(T, n, 'select')
    assert rec >= floor + 8 * n * n                                 # every shape here is stored at the recommended size
    for k in ranks_to_try(n):
        want = select_np(dev, k)
        stored = engine.curve_sqdist_select(X, k)
        again = engine.curve_sqdist_select(X, k, ws_bytes=floor)
        assert stored == want and again == want, (k, stored, again, want)
        assert math.copysign(1.0, stored) == 1.0
        if n <= WHOLE:
            assert stored == select_np(exact, k)
    F = np.asfortranarray(X)
    k = rank_of(0.5, n)
    frec, ffloor = engine.curve_sqdist_workspace_bytes(T, n, 'select', curve_major=T > 1)
    assert engine.curve_sqdist_select(F, k) == select_np(dev, k) == engine.curve_sqdist_select(F, k, ws_bytes=ffloor)
    with pytest.raises(StatdepthHipError) as e:
        engine.curve_sqdist_select(X, k, ws_bytes=floor - 1)
    assert e.value.code == SD_ERR_WORKSPACE
    for bad in (0, pairs_of(n) + 1):
        with pytest.raises(ValueError, match='pairs'):
            engine.curve_sqdist_select(X, bad)


def case_g(n, T, kind):
    """g of a case: from the type-1 quantile 0.15 of the (verified) device matrix, as the depth layer forms it."""
    return g_of(select_np(case(n, T, kind)[3], rank_of(0.15, n)))


def check_sums(S, D2_exact, g, n):
    """S against the reference on the exact squared distances; every compared sum has a term above 2^-1000."""
    ref, amax = hmodal_reference(D2_exact, g)
    assert ((D2_exact * g).min(axis=1) < 1000 * math.log(2)).all()
    for k, (got, want, a) in enumerate(zip(S, ref, amax)):
        err = abs(float(got) - want)
        assert a <= UNDERFLOW and err <= hmodal_bound(n, a) * want, (k, float(got), float(want), float(err / want), a)


@pytest.mark.parametrize('n,T,kind', [c for c in CASES if c[2] != 'identical'])
def test_hmodal_sums(n, T, kind):
    """|S - ref| <= 4 (n + a + 3) 2^-53 ref against the 50-digit sums over the exact squared distances (hmodal_bound has
    the derivation; the device exp is documented to lie within 1 ulp)."""
    X, pick, exact, dev = case(n, T, kind)
    g = case_g(n, T, kind)
    S = engine.hmodal_sums(X, g, targets=pick)
    assert S.shape == (len(pick),) and S.dtype == np.float64 and (S >= 1.0).all() and (S <= n).all()
    check_sums(S, exact, g, n)
    far = far_curve(n, kind)
    if far is not None:                                             # every other term underflows: exactly the curve's own 1.0
        assert far in pick and S[list(pick).index(far)] == 1.0
    assert same_bits(engine.hmodal_external_sums(X, X[:, pick], g), S)      # the same sums in the same order
    # external curves that are no sample curves: midpoints of pairs of them
    near = [p for p in pick if p != far]
    a, b = near[:-1][:4], near[1:][:4]
    Q = (X[:, a] + X[:, b]) / 2
    E = engine.hmodal_external_sums(X, Q, g)
    check_sums(E, sqdist_exact(np.concatenate([X, Q], axis=1), n + np.arange(Q.shape[1]))[:, :n], g, n)


def test_hmodal_sums_of_identical_curves_are_n():
    for n, T in ((9, 5), (129, 17), (300, 2)):
        X = curves(T, n, 'identical')
        assert np.array_equal(engine.hmodal_sums(X, 1.0), np.full(n, float(n)))
        assert engine.curve_sqdist_select(X, pairs_of(n)) == 0.0


@pytest.mark.parametrize('n,T,kind', FORMS)
def test_forms_of_the_sums(n, T, kind):
    """S holds the same bits for both layouts, any target list, and every workspace size between the floor and the
    recommended one that changes the targets of a batch; below the floor the library refuses."""
    X, pick, exact, dev = case(n, T, kind)
    g = case_g(n, T, kind)
    full = engine.hmodal_sums(X, g)
    rng = np.random.default_rng(n * T)
    tg = rng.permutation(n)[:max(2, n // 3)]
    tg[-1] = tg[0]
    assert same_bits(engine.hmodal_sums(X, g, targets=pick), full[pick])
    for M in (np.ascontiguousarray(X), np.asfortranarray(X)):
        cm = M.flags.f_contiguous and not M.flags.c_contiguous
        assert same_bits(engine.hmodal_sums(M, g, targets=tg), full[tg])
        rec, floor = engine.curve_sqdist_workspace_bytes(T, n, 'hmodal', curve_major=cm)
        sizes = {}
        for ws in range(floor, rec + 1, 256):
            sizes.setdefault(engine.curve_sqdist_targets_per_batch(T, n, ws, 'hmodal', curve_major=cm), ws)
        assert sizes[min(n, TILE)] == floor and sizes[n] <= rec and len(sizes) == -(-n // TILE), sizes
        assert engine.curve_sqdist_targets_per_batch(T, n, floor - 1, 'hmodal', curve_major=cm) == 0
        for per_batch, ws in sizes.items():
            assert same_bits(engine.hmodal_sums(M, g, ws_bytes=ws), full), per_batch
        with pytest.raises(StatdepthHipError) as e:
            engine.hmodal_sums(M, g, ws_bytes=floor - 1)
        assert e.value.code == SD_ERR_WORKSPACE
    efloor = engine.curve_sqdist_workspace_bytes(T, n, 'hmodal', m=len(tg))[1]
    assert same_bits(engine.hmodal_external_sums(X, X[:, tg], g, ws_bytes=efloor), full[tg])
    with pytest.raises(ValueError, match='positive and finite'):
        engine.hmodal_sums(X, 0.0)


def test_external_sums_in_several_batches():
    """External targets in more than one batch: 2 * 128 + 1 columns drawn from the sample with repeats take three batches
    at the floor and one at the recommended size, and either way a column's S holds the bits of the sample curve's."""
    n, T, kind = 129, 17, 'duplicated'
    X, pick, exact, dev = case(n, T, kind)
    g = case_g(n, T, kind)
    full = engine.hmodal_sums(X, g)
    t = np.random.default_rng(n + T).integers(0, n, size=2 * TILE + 1)
    assert len(np.unique(t)) < len(t)
    rec, floor = engine.curve_sqdist_workspace_bytes(T, n, 'hmodal', m=len(t))
    assert engine.curve_sqdist_targets_per_batch(T, n, floor, 'hmodal', m=len(t)) == TILE     # three batches
    assert engine.curve_sqdist_targets_per_batch(T, n, rec, 'hmodal', m=len(t)) == len(t)
    for ws in (floor, rec):
        assert same_bits(engine.hmodal_external_sums(X, X[:, t], g, ws_bytes=ws), full[t]), ws


def test_public_api():
    df = two_outlier_example()
    X = df.to_numpy()
    T, n = X.shape
    D2 = engine.curve_sqdist(X)
    assert same_bits(D2[[10, 20]], sqdist_exact(X, [10, 20]))
    for q in (0.15, 0.5, 1.0):
        h2 = engine.curve_sqdist_select(X, rank_of(q, n))
        assert h2 == select_np(D2, rank_of(q, n))
        res = FunctionalDepth([df], containment='hmodal') if q == 0.15 else FunctionalDepth([df], containment='hmodal', quantile=q)
        assert res.bandwidth == math.sqrt(h2)
        assert list(res.index) == list(df.columns)
        assert np.array_equal(res.to_numpy(), engine.hmodal_sums(X, 1.0 / (2.0 * h2)) / n)
        assert ((res.to_numpy() > 0) & (res.to_numpy() <= 1)).all()
    res = FunctionalDepth([df], containment='hmodal')
    assert set(res.outlying(2).index) == {'osc', 'far'}             # the ranking flags the oscillating curve
    fm = FunctionalDepth([df], containment='fm')
    assert fm['osc'] > np.median(fm.to_numpy()) and not hasattr(fm, 'bandwidth')
    part = FunctionalDepth([df], to_compute=['far', 'c3', 'osc'], containment='hmodal', bandwidth=2.5)
    assert list(part.index) == ['far', 'c3', 'osc'] and part.bandwidth == 2.5
    assert np.array_equal(part.to_numpy(), engine.hmodal_sums(X, 1.0 / (2.0 * 6.25), targets=[20, 3, 10]) / n)
    shuffled = df[list(df.columns[::-1])]
    back = FunctionalDepth([shuffled], containment='hmodal')
    assert back.bandwidth == res.bandwidth and list(back.index) == list(shuffled.columns)
    dist = CurveDistances(df)
    assert isinstance(dist, pd.DataFrame) and list(dist.index) == list(df.columns) == list(dist.columns)
    assert np.array_equal(dist.to_numpy(), np.sqrt(D2))
    some = CurveDistances([df], to_compute=['osc', 'c0'])
    assert list(some.index) == ['osc', 'c0'] and np.array_equal(some.to_numpy(), np.sqrt(D2[[10, 0]]))
    tiny = pd.DataFrame(X * 2.0 ** -530, columns=df.columns)        # the squares are subnormal: 1 / (2 h^2) overflows
    with pytest.raises(ValueError, match='too small'):
        FunctionalDepth([tiny], containment='hmodal')
