"""The functional spatial depth of curves (K21) on the host: the restatement the GPU tests compare with (the specified
recurrences with every fma in rational arithmetic), the 50-digit reference of the depth, the restatement against the
reference within the derived bound, known values, the exact scale invariance of the recurrences, the condition of the
case generator that the bound rests on, the refusals that come before any device call, and the C ABI's declarations and
host-side refusals."""
import functools
import math
import os
import re
from fractions import Fraction

import mpmath
import numpy as np
import pandas as pd
import pytest

from test_curve_dist_host import KINDS, curves, sqdist_exact
from statdepth_amd import FunctionalDepth, engine
from statdepth_amd.depth.calculations._containment import METRIC_DEPTHS, SPATIAL_DEPTHS, _is_metric_depth, _is_spatial_depth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SP_TILE, SP_JK, SP_WIDE, SP_NARROW = 128, 16, 64, 32               # pass 2: targets of a tile, sample curves of a chunk, its two time tiles
SHAPES_REF = ((65, 5), (129, 17))                                  # (n, T) of the comparisons with the 50-digit reference
KINDS_REF = tuple(k for k in KINDS if k != 'subnormal')


# ---- the restatement ----
def fma(a, b, c):
    """a * b + c rounded once (a Fraction converts to the nearest double, subnormals included)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def weights_exact(D2):
    """w = 0.0 where D2 == 0.0, else 1.0 / sqrt(D2): math.sqrt and / are correctly rounded."""
    return [[0.0 if v == 0.0 else 1.0 / math.sqrt(v) for v in map(float, row)] for row in np.atleast_2d(D2)]


def spatial_exact(X, targets=None, Q=None):
    """(S float64[m], E float64[m, T]) of the definition: D2 as sqdist_exact forms it, the weights, per (target, timepoint)
    one accumulator over ascending j from +0.0, d = x[t] - X[t][j] rounded, E = fma(w[j], d, E); per target one accumulator
    over ascending t from +0.0, S = fma(E[t], E[t], S).  targets: indices of sample curves (None: all); Q: external
    targets, its columns (their distances are those of the columns appended to X)."""
    X = np.asarray(X, dtype=np.float64)
    T, n = X.shape
    if Q is not None:
        Q = np.asarray(Q, dtype=np.float64)
        D2 = sqdist_exact(np.concatenate([X, Q], axis=1), n + np.arange(Q.shape[1]))[:, :n]
        own = [[float(v) for v in Q[:, q]] for q in range(Q.shape[1])]
    else:
        tg = np.arange(n) if targets is None else np.asarray(targets)
        D2 = sqdist_exact(X, tg)
        own = [[float(v) for v in X[:, int(i)]] for i in tg]
    W = weights_exact(D2)
    rows = [[float(v) for v in X[t]] for t in range(T)]
    S, E = np.empty(len(own)), np.empty((len(own), T))
    for q, (x, w) in enumerate(zip(own, W)):
        s = 0.0
        for t in range(T):
            e = 0.0
            for wj, yj in zip(w, rows[t]):
                e = fma(wj, x[t] - yj, e)
            E[q, t] = e
            s = fma(e, e, s)
        S[q] = s
    return S, E


def depth_of(S, N):
    """The host's last step: 1 - sqrt(S) / N."""
    return 1.0 - np.sqrt(np.asarray(S, dtype=np.float64)) / N


# ---- the reference ----
def spatial_reference(X, targets=None, Q=None):
    """The depth at 50 digits, as mpf: 1 - |sum_j (x - x_j) / |x - x_j|| / N over the sample curves that differ from x in some
    entry (exactly coincident curves are skipped), N = n, or n + 1 for the columns of Q."""
    X = np.asarray(X, dtype=np.float64)
    T, n = X.shape
    with mpmath.workdps(50):
        cols = [[mpmath.mpf(float(v)) for v in X[:, j]] for j in range(n)]
        if Q is not None:
            own = [[mpmath.mpf(float(v)) for v in np.asarray(Q, dtype=np.float64)[:, q]] for q in range(np.shape(Q)[1])]
        else:
            own = [cols[int(i)] for i in (range(n) if targets is None else targets)]
        N = n if Q is None else n + 1
        out = []
        for x in own:
            e = [mpmath.mpf(0)] * T
            for y in cols:
                d = [a - b for a, b in zip(x, y)]
                r = mpmath.sqrt(mpmath.fsum(v * v for v in d))
                if r != 0:
                    e = [a + v / r for a, v in zip(e, d)]
            out.append(1 - mpmath.sqrt(mpmath.fsum(v * v for v in e)) / N)
        return out


def depth_bound(n, T):
    """|depth - ref| <= 4 (n + T + 8) 2^-53, absolute.  First order: each unit vector (x - x_j) / |x - x_j| carries about
    (T / 2 + 5) u relatively (the T fmas of D2 average T / 2, the difference, the root, the division, the product), the
    sum over j adds about n u, and sum_j |u_j| <= n, so |E| is off by about n (n + T / 2 + 5) u and the depth, |E| / n with
    the fold (T / 2 u), the root and the division, by about (n + T + 8) u; the factor 4 is the margin.  It holds where every
    nonzero squared difference is a normal number (normal_squares)."""
    return 4 * (n + T + 8) * 2.0 ** -53


def normal_squares(X):
    """Every nonzero d * d of the distances is a normal number: then each fma of D2 has a relative error of u."""
    X = np.asarray(X, dtype=np.float64)
    with np.errstate(under='ignore'):
        d = np.abs(X[:, :, None] - X[:, None, :])
    d = d[d > 0]
    return d.size == 0 or float(d.min()) >= 2.0 ** -511


@functools.lru_cache(maxsize=None)
def restated(n, T, kind):
    """(X, S, E) of the restatement for every curve of a case as a target, computed once."""
    X = curves(T, n, kind)
    S, E = spatial_exact(X)
    for a in (X, S, E):
        a.setflags(write=False)
    return X, S, E


# ---- the restatement against the reference ----
@pytest.mark.parametrize('kind', KINDS)
def test_the_condition_of_the_bound(kind):
    for n, T in SHAPES_REF:
        assert normal_squares(curves(T, n, kind)) == (kind != 'subnormal')


@pytest.mark.parametrize('n,T', SHAPES_REF)
@pytest.mark.parametrize('kind', KINDS_REF)
def test_restatement_against_the_reference(n, T, kind):
    X, S, E = restated(n, T, kind)
    assert normal_squares(X)
    depth = depth_of(S, n)
    ref = spatial_reference(X)
    err = max(abs(float(mpmath.mpf(float(d)) - r)) for d, r in zip(depth, ref))
    print(f'{kind} n={n} T={T}: largest error {err / depth_bound(n, T):.4f} of the bound')
    assert err <= depth_bound(n, T)
    assert (depth >= 0.0).all() and (depth <= 1.0).all()


# ---- known values ----
def test_two_curves_have_depth_one_half():
    """The one unit vector has norm 1: exactly where the arithmetic is exact, within the bound otherwise."""
    S, E = spatial_exact(np.array([[0.0, 1.0], [3.0, 3.0]]))
    assert np.array_equal(S, [1.0, 1.0]) and np.array_equal(depth_of(S, 2), [0.5, 0.5])
    for X in (curves(7, 2, 'normal'), curves(3, 2, 'up470'), curves(3, 2, 'down470')):
        S, E = spatial_exact(X)
        assert S[0] == S[1] and np.array_equal(E[0], -E[1])
        assert (np.abs(depth_of(S, 2) - 0.5) <= depth_bound(2, X.shape[0])).all()
        assert [float(r) for r in spatial_reference(X)] == [0.5, 0.5]


def test_identical_curves_have_depth_one():
    X = curves(5, 9, 'identical')
    S, E = spatial_exact(X)
    assert not S.any() and not E.any() and np.array_equal(depth_of(S, 9), np.ones(9))
    assert [float(r) for r in spatial_reference(X)] == [1.0] * 9


def test_three_shifted_curves():
    """x, x + c, x + 2 c: the unit vectors of the middle curve cancel exactly, the ends see two equal ones."""
    x = np.arange(8, dtype=np.float64)
    X = np.stack([x, x + 0.5, x + 1.0], axis=1)
    S, E = spatial_exact(X)
    depth = depth_of(S, 3)
    assert depth[1] == 1.0 and abs(depth[0] - (1 - 2 / 3)) <= 4 * 2.0 ** -53 and depth[0] == depth[2]


def test_a_coincident_curve_counts_in_the_sample_size_only():
    X = curves(4, 6, 'normal')
    X[:, 3] = X[:, 1]                                               # a duplicate
    S, E = spatial_exact(X)
    assert S[1] == S[3] and np.array_equal(E[1], E[3])
    others = np.delete(X, 3, axis=1)                                # without the duplicate: the same sum, one curve fewer
    S5, E5 = spatial_exact(others, [1])
    assert S5[0] == S[1] and np.array_equal(E5[0], E[1])
    ext = spatial_exact(X, Q=X[:, [1, 0]])                          # external targets equal to sample curves
    assert np.array_equal(ext[0], S[[1, 0]]) and np.array_equal(ext[1], E[[1, 0]])
    assert np.array_equal(depth_of(ext[0], 7), 1.0 - np.sqrt(S[[1, 0]]) / 7)


@pytest.mark.parametrize('n,T', SHAPES_REF)
def test_the_far_curve_has_depth_one_over_n(n, T):
    X, S, E = restated(n, T, 'far')
    depth = depth_of(S, n)
    assert abs(depth[n - 1] - 1 / n) <= 1e-6 and depth.argmin() == n - 1


@pytest.mark.parametrize('n,T', SHAPES_REF)
@pytest.mark.parametrize('kind', KINDS)
def test_depths_lie_in_the_unit_interval(n, T, kind):
    X, S, E = restated(n, T, kind)
    depth = depth_of(S, n)
    assert (depth >= 0.0).all() and (depth <= 1.0).all()
    pick = [n - 1, 0, n // 2, 0]
    sub = spatial_exact(X, pick)
    assert np.array_equal(sub[0], S[pick]) and np.array_equal(sub[1], E[pick])   # no dependence on the target list


@pytest.mark.parametrize('k', [100, -100, 470, -470])
def test_scaling_by_a_power_of_two_leaves_the_sums_bit_identical(k):
    """X 2^k: d and D2 scale exactly (by 2^k and 4^k), so does the root, the weight scales by 2^-k exactly, and w d is the
    same number: E and S hold the same bits."""
    X = curves(5, 12, 'normal')
    S, E = spatial_exact(X)
    S2, E2 = spatial_exact(X * 2.0 ** k)
    assert np.array_equal(S.view(np.uint64), S2.view(np.uint64)) and np.array_equal(E.view(np.uint64), E2.view(np.uint64))


# ---- refusals: raised before the engine is reached ----
@pytest.fixture
def no_engine(monkeypatch):
    def boom(*a, **k):
        raise AssertionError('the engine was reached')
    for name in ('spatial_sums', 'spatial_external_sums', 'curve_sqdist', 'hmodal_sums', 'to_device_matrix'):
        monkeypatch.setattr(engine, name, boom)


def _frame(T=6, n=5, seed=3):
    return pd.DataFrame(np.random.default_rng(seed).normal(size=(T, n)), columns=[f'c{i}' for i in range(n)])


def test_names():
    assert SPATIAL_DEPTHS == ('spatial',) and _is_spatial_depth('spatial') and not _is_spatial_depth('hmodal')
    assert METRIC_DEPTHS == ('hmodal',) and not _is_metric_depth('spatial')
    assert not _is_spatial_depth(lambda data, curve, relax: 0.0)
    with pytest.raises(ValueError) as e:
        FunctionalDepth([_frame()], containment='spatal')
    assert 'is invalid' in str(e.value) and "'spatial'" in str(e.value) and "'hmodal'" in str(e.value)


def test_the_depth_reaches_the_engine(no_engine):
    with pytest.raises(AssertionError, match='engine was reached'):
        FunctionalDepth([_frame()], containment='spatial')
    with pytest.raises(AssertionError, match='engine was reached'):   # `relax` has nothing to select, as for 'hmodal'
        FunctionalDepth([_frame()], containment='spatial', relax=True)


@pytest.mark.parametrize('bad', [np.nan, np.inf, -np.inf, 2.0 ** 481, -2.0 ** 481])
def test_refuses_values_without_a_distance(bad, no_engine):
    df = _frame()
    df.iloc[2, 1] = bad
    with pytest.raises(ValueError, match="containment 'spatial'"):
        FunctionalDepth([df], containment='spatial')
    df.iloc[2, 1] = math.copysign(2.0 ** 480, -1.0)                 # the largest magnitude taken
    with pytest.raises(AssertionError, match='engine was reached'):
        FunctionalDepth([df], containment='spatial')


def test_refuses_what_hmodal_refuses(no_engine):
    with pytest.raises(ValueError, match="containment 'spatial' is defined for univariate"):
        FunctionalDepth([_frame(6, 2, s) for s in range(3)], containment='spatial')
    for J in (3, np.int64(3), True, 2.0):
        with pytest.raises(ValueError, match="containment 'spatial' has no band size"):
            FunctionalDepth([_frame()], J=J, containment='spatial')
    with pytest.raises(ValueError, match="containment 'spatial' needs at least 2 curves"):
        FunctionalDepth([_frame(6, 1)], containment='spatial')
    with pytest.raises(ValueError, match="containment 'spatial' has no K-block estimator"):
        FunctionalDepth([_frame()], K=2, containment='spatial')
    df = _frame()
    df.columns = ['a', 'b', 'a', 'c', 'd']
    with pytest.raises(ValueError, match='unique'):
        FunctionalDepth([df], containment='spatial')
    with pytest.raises(ValueError, match='as a list'):
        FunctionalDepth(_frame(), containment='spatial')


@pytest.mark.parametrize('kw', [dict(quantile=0.3), dict(bandwidth=1.0), dict(quantile=0.3, bandwidth=1.0), dict(quantile=None),
                                dict(bandwidth=0.0), dict(quantile=True)])
def test_refuses_the_arguments_of_hmodal(kw, no_engine):
    with pytest.raises(ValueError, match="containment 'spatial' has no bandwidth"):
        FunctionalDepth([_frame()], containment='spatial', **kw)


def test_api_on_the_restatement(monkeypatch):
    """Labels, `to_compute`, order and the host formula with the engine replaced by the restatement."""
    df = _frame(6, 7)
    X = df.to_numpy()
    S, E = spatial_exact(X)
    seen = {}

    def sums(M, targets=None, device=None, ws_bytes=None, field=False):
        seen['targets'] = None if targets is None else list(targets)
        return S if targets is None else S[np.asarray(targets)]

    monkeypatch.setattr(engine, 'to_device_matrix', lambda M, device=None: M)
    monkeypatch.setattr(engine, 'spatial_sums', sums)
    res = FunctionalDepth([df], containment='spatial')
    assert list(res.index) == list(df.columns) and np.array_equal(res.to_numpy(), depth_of(S, 7))
    assert not hasattr(res, 'bandwidth')
    part = FunctionalDepth([df], to_compute=['c5', 'c0', 'c3'], containment='spatial')
    assert list(part.index) == ['c5', 'c0', 'c3'] and seen['targets'] == [5, 0, 3]
    assert np.array_equal(part.to_numpy(), depth_of(S[[5, 0, 3]], 7))
    assert isinstance(res.ordered(), pd.Series) and res.deepest(1).index[0] == df.columns[int(np.argmax(depth_of(S, 7)))]


# ---- the C ABI is declared and bound ----
ABI = [('sd_spatial_time_tile', 'int64_t', 3), ('sd_spatial_workspace_bytes', 'size_t', 5), ('sd_spatial_min_workspace_bytes', 'size_t', 5),
       ('sd_spatial_targets_per_batch', 'int64_t', 6), ('sd_spatial_sums', 'int', 12), ('sd_spatial_external_sums', 'int', 12)]


@pytest.mark.parametrize('fn,res,count', ABI)
def test_header_and_signatures_carry_the_entry_points(fn, res, count):
    from statdepth_amd import _native
    src = open(os.path.join(ROOT, 'include', 'statdepth_hip.h')).read()
    decl = re.search(r'\b%s\s+%s\s*\(([^;]*)\)\s*;' % (res, fn), src)
    assert decl, f'{fn} is not declared in statdepth_hip.h'
    assert len(re.sub(r'/\*.*?\*/', '', decl.group(1), flags=re.S).split(',')) == count
    got_res, args = _native.SIGNATURES[fn]
    assert len(args) == count and got_res is {'size_t': _native._sz, 'int': _native._int, 'int64_t': _native._i64}[res]
    assert args[-3:] == [_native._vp, _native._sz, _native._vp] or res != 'int'     # (ws, ws_bytes, stream) last


@pytest.fixture(scope='module')
def native():
    from statdepth_amd import _native
    return _native, _native.load()


def test_abi_refusals_come_before_any_device_work(native):
    nv, lib = native
    base = dict(X=1, T=4, n=10, st=10, sn=1, targets=None, m=10, out=1, field=None, ws=None, ws_bytes=0, stream=None)
    order = ('X', 'T', 'n', 'st', 'sn', 'targets', 'm', 'out', 'field', 'ws', 'ws_bytes', 'stream')
    sums = lambda **k: lib.sd_spatial_sums(*[{**base, **k}[a] for a in order])                        # noqa: E731
    ext = lambda **k: lib.sd_spatial_external_sums(*[{**base, 'targets': 1, **k}[a] for a in order])   # noqa: E731
    for call in (sums, ext):
        assert call(X=None) == nv.SD_ERR_INVALID and call(out=None) == nv.SD_ERR_INVALID and call(T=0) == nv.SD_ERR_INVALID
        assert call(n=1, st=1, m=1) == nv.SD_ERR_UNSUPPORTED and b'two curves' in lib.sd_last_error()
        assert call(n=2 ** 31, st=2 ** 31, m=2 ** 31) == nv.SD_ERR_UNSUPPORTED
        assert call(st=3, sn=7) == nv.SD_ERR_INVALID
        assert call() == nv.SD_ERR_WORKSPACE and b'sd_spatial_min_workspace_bytes' in lib.sd_last_error()
        assert call(ws=1, ws_bytes=engine.spatial_workspace_bytes(4, 10)[1] - 1) == nv.SD_ERR_WORKSPACE
    assert ext(targets=None) == nv.SD_ERR_INVALID                  # Q is required
    assert sums(m=9) == nv.SD_ERR_INVALID and sums(m=-1, targets=1) == nv.SD_ERR_INVALID
    assert sums(m=0, targets=1) == nv.SD_OK and ext(m=0) == nv.SD_OK   # nothing to do, no workspace asked for
    # the budget counts both passes: 2 n m T
    assert sums(n=10 ** 5, st=10 ** 5, m=10 ** 5, T=5001) == nv.SD_ERR_UNSUPPORTED and b'cap' in lib.sd_last_error()
    assert sums(n=10 ** 5, st=10 ** 5, m=10 ** 5, T=4999) == nv.SD_ERR_WORKSPACE


def test_workspace_sizes_and_the_batch_plan():
    up = lambda x: -(-x // 256) * 256                              # noqa: E731
    cap = 8 << 30                                                   # weights of a batch at the recommended size
    for T, n, m in [(1, 2, 2), (7, 65, 65), (70, 300, 10), (5, 300, 300), (1000, 10000, 10000), (256, 100000, 100000),
                    (3, 5, 2049)]:
        block = SP_TILE * 8 * (n + T)                               # weights and field of 128 targets
        for cm in (False, True):
            tm = up(8 * T * n) if cm and T > 1 else 0
            rec, floor = engine.spatial_workspace_bytes(T, n, cm, m)
            blocks = min(-(-m // SP_TILE), max(1, cap // (SP_TILE * 8 * n)))
            assert floor == tm + block and rec == tm + blocks * block
            assert engine.spatial_targets_per_batch(T, n, rec, cm, m) == min(m, blocks * SP_TILE)
            assert engine.spatial_targets_per_batch(T, n, floor, cm, m) == min(m, SP_TILE)
            assert engine.spatial_targets_per_batch(T, n, floor + block, cm, m) == min(m, min(blocks, 2) * SP_TILE)
            assert engine.spatial_targets_per_batch(T, n, floor + block - 1, cm, m) == min(m, SP_TILE)
            assert engine.spatial_targets_per_batch(T, n, floor - 1, cm, m) == 0
    assert engine.spatial_workspace_bytes(5, 1) == (0, 0) == engine.spatial_workspace_bytes(0, 5)
    assert engine.spatial_workspace_bytes(5, 9, m=0) == (SP_TILE * 8 * 14, 0)
    # 100 000 x 256: a batch of the recommended size gives the second pass two workgroups per compute unit
    per_batch = engine.spatial_targets_per_batch(256, 100000, engine.spatial_workspace_bytes(256, 100000)[0])
    assert -(-per_batch // SP_TILE) * -(-256 // SP_NARROW) >= 2 * 256
