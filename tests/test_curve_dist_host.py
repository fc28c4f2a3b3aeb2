"""Squared L2 distances between curves, their k-th smallest and the h-modal depth (K20) on the host: the restatements the
GPU tests compare with (the specified recurrence in rational arithmetic, the selection by np.partition, the h-modal sums
at 50 digits), checks of the restatements themselves, the conditions of the GPU tests' case generator, the refusals that
come before any device call, and the C ABI's declarations and host-side refusals."""
import math
import os
import re
from fractions import Fraction

import mpmath
import numpy as np
import pandas as pd
import pytest

from test_tvd_host import two_outlier_example
from statdepth_amd import CurveDistances, FunctionalDepth, engine
from statdepth_amd.depth.calculations._containment import METRIC_DEPTHS, _is_metric_depth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE, COLS, CHUNK = 128, 64, 16                                    # the tile kernel's targets and sample curves per tile, timepoints per chunk

# ---- the cases of the GPU tests ----
KINDS = ('normal', 'rounded', 'duplicated', 'identical', 'up470', 'down470', 'subnormal', 'far')
# n around the tile's 64 sample curves and its 128 targets, several tiles and a part; T one above one and above two chunks
SHAPES = [(n, T) for n in (2, 3, 63, 64, 65, 127, 128, 129, 257) for T in (1, 2, 5, 17, 33)] + [(1025, 3), (4097, 2)]
# every shape with one kind, the kinds in rotation; every kind at two shapes
CASES = sorted(set([(n, T, KINDS[i % len(KINDS)]) for i, (n, T) in enumerate(SHAPES)] +
                   [(n, T, kind) for n, T in ((65, 5), (129, 17)) for kind in KINDS]))
G_MAX = 2.0 ** 1000                                                # the g of a case is capped here ('subnormal': 1 / (2 h2) overflows)
UNDERFLOW = 746.0                                                  # exp(-a) is 0.0 in fp64 for a > 745.14


def curves(T, n, kind, seed=0):
    rng = np.random.default_rng([seed, T, n, KINDS.index(kind)])
    X = rng.normal(size=(T, n))
    if kind == 'rounded':
        X = np.round(X, 1)
    elif kind == 'duplicated':                                      # 10 % of the curves are copies of other curves
        k = n // 10
        if k:
            X[:, rng.choice(n, k, replace=False)] = X[:, rng.choice(n, k)]
    elif kind == 'identical':
        X[:] = X[:, :1]
    elif kind == 'up470':
        X = X * 2.0 ** 470
    elif kind == 'down470':
        X = X * 2.0 ** -470
    elif kind == 'subnormal':                                       # every squared difference is a subnormal number or 0
        X = X * 2.0 ** -530
    elif kind == 'far':                                             # the last curve at 10^6 times the others
        X[:, n - 1] = (np.abs(X[:, n - 1]) + 1.0) * 1e6
    return X


def pairs_of(n):
    return n * (n - 1) // 2


def rank_of(q, n):
    """k of the type-1 quantile q of the distances between n curves."""
    return max(1, math.ceil(q * pairs_of(n)))


def g_of(h2):
    """g = 1 / (2 h^2) as the depth layer forms it, capped for the engine tests where it overflows."""
    return min(1.0 / (2.0 * h2), G_MAX)


# ---- the restatements ----
def sqdist_exact(X, targets=None):
    """float64 [m, n]: per pair one accumulator over ascending t, d = x - y rounded, acc = fma(d, d, acc) correctly
    rounded (a Fraction converts to the nearest double, subnormals included).  Each unordered pair is computed once."""
    X = np.asarray(X, dtype=np.float64)
    T, n = X.shape
    tg = np.arange(n) if targets is None else np.asarray(targets)
    cols = [[float(v) for v in X[:, j]] for j in range(n)]
    done = {}
    out = np.empty((len(tg), n))
    for r, i in enumerate(tg):
        i = int(i)
        for j in range(n):
            key = (i, j) if i <= j else (j, i)
            if key not in done:
                acc = 0.0
                for a, b in zip(cols[key[0]], cols[key[1]]):
                    d = Fraction(a - b)
                    acc = float(d * d + Fraction(acc))
                done[key] = acc
            out[r, j] = done[key]
    return out


def sqdist_np(X, targets=None):
    """The same recurrence in numpy with a rounded product and a rounded addition in place of the fma: within a few ulp of
    sqdist_exact, at any size.  For the conditions of the case generator, not for equality."""
    X = np.asarray(X, dtype=np.float64)
    T, n = X.shape
    tg = np.arange(n) if targets is None else np.asarray(targets)
    acc = np.zeros((len(tg), n))
    for t in range(T):
        d = X[t, tg][:, None] - X[t][None, :]
        acc += d * d
    return acc


def select_np(D2, k):
    """The k-th smallest (1-based) entry of the upper triangle of the square matrix D2."""
    v = D2[np.triu_indices(D2.shape[0], 1)]
    return float(np.partition(v, k - 1)[k - 1])


def hmodal_reference(D2, g):
    """Per row of D2 (mpf, 50 digits): sum_j exp(-(D2[j] g)) with the exact product, and a = the largest product among the
    terms that do not underflow in fp64 (0 when every term does)."""
    with mpmath.workdps(50):
        gm = mpmath.mpf(float(g))
        sums, amax = [], []
        for row in np.atleast_2d(D2):
            prods = [mpmath.mpf(float(v)) * gm for v in row]
            sums.append(mpmath.fsum(mpmath.exp(-p) for p in prods))
            amax.append(max([float(p) for p in prods if p <= UNDERFLOW], default=0.0))
        return sums, amax


def hmodal_bound(n, a):
    """|S - ref| <= 4 (n + a + 3) 2^-53 ref.  First order, all terms nonnegative: one rounding of D2 g moves a term by at
    most a u relatively, the device exp is within 1 ulp, a sum of n terms in any order adds at most (n - 1) u: n + a + 2
    with the conversion of the reference; the factor 4 is the margin."""
    return 4 * (n + a + 3) * 2.0 ** -53


def fm_depth_np(X):
    """Fraiman-Muniz depth with the "<=" empirical CDF, as containment='fm' defines it."""
    n = X.shape[1]
    F = (X[:, None, :] <= X[:, :, None]).sum(axis=2) / n
    return (1.0 - np.abs(0.5 - F)).mean(axis=0)


# ---- checks of the restatements ----
@pytest.mark.parametrize('kind', KINDS)
def test_symmetry_and_zero_diagonal(kind):
    X = curves(5, 9, kind)
    D = sqdist_exact(X)
    assert np.array_equal(D, D.T) and np.array_equal(D.view(np.uint64).diagonal(), np.zeros(9, dtype=np.uint64))
    rel = np.abs(sqdist_np(X) - D) <= 8 * 2.0 ** -53 * D + 5 * 2.0 ** -1074
    assert rel.all()
    sub = sqdist_exact(X, [7, 2, 7])
    assert np.array_equal(sub, D[[7, 2, 7]])
    if kind == 'identical':
        assert not D.any()
    if kind == 'subnormal':
        assert 0 < D.max() < 2.0 ** -1022                           # subnormal products are kept, not flushed


@pytest.mark.parametrize('T,c', [(1, 3.0), (7, 0.5), (33, 2.0 ** -20), (1000, 1.5), (5, 2.0 ** 400), (3, 2.0 ** -530)])
def test_constant_offset_gives_T_c_squared(T, c):
    """Two curves that differ by c at T points: T c^2, exact where c^2 and its multiples up to T are doubles."""
    base = np.arange(T, dtype=np.float64) * c                       # multiples of c: the differences are exact
    X = np.stack([base, base + c], axis=1)
    assert (X[:, 1] - X[:, 0] == c).all()
    D = sqdist_exact(X)
    assert D[0, 1] == D[1, 0] == T * c * c and D[0, 0] == D[1, 1] == 0.0
    assert Fraction(D[0, 1]) == T * Fraction(c) ** 2


def test_select_np_counts_ties_and_ranks():
    D = np.array([[0, 3, 1, 1], [3, 0, 2, 1], [1, 2, 0, 5], [1, 1, 5, 0]], dtype=np.float64)
    assert [select_np(D, k) for k in range(1, 7)] == [1.0, 1.0, 1.0, 2.0, 3.0, 5.0]
    assert rank_of(0.15, 4) == 1 and rank_of(0.5, 4) == 3 and rank_of(1.0, 4) == 6 and rank_of(1e-9, 2) == 1


def test_hmodal_reference_known_values():
    sums, amax = hmodal_reference(np.array([[0.0, 2.0, 4.0], [0.0, 1e6, 800.0]]), 0.5)
    assert abs(float(sums[0]) - (1 + math.exp(-1) + math.exp(-2))) < 1e-15 and amax[0] == 2.0
    assert abs(float(sums[1]) - (1 + math.exp(-400))) < 1e-15 and amax[1] == 400.0   # 5e5 underflows and does not count in a


def hmodal_depth_np(X, q=0.15):
    D = sqdist_exact(X)
    n = X.shape[1]
    g = 1.0 / (2.0 * select_np(D, rank_of(q, n)))
    sums, _ = hmodal_reference(D, g)
    return np.array([float(s) for s in sums]) / n


def test_outlying_curve_is_the_least_deep():
    rng = np.random.default_rng(11)
    X = rng.normal(size=(12, 15))
    X[:, 4] += 25.0
    depth = hmodal_depth_np(X)
    assert depth.argmin() == 4 and depth[4] == pytest.approx(1 / 15) and (depth > 0).all() and (depth <= 1).all()


def test_oscillating_curve_is_shallow_by_distance_and_unremarkable_by_rank():
    df = two_outlier_example()
    X = df.to_numpy()
    depth = pd.Series(hmodal_depth_np(X), index=df.columns)
    order = list(depth.sort_values().index)
    assert set(order[:2]) == {'osc', 'far'}                        # the two planted curves are the two shallowest
    fm = pd.Series(fm_depth_np(X), index=df.columns)
    assert fm['osc'] > fm.median()                                  # pointwise it sits in the middle of the bulk


# ---- the case generator's own conditions ----
def far_curve(n, kind):
    return n - 1 if kind == 'far' and n > 2 else None


@pytest.mark.parametrize('n,T,kind', [c for c in CASES if c[2] != 'identical'])
def test_conditions_of_the_gpu_cases(n, T, kind):
    """h2 > 0 at q = 0.15 and q = 0.5, and with the case's g (from q = 0.15) every target has an off-diagonal term above
    2^-1000, so no compared sum is made of underflowed terms only.  The one stated exception: the far curve of kind 'far'
    (n > 2), whose every other term underflows to 0.0 -- the GPU test asserts S == 1.0 exactly for it."""
    X = curves(T, n, kind)
    D = sqdist_np(X)
    h2 = select_np(D, rank_of(0.15, n))
    assert h2 > 0 and select_np(D, rank_of(0.5, n)) > 0
    g = g_of(h2)
    prod = D * g
    np.fill_diagonal(prod, np.inf)
    nearest = prod.min(axis=1)
    far = far_curve(n, kind)
    ok = nearest < 1000 * math.log(2)
    if far is not None:
        assert nearest[far] > 2 * UNDERFLOW
        ok[far] = True
    assert ok.all(), (np.flatnonzero(~ok)[:5], nearest[~ok][:5])


def test_identical_curves_have_no_bandwidth():
    X = curves(5, 9, 'identical')
    assert select_np(sqdist_exact(X), pairs_of(9)) == 0.0


# ---- refusals: raised before the engine is reached ----
@pytest.fixture
def no_engine(monkeypatch):
    def boom(*a, **k):
        raise AssertionError('the engine was reached')
    for name in ('curve_sqdist', 'curve_sqdist_external', 'curve_sqdist_select', 'hmodal_sums', 'hmodal_external_sums',
                 'to_device_matrix'):
        monkeypatch.setattr(engine, name, boom)


def _frame(T=6, n=5, seed=3):
    return pd.DataFrame(np.random.default_rng(seed).normal(size=(T, n)), columns=[f'c{i}' for i in range(n)])


def test_names():
    assert METRIC_DEPTHS == ('hmodal',) and _is_metric_depth('hmodal') and not _is_metric_depth('fm')
    assert not _is_metric_depth(lambda data, curve, relax: 0.0)
    with pytest.raises(ValueError) as e:
        FunctionalDepth([_frame()], containment='hmode')
    assert "'hmodal'" in str(e.value) and "'tvd'" in str(e.value)


@pytest.mark.parametrize('bad', [np.nan, np.inf, -np.inf, 2.0 ** 481, -2.0 ** 481])
def test_refuses_values_without_a_distance(bad, no_engine):
    df = _frame()
    df.iloc[2, 1] = bad
    with pytest.raises(ValueError, match='hmodal'):
        FunctionalDepth([df], containment='hmodal')
    with pytest.raises(ValueError, match='CurveDistances'):
        CurveDistances(df)
    df.iloc[2, 1] = math.copysign(2.0 ** 480, -1.0)                 # the largest magnitude taken: no refusal of the values
    with pytest.raises(AssertionError, match='engine was reached'):
        CurveDistances(df)


def test_refuses_what_the_rank_depths_refuse(no_engine):
    with pytest.raises(ValueError, match='univariate'):             # multivariate data
        FunctionalDepth([_frame(6, 2, s) for s in range(3)], containment='hmodal')
    for J in (3, np.int64(3), True, 2.0):
        with pytest.raises(ValueError, match='hmodal'):
            FunctionalDepth([_frame()], J=J, containment='hmodal')
    with pytest.raises(ValueError, match='at least 2 curves'):
        FunctionalDepth([_frame(6, 1)], containment='hmodal')
    with pytest.raises(ValueError, match='has no K-block estimator'):
        FunctionalDepth([_frame()], K=2, containment='hmodal')
    df = _frame()
    df.columns = ['a', 'b', 'a', 'c', 'd']
    with pytest.raises(ValueError, match='unique'):
        FunctionalDepth([df], containment='hmodal')
    with pytest.raises(ValueError, match='unique'):
        CurveDistances(df)
    with pytest.raises(ValueError, match='univariate'):
        CurveDistances([_frame(), _frame()])


@pytest.mark.parametrize('q', [0, 0.0, -0.1, 1.0000001, 2, np.nan, np.inf, '0.15', None, True])
def test_refuses_a_bad_quantile(q, no_engine):
    with pytest.raises(ValueError, match='quantile'):
        FunctionalDepth([_frame()], containment='hmodal', quantile=q)


@pytest.mark.parametrize('h', [0, 0.0, -1.0, np.inf, np.nan, '1', True])
def test_refuses_a_bad_bandwidth(h, no_engine):
    with pytest.raises(ValueError, match='bandwidth'):
        FunctionalDepth([_frame()], containment='hmodal', bandwidth=h)


def test_refuses_bandwidth_and_quantile_together(no_engine):
    with pytest.raises(ValueError, match='not both'):
        FunctionalDepth([_frame()], containment='hmodal', bandwidth=1.0, quantile=0.3)


def test_refuses_a_zero_bandwidth_of_coincident_curves(no_engine):
    X = curves(5, 9, 'identical')
    with pytest.raises(ValueError, match=r'100\.0% of the pairs'):
        FunctionalDepth([pd.DataFrame(X)], containment='hmodal')
    Y = curves(5, 10, 'normal')
    Y[:, 5:] = Y[:, :1]                                             # 6 equal curves: 15 of 45 pairs coincide
    Y[0, 7] = -0.0 if Y[0, 0] == 0 else Y[0, 7]
    with pytest.raises(ValueError, match=r'33\.3% of the pairs'):
        FunctionalDepth([pd.DataFrame(Y)], containment='hmodal', quantile=1 / 3)
    with pytest.raises(AssertionError, match='engine was reached'):  # one pair more than coincide: the device is asked
        FunctionalDepth([pd.DataFrame(Y)], containment='hmodal', quantile=16 / 45)


def test_api_on_the_restatements(monkeypatch):
    """Labels, `to_compute`, order and `.bandwidth` with the engine replaced by the restatements."""
    df = two_outlier_example()
    X = df.to_numpy()
    D = sqdist_exact(X)
    seen = {}

    def select(M, k, device=None, ws_bytes=None):
        seen['k'] = k
        return select_np(D, k)

    def sums(M, g, targets=None, device=None, ws_bytes=None):
        seen['g'] = g
        s, _ = hmodal_reference(D[np.asarray(targets)], g)
        return np.array([float(v) for v in s])

    monkeypatch.setattr(engine, 'to_device_matrix', lambda M, device=None: M)
    monkeypatch.setattr(engine, 'curve_sqdist_select', select)
    monkeypatch.setattr(engine, 'hmodal_sums', sums)
    monkeypatch.setattr(engine, 'curve_sqdist', lambda M, targets=None, device=None, ws_bytes=None: D[np.asarray(targets)])
    res = FunctionalDepth([df], containment='hmodal')
    n = X.shape[1]
    assert seen['k'] == rank_of(0.15, n) and res.bandwidth == math.sqrt(select_np(D, seen['k']))
    assert seen['g'] == 1.0 / (2.0 * select_np(D, seen['k']))
    assert list(res.index) == list(df.columns) and set(res.outlying(2).index) == {'osc', 'far'}
    assert np.allclose(res.to_numpy(), hmodal_depth_np(X), rtol=1e-14, atol=0)
    part = FunctionalDepth([df], to_compute=['far', 'c3', 'osc'], containment='hmodal', quantile=0.5)
    assert list(part.index) == ['far', 'c3', 'osc'] and seen['k'] == rank_of(0.5, n)
    given = FunctionalDepth([df], containment='hmodal', bandwidth=2.5)
    assert given.bandwidth == 2.5 and seen['g'] == 1.0 / (2.0 * 6.25)
    assert isinstance(given.ordered(), pd.Series) and given.deepest(1).index[0] in df.columns   # the Series API is undisturbed
    dist = CurveDistances(df, to_compute=['osc', 'c0'])
    assert list(dist.index) == ['osc', 'c0'] and list(dist.columns) == list(df.columns)
    assert np.array_equal(dist.to_numpy(), np.sqrt(D[[10, 0]]))
    assert np.array_equal(CurveDistances([df]).to_numpy(), np.sqrt(D))


# ---- the C ABI is declared and bound ----
ABI = [('sd_curve_sqdist_workspace_bytes', 'size_t', 6), ('sd_curve_sqdist_min_workspace_bytes', 'size_t', 6),
       ('sd_curve_sqdist_targets_per_batch', 'int64_t', 7), ('sd_curve_sqdist', 'int', 11), ('sd_curve_sqdist_external', 'int', 11),
       ('sd_curve_sqdist_select', 'int', 10), ('sd_hmodal_sums', 'int', 12), ('sd_hmodal_external_sums', 'int', 12)]


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
    base = dict(X=1, T=4, n=10, st=10, sn=1, targets=None, m=10, g=0.5, out=1, ws=None, ws_bytes=0, stream=None)
    order = ('X', 'T', 'n', 'st', 'sn', 'targets', 'm', 'g', 'out', 'ws', 'ws_bytes', 'stream')
    sums = lambda **k: lib.sd_hmodal_sums(*[{**base, **k}[a] for a in order])                       # noqa: E731
    dist = lambda **k: lib.sd_curve_sqdist(*[{**base, **k}[a] for a in order if a != 'g'])          # noqa: E731
    ext = lambda **k: lib.sd_hmodal_external_sums(*[{**base, 'targets': 1, **k}[a] for a in order])  # noqa: E731
    sel = lambda **k: lib.sd_curve_sqdist_select(*[{**base, 'k': 1, **k}[a] for a in                 # noqa: E731
                                                   ('X', 'T', 'n', 'st', 'sn', 'k', 'out', 'ws', 'ws_bytes', 'stream')])
    for call in (sums, dist, ext, sel):
        assert call(X=None) == nv.SD_ERR_INVALID and call(out=None) == nv.SD_ERR_INVALID and call(T=0) == nv.SD_ERR_INVALID
        assert call(n=1, st=1, m=1) == nv.SD_ERR_UNSUPPORTED and b'two curves' in lib.sd_last_error()
        assert call(n=2 ** 31, st=2 ** 31, m=2 ** 31) == nv.SD_ERR_UNSUPPORTED
        assert call(st=3, sn=7) == nv.SD_ERR_INVALID
    assert ext(targets=None) == nv.SD_ERR_INVALID                  # Q is required
    assert sums(m=9) == nv.SD_ERR_INVALID and dist(m=-1, targets=1) == nv.SD_ERR_INVALID
    for g in (0.0, -1.0, math.inf, math.nan):
        assert sums(g=g) == nv.SD_ERR_INVALID and ext(g=g) == nv.SD_ERR_INVALID and b'positive and finite' in lib.sd_last_error()
    for k in (0, -1, 46):
        assert sel(k=k) == nv.SD_ERR_INVALID and b'[1, 45]' in lib.sd_last_error()
    assert sums() == nv.SD_ERR_WORKSPACE and sel() == nv.SD_ERR_WORKSPACE and dist(st=1, sn=4) == nv.SD_ERR_WORKSPACE
    assert sums(n=10 ** 6, st=10 ** 6, m=10 ** 6, T=1000) == nv.SD_ERR_UNSUPPORTED and b'cap' in lib.sd_last_error()


def test_workspace_sizes_and_the_batch_plan():
    up = lambda x: -(-x // 256) * 256                              # noqa: E731
    for T, n, m in [(1, 2, 2), (7, 65, 65), (70, 300, 10), (5, 300, 300), (1000, 10000, 10000), (256, 100000, 100000)]:
        nb = -(-n // COLS)
        for cm in (False, True):
            tm = up(8 * T * n) if cm and T > 1 else 0
            assert engine.curve_sqdist_workspace_bytes(T, n, 'sqdist', cm, m) == (tm, tm)
            assert engine.curve_sqdist_targets_per_batch(T, n, tm, 'sqdist', cm, m) == m
            rec, floor = engine.curve_sqdist_workspace_bytes(T, n, 'hmodal', cm, m)
            blocks = min(-(-m // TILE), max(1, (256 << 20) // (TILE * nb * 8)))
            assert floor == tm + up(TILE * nb * 8) and rec == tm + up(blocks * TILE * nb * 8)
            assert engine.curve_sqdist_targets_per_batch(T, n, rec, 'hmodal', cm, m) == min(m, blocks * TILE)
            assert engine.curve_sqdist_targets_per_batch(T, n, floor, 'hmodal', cm, m) == min(m, TILE)
            assert engine.curve_sqdist_targets_per_batch(T, n, floor - 1, 'hmodal', cm, m) == 0
            rec, floor = engine.curve_sqdist_workspace_bytes(T, n, 'select', cm)
            slab = 8 * n * n
            assert floor == tm + 16640 and rec == floor + (up(slab) if slab <= 1 << 30 else 0)
            assert engine.curve_sqdist_targets_per_batch(T, n, floor, 'select', cm) == n
            assert engine.curve_sqdist_targets_per_batch(T, n, floor - 1, 'select', cm) == 0
    assert engine.curve_sqdist_workspace_bytes(5, 1, 'hmodal') == (0, 0) == engine.curve_sqdist_workspace_bytes(0, 5, 'select')
    assert engine.curve_sqdist_workspace_bytes(256, 100000, 'hmodal')[0] < (256 << 20) + 256       # batches, not 625 MB
    with pytest.raises(KeyError):
        engine.curve_sqdist_workspace_bytes(5, 5, 'gram')
