"""Functional boxplot (K16, sd_central_regions) without a GPU: the numpy restatement of the definitions (central regions,
fence, outside counts, whiskers) against a hand-worked example, the level rule, the invariant that members of the box
region are never outliers, every refusal of the public API (raised before the engine is reached), the C ABI's refusals
and workspace sizes, and the plot helper.  tests/test_boxplot_gpu.py compares the device with `boxplot_np`."""
import math
import os
import re

import numpy as np
import pandas as pd
import pytest

from statdepth_amd import FunctionalBoxplot, engine
from statdepth_amd.depth.calculations._boxplot import FunctionalBoxplotResult, _region_levels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement ----
def levels_np(depth, alphas, n):
    """The level rule as the definition writes it."""
    order = np.argsort(-np.asarray(depth, dtype=np.float64), kind='stable')     # ties: the earlier column is deeper
    rank = np.empty(n, dtype=np.int64)
    rank[order] = np.arange(n)
    L = len(alphas)
    sizes = [min(n, max(1, math.ceil(alphas[l] * n))) for l in range(L)]
    level = np.full(n, L, dtype=np.uint8)
    for i in range(n):
        for l in range(L):
            if rank[i] < sizes[l]:
                level[i] = l
                break
    return level


def _minmax(X, members):
    """(2, T): min and max over the columns `members` (a boolean mask); +inf / -inf where there are none."""
    T = X.shape[0]
    if not members.any():
        return np.stack([np.full(T, np.inf), np.full(T, -np.inf)])
    sub = X[:, members]
    return np.stack([sub.min(axis=1), sub.max(axis=1)])


def boxplot_np(X, level, L, box=None, factor=1.5):
    """(env [L, 2, T], fence [2, T], outside int32 [n, 2], whisker [2, T]); the last three None with box=None.  Each line
    of the fence is one rounded fp64 operation."""
    X = np.asarray(X, dtype=np.float64)
    level = np.asarray(level)
    env = np.stack([_minmax(X, level <= l) for l in range(L)])
    if box is None:
        return env, None, None, None
    lower, upper = env[box]
    with np.errstate(invalid='ignore', over='ignore'):
        r = upper - lower
        w = np.float64(factor) * r
        lf = lower - w
        uf = upper + w
        below = (X < lf[:, None]).sum(axis=0)
        above = (X > uf[:, None]).sum(axis=0)
    outside = np.stack([below, above], axis=1).astype(np.int32)
    whisker = _minmax(X, (outside == 0).all(axis=1))
    return env, np.stack([lf, uf]), outside, whisker


KNOWN_X = np.array([[1.0, 2, 3, 4, 9], [2, 2, 2, 2, -7], [0, 5, 1, 3, 2]])
KNOWN_LEVEL = np.array([1, 0, 0, 1, 2], dtype=np.uint8)


def test_restatement_on_a_hand_worked_example():
    """T = 3, n = 5, L = 2, box = 0, F = 1.5.  Region 0 = curves {1, 2}, region 1 = {0, 1, 2, 3}, curve 4 in none."""
    env, fence, outside, whisker = boxplot_np(KNOWN_X, KNOWN_LEVEL, 2, box=0, factor=1.5)
    assert np.array_equal(env[0], [[2, 2, 1], [3, 2, 5]])
    assert np.array_equal(env[1], [[1, 2, 0], [4, 2, 5]])
    # widths 1, 0, 4 -> w = 1.5, 0, 6
    assert np.array_equal(fence, [[0.5, 2, -5], [4.5, 2, 11]])
    # curve 4: 9 > 4.5 at t = 0 and -7 < 2 at t = 1; nobody else leaves the fence (4 <= 4.5, ties with the fence are inside)
    assert outside.dtype == np.int32 and np.array_equal(outside, [[0, 0], [0, 0], [0, 0], [0, 0], [1, 1]])
    assert np.array_equal(whisker, [[1, 2, 0], [4, 2, 5]])
    only_env = boxplot_np(KNOWN_X, KNOWN_LEVEL, 2)
    assert np.array_equal(only_env[0], env) and only_env[1:] == (None, None, None)
    # an empty region: the identities
    e = boxplot_np(KNOWN_X, np.array([1, 1, 1, 1, 1], dtype=np.uint8), 2)[0]
    assert np.all(e[0, 0] == np.inf) and np.all(e[0, 1] == -np.inf)
    # a NaN fence flags nobody: with the box all +inf at t = 0, curve 4 keeps only its -7 < 2 at t = 1
    Xi = KNOWN_X.copy()
    Xi[0, 1:3] = np.inf
    _, f, o, _ = boxplot_np(Xi, KNOWN_LEVEL, 2, box=0, factor=1.5)
    assert np.isnan(f[:, 0]).all() and np.array_equal(o, [[0, 0], [0, 0], [0, 0], [0, 0], [1, 0]])


# ---- _region_levels ----
def test_region_levels_ties_go_by_column_order():
    depth = np.array([0.5, 0.9, 0.5, 0.9, 0.5, 0.1])
    # descending stable order: 1, 3, 0, 2, 4, 5
    assert list(_region_levels(depth, [0.5], 6)) == [0, 0, 1, 0, 1, 1]
    assert list(_region_levels(depth, [1 / 3, 2 / 3], 6)) == [1, 0, 1, 0, 2, 2]
    assert _region_levels(depth, [0.5], 6).dtype == np.uint8


def test_region_levels_size_one_and_size_n():
    depth = np.array([0.2, 0.7, 0.7, 0.1])
    assert list(_region_levels(depth, [1e-9], 4)) == [1, 0, 1, 1]          # ceil -> 1: the deepest curve alone
    assert list(_region_levels(depth, [0.25], 4)) == [1, 0, 1, 1]
    assert list(_region_levels(depth, [1.0], 4)) == [0, 0, 0, 0]
    assert list(_region_levels(depth, [0.76], 4)) == [0, 0, 0, 0]          # ceil(3.04) = 4
    assert list(_region_levels(np.array([3.0]), [0.5], 1)) == [0]


def test_region_levels_equal_sizes_leave_the_upper_level_empty():
    depth = np.array([5.0, 4, 3, 2, 1, 0, -1, -2, -3, -4])
    level = _region_levels(depth, [0.41, 0.5, 0.9], 10)                     # sizes 5, 5, 9
    assert list(level) == [0, 0, 0, 0, 0, 2, 2, 2, 2, 3]
    assert not (level == 1).any() and ((level <= 1) == (level <= 0)).all()  # region 1 is region 0
    env = boxplot_np(np.arange(20.0).reshape(2, 10), level, 3)[0]
    assert np.array_equal(env[1], env[0]) and np.array_equal(env[0], [[0, 10], [4, 14]])


@pytest.mark.parametrize('seed', range(6))
def test_region_levels_cumulative_counts_are_the_sizes(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 300))
    depth = np.round(rng.random(n), 2) if seed % 2 else rng.random(n)
    alphas = sorted(rng.random(int(rng.integers(1, 9))))
    alphas = [max(a, 1e-6) for a in alphas]
    level = _region_levels(depth, alphas, n)
    assert np.array_equal(level, levels_np(depth, alphas, n))
    for l, a in enumerate(alphas):
        assert int((level <= l).sum()) == min(n, max(1, math.ceil(a * n)))
    # a deeper curve is never at a higher level
    order = np.argsort(-depth, kind='stable')
    assert (np.diff(level[order].astype(int)) >= 0).all()


# ---- box members are never outliers ----
KINDS = ('walk', 'tenths', 'duplicated', 'constant_row', 'infinities')


def far_curves(n, seed):
    """The curves that boxplot_data scales by 8: three, fewer when n is small."""
    return np.random.default_rng(seed + 13).permutation(n)[:min(3, n // 2)]


def boxplot_data(T, n, kind, seed):
    """The data kinds of the device tests: random walks, the far curves scaled by 8."""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(T, n)).cumsum(axis=0)
    X[:, far_curves(n, seed)] *= 8
    if kind == 'tenths':
        X = np.round(X, 1)
    elif kind == 'duplicated':                                     # 10 % of the curves are copies of others
        k = max(1, n // 10)
        X[:, n - k:] = X[:, :k]
    elif kind == 'constant_row':
        X[T // 2] = 1.5
    elif kind == 'infinities':                                     # 3 % in all
        u = rng.random(size=(T, n))
        X[u < 0.015] = np.inf
        X[u > 0.985] = -np.inf
    return X


def boxplot_depth(n, seed):
    """A random depth with a third of its values rounded (ties); the far curves are the shallowest, so that they lie
    outside the box region and some of them are flagged."""
    rng = np.random.default_rng(seed + 7)
    d = rng.random(n)
    k = rng.random(n) < 1 / 3
    d[k] = np.round(d[k], 1)
    d[far_curves(n, seed)] = -1.0
    return d


ALPHAS = (0.25, 0.5, 0.75)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('factor', [0.0, 0.5, 1.5])
def test_box_members_are_never_outliers(kind, factor):
    for T, n, seed in [(1, 1, 0), (3, 4, 1), (40, 30, 2), (7, 200, 3), (25, 64, 4)]:
        X = boxplot_data(T, n, kind, seed)
        level = levels_np(boxplot_depth(n, seed), ALPHAS, n)
        for box in range(3):
            env, fence, outside, whisker = boxplot_np(X, level, 3, box=box, factor=factor)
            assert not outside[level <= box].any(), (kind, T, n, box)
            # hence the whiskers contain the box
            assert (whisker[0] <= env[box, 0]).all() and (whisker[1] >= env[box, 1]).all()


# ---- refusals of the public API: raised before the engine is reached ----
@pytest.fixture
def no_engine(monkeypatch):
    def boom(*a, **k):
        raise AssertionError('the engine was reached')
    for name in ('central_regions', 'mbd_counts', 'bd_strict_counts', 'extremal_counts', 'rank_depth_sums', 'to_device_matrix'):
        monkeypatch.setattr(engine, name, boom)


def _frame(T=6, n=5, seed=3):
    return pd.DataFrame(np.random.default_rng(seed).normal(size=(T, n)), columns=[f'c{i}' for i in range(n)])


def _depths(df, seed=1):
    return pd.Series(np.random.default_rng(seed).random(df.shape[1]), index=df.columns)


def test_refuses_more_than_one_frame(no_engine):
    with pytest.raises(ValueError, match='exactly one DataFrame'):
        FunctionalBoxplot([_frame(), _frame()], _depths(_frame()))
    with pytest.raises(ValueError, match='DataFrame'):
        FunctionalBoxplot([], _depths(_frame()))


def test_refuses_duplicate_labels(no_engine):
    df = _frame()
    d = _depths(df)
    df.columns = ['a', 'b', 'a', 'c', 'd']
    with pytest.raises(ValueError, match='unique'):
        FunctionalBoxplot(df, d)
    with pytest.raises(ValueError, match='unique'):
        FunctionalBoxplot([df])


def test_refuses_nan_in_data_or_depths(no_engine):
    df = _frame()
    bad = df.copy()
    bad.iloc[2, 1] = np.nan
    with pytest.raises(ValueError, match='NaN in the data'):
        FunctionalBoxplot(bad, _depths(df))
    with pytest.raises(ValueError, match='NaN in the data'):
        FunctionalBoxplot(bad)                                     # before the depth would be computed
    d = _depths(df)
    d.iloc[3] = np.nan
    with pytest.raises(ValueError, match='depths must not hold NaN'):
        FunctionalBoxplot(df, d)


def test_refuses_depths_that_do_not_cover_the_columns(no_engine):
    df = _frame()
    d = _depths(df)
    for wrong in (d.iloc[:4], pd.concat([d, pd.Series([0.5], index=['zz'])]), pd.concat([d.iloc[:4], d.iloc[:1]]),
                  d.rename({'c4': 'other'})):
        with pytest.raises(ValueError, match='cover every column'):
            FunctionalBoxplot(df, wrong)
    with pytest.raises(ValueError, match='Series'):
        FunctionalBoxplot(df, d.to_numpy())


@pytest.mark.parametrize('alpha,levels', [(0.0, ()), (-0.1, ()), (1.0001, ()), (float('nan'), ()), (0.5, (0.0,)),
                                          (0.5, (0.25, 1.5)), ('half', ())])
def test_refuses_fractions_outside_the_unit_interval(alpha, levels, no_engine):
    df = _frame()
    with pytest.raises(ValueError, match=r'\(0, 1\]'):
        FunctionalBoxplot(df, _depths(df), alpha=alpha, levels=levels)


def test_refuses_more_than_eight_fractions(no_engine):
    df = _frame()
    with pytest.raises(ValueError, match='at most 8'):
        FunctionalBoxplot(df, _depths(df), alpha=0.5, levels=[0.1 * k for k in range(1, 10) if k != 5])
    with pytest.raises(ValueError, match='at most 8'):
        FunctionalBoxplot(df, alpha=0.5, levels=np.linspace(0.05, 0.45, 8))


@pytest.mark.parametrize('factor', [-1.0, -1e-300, float('inf'), float('nan'), None])
def test_refuses_a_bad_factor(factor, no_engine):
    df = _frame()
    with pytest.raises(ValueError, match='factor'):
        FunctionalBoxplot(df, _depths(df), factor=factor)


def test_result_methods_refuse_the_same_way(no_engine):
    from statdepth_amd.depth.depth import _FunctionalDepthUnivariate
    df = _frame()
    res = _FunctionalDepthUnivariate(df=df, depths=_depths(df))
    with pytest.raises(ValueError, match=r'\(0, 1\]'):
        res.central_region(alpha=0.0)
    with pytest.raises(ValueError, match='factor'):
        res.boxplot(factor=-2)
    part = _FunctionalDepthUnivariate(df=df, depths=_depths(df).iloc[:3])     # a `to_compute` result
    with pytest.raises(ValueError, match='cover every column'):
        part.boxplot()
    with pytest.raises(ValueError, match='cover every column'):
        part.central_region()


def test_engine_refuses_before_the_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError('the device was reached')
    monkeypatch.setattr(engine, 'to_device_matrix', boom)
    X = np.zeros((3, 4))
    lv = np.zeros(4, dtype=np.uint8)
    with pytest.raises(ValueError, match='one byte per curve'):
        engine.central_regions(X, lv[:3])
    with pytest.raises(ValueError, match=r'\[1, 8\]'):
        engine.central_regions(X, lv, L=9)
    with pytest.raises(ValueError, match='box'):
        engine.central_regions(X, lv, L=2, box=2)
    with pytest.raises(ValueError, match='factor'):
        engine.central_regions(X, lv, L=1, box=0, factor=float('inf'))


# ---- the public API over a stand-in engine ----
def test_api_labels_index_median_and_outliers(monkeypatch):
    idx = pd.Index([10.0, 20.0, 30.0], name='time')
    df = pd.DataFrame(KNOWN_X, index=idx, columns=list('abcde'))
    depths = pd.Series([0.3, 0.9, 0.9, 0.3, 0.0], index=list('abcde')).sample(frac=1, random_state=0)   # any order
    seen = {}

    def fake(X, level, L=None, box=None, factor=1.5, whiskers=True, device=None):
        seen.update(level=np.asarray(level).copy(), L=L, box=box, factor=factor)
        return boxplot_np(X, level, L, box, factor)
    monkeypatch.setattr(engine, 'central_regions', fake)
    res = FunctionalBoxplot(df, depths, alpha=0.4, levels=(0.8,))
    assert isinstance(res, FunctionalBoxplotResult)
    assert list(seen['level']) == list(KNOWN_LEVEL) and (seen['L'], seen['box'], seen['factor']) == (2, 0, 1.5)
    assert res.median == 'b' and res.alpha == 0.4
    assert list(res.regions) == [0.4, 0.8] and res.envelope is res.regions[0.4]
    for frame in (res.envelope, res.fence, res.whiskers, res.regions[0.8]):
        assert frame.index.equals(idx) and list(frame.columns) == ['lower', 'upper']
    assert list(res.fence['lower']) == [0.5, 2, -5] and list(res.fence['upper']) == [4.5, 2, 11]
    assert list(res.outside.index) == list('abcde') and list(res.outside.columns) == ['below', 'above']
    assert list(res.outside.loc['e']) == [1, 1] and list(res.outliers) == ['e']
    assert list(res.depths.index) == list('abcde') and res.depths['b'] == 0.9
    # box drawn beside a smaller region: alpha is the second fraction
    FunctionalBoxplot([df], depths, alpha=0.8, levels=(0.4, 0.8))
    assert (seen['L'], seen['box']) == (2, 1)
    # the result object's methods use their own depths and data
    from statdepth_amd.depth.depth import _FunctionalDepthUnivariate
    own = _FunctionalDepthUnivariate(df=df, depths=depths.reindex(df.columns))
    assert list(own.boxplot(alpha=0.4, levels=(0.8,)).outliers) == ['e']
    region = own.central_region(alpha=0.4)
    assert (seen['L'], seen['box']) == (1, None)
    assert region.index.equals(idx) and list(region['lower']) == [2, 2, 1] and list(region['upper']) == [3, 2, 5]


def test_default_depth_is_the_modified_band_depth(monkeypatch):
    df = _frame(5, 6)
    asked = {}

    def fake_counts(X, targets=None, J=2, algo='auto', device=None, return_tensor=False):
        asked['relax'] = True
        return np.arange(6, dtype=np.int64)[:, None]
    monkeypatch.setattr(engine, 'mbd_counts', fake_counts)
    monkeypatch.setattr(engine, 'central_regions', lambda X, level, L=None, box=None, factor=1.5, whiskers=True, device=None:
                        boxplot_np(X, level, L, box, factor))
    res = FunctionalBoxplot([df])
    assert asked == {'relax': True} and res.median == 'c5'
    with pytest.raises(ValueError, match='no effect'):
        FunctionalBoxplot(df, _depths(df), relax=False)


def test_no_cpu_fallback():
    """Without a device the boxplot raises; there is no host path behind it."""
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    df = _frame()
    with pytest.raises(RuntimeError, match='no HIP device'):
        FunctionalBoxplot(df, _depths(df))
    with pytest.raises(RuntimeError, match='no HIP device'):
        FunctionalBoxplot([df])
    with pytest.raises(RuntimeError, match='no HIP device'):
        engine.central_regions(df.to_numpy(), np.zeros(5, dtype=np.uint8), L=1)


# ---- the C ABI ----
@pytest.fixture(scope='module')
def native():
    import __graft_entry__ as g
    g.build()
    from statdepth_amd import _native
    return _native


def _call(lib, X=1, T=10, n=10, st=10, sn=1, level=1, L=3, box=1, factor=1.5, env=1, fence=1, outside=1, whisker=1, ws=1,
          ws_bytes=1 << 40):
    return lib.sd_central_regions(X, T, n, st, sn, level, L, box, factor, env, fence, outside, whisker, ws, ws_bytes, None)


def test_abi_refusals_come_before_any_device_work(native):
    """Dummy pointers: every call below must return from the argument checks."""
    lib = native.load()
    assert lib.sd_abi_version() == 1
    inv, uns, wsp = native.SD_ERR_INVALID, native.SD_ERR_UNSUPPORTED, native.SD_ERR_WORKSPACE
    for kw in (dict(X=None), dict(level=None), dict(env=None)):
        assert _call(lib, **kw) == inv and b'null' in lib.sd_last_error()
    for kw in (dict(T=0), dict(n=0), dict(T=-3)):
        assert _call(lib, **kw) == inv and b'shape' in lib.sd_last_error()
    assert _call(lib, st=3, sn=7) == inv and b'time-major' in lib.sd_last_error()
    assert _call(lib, st=9, sn=1) == inv and b'time-major' in lib.sd_last_error()
    for L in (0, 9, -1):
        assert _call(lib, L=L, box=-1, fence=None, outside=None, whisker=None) == inv and b'L=' in lib.sd_last_error()
    for box in (-2, 3, 8):
        assert _call(lib, box=box) == inv and b'box=' in lib.sd_last_error()
    for factor in (-0.5, float('nan'), float('inf'), -float('inf')):
        assert _call(lib, factor=factor) == inv and b'factor' in lib.sd_last_error()
    for kw in (dict(outside=None, whisker=None), dict(fence=None, whisker=None), dict(fence=None, outside=None)):
        assert _call(lib, box=-1, **kw) == inv and b'envelopes only' in lib.sd_last_error()
    big = 1 << 31
    assert _call(lib, n=big, st=big) == uns and b'2^31' in lib.sd_last_error()
    assert _call(lib, T=big) == uns
    need = lib.sd_central_regions_workspace_bytes(10, 10, 10, 1, 3)
    assert need > 0
    assert _call(lib, ws_bytes=need - 1) == wsp and b'sd_central_regions_workspace_bytes' in lib.sd_last_error()
    assert _call(lib, ws=None, ws_bytes=need) == wsp
    assert _call(lib, st=1, sn=10, ws_bytes=need) == wsp           # curve-major: the time-major copy is missing


def test_abi_workspace_sizes_and_capacity(native):
    lib = native.load()
    cap = lib.sd_central_regions_row_capacity()
    assert cap >= 1024 and cap == engine.central_regions_row_capacity()
    up = lambda x: -(-x // 256) * 256                              # noqa: E731
    T = 7
    sizes = [lib.sd_central_regions_workspace_bytes(T, n, n, 1, 3) for n in
             (1, 2, 63, 64, 1000, cap - 1, cap, cap + 1, 2 * cap, 70000, 200001, 10 ** 7)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes)
    assert lib.sd_central_regions_workspace_bytes(T, cap, cap, 1, 3) == up(16 * T) + up(8 * cap)
    blocks = -(-(cap + 1) // 8192)
    assert lib.sd_central_regions_workspace_bytes(T, cap + 1, cap + 1, 1, 3) == up(16 * T) + up(8 * (cap + 1)) + up(16 * T * 3 * blocks)
    for T, n, L in [(5, 300, 1), (100, 1000, 8), (3, 70000, 2)]:
        tm = lib.sd_central_regions_workspace_bytes(T, n, n, 1, L)
        cm = lib.sd_central_regions_workspace_bytes(T, n, 1, T, L)
        assert cm >= 8 * T * n and cm == tm + up(8 * T * n)
        assert engine.central_regions_workspace_bytes(T, n, L) == tm
        assert engine.central_regions_workspace_bytes(T, n, L, curve_major=True) == cm
    for bad in [(0, 5, 5, 1, 3), (5, 0, 0, 1, 3), (5, 5, 5, 1, 0), (5, 5, 5, 1, 9), (1 << 31, 5, 5, 1, 3)]:
        assert lib.sd_central_regions_workspace_bytes(*bad) == 0


@pytest.mark.parametrize('fn,res,count', [('sd_central_regions_row_capacity', 'int64_t', 1),
                                          ('sd_central_regions_workspace_bytes', 'size_t', 5), ('sd_central_regions', 'int', 16)])
def test_header_and_signatures_carry_the_entry_points(fn, res, count):
    from statdepth_amd import _native
    src = open(os.path.join(ROOT, 'include', 'statdepth_hip.h')).read()
    decl = re.search(r'\b%s\s+%s\s*\(([^;]*)\)\s*;' % (res, fn), src)
    assert decl, f'{fn} is not declared in statdepth_hip.h'
    params = [p for p in re.sub(r'/\*.*?\*/', '', decl.group(1), flags=re.S).split(',') if p.strip() != 'void']
    got_res, args = _native.SIGNATURES[fn]
    assert len(params) == len(args) == (0 if count == 1 and fn.endswith('capacity') else count)
    assert got_res is {'size_t': _native._sz, 'int': _native._int, 'int64_t': _native._i64}[res]


# ---- the plot helper ----
def test_boxplot_figure_from_a_hand_made_result():
    import plotly.graph_objects as go
    from statdepth_amd.depth import _plotting
    idx = pd.Index([0.0, 0.5, 1.0])
    df = pd.DataFrame(KNOWN_X, index=idx, columns=list('abcde'))
    env, fence, outside, whisker = boxplot_np(KNOWN_X, KNOWN_LEVEL, 2, box=0)
    pair = lambda p: pd.DataFrame({'lower': p[0], 'upper': p[1]}, index=idx)     # noqa: E731
    regions = {0.4: pair(env[0]), 0.8: pair(env[1])}
    res = FunctionalBoxplotResult(data=df, depths=pd.Series([.3, .9, .9, .3, 0], index=df.columns), alpha=0.4, factor=1.5,
                                  median='b', envelope=regions[0.4], regions=regions, fence=pair(fence),
                                  outside=pd.DataFrame(outside, index=df.columns, columns=['below', 'above']),
                                  outliers=pd.Index(['e']), whiskers=pair(whisker))
    fig = _plotting.boxplot_figure(res, title='t', return_plot=True)
    assert isinstance(fig, go.Figure)
    assert len(fig.data) == 2 * 2 + 2 + 1 + 1                      # two bands, two whiskers, the median, one outlier
    assert fig.data[-1].name == 'e' and fig.data[-1].line.color == 'Red'
    assert fig.data[-2].name == 'median b' and list(fig.data[-2].y) == list(KNOWN_X[:, 1])
    assert fig.data[1].fill == 'tonexty' and list(fig.data[0].y) == [1, 2, 0]     # the widest band first
    same = res.plot(return_plot=True, showlegend=True)
    assert len(same.data) == len(fig.data) and same.layout.showlegend is True
    assert 'outliers=[\'e\']' in repr(res)
