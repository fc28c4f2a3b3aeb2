"""Total variation depth and modified shape similarity (K17), the part that needs no GPU: the definition restated by
brute-force comparison and in exact rational arithmetic, the known values, the host normalisation against the exact
values, the public API and the two-step outlier rule over a stand-in engine, every refusal of the host layer, and the
declaration of the C entry points."""
import os
import re
from fractions import Fraction

import numpy as np
import pandas as pd
import pytest

from conftest import ROOT
from test_boxplot_host import boxplot_np
from statdepth_amd import FunctionalDepth, TotalVariationOutliers, engine
from statdepth_amd.depth.calculations._containment import ORDER_DEPTHS, RANK_DEPTHS, SHAPE_DEPTHS, _is_shape_depth
from statdepth_amd.depth.calculations._shape import _shape_depth_values
from statdepth_amd.homogeneity import FunctionalHomogeneity

U = 2.0 ** -53                                                     # unit roundoff of fp64

# four curves over three timepoints (rows are timepoints), curves 1 and 2 tied at t = 0, curves 2 and 3 at t = 1
KNOWN_X = np.array([[1.0, 2.0, 2.0, 4.0], [2.0, 1.0, 3.0, 3.0], [1.0, 3.0, 2.0, 4.0]])
KNOWN_A = np.array([[1, 3, 3, 4], [2, 1, 4, 4], [1, 3, 2, 4]], dtype=np.int64)
KNOWN_C = np.array([[1, 1, 3, 4], [1, 1, 2, 4]], dtype=np.int64)
KNOWN_SD = np.array([10, 9, 7, 0], dtype=np.int64)
KNOWN_S = [[Fraction(1, 3), Fraction(1, 9), Fraction(1), Fraction(1)], [Fraction(1, 3), Fraction(1, 9), Fraction(1), Fraction(1)]]


def tvd_counts_np(X, targets=None, chunk=1 << 22):
    """(a int64 [T, m], c int64 [T - 1, m]) by comparison: a[t, q] = #{j : X[t, j] <= X[t, q]}, c[t - 1, q] = #{j : X[t - 1, j]
    <= X[t - 1, q] and X[t, j] <= X[t, q]}, over the whole sample, for the curves `targets` (None: all).  The comparison
    matrices are formed for a block of targets at a time."""
    X = np.asarray(X, dtype=np.float64)
    T, n = X.shape
    tg = np.arange(n) if targets is None else np.asarray(targets, dtype=np.int64)
    m = len(tg)
    a = np.empty((T, m), dtype=np.int64)
    c = np.empty((max(T - 1, 0), m), dtype=np.int64)
    step = max(1, chunk // n)
    for q0 in range(0, m, step):
        q = tg[q0:q0 + step]
        prev = None
        for t in range(T):
            le = X[t][None, :] <= X[t][q][:, None]                 # [targets, curves]
            a[t, q0:q0 + step] = le.sum(axis=1)
            if t:
                c[t - 1, q0:q0 + step] = (le & prev).sum(axis=1)
            prev = le
    return a, c


def shape_terms_exact(X, targets=None):
    """Per target the exact SD (int) and SS, SN, SW (Fraction) of the definition, and the list of S_t: doubles are rationals,
    so nothing here is rounded.  S_t = 1 where its denominator is 0.  SN and SW are None for a curve with an infinite
    value."""
    X = np.asarray(X, dtype=np.float64)
    T, n = X.shape
    tg = np.arange(n) if targets is None else np.asarray(targets, dtype=np.int64)
    a, c = tvd_counts_np(X, tg)
    out = []
    for k, q in enumerate(tg):
        sd = sum(int(a[t, k]) * (n - int(a[t, k])) for t in range(T))
        S, D = [], []
        finite = bool(np.isfinite(X[:, q]).all())
        for t in range(1, T):
            a_s, a_t, ct = int(a[t - 1, k]), int(a[t, k]), int(c[t - 1, k])
            den = a_s * (n - a_s) * a_t * (n - a_t)
            num = (n * ct - a_s * a_t) ** 2
            assert den != 0 or num == 0
            S.append(Fraction(num, den) if den else Fraction(1))
            if finite:
                D.append(abs(Fraction(float(X[t, q])) - Fraction(float(X[t - 1, q]))))
        out.append(dict(SD=sd, SS=sum(S, Fraction(0)), SN=sum((d * s for d, s in zip(D, S)), Fraction(0)) if finite else None,
                        SW=sum(D, Fraction(0)) if finite else None, S=S))
    return out


def tvd_exact(X, targets=None):
    """(TVD, MSS) per target as Fractions (MSS None for T = 1; finite values)."""
    T, n = np.shape(X)
    tvd, mss = [], []
    for r in shape_terms_exact(X, targets):
        tvd.append(Fraction(r['SD'], n * n * T))
        mss.append(None if T < 2 else (r['SN'] / r['SW'] if r['SW'] > 0 else r['SS'] / (T - 1)))
    return tvd, mss


def tvd_sums_np(X, targets=None, device=None, algo='auto', ws_bytes=None, counts=False):
    """A stand-in for engine.tvd_sums: the exact sums rounded to fp64."""
    terms = shape_terms_exact(X, targets)
    sd = np.array([r['SD'] for r in terms], dtype=np.int64)
    num = lambda v: np.nan if v is None else float(v)               # noqa: E731
    shape = np.array([[float(r['SS']), num(r['SN']), num(r['SW'])] for r in terms], dtype=np.float64).reshape(-1, 3)
    return (sd, shape, tvd_counts_np(X, targets)[1].astype(np.uint32)) if counts else (sd, shape)


def parallel_family(T, n):
    return np.tile(np.arange(n, dtype=np.float64), (T, 1))


def two_outlier_example(T=24, n=21, seed=5):
    """Smooth parallel-ish curves, one that oscillates inside the bulk ('osc') and one shifted far above ('far')."""
    rng = np.random.default_rng(seed)
    t = np.linspace(0.0, 1.0, T)
    X = np.sin(2 * np.pi * t)[:, None] + np.linspace(-1.0, 1.0, n)[None, :] + 0.01 * rng.normal(size=(T, n))
    X[:, 10] = np.sin(2 * np.pi * t) + 0.45 * (-1.0) ** np.arange(T)
    X[:, 20] = np.sin(2 * np.pi * t) + 9.0
    cols = [f'c{i}' for i in range(n)]
    cols[10], cols[20] = 'osc', 'far'
    return pd.DataFrame(X, columns=cols)


# ---- the restatement ----
def test_known_answer_restated():
    a, c = tvd_counts_np(KNOWN_X)
    assert np.array_equal(a, KNOWN_A) and np.array_equal(c, KNOWN_C)
    terms = shape_terms_exact(KNOWN_X)
    assert [r['SD'] for r in terms] == list(KNOWN_SD)
    assert [[r['S'][t] for r in terms] for t in range(2)] == KNOWN_S
    tvd, mss = tvd_exact(KNOWN_X)
    assert tvd == [Fraction(10, 48), Fraction(9, 48), Fraction(7, 48), Fraction(0)]
    # curve 0 moves by 1 and 1, curve 1 by 1 and 2: equal S at both steps, so the weights do not matter; 2 and 3 have S = 1
    assert mss == [Fraction(1, 3), Fraction(1, 9), Fraction(1), Fraction(1)]


def test_counts_of_a_subset_and_chunks():
    rng = np.random.default_rng(0)
    X = np.round(rng.normal(size=(5, 37)), 1)
    a, c = tvd_counts_np(X)
    tg = np.array([36, 0, 7, 7])
    a2, c2 = tvd_counts_np(X, tg, chunk=37 * 3)
    assert np.array_equal(a2, a[:, tg]) and np.array_equal(c2, c[:, tg])
    assert a.min() >= 1 and a.max() <= 37 and (c <= np.minimum(a[:-1], a[1:])).all() and c.min() >= 1


@pytest.mark.parametrize('T,n', [(2, 2), (4, 7), (3, 64)])
def test_parallel_family(T, n):
    X = parallel_family(T, n)
    tvd, mss = tvd_exact(X)
    assert mss == [Fraction(1)] * n
    assert tvd == [Fraction((i + 1) * (n - 1 - i), n * n) for i in range(n)]
    assert max(tvd) <= Fraction(1, 4)


@pytest.mark.parametrize('n', [3, 8, 65])
def test_jump_from_the_bottom_to_second_from_the_top(n):
    X = parallel_family(4, n)
    X[2:, 0] = n - 1.5                                              # between curves n - 2 and n - 1 from step 2 on
    S = shape_terms_exact(X, [0])[0]['S']
    assert S == [Fraction(1), Fraction(1, (n - 1) ** 2), Fraction(1)]


def test_constant_curve_takes_the_plain_mean():
    X = parallel_family(3, 5)
    X[1, [0, 1]] = X[1, [1, 0]]                                     # curves 0 and 1 cross and cross back
    X[:, 2] = 2.0
    terms = shape_terms_exact(X)
    assert terms[2]['SW'] == 0
    assert tvd_exact(X)[1][2] == terms[2]['SS'] / 2


@pytest.mark.parametrize('seed', range(8))
def test_shape_similarity_lies_in_the_unit_interval(seed):
    rng = np.random.default_rng(seed)
    T, n = int(rng.integers(2, 8)), int(rng.integers(2, 30))
    X = rng.normal(size=(T, n))
    if seed % 2:
        X = np.round(X, 0)
    for r in shape_terms_exact(X):
        assert all(0 <= s <= 1 for s in r['S'])
    tvd, mss = tvd_exact(X)
    assert all(0 <= v <= Fraction(1, 4) for v in tvd) and all(0 <= v <= 1 for v in mss)


def test_names():
    assert tuple(SHAPE_DEPTHS) == ('tvd', 'mss')
    assert _is_shape_depth('tvd') and _is_shape_depth('mss') and not _is_shape_depth('fm') and not _is_shape_depth(len)
    assert tuple(ORDER_DEPTHS) == ('extremal',)
    assert tuple(RANK_DEPTHS) == ('fm', 'mei', 'mhi', 'half_region', 'integrated_halfspace', 'infimal_halfspace')


# ---- the host normalisation ----
@pytest.mark.parametrize('seed', range(6))
def test_shape_depth_values_against_the_exact_values(seed):
    """_shape_depth_values on the correctly rounded sums: TVD is one division of exact integers; MSS is one division of two
    numbers that each carry one rounding, so 3 u relative to first order (4 u asserted)."""
    rng = np.random.default_rng(seed)
    T, n = int(rng.integers(2, 9)), int(rng.integers(2, 40))
    X = rng.normal(size=(T, n))
    if seed % 3 == 1:
        X = np.round(X, 1)
    if seed % 3 == 2:
        X[:, -1] = 0.25                                             # a constant curve
    sd, shape = tvd_sums_np(X)
    tvd, mss = tvd_exact(X)
    got = _shape_depth_values(sd, shape, n, T, 'tvd')
    assert got.dtype == np.float64 and [float(v) for v in tvd] == list(got)
    got = _shape_depth_values(sd, shape, n, T, 'mss')
    for g, w in zip(got, mss):
        assert abs(Fraction(float(g)) - w) <= 4 * Fraction(U) * w


def test_shape_depth_values_refusals():
    with pytest.raises(ValueError, match='fm'):
        _shape_depth_values([1], [[1.0, 1.0, 1.0]], 2, 2, 'fm')
    with pytest.raises(ValueError, match='2 timepoints'):
        _shape_depth_values([1], [[0.0, 0.0, 0.0]], 2, 1, 'mss')
    assert list(_shape_depth_values([1], [[0.0, 0.0, 0.0]], 2, 1, 'tvd')) == [0.25]


# ---- the public API over a stand-in engine ----
def test_api_known_answer_labels_and_order(monkeypatch):
    df = pd.DataFrame(KNOWN_X, columns=['a', 'b', 'c', 'd'])
    calls = []

    def fake(X, targets=None, **kw):
        assert np.array_equal(np.asarray(X), KNOWN_X)
        calls.append(list(np.asarray(targets)))
        return tvd_sums_np(X, targets)
    monkeypatch.setattr(engine, 'tvd_sums', fake)
    d = FunctionalDepth([df], containment='tvd')
    assert list(d.index) == ['a', 'b', 'c', 'd']
    assert np.array_equal(d.to_numpy(), KNOWN_SD / 48.0)
    assert list(d.deepest(1).index) == ['a'] and list(d.outlying(1).index) == ['d']
    s = FunctionalDepth([df], containment='mss')
    assert np.allclose(s.to_numpy(), [1 / 3, 1 / 9, 1, 1], rtol=1e-15, atol=0)
    for relax in (False, True):                                    # accepted and ignored
        sub = FunctionalDepth([df], to_compute=['d', 'a', 'd'], containment='tvd', relax=relax)
        assert list(sub.index) == ['d', 'a', 'd'] and np.array_equal(sub.to_numpy(), np.array([0, 10, 0]) / 48.0)
    assert calls == [[0, 1, 2, 3], [0, 1, 2, 3], [3, 0, 3], [3, 0, 3]]
    with pytest.raises(KeyError):
        FunctionalDepth([df], to_compute=['a', 'zz'], containment='mss')


def test_tvd_accepts_one_timepoint_and_infinities(monkeypatch):
    monkeypatch.setattr(engine, 'tvd_sums', tvd_sums_np)
    d = FunctionalDepth([pd.DataFrame([[3.0, 1.0, 2.0, 2.0]], columns=list('abcd'))], containment='tvd')
    assert np.array_equal(d.to_numpy(), np.array([0, 3, 3, 3]) / 16.0)
    df = pd.DataFrame([[1.0, -np.inf, np.inf], [np.inf, 0.0, 1.0]], columns=list('abc'))
    d = FunctionalDepth([df], containment='tvd')
    assert np.array_equal(d.to_numpy(), np.array([2, 4, 2]) / 18.0)


def test_total_variation_outliers_two_step(monkeypatch):
    """One oscillating curve inside the bulk is a shape outlier and not a magnitude outlier; one shifted curve is the
    reverse.  The engine is replaced by the restatements (tvd_sums_np, test_boxplot_host.boxplot_np)."""
    df = two_outlier_example()
    monkeypatch.setattr(engine, 'tvd_sums', tvd_sums_np)

    def regions(X, level, L=None, box=None, factor=1.5, whiskers=True, device=None, outside=True, fence=True):
        return boxplot_np(X, level, L, box=box, factor=factor)
    monkeypatch.setattr(engine, 'central_regions', regions)
    r = TotalVariationOutliers(df)
    assert list(r.shape_outliers) == ['osc'] and list(r.magnitude_outliers) == ['far'] and list(r.outliers) == ['osc', 'far']
    assert list(r.mss.index) == list(df.columns) and 'osc' not in r.tvd.index and len(r.tvd) == df.shape[1] - 1
    q1, q3 = np.quantile(r.mss.to_numpy(), [0.25, 0.75])
    assert r.shape_fence == q1 - 3.0 * (q3 - q1) and r.mss['osc'] < r.shape_fence <= r.mss.drop('osc').min()
    assert list(r.boxplot.outliers) == ['far'] and r.boxplot.data.shape[1] == df.shape[1] - 1
    # the pointwise boxplot alone does not see the oscillating curve
    plain = FunctionalDepth([df], containment='tvd').boxplot()
    assert list(plain.outliers) == ['far']
    assert 'osc' in repr(r)
    # a fence that nothing passes: no shape outlier, the same magnitude outlier
    none = TotalVariationOutliers([df], shape_factor=1e6)
    assert list(none.shape_outliers) == [] and list(none.outliers) == ['far']


def test_total_variation_outliers_refusals(monkeypatch):
    df = two_outlier_example()
    monkeypatch.setattr(engine, 'tvd_sums', tvd_sums_np)
    for bad in (-1.0, np.nan, np.inf, 'x'):
        with pytest.raises(ValueError, match='shape_factor'):
            TotalVariationOutliers(df, shape_factor=bad)
    with pytest.raises(ValueError, match='exactly one DataFrame'):
        TotalVariationOutliers([df, df])
    # two curves with MSS 0 and 1 and the fence at Q1 = 0.25: one curve left for the boxplot
    two = pd.DataFrame(np.zeros((3, 2)) + np.arange(2), columns=list('ab'))

    def lopsided(X, targets=None, **kw):
        sd, shape = tvd_sums_np(X, targets)
        shape[:, 1], shape[:, 2] = [0.0, 1.0], 1.0
        return sd, shape
    monkeypatch.setattr(engine, 'tvd_sums', lopsided)
    with pytest.raises(ValueError, match='left after the shape outliers'):
        TotalVariationOutliers(two, shape_factor=0.0)


# ---- refusals: raised before the engine is reached ----
@pytest.fixture
def no_engine(monkeypatch):
    def boom(*a, **k):
        raise AssertionError('engine.tvd_sums was reached')
    monkeypatch.setattr(engine, 'tvd_sums', boom)


def _frame(T=6, n=5, seed=3):
    return pd.DataFrame(np.random.default_rng(seed).normal(size=(T, n)), columns=[f'c{i}' for i in range(n)])


@pytest.mark.parametrize('name', SHAPE_DEPTHS)
def test_refuses_what_the_rank_depths_refuse(name, no_engine):
    with pytest.raises(ValueError, match=name):                    # two frames
        FunctionalDepth([_frame(6, 2, s) for s in range(2)], containment=name)
    df = _frame()
    df.iloc[4, 2] = np.nan
    with pytest.raises(ValueError, match='NaN'):
        FunctionalDepth([df], containment=name)
    for J in (3, np.int64(3), True, 2.0):
        with pytest.raises(ValueError, match=name):
            FunctionalDepth([_frame()], J=J, containment=name)
    with pytest.raises(ValueError, match=name):
        FunctionalDepth([_frame(6, 1)], containment=name)
    with pytest.raises(ValueError, match='has no K-block estimator'):
        FunctionalDepth([_frame()], K=2, containment=name)
    df = _frame()
    df.columns = ['a', 'b', 'a', 'c', 'd']
    with pytest.raises(ValueError, match='unique'):
        FunctionalDepth([df], containment=name)
    with pytest.raises(ValueError, match=name):
        FunctionalHomogeneity([_frame(6, 5, 1)], [_frame(6, 5, 2)], containment=name, relax=True)


def test_mss_refuses_one_timepoint_and_infinities(no_engine):
    with pytest.raises(ValueError, match='2 timepoints'):
        FunctionalDepth([_frame(1, 5)], containment='mss')
    for bad in (np.inf, -np.inf):
        df = _frame()
        df.iloc[2, 1] = bad
        with pytest.raises(ValueError, match='infinite'):
            FunctionalDepth([df], containment='mss')


def test_unknown_containment_mentions_the_names():
    with pytest.raises(ValueError) as e:
        FunctionalDepth([_frame()], containment='tv')
    assert "'tvd'" in str(e.value) and "'mss'" in str(e.value) and "'fm'" in str(e.value) and "'extremal'" in str(e.value)


def test_engine_refuses_an_unknown_algo():
    with pytest.raises(ValueError, match='algo'):
        engine.tvd_workspace_bytes(3, 5, algo='merge')


# ---- the C ABI is declared and bound ----
@pytest.mark.parametrize('fn,res,count', [('sd_tvd_workspace_bytes', 'size_t', 6), ('sd_tvd_min_workspace_bytes', 'size_t', 6),
                                          ('sd_tvd_rows_per_batch', 'int64_t', 7), ('sd_tvd_sums', 'int', 14)])
def test_header_and_signatures_carry_the_entry_points(fn, res, count):
    from statdepth_amd import _native
    src = open(os.path.join(ROOT, 'include', 'statdepth_hip.h')).read()
    decl = re.search(r'\b%s\s+%s\s*\(([^;]*)\)\s*;' % (res, fn), src)
    assert decl, f'{fn} is not declared in statdepth_hip.h'
    assert len(re.sub(r'/\*.*?\*/', '', decl.group(1), flags=re.S).split(',')) == count
    got_res, args = _native.SIGNATURES[fn]
    assert len(args) == count and got_res is {'size_t': _native._sz, 'int': _native._int, 'int64_t': _native._i64}[res]


def test_signature_of_sd_tvd_sums():
    """X, T, n, st, sn, targets, m, algo, sd_sum, shape, counts, ws, ws_bytes, stream."""
    from statdepth_amd import _native as nv
    res, args = nv.SIGNATURES['sd_tvd_sums']
    assert res is nv._int
    assert args == [nv._vp, nv._i64, nv._i64, nv._i64, nv._i64, nv._vp, nv._i64, nv._int, nv._vp, nv._vp, nv._vp, nv._vp, nv._sz,
                    nv._vp]
    src = open(os.path.join(ROOT, 'include', 'statdepth_hip.h')).read()
    decl = re.search(r'int sd_tvd_sums\(([^;]*)\);', src).group(1)
    names = [p.split()[-1].lstrip('*') for p in decl.split(',')]
    assert names == ['X', 'T', 'n', 'st', 'sn', 'targets', 'm', 'algo', 'sd_sum', 'shape', 'counts', 'ws', 'ws_bytes', 'stream']
    assert 'S_t = 1' in src and 'Huang & Sun' in src                # the definition and the convention are in the header


@pytest.fixture(scope='module')
def native():
    from statdepth_amd import _native
    return _native, _native.load()


def test_abi_refusals_come_before_any_device_work(native):
    nv, lib = native
    call = lambda **k: lib.sd_tvd_sums(*[{**dict(X=1, T=4, n=10, st=10, sn=1, targets=None, m=10, algo=0, sd_sum=1, shape=1,  # noqa: E731
                                                 counts=None, ws=None, ws_bytes=0, stream=None), **k}[a] for a in
                                         ('X', 'T', 'n', 'st', 'sn', 'targets', 'm', 'algo', 'sd_sum', 'shape', 'counts', 'ws',
                                          'ws_bytes', 'stream')])
    assert call(X=None) == nv.SD_ERR_INVALID and call(shape=None) == nv.SD_ERR_INVALID and call(sd_sum=None) == nv.SD_ERR_INVALID
    assert call(T=0) == nv.SD_ERR_INVALID and call(algo=3) == nv.SD_ERR_INVALID and call(algo=-1) == nv.SD_ERR_INVALID
    assert call(n=1, st=1, m=1) == nv.SD_ERR_UNSUPPORTED and b'two curves' in lib.sd_last_error()
    # the no-fault rule: the LDS route above its capacity is refused, nothing is launched
    assert call(n=16385, st=16385, m=16385, algo=1) == nv.SD_ERR_UNSUPPORTED and b'16384' in lib.sd_last_error()
    assert call(st=3, sn=7) == nv.SD_ERR_INVALID
    assert call() == nv.SD_ERR_WORKSPACE                            # a valid shape, no workspace
    assert call(n=10 ** 6, st=10 ** 6, m=10 ** 6, T=1000, algo=2) == nv.SD_ERR_UNSUPPORTED and b'cap' in lib.sd_last_error()


def test_workspace_sizes(native):
    up = lambda x: -(-x // 256) * 256                              # noqa: E731
    for T, n, m in [(1, 2, 2), (7, 65, 65), (70, 300, 10), (1000, 10000, 10000), (2, 16384, 16384)]:
        for cm in (False, True):
            rec, floor = engine.tvd_workspace_bytes(T, n, algo='lds', curve_major=cm, m=m)
            tm = up(8 * T * n) if cm and T > 1 else 0
            krec, kfloor = engine.rank_depth_workspace_bytes(T, n, algo='image')
            rows = engine.tvd_rows_per_batch(T, n, rec, algo='lds', curve_major=cm, m=m)
            assert rows == T, (T, n, rows)                          # the recommended size takes the matrix in one batch
            assert rec == tm + up(512 * m) + up(4 * n) + up(2 * n * rows) + krec
            one = engine.tvd_rows_per_batch(T, n, floor, algo='lds', curve_major=cm, m=m)
            assert 1 <= one <= T and floor == tm + up(512 * m) + up(4 * n) + up(2 * n * one) + kfloor and floor <= rec
            assert engine.tvd_rows_per_batch(T, n, floor - 1, algo='lds', curve_major=cm, m=m) == 0
            pw = engine.tvd_workspace_bytes(T, n, algo='pairwise', curve_major=cm, m=m)
            assert pw == (tm + up(512 * m), tm + up(512 * m))
    assert engine.tvd_workspace_bytes(2, 16385, algo='lds') == (0, 0)
    assert engine.tvd_workspace_bytes(2, 16385, algo='auto') == engine.tvd_workspace_bytes(2, 16385, algo='pairwise')
    assert engine.tvd_workspace_bytes(5, 1) == (0, 0)
