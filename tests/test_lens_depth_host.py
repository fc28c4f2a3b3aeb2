"""The lens, spherical and beta-skeleton depth (K22) on the host: the restatement the GPU tests compare with (the specified
predicate in vectorised numpy, one ufunc per rounded operation), the restatement against the two-ball definition in rational
arithmetic, against the integer dot product and against the order on the line, the three forms against each other, the
exact properties of the counts (monotone in kappa, permutation, scale), the refusals that come before any device call, and
the C ABI's declarations, host-side refusals and workspace sizes."""
import functools
import math
import os
import re
from fractions import Fraction

import numpy as np
import pandas as pd
import pytest

from test_curve_dist_host import KINDS, curves, sqdist_exact
from statdepth_amd import FunctionalDepth, PointcloudDepth, engine
from statdepth_amd.depth.calculations._containment import (LENS_DEPTHS, METRIC_DEPTHS, SPATIAL_DEPTHS, _is_lens_depth,
                                                           _is_metric_depth, _is_spatial_depth)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the count kernel: targets of a block, sample curves of a tile (i and j alike), sample curves j of a chunk; the workgroups
# (half of them empty) the launcher aims for when it chooses how many tiles j one workgroup walks; the most curves
LN_TILE, LN_COLS, LN_JK, LN_GROUPS, LN_MAX_N = 128, 64, 16, 8192, 16384
LN_ROWS_MAX = 1 << 30                                              # external rows of a batch at the recommended size
KAPPAS = (1.0, 0.5, 0.0, -0.5, -1.0)                               # beta = 1, 4/3, 2, 4, inf


def pairs_of(n):
    return n * (n - 1) // 2


def lens_span(n, m):
    """Tiles of 64 sample curves j that one workgroup walks for m targets (csrc/lens_depth.hip, lens_span)."""
    nt, tb = -(-n // LN_COLS), -(-m // LN_TILE)
    return min(nt, max(1, tb * nt * nt // LN_GROUPS))


# ---- the restatement ----
def lens_counts_np(D2, A, kappa, form='general'):
    """int64[m]: per row a of A (the target's squared distances to the n sample curves) the pairs i < j with
    t1 = kappa * b; s1 = a_i + t1; t2 = kappa * a_i; s2 = b + t2; s1 <= c and s2 <= c, where b = a_j and c = D2[i][j]: one
    numpy ufunc per rounded operation.  form 'lens' (kappa == 0): a <= c and b <= c; 'sphere' (kappa == 1): a + b <= c."""
    D2 = np.asarray(D2, dtype=np.float64)
    n = D2.shape[0]
    upper = np.triu(np.ones((n, n), dtype=bool), 1)
    kappa = np.float64(kappa)
    out = np.empty(len(A), dtype=np.int64)
    with np.errstate(under='ignore'):
        for q, row in enumerate(np.asarray(A, dtype=np.float64)):
            a, b = row[:, None], row[None, :]
            if form == 'lens':
                assert kappa == 0.0
                inside = (a <= D2) & (b <= D2)
            elif form == 'sphere':
                assert kappa == 1.0
                inside = np.add(a, b) <= D2
            else:
                s1 = np.add(a, np.multiply(kappa, b))
                s2 = np.add(b, np.multiply(kappa, a))
                inside = (s1 <= D2) & (s2 <= D2)
            out[q] = np.count_nonzero(inside & upper)
    return out


def form_of(kappa):
    return 'lens' if kappa == 0.0 else 'sphere' if kappa == 1.0 else 'general'


# ---- the definitions the restatement is checked against ----
def two_ball_counts(X, kappa):
    """G of every column of the integer matrix X by the two balls of the beta-lune in Fractions: x is in the lune of (u, v)
    iff |x - (l u + (1 - l) v)| <= l |u - v| and the same with u, v swapped, l = beta / 2 = 1 / (kappa + 1); for kappa = -1
    (beta = inf) the balls are the two halfspaces 0 <= <x - u, v - u> <= |v - u|^2."""
    T, n = X.shape
    P = [[Fraction(int(v)) for v in X[:, j]] for j in range(n)]
    sq = lambda w: sum(c * c for c in w)                           # noqa: E731
    out = np.zeros(n, dtype=np.int64)
    for q in range(n):
        x = P[q]
        for i in range(n):
            for j in range(i + 1, n):
                u, v = P[i], P[j]
                if kappa == -1:
                    dot = sum((a - b) * (c - b) for a, b, c in zip(x, u, v))
                    inside = 0 <= dot <= sq([c - b for b, c in zip(u, v)])
                else:
                    lam = 1 / (Fraction(kappa) + 1)
                    r2 = lam * lam * sq([c - b for b, c in zip(u, v)])
                    inside = all(sq([a - (lam * b + (1 - lam) * c) for a, b, c in zip(x, s, t)]) <= r2 for s, t in ((u, v), (v, u)))
                out[q] += inside
    return out


def small_integers(T, n, seed):
    """Integer-valued curves of small magnitude with repeats: D2 and kappa * D2 (kappa a multiple of 1/2) are exact."""
    X = np.random.default_rng([seed, T, n]).integers(-4, 5, size=(T, n)).astype(np.float64)
    if n > 4:
        X[:, n - 1] = X[:, 1]                                      # a coincident pair
    return X


@functools.lru_cache(maxsize=None)
def exact_matrix(n, T, kind):
    X = curves(T, n, kind)
    D2 = sqdist_exact(X)
    for a in (X, D2):
        a.setflags(write=False)
    return X, D2


@pytest.mark.parametrize('kappa', KAPPAS)
@pytest.mark.parametrize('T,n', [(1, 9), (2, 14), (3, 11), (2, 2), (3, 3)])
def test_restatement_equals_the_two_ball_definition(T, n, kappa):
    X = small_integers(T, n, 1)
    D2 = sqdist_exact(X)
    assert np.array_equal(D2, np.round(D2)) and np.array_equal(D2, D2.T) and not np.diag(D2).any()
    want = two_ball_counts(X, kappa)
    assert np.array_equal(lens_counts_np(D2, D2, kappa), want)
    if form_of(kappa) != 'general':
        assert np.array_equal(lens_counts_np(D2, D2, kappa, form_of(kappa)), want)
    assert want.max() <= pairs_of(n) and (want >= n - 1).all()     # a target's own n - 1 pairs always count


@pytest.mark.parametrize('T,n', [(1, 9), (2, 14), (3, 11)])
def test_the_spherical_count_is_the_sign_of_the_dot_product(T, n):
    X = small_integers(T, n, 2).astype(np.int64)
    want = np.zeros(n, dtype=np.int64)
    for q in range(n):
        V = X - X[:, [q]]
        want[q] = np.count_nonzero(np.triu(V.T @ V <= 0, 1))
    D2 = sqdist_exact(X.astype(np.float64))
    assert np.array_equal(lens_counts_np(D2, D2, 1.0), want) and np.array_equal(lens_counts_np(D2, D2, 1.0, 'sphere'), want)


@pytest.mark.parametrize('kappa', KAPPAS + (2 / 1.5 - 1, 0.25))
def test_on_the_line_every_lune_is_the_segment(kappa):
    x = (np.random.default_rng(5).permutation(41)[:14] - 20.0)[None, :]    # distinct: see the test of coincident curves
    D2 = sqdist_exact(x)
    lo, hi = np.minimum(x[0][:, None], x[0][None, :]), np.maximum(x[0][:, None], x[0][None, :])
    want = np.array([np.count_nonzero(np.triu((lo <= v) & (v <= hi), 1)) for v in x[0]])
    assert np.array_equal(lens_counts_np(D2, D2, kappa), want)


@pytest.mark.parametrize('kind', KINDS)
def test_the_three_forms_agree(kind):
    X, D2 = exact_matrix(33, 5, kind)
    assert np.array_equal(lens_counts_np(D2, D2, 0.0), lens_counts_np(D2, D2, 0.0, 'lens'))
    assert np.array_equal(lens_counts_np(D2, D2, 1.0), lens_counts_np(D2, D2, 1.0, 'sphere'))


@pytest.mark.parametrize('kind', KINDS)
def test_counts_do_not_increase_with_kappa(kind):
    """b >= 0 and rounding is monotone: kappa * b, then a + kappa * b, do not decrease with kappa, so no pair enters."""
    X, D2 = exact_matrix(33, 5, kind)
    ks = np.sort(np.concatenate([np.linspace(-1.0, 1.0, 21), [2 / 1.5 - 1, np.nextafter(0.0, 1.0), np.nextafter(1.0, 0.0)]]))
    G = np.stack([lens_counts_np(D2, D2, k) for k in ks])
    assert (np.diff(G, axis=0) <= 0).all()
    assert (G[-1] >= 32).all() and (G[0] <= pairs_of(33)).all()


def test_a_permutation_of_the_curves_permutes_the_counts():
    X, D2 = exact_matrix(33, 5, 'duplicated')
    p = np.random.default_rng(9).permutation(33)
    Dp = sqdist_exact(X[:, p])
    assert np.array_equal(Dp, D2[np.ix_(p, p)])
    for kappa in KAPPAS:
        assert np.array_equal(lens_counts_np(Dp, Dp, kappa), lens_counts_np(D2, D2, kappa)[p])


@pytest.mark.parametrize('k', [100, -100, 240, -240])
def test_scaling_by_a_power_of_two_leaves_the_counts_unchanged(k):
    """X 2^k: D2 scales by 4^k exactly, and so do kappa * b and the sums (no operand leaves the normal range)."""
    X = curves(5, 12, 'normal')
    D2, Dk = sqdist_exact(X), sqdist_exact(X * 2.0 ** k)
    assert np.array_equal(Dk, D2 * 4.0 ** k)
    for kappa in KAPPAS + (2 / 1.5 - 1,):
        assert np.array_equal(lens_counts_np(Dk, Dk, kappa), lens_counts_np(D2, D2, kappa))


def test_identical_curves_count_every_pair():
    X, D2 = exact_matrix(33, 5, 'identical')
    assert not D2.any()
    for kappa in KAPPAS:
        assert np.array_equal(lens_counts_np(D2, D2, kappa), np.full(33, pairs_of(33)))


def test_coincident_curves_count_only_for_a_coincident_target():
    """c = 0: a + kappa a <= 0 needs a = 0 -- unless kappa = -1 (beta = inf), where the lune of a coincident pair, the slab
    between two equal hyperplanes' halfspaces 0 <= <x - u, 0> <= 0, is the whole space and the pair counts for every target."""
    X = small_integers(3, 11, 4)
    D2 = sqdist_exact(X)
    assert D2[1, 10] == 0.0
    for kappa in KAPPAS:
        inside = [bool(D2[q, 1] + kappa * D2[q, 10] <= 0.0 and D2[q, 10] + kappa * D2[q, 1] <= 0.0) for q in range(11)]
        assert inside == ([True] * 11 if kappa == -1.0 else [bool(D2[q, 1] == 0.0) for q in range(11)])
    assert two_ball_counts(X, -1.0).min() >= 1 + 10                 # that pair, and the target's own


def test_an_external_target_equal_to_a_sample_curve_gets_its_count():
    X = small_integers(3, 11, 6)
    D2 = sqdist_exact(X)
    Q = X[:, [4, 1]]
    A = sqdist_exact(np.concatenate([X, Q], axis=1), 11 + np.arange(2))[:, :11]
    for kappa in KAPPAS:
        assert np.array_equal(lens_counts_np(D2, A, kappa), lens_counts_np(D2, D2, kappa)[[4, 1]])


# ---- refusals: raised before the engine is reached ----
@pytest.fixture
def no_engine(monkeypatch):
    def boom(*a, **k):
        raise AssertionError('the engine was reached')
    for name in ('lens_counts', 'lens_external_counts', 'curve_sqdist', 'to_device_matrix'):
        monkeypatch.setattr(engine, name, boom)


def _frame(T=6, n=5, seed=3):
    return pd.DataFrame(np.random.default_rng(seed).normal(size=(T, n)), columns=[f'c{i}' for i in range(n)])


def test_names():
    assert LENS_DEPTHS == ('lens', 'spherical', 'beta_skeleton') and all(_is_lens_depth(c) for c in LENS_DEPTHS)
    assert METRIC_DEPTHS == ('hmodal',) and SPATIAL_DEPTHS == ('spatial',)
    assert not _is_lens_depth('spatial') and not _is_metric_depth('lens') and not _is_spatial_depth('spherical')
    assert not _is_lens_depth(lambda data, curve, relax: 0.0)
    with pytest.raises(ValueError) as e:
        FunctionalDepth([_frame()], containment='lense')
    assert 'is invalid' in str(e.value) and all(f"'{c}'" in str(e.value) for c in LENS_DEPTHS + ('spatial', 'hmodal'))


@pytest.mark.parametrize('containment,kw', [('lens', {}), ('spherical', {}), ('beta_skeleton', dict(beta=1.5)),
                                            ('lens', dict(relax=True))])
def test_the_depth_reaches_the_engine(containment, kw, no_engine):
    with pytest.raises(AssertionError, match='engine was reached'):
        FunctionalDepth([_frame()], containment=containment, **kw)
    if 'beta' not in kw and not kw:
        with pytest.raises(AssertionError, match='engine was reached'):
            PointcloudDepth(_frame(), containment=containment)


@pytest.mark.parametrize('containment', LENS_DEPTHS)
@pytest.mark.parametrize('bad', [np.nan, np.inf, -np.inf, 2.0 ** 481, -2.0 ** 481])
def test_refuses_values_without_a_distance(containment, bad, no_engine):
    kw = dict(beta=3) if containment == 'beta_skeleton' else {}
    df = _frame()
    df.iloc[2, 1] = bad
    with pytest.raises(ValueError, match=f"containment '{containment}'"):
        FunctionalDepth([df], containment=containment, **kw)
    if not kw:
        with pytest.raises(ValueError, match=f"containment '{containment}'"):
            PointcloudDepth(df, containment=containment)
    df.iloc[2, 1] = math.copysign(2.0 ** 480, -1.0)                 # the largest magnitude taken
    with pytest.raises(AssertionError, match='engine was reached'):
        FunctionalDepth([df], containment=containment, **kw)


@pytest.mark.parametrize('containment', LENS_DEPTHS)
def test_refuses_what_spatial_refuses(containment, no_engine):
    kw = dict(beta=3) if containment == 'beta_skeleton' else {}
    what = f"containment '{containment}'"
    with pytest.raises(ValueError, match=f'{what} is defined for univariate'):
        FunctionalDepth([_frame(6, 2, s) for s in range(3)], containment=containment, **kw)
    for J in (3, np.int64(3), True, 2.0):
        with pytest.raises(ValueError, match=f'{what} has no band size'):
            FunctionalDepth([_frame()], J=J, containment=containment, **kw)
    with pytest.raises(ValueError, match=f'{what} needs at least 2 curves'):
        FunctionalDepth([_frame(6, 1)], containment=containment, **kw)
    with pytest.raises(ValueError, match=f'{what} has no K-block estimator'):
        FunctionalDepth([_frame()], K=2, containment=containment, **kw)
    for bad in (dict(quantile=0.3), dict(bandwidth=1.0), dict(quantile=None)):
        with pytest.raises(ValueError, match=f'{what} has no bandwidth'):
            FunctionalDepth([_frame()], containment=containment, **kw, **bad)
    df = _frame()
    df.columns = ['a', 'b', 'a', 'c', 'd']
    with pytest.raises(ValueError, match='unique'):
        FunctionalDepth([df], containment=containment, **kw)
    with pytest.raises(ValueError, match=f'{what} .*at most 16384'):
        FunctionalDepth([pd.DataFrame(np.zeros((1, LN_MAX_N + 1)))], containment=containment, **kw)


def test_beta(no_engine):
    for containment in ('lens', 'spherical'):
        for beta in (2, 1, 2.0, math.inf):
            with pytest.raises(ValueError, match=f"containment '{containment}' has its beta fixed"):
                FunctionalDepth([_frame()], containment=containment, beta=beta)
    for beta in (None, 0.5, 0, -1, math.nan, True, '2', 1 - 2.0 ** -53):
        with pytest.raises(ValueError, match="containment 'beta_skeleton' takes a real beta >= 1"):
            FunctionalDepth([_frame()], containment='beta_skeleton', beta=beta)
    with pytest.raises(AssertionError, match='engine was reached'):    # every other containment ignores beta
        FunctionalDepth([_frame()], containment='spatial', beta='anything')


def test_the_point_cloud_form_refuses(no_engine):
    with pytest.raises(ValueError, match="containment 'lens' has no K-block estimator"):
        PointcloudDepth(_frame(), K=2, containment='lens')
    with pytest.raises(ValueError, match="containment 'spherical' needs at least 2 points"):
        PointcloudDepth(_frame(1, 3), containment='spherical')
    with pytest.raises(ValueError, match="containment 'beta_skeleton' needs a beta"):
        PointcloudDepth(_frame(), containment='beta_skeleton')
    with pytest.raises(ValueError, match="containment 'lens' .*at most 16384"):
        PointcloudDepth(pd.DataFrame(np.zeros((LN_MAX_N + 1, 1))), containment='lens')


def test_api_on_the_restatement(monkeypatch):
    """Labels, `to_compute`, order, kappa = 2 / beta - 1, the normaliser and attrs['beta'] with the engine replaced by the
    restatement; the point cloud is the transposed frame."""
    df = _frame(6, 7)
    X = df.to_numpy()
    D2 = sqdist_exact(X)
    seen = {}

    def counts(M, kappa, targets=None, device=None, ws_bytes=None, algo=0):
        seen.update(kappa=kappa, targets=None if targets is None else list(targets), shape=np.shape(M))
        G = lens_counts_np(D2, D2, kappa)
        return G if targets is None else G[np.asarray(targets)]

    monkeypatch.setattr(engine, 'to_device_matrix', lambda M, device=None: M)
    monkeypatch.setattr(engine, 'lens_counts', counts)
    for containment, beta, kappa in [('lens', None, 0.0), ('spherical', None, 1.0), ('beta_skeleton', 1.5, 2.0 / 1.5 - 1.0),
                                     ('beta_skeleton', math.inf, -1.0), ('beta_skeleton', 2, 0.0), ('beta_skeleton', 1, 1.0),
                                     ('beta_skeleton', np.float64(4.0), -0.5)]:
        res = FunctionalDepth([df], containment=containment, beta=beta)
        G = lens_counts_np(D2, D2, kappa)
        assert seen['kappa'] == kappa and type(seen['kappa']) is float and seen['shape'] == (6, 7)
        assert list(res.index) == list(df.columns) and np.array_equal(res.to_numpy(), G / 21.0)
        assert res.attrs['beta'] == (beta if beta is not None else {'lens': 2.0, 'spherical': 1.0}[containment])
        part = FunctionalDepth([df], to_compute=['c5', 'c0', 'c3'], containment=containment, beta=beta)
        assert list(part.index) == ['c5', 'c0', 'c3'] and seen['targets'] == [5, 0, 3]
        assert np.array_equal(part.to_numpy(), G[[5, 0, 3]] / 21.0)
        assert isinstance(res.ordered(), pd.Series) and res.deepest(1).index[0] == df.columns[int(np.argmax(G))]
    cloud = df.T                                                    # 7 points of R^6
    for containment, kappa in (('lens', 0.0), ('spherical', 1.0)):
        res = PointcloudDepth(cloud, containment=containment)
        G = lens_counts_np(D2, D2, kappa)
        assert seen['kappa'] == kappa and seen['shape'] == (6, 7)
        assert list(res.index) == list(cloud.index) and np.array_equal(res.to_numpy(), G / 21.0)
        assert res.attrs['beta'] == 2.0 - kappa
        part = PointcloudDepth(cloud, to_compute=['c6', 'c2'], containment=containment)
        assert list(part.index) == ['c6', 'c2'] and seen['targets'] == [6, 2] and np.array_equal(part.to_numpy(), G[[6, 2]] / 21.0)


def test_engine_refuses_a_kappa_outside_the_unit_interval(no_engine):
    for kappa in (1.0000001, -1.5, math.nan, math.inf):
        with pytest.raises(ValueError, match='kappa'):
            engine._kappa(kappa)
    assert engine._kappa(np.float64(-1.0)) == -1.0 and engine._kappa(1) == 1.0


# ---- the C ABI is declared and bound ----
ABI = [('sd_lens_workspace_bytes', 'size_t', 5), ('sd_lens_min_workspace_bytes', 'size_t', 5), ('sd_lens_targets_per_batch', 'int64_t', 6),
       ('sd_lens_counts', 'int', 13), ('sd_lens_external_counts', 'int', 13)]


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
    if res == 'int':
        assert args[7:9] == [_native._dbl, _native._int]            # kappa, algo


@pytest.fixture(scope='module')
def native():
    from statdepth_amd import _native
    return _native, _native.load()


def test_abi_refusals_come_before_any_device_work(native):
    nv, lib = native
    base = dict(X=1, T=4, n=10, st=10, sn=1, targets=None, m=10, kappa=0.0, algo=0, out=1, ws=None, ws_bytes=0, stream=None)
    order = ('X', 'T', 'n', 'st', 'sn', 'targets', 'm', 'kappa', 'algo', 'out', 'ws', 'ws_bytes', 'stream')
    counts = lambda **k: lib.sd_lens_counts(*[{**base, **k}[a] for a in order])                        # noqa: E731
    ext = lambda **k: lib.sd_lens_external_counts(*[{**base, 'targets': 1, **k}[a] for a in order])    # noqa: E731
    for call in (counts, ext):
        assert call(X=None) == nv.SD_ERR_INVALID and call(out=None) == nv.SD_ERR_INVALID and call(T=0) == nv.SD_ERR_INVALID
        assert call(n=0, st=1) == nv.SD_ERR_INVALID
        for kappa in (math.nan, 1.0000001, -1.0000001, math.inf, -math.inf):
            assert call(kappa=kappa) == nv.SD_ERR_INVALID and b'kappa' in lib.sd_last_error()
        for algo in (-1, 2):
            assert call(algo=algo) == nv.SD_ERR_INVALID and b'algo' in lib.sd_last_error()
        # what is invalid is named before what is unsupported
        assert call(n=1, st=1, m=1, kappa=2.0) == nv.SD_ERR_INVALID and call(n=LN_MAX_N + 1, st=LN_MAX_N + 1, algo=3) == nv.SD_ERR_INVALID
        assert call(n=1, st=1, m=1) == nv.SD_ERR_UNSUPPORTED and b'two curves' in lib.sd_last_error()
        n = LN_MAX_N + 1
        assert call(n=n, st=n, m=n) == nv.SD_ERR_UNSUPPORTED and b'16384' in lib.sd_last_error()
        assert call(n=2 ** 31, st=2 ** 31, m=2 ** 31) == nv.SD_ERR_UNSUPPORTED
        assert call(T=2 ** 31) == nv.SD_ERR_UNSUPPORTED
        assert call(st=3, sn=7) == nv.SD_ERR_INVALID
        for kappa in (-1.0, 0.0, 0.5, 1.0):                        # taken: the refusal is the workspace's
            for algo in (0, 1):
                assert call(kappa=kappa, algo=algo) == nv.SD_ERR_WORKSPACE and b'sd_lens_min_workspace_bytes' in lib.sd_last_error()
        assert call(ws=1, ws_bytes=engine.lens_workspace_bytes(4, 10)[1] - 1) == nv.SD_ERR_WORKSPACE
        assert call(n=LN_MAX_N, st=LN_MAX_N, m=LN_MAX_N) == nv.SD_ERR_WORKSPACE
    assert ext(targets=None) == nv.SD_ERR_INVALID                  # Q is required
    assert counts(m=9) == nv.SD_ERR_INVALID and counts(m=-1, targets=1) == nv.SD_ERR_INVALID and ext(m=-1) == nv.SD_ERR_INVALID
    assert counts(m=0, targets=1) == nv.SD_OK and ext(m=0) == nv.SD_OK   # nothing to do, no workspace asked for
    # the budget counts the matrix and the targets' rows: n (n + m) T
    n = LN_MAX_N
    assert counts(n=n, st=n, m=n, T=186265) == nv.SD_ERR_UNSUPPORTED and b'cap' in lib.sd_last_error()
    assert counts(n=n, st=n, m=n, T=186264) == nv.SD_ERR_WORKSPACE
    assert ext(n=n, st=n, m=3 * n, T=93133) == nv.SD_ERR_UNSUPPORTED and ext(n=n, st=n, m=3 * n, T=93132) == nv.SD_ERR_WORKSPACE


def test_workspace_sizes_and_the_batch_plan():
    up = lambda x: -(-x // 256) * 256                              # noqa: E731
    for T, n, m in [(1, 2, 2), (7, 65, 65), (70, 300, 10), (5, 300, 300), (1000, 10000, 10000), (3, 5, 2049), (2, LN_MAX_N, 10 ** 6),
                    (4, 1000, 200000)]:
        block = LN_TILE * 8 * n                                     # the rows of 128 external targets
        for cm in (False, True):
            tm = up(8 * T * n) if cm and T > 1 else 0
            rec, floor = engine.lens_workspace_bytes(T, n, cm, m)
            blocks = min(-(-m // LN_TILE), max(1, LN_ROWS_MAX // block))
            assert floor == tm + up(8 * n * n) + block and rec == tm + up(8 * n * n) + blocks * block and floor <= rec
            assert engine.lens_targets_per_batch(T, n, rec, cm, m) == min(m, blocks * LN_TILE)
            assert engine.lens_targets_per_batch(T, n, floor, cm, m) == min(m, LN_TILE)
            assert engine.lens_targets_per_batch(T, n, floor + block, cm, m) == min(m, min(blocks, 2) * LN_TILE)
            assert engine.lens_targets_per_batch(T, n, floor + block - 1, cm, m) == min(m, LN_TILE)
            assert engine.lens_targets_per_batch(T, n, floor - 1, cm, m) == 0
    assert engine.lens_workspace_bytes(5, 1) == (0, 0) == engine.lens_workspace_bytes(0, 5)
    assert engine.lens_workspace_bytes(5, LN_MAX_N + 1) == (0, 0) == engine.lens_workspace_bytes(2 ** 31, 5)
    assert engine.lens_workspace_bytes(5, 9, m=-1) == (0, 0)
    assert engine.lens_workspace_bytes(5, 9, m=0) == (up(8 * 81) + LN_TILE * 8 * 9, 0)
    assert engine.lens_targets_per_batch(5, LN_MAX_N + 1, 1 << 40) == 0


def test_the_span_rule_restated_here():
    """What the GPU tests rely on to reach a workgroup that walks more than one tile of sample curves j."""
    assert lens_span(129, 129) == 1 and lens_span(1025, 1025) == 1
    assert lens_span(129, LN_TILE * 1821) == 2 and lens_span(129, LN_TILE * 1820) == 1
    assert lens_span(10000, 10000) == 157 and lens_span(4096, 4096) == 16
