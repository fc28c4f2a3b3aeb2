"""Total variation depth and modified shape similarity (K17) on the GPU: the counts c_t and the sums SD of both routes are
equal to the restatement by comparison (tests/test_tvd_host.py), SS, SN and SW lie within their rounding bound of the exact
rational values, the batches of the LDS route meet at their boundaries, and the public API returns the exact depths."""
from fractions import Fraction

import numpy as np
import pandas as pd
import pytest

from test_boxplot_host import boxplot_np
from test_tvd_host import shape_terms_exact, tvd_counts_np, tvd_exact, two_outlier_example
from statdepth_amd import FunctionalDepth, TotalVariationOutliers, engine
from statdepth_amd._native import SD_ERR_UNSUPPORTED, StatdepthHipError
from statdepth_amd.depth.calculations._boxplot import _region_levels

pytestmark = pytest.mark.gpu

U = Fraction(1, 2 ** 53)                                           # unit roundoff of fp64
ALGOS = ('lds', 'pairwise')
KINDS = ('normal', 'rounded', 'duplicated', 'constant_row', 'identical', 'inf', 'same_row', 'negated_row')
SHAPES = [(n, T) for n in (2, 3, 63, 64, 65, 257, 1025, 4097) for T in (2, 3, 5)] + [(16384, 2)]
EXACT_TARGETS = 192                                                # curves whose doubles are checked in rational arithmetic


def curves(T, n, kind, seed=0):
    rng = np.random.default_rng([seed, T, n, KINDS.index(kind)])
    X = rng.normal(size=(T, n))
    if kind == 'rounded':
        X = np.round(X, 1)
    elif kind == 'duplicated':                                      # 10 % of the curves are copies of other curves
        k = max(1, n // 10)
        X[:, rng.choice(n, k, replace=False)] = X[:, rng.choice(n, k)]
    elif kind == 'constant_row':
        X[T // 2] = 0.5
    elif kind == 'identical':
        X[:] = X[:, :1]
    elif kind == 'inf':
        X[rng.random(size=X.shape) < 0.15] = np.inf
        X[rng.random(size=X.shape) < 0.15] = -np.inf
    elif kind == 'same_row':
        X = np.round(X, 1)
        X[1] = X[0]
    elif kind == 'negated_row':
        X = np.round(X, 1)
        X[1] = -X[0]
    return X


def sd_of(a, n):
    return (a * (n - a)).sum(axis=0)


def check_doubles(X, shape, targets, T):
    """SS, SN, SW of `targets` (positions in `shape` = positions in `targets`) against the exact values:
    |got - exact| <= 4 (T + 4) 2^-53 exact.  All terms are non-negative; per term 1 rounding for D_t, 3 for S_t, 1 for the
    product, and a sum of T - 1 terms adds at most T - 2 more in any order: T + 4 to first order, the factor 4 is the margin.
    SN and SW are not defined for a curve with an infinite value."""
    bound = 4 * (T + 4) * U
    for k, r in enumerate(shape_terms_exact(X, targets)):
        for name, got in zip(('SS', 'SN', 'SW'), shape[k]):
            want = r[name]
            if want is None:
                continue
            err = abs(Fraction(float(got)) - want)
            assert err <= bound * want, (name, int(targets[k]), float(got), float(want), float(err / want) if want else None)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('n,T', SHAPES)
def test_counts_and_sums_of_both_routes(n, T, kind):
    X = curves(T, n, kind)
    a, c = tvd_counts_np(X)
    if kind == 'same_row':
        assert np.array_equal(c[0], np.minimum(a[0], a[1]))
    if kind == 'identical':
        assert (a == n).all() and (c == n).all()
    pick = np.arange(n) if n <= EXACT_TARGETS else np.random.default_rng(n).choice(n, EXACT_TARGETS, replace=False)
    for algo in ALGOS:
        sd, shape, counts = engine.tvd_sums(X, algo=algo, counts=True)
        assert sd.dtype == np.int64 and counts.dtype == np.uint32 and shape.shape == (n, 3)
        assert np.array_equal(counts, c), (algo, np.argwhere(counts != c)[:5])
        assert np.array_equal(sd, sd_of(a, n)), algo
        check_doubles(X, shape[pick], pick, T)
    auto = engine.tvd_sums(X)
    assert np.array_equal(auto[0], sd) and len(auto) == 2


@pytest.mark.parametrize('algo', ALGOS)
@pytest.mark.parametrize('n,T,kind', [(65, 3, 'rounded'), (257, 5, 'duplicated'), (1025, 2, 'normal'), (4097, 3, 'rounded')])
def test_forms(n, T, kind, algo):
    """Both memory layouts, a shuffled target list with one index twice, and no counts buffer."""
    X = curves(T, n, kind, seed=1)
    a, c = tvd_counts_np(X)
    rng = np.random.default_rng(n)
    tg = rng.permutation(n)[:max(2, n // 3)]
    tg[-1] = tg[0]
    ref = None
    for M in (np.ascontiguousarray(X), np.asfortranarray(X)):
        sd, shape, counts = engine.tvd_sums(M, targets=tg, algo=algo, counts=True)
        assert np.array_equal(counts, c[:, tg]) and np.array_equal(sd, sd_of(a, n)[tg])
        assert np.array_equal(sd[-1:], sd[:1]) and np.array_equal(shape[-1], shape[0])
        sd2, shape2 = engine.tvd_sums(M, targets=tg, algo=algo)     # counts = NULL
        assert np.array_equal(sd2, sd) and np.array_equal(shape2, shape)
        if ref is None:
            ref = shape
            check_doubles(X, shape[:EXACT_TARGETS], tg[:EXACT_TARGETS], T)
        assert np.array_equal(shape, ref)                           # the layout changes nothing
    full = engine.tvd_sums(X, algo=algo)[1]
    assert np.array_equal(full[tg], ref)                            # a target's sums do not depend on the target list


@pytest.mark.parametrize('curve_major', [False, True])
def test_batch_boundaries(curve_major):
    """T = 7 at n = 65 with the workspace at the floor (one row per batch), then with room for two and three rows: a row
    pair straddles every boundary; the integers -- and the doubles, each slice adding its rows in ascending order -- equal
    those of the recommended size."""
    T, n = 7, 65
    X = curves(T, n, 'rounded', seed=2)
    M = np.asfortranarray(X) if curve_major else X
    a, c = tvd_counts_np(X)
    rec, floor = engine.tvd_workspace_bytes(T, n, algo='lds', curve_major=curve_major)
    assert engine.tvd_rows_per_batch(T, n, rec, algo='lds', curve_major=curve_major) == T
    sd0, shape0, counts0 = engine.tvd_sums(M, algo='lds', counts=True)
    assert np.array_equal(counts0, c) and np.array_equal(sd0, sd_of(a, n))
    sizes = {}
    for ws in range(floor, rec + 1, 2):                             # the smallest workspace for 1, 2 and 3 rows per batch
        sizes.setdefault(engine.tvd_rows_per_batch(T, n, ws, algo='lds', curve_major=curve_major), ws)
    assert sizes[1] == floor and {1, 2, 3} <= set(sizes)
    for rows in (1, 2, 3):
        sd, shape, counts = engine.tvd_sums(M, algo='lds', counts=True, ws_bytes=sizes[rows])
        assert np.array_equal(counts, counts0) and np.array_equal(sd, sd0), rows
        assert np.array_equal(shape, shape0), rows
    with pytest.raises(StatdepthHipError):
        engine.tvd_sums(M, algo='lds', ws_bytes=floor - 1)


@pytest.mark.parametrize('curve_major', [False, True])
@pytest.mark.parametrize('n,floor_rows', [(2, 32), (5, 12)])
def test_floor_whose_image_holds_several_rows(n, floor_rows, curve_major):
    """T = 70 with so few curves that the 256-byte padding of the floor's image leaves room for more than the one row it
    is sized for (64 / n of them): stage 1 takes them all, and C has to hold what stage 1 takes.  At the floor, half-way to
    the recommended size and at it, the integers equal the model and the doubles those of the recommended size."""
    T = 70
    X = curves(T, n, 'rounded', seed=4)
    M = np.asfortranarray(X) if curve_major else X
    a, c = tvd_counts_np(X)
    shape0 = engine.tvd_sums(M, algo='lds')[1]                       # the recommended size
    rec, floor = engine.tvd_workspace_bytes(T, n, algo='lds', curve_major=curve_major)
    sizes = (floor, (floor + rec) // 2, rec)
    rows = [engine.tvd_rows_per_batch(T, n, ws, algo='lds', curve_major=curve_major) for ws in sizes]
    assert rows[0] == floor_rows > 1 and rows[0] < rows[1] <= rows[2] == T, rows
    for ws in sizes:
        sd, shape, counts = engine.tvd_sums(M, algo='lds', counts=True, ws_bytes=ws)
        assert np.array_equal(counts, c) and np.array_equal(sd, sd_of(a, n)), ws
        assert np.array_equal(shape, shape0), ws


def test_one_timepoint_gives_sd_only():
    X = curves(1, 300, 'rounded')
    a, _ = tvd_counts_np(X)
    for algo in ALGOS:
        sd, shape, counts = engine.tvd_sums(X, algo=algo, counts=True)
        assert np.array_equal(sd, sd_of(a, 300)) and not shape.any() and counts.shape == (0, 300)


def test_lds_route_above_its_capacity_is_refused():
    """The refusal only: nothing is launched."""
    with pytest.raises(StatdepthHipError) as e:
        engine.tvd_sums(np.zeros((2, 16385)), algo='lds')
    assert e.value.code == SD_ERR_UNSUPPORTED


# ---- the public API ----
@pytest.mark.parametrize('n,T,kind', [(40, 9, 'normal'), (300, 6, 'rounded'), (513, 4, 'constant_row')])
def test_functional_depth_tvd_and_mss(n, T, kind):
    X = curves(T, n, kind, seed=3)
    if kind == 'rounded':
        X[:, 7] = 0.3                                               # a constant curve: the plain mean of S_t
    df = pd.DataFrame(X, columns=[f'c{i}' for i in range(n)])
    tvd, mss = tvd_exact(X)
    d = FunctionalDepth([df], containment='tvd')
    assert list(d.index) == list(df.columns)
    assert list(d.to_numpy()) == [float(v) for v in tvd]            # one division of exact integers: correctly rounded
    s = FunctionalDepth([df], containment='mss')
    # SN / SW: numerator and denominator within 4 (T + 4) u each, plus the division
    bound = (8 * (T + 4) + 2) * U
    for g, w in zip(s.to_numpy(), mss):
        assert abs(Fraction(float(g)) - w) <= bound * w
    sub = FunctionalDepth([df], containment='mss', to_compute=['c7', 'c0', 'c7'])
    assert np.array_equal(sub.to_numpy(), s.to_numpy()[[7, 0, 7]])


def test_boxplot_of_the_tvd_result():
    df = two_outlier_example()
    d = FunctionalDepth([df], containment='tvd')
    b = d.boxplot()
    X = df.to_numpy()
    level = _region_levels(d.to_numpy(), [0.5], X.shape[1])
    env, fence, outside, whisker = boxplot_np(X, level, 1, box=0, factor=1.5)
    assert np.array_equal(b.envelope.to_numpy().T, env[0]) and np.array_equal(b.fence.to_numpy().T, fence)
    assert np.array_equal(b.outside.to_numpy(), outside) and list(b.outliers) == ['far']
    region = d.central_region(alpha=0.5)
    assert np.array_equal(region.to_numpy().T, env[0])


def test_total_variation_outliers_end_to_end():
    df = two_outlier_example()
    r = TotalVariationOutliers(df)
    assert list(r.shape_outliers) == ['osc'] and list(r.magnitude_outliers) == ['far'] and list(r.outliers) == ['osc', 'far']
    tvd, mss = tvd_exact(df.to_numpy())
    assert np.allclose(r.mss.to_numpy(), [float(v) for v in mss], rtol=1e-13, atol=0)
    rest = df.drop(columns=['osc'])
    assert list(r.tvd.to_numpy()) == [float(v) for v in tvd_exact(rest.to_numpy())[0]]
