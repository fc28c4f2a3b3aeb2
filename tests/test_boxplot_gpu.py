"""Functional boxplot on the GPU (K16, sd_central_regions) against the numpy restatement of tests/test_boxplot_host.py:
envelopes, fence and whiskers equal as fp64 values (NaN where the restatement has NaN; the sign of a zero is not
specified), the outside counts equal as int32 -- over the data kinds, the shapes at which the kernels change path, both
memory layouts, the special rows, the outputs left out, and the public API."""
import functools

import numpy as np
import pandas as pd
import pytest

from test_boxplot_host import ALPHAS, KINDS, KNOWN_LEVEL, KNOWN_X, boxplot_data, boxplot_depth, boxplot_np, levels_np

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from statdepth_amd import engine
    return engine


def _same(got, want, what=""):
    """Device output against the restatement: (env, fence, outside, whisker), None where not asked for."""
    for name, g, w in zip(("env", "fence", "outside", "whisker"), got, want):
        if w is None or g is None:
            assert g is None and w is None, (what, name)
        elif name == "outside":
            assert g.dtype == np.int32 and g.shape == w.shape and np.array_equal(g, w), (what, name)
        else:
            assert g.dtype == np.float64 and g.shape == w.shape and np.array_equal(g, w, equal_nan=True), (what, name)


@functools.lru_cache(maxsize=None)
def _case(T, n, kind):
    """(X, level, the restatement with ALPHAS and box = 1), computed once per case and not modified."""
    seed = 100 * T + n
    X = boxplot_data(T, n, kind, seed)
    level = _levels(n, seed)
    want = boxplot_np(X, level, 3, box=1, factor=1.5)
    for a in (X,) + want:
        a.setflags(write=False)
    return X, level, want


@functools.lru_cache(maxsize=None)
def _levels(n, seed):
    """Levels from a random depth with ties, ALPHAS = (0.25, 0.5, 0.75)."""
    level = levels_np(boxplot_depth(n, seed), ALPHAS, n)
    level.setflags(write=False)
    return level


def _layout(X, order):
    return np.asfortranarray(X) if order == "F" else np.ascontiguousarray(X)


SHAPES = [(1, 1), (1, 2), (3, 4),                                  # smallest
          (7, 64), (33, 257), (17, 1025), (5, 4097),              # wave and workgroup edges
          (9, 513), (5, 2049), (3, 8193),                          # ... and the other values-per-thread variants (2, 8, 16 at 576 threads)
          (2, "cap"), (2, "cap+1"),                                # the route boundary
          (3, 70000), (5, 200001),                                 # ragged column blocks
          (2500, 5)]                                               # more rows than workgroups: the row loop, the counts


@pytest.mark.parametrize("order", ["C", "F"])
@pytest.mark.parametrize("T,n", SHAPES, ids=lambda v: str(v))
def test_matches_the_restatement(eng, T, n, order):
    cap = eng.central_regions_row_capacity()
    n = {"cap": cap, "cap+1": cap + 1}.get(n, n)
    flagged = 0
    for kind in KINDS:
        X, level, want = _case(T, n, kind)
        got = eng.central_regions(_layout(X, order), level, L=3, box=1, factor=1.5)
        _same(got, want, (T, n, kind, order))
        flagged += int((want[2] != 0).any())
    if T >= 17 and n >= 64:
        assert flagged, "the cases are meant to flag somebody"


def test_hand_worked_example(eng):
    env, fence, outside, whisker = eng.central_regions(KNOWN_X, KNOWN_LEVEL, L=2, box=0, factor=1.5)
    assert np.array_equal(env, [[[2, 2, 1], [3, 2, 5]], [[1, 2, 0], [4, 2, 5]]])
    assert np.array_equal(fence, [[0.5, 2, -5], [4.5, 2, 11]])
    assert np.array_equal(outside, [[0, 0], [0, 0], [0, 0], [0, 0], [1, 1]])
    assert np.array_equal(whisker, [[1, 2, 0], [4, 2, 5]])


@pytest.mark.parametrize("n", [40, 5000, 20000])
def test_box_region_all_plus_inf_gives_a_nan_fence(eng, n):
    X, level, _ = _case(6, n, "walk")
    X = X.copy()
    X[2, level <= 1] = np.inf                                      # the whole box region
    X[4, np.flatnonzero(level <= 1)[0]] = np.inf                   # a finite lower and a +inf upper
    want = boxplot_np(X, level, 3, box=1, factor=1.5)
    assert np.isnan(want[1][:, 2]).all() and want[1][0, 4] == -np.inf and want[1][1, 4] == np.inf
    for order in "CF":
        got = eng.central_regions(_layout(X, order), level, L=3, box=1, factor=1.5)
        _same(got, want, (n, order))
        assert np.isnan(got[1][:, 2]).all() and got[1][0, 4] == -np.inf and got[1][1, 4] == np.inf
    # nobody is flagged at those two rows: the counts are those of the other rows
    rest = np.delete(X, [2, 4], axis=0)
    assert np.array_equal(got[2], boxplot_np(rest, level, 3, box=1, factor=1.5)[2])


@pytest.mark.parametrize("T,n", [(9, 300), (4, 20000)])
def test_outputs_left_out_do_not_change_the_others(eng, T, n):
    X, level, want = _case(T, n, "tenths")
    full = eng.central_regions(X, level, L=3, box=1)
    _same(full, want)
    env, fence, outside, whisker = full
    got = eng.central_regions(X, level, L=3, box=None)             # box = -1: envelopes only
    _same(got, (env, None, None, None), "box=None")
    got = eng.central_regions(X, level, L=3, box=1, whiskers=False)
    _same(got, (env, fence, outside, None), "whiskers=False")
    got = eng.central_regions(X, level, L=3, box=1, outside=False)  # the counts stay in the workspace
    _same(got, (env, fence, None, whisker), "outside=False")
    got = eng.central_regions(X, level, L=3, box=1, outside=False, fence=False)
    _same(got, (env, None, None, whisker), "whisker alone")
    got = eng.central_regions(X, level, L=3, box=1, whiskers=False, outside=False, fence=False)
    _same(got, (env, None, None, None), "nothing but env")
    got = eng.central_regions(X, level, L=3, box=1, whiskers=False, fence=False)
    _same(got, (env, None, outside, None), "counts alone")


@pytest.mark.parametrize("T,n", [(9, 300), (4, 20000)])
def test_level_counts(eng, T, n):
    X, _, _ = _case(T, n, "walk")
    depth = boxplot_depth(n, T)
    # an empty exact level with L = 2: both fractions give the same size
    level = levels_np(depth, (0.5 - 0.1 / n, 0.5), n)
    assert not (level == 1).any()
    for box in (0, 1):
        _same(eng.central_regions(X, level, L=2, box=box), boxplot_np(X, level, 2, box=box), ("empty level", box))
    # L = 1 and L = 8; a level byte above L is in no region
    level = levels_np(depth, (0.3,), n)
    _same(eng.central_regions(X, level, L=1, box=0), boxplot_np(X, level, 1, box=0), "L=1")
    wide = np.where(level == 1, 200, 0).astype(np.uint8)
    _same(eng.central_regions(X, wide, L=1, box=0), boxplot_np(X, level, 1, box=0), "byte above L")
    alphas = (0.05, 0.1, 0.2, 0.3, 0.5, 0.7, 0.9, 1.0)
    level = levels_np(depth, alphas, n)
    for box in (0, 4, 7):
        _same(eng.central_regions(X, level, L=8, box=box, factor=0.5), boxplot_np(X, level, 8, box=box, factor=0.5), ("L=8", box))
    # the default L: one region per level present
    level = levels_np(depth, (0.25, 0.5), n)
    assert eng.central_regions(X, level)[0].shape == (3, 2, T)
    _same(eng.central_regions(X, level), boxplot_np(X, level, 3), "default L")


@pytest.mark.parametrize("T,n", [(3000, 6), (3000, 2000), (400, 17000)])
def test_a_curve_outside_everywhere_counts_every_timepoint(eng, T, n):
    rng = np.random.default_rng(n)
    X = rng.normal(size=(T, n))
    X[:, 3] = 1e6
    X[:, 4] = -1e6
    level = np.ones(n, dtype=np.uint8)
    level[[0, 1, 2, 5]] = 0
    for order in "CF":
        env, fence, outside, whisker = eng.central_regions(_layout(X, order), level, L=1, box=0)
        assert list(outside[3]) == [0, T] and list(outside[4]) == [T, 0]
        _same((env, fence, outside, whisker), boxplot_np(X, level, 1, box=0), (n, order))


@pytest.mark.parametrize("T,n", [(50, 700), (6, 20000)])
def test_factor_zero_and_a_large_factor(eng, T, n):
    X, level, _ = _case(T, n, "walk")
    got = eng.central_regions(X, level, L=3, box=0, factor=0.0)
    want = boxplot_np(X, level, 3, box=0, factor=0.0)
    _same(got, want, "factor 0")
    assert np.array_equal(got[1], got[0][0])                       # the fence is the box itself
    assert (got[2][level > 0] != 0).any()
    got = eng.central_regions(X, level, L=3, box=0, factor=1e6)
    _same(got, boxplot_np(X, level, 3, box=0, factor=1e6), "large factor")
    assert not got[2].any()                                        # nobody is flagged ...
    assert np.array_equal(got[3], np.stack([X.min(axis=1), X.max(axis=1)]))      # ... so the whiskers are the envelope of all


# ---- the public API on the device ----
def _frame(T, n, seed):
    X = boxplot_data(T, n, "tenths", seed)
    return pd.DataFrame(X, index=pd.Index(np.linspace(0.0, 1.0, T), name="time"), columns=[f"c{i}" for i in range(n)])


def _check_result(res, df, depths, fractions, box, factor):
    """A FunctionalBoxplotResult against the restatement applied to `depths` (in column order)."""
    X = df.to_numpy()
    d = np.asarray(depths, dtype=np.float64)
    level = levels_np(d, fractions, X.shape[1])
    env, fence, outside, whisker = boxplot_np(X, level, len(fractions), box=box, factor=factor)
    assert res.median == df.columns[np.argsort(-d, kind="stable")[0]]
    assert list(res.regions) == list(fractions) and res.alpha == fractions[box]
    for l, a in enumerate(fractions):
        assert res.regions[a].index.equals(df.index) and list(res.regions[a].columns) == ["lower", "upper"]
        assert np.array_equal(res.regions[a].to_numpy().T, env[l])
    assert np.array_equal(res.envelope.to_numpy().T, env[box])
    assert res.fence.index.equals(df.index) and np.array_equal(res.fence.to_numpy().T, fence, equal_nan=True)
    assert res.whiskers.index.equals(df.index) and np.array_equal(res.whiskers.to_numpy().T, whisker)
    assert list(res.outside.index) == list(df.columns) and np.array_equal(res.outside.to_numpy(), outside)
    assert list(res.outliers) == [c for c, o in zip(df.columns, outside) if o.any()]
    assert list(res.depths.index) == list(df.columns) and np.array_equal(res.depths.to_numpy(), d)
    return outside


def test_depth_result_boxplot_and_central_region():
    from statdepth_amd import FunctionalDepth
    df = _frame(30, 80, 5)
    depth = FunctionalDepth([df], relax=True)
    outside = _check_result(depth.boxplot(), df, depth.to_numpy(), (0.5,), 0, 1.5)
    assert outside.any()
    _check_result(depth.boxplot(alpha=0.5, factor=0.75, levels=(0.25, 0.9)), df, depth.to_numpy(), (0.25, 0.5, 0.9), 1, 0.75)
    region = depth.central_region()
    level = levels_np(depth.to_numpy(), (0.5,), 80)
    assert region.index.equals(df.index) and np.array_equal(region.to_numpy().T, boxplot_np(df.to_numpy(), level, 1)[0][0])
    assert np.array_equal(depth.central_region(alpha=1.0).to_numpy().T,
                          np.stack([df.to_numpy().min(axis=1), df.to_numpy().max(axis=1)]))


def test_functional_boxplot_extremal_default_and_own_depths():
    from statdepth_amd import FunctionalBoxplot, FunctionalDepth
    df = _frame(25, 60, 9)
    res = FunctionalBoxplot([df], containment="extremal")
    _check_result(res, df, FunctionalDepth([df], containment="extremal").to_numpy(), (0.5,), 0, 1.5)
    res = FunctionalBoxplot(df)                                    # the modified band depth
    _check_result(res, df, FunctionalDepth([df], relax=True).to_numpy(), (0.5,), 0, 1.5)
    # a user's depths, in another order than the columns, with ties
    own = pd.Series(np.round(np.random.default_rng(2).random(60), 1), index=df.columns).sample(frac=1, random_state=1)
    res = FunctionalBoxplot(df, own, alpha=0.6, factor=1.0, levels=(0.3,))
    _check_result(res, df, own.reindex(df.columns).to_numpy(), (0.3, 0.6), 1, 1.0)
    # a column-built (curve-major) frame gives the same
    built = pd.DataFrame({c: df[c].to_numpy() for c in df.columns}, index=df.index)
    again = FunctionalBoxplot(built, own, alpha=0.6, factor=1.0, levels=(0.3,))
    assert again.outside.equals(res.outside) and again.fence.equals(res.fence) and list(again.outliers) == list(res.outliers)
