"""The functional spatial depth of curves (K21) on the GPU: the squared norms S and the sum field E equal the specified
recurrences in rational arithmetic bit for bit (tests/test_spatial_depth_host.py) at every extent of the two kernels and
on both time tiles of the sum kernel, nothing depends on the memory layout, the target list, the external form, the field
argument or the workspace size, the depth agrees with K5's L1 depth of the same vectors as a point cloud and lies within
its derived bound of the 50-digit reference, and the public API returns what the engine call gives."""
import functools

import mpmath
import numpy as np
import pandas as pd
import pytest

from test_curve_dist_host import KINDS, curves
from test_spatial_depth_host import (SHAPES_REF, SP_JK, SP_NARROW, SP_TILE, SP_WIDE, depth_bound, depth_of, normal_squares,
                                     spatial_exact, spatial_reference)
from statdepth_amd import FunctionalDepth, engine
from statdepth_amd._native import SD_ERR_WORKSPACE, StatdepthHipError

pytestmark = pytest.mark.gpu

WHOLE = 129                                                        # up to here every curve is restated
DRAWN = 16                                                         # targets restated above


def picked(X):
    """The targets restated: all up to 129 curves; above, at most 16 with the first, the last and, where the matrix has
    one, a curve and its duplicate."""
    n = X.shape[1]
    if n <= WHOLE:
        return np.arange(n)
    pick = {0, n - 1}
    _, first, counts = np.unique(X, axis=1, return_index=True, return_counts=True)
    if (counts > 1).any() and not (counts == n).all():
        a = int(first[np.argmax(counts > 1)])
        pick |= {a, int(np.flatnonzero((X == X[:, [a]]).all(axis=0))[1])}
    rest = [i for i in np.random.default_rng(n).permutation(n) if i not in pick]
    return np.array(sorted(pick | set(map(int, rest[:DRAWN - len(pick)]))))


@functools.lru_cache(maxsize=None)
def case(n, T, kind):
    """(X, the targets restated, their exact S and E, the device's S and E of every curve), computed once per case."""
    X = curves(T, n, kind)
    pick = picked(X)
    S, E = spatial_exact(X, pick)
    dS, dE = engine.spatial_sums(X, field=True)
    for a in (pick, S, E, dS, dE):
        a.setflags(write=False)
    return X, pick, S, E, dS, dE


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same(a, b):
    """np.array_equal, on values (the sign of a zero is not part of the definition's comparison)."""
    return a.shape == b.shape and np.array_equal(a, b)


# n one below, at and one above the sample curves of a chunk of pass 2 (16), of a tile of pass 1 (64) and the targets of a
# tile of both (128), with all curves as targets (so m = n); T one below, at and one above the two time tiles (32, 64) and
# twice them; n = 2, T = 1; several tiles in both grid dimensions of pass 2 (257 x 65: 3 x 3 at the 32-wide tile)
EDGES = sorted(set([(n, 3) for n in (2, SP_JK - 1, SP_JK, SP_JK + 1, 63, 64, 65, SP_TILE - 1, SP_TILE, SP_TILE + 1)] +
                   [(5, T) for T in (1, SP_NARROW - 1, SP_NARROW, SP_NARROW + 1, SP_WIDE - 1, SP_WIDE, SP_WIDE + 1,
                                     2 * SP_WIDE - 1, 2 * SP_WIDE, 2 * SP_WIDE + 1)] +
                   [(2, 1), (33, SP_NARROW + 1), (257, 2 * SP_NARROW + 1)]))
CASES = sorted(set([(n, T, KINDS[i % len(KINDS)]) for i, (n, T) in enumerate(EDGES)] +
                   [(n, T, kind) for n, T in SHAPES_REF for kind in KINDS]))


@pytest.mark.parametrize('n,T,kind', CASES)
def test_sums_and_field_equal_the_restatement(n, T, kind):
    X, pick, S, E, dS, dE = case(n, T, kind)
    assert dS.shape == (n,) and dE.shape == (n, T) and dS.dtype == dE.dtype == np.float64
    assert same(dE[pick], E), np.argwhere(dE[pick] != E)[:5]
    assert same(dS[pick], S), np.flatnonzero(dS[pick] != S)[:5]
    assert not np.signbit(dS).any()
    if kind == 'identical':
        assert not bits(dS).any() and not dE.any()
    # a target list with the restated targets, one of them twice
    tg = np.append(pick, pick[0])
    lS, lE = engine.spatial_sums(X, targets=tg, field=True)
    assert same(lS, np.append(S, S[0])) and same(lE, np.concatenate([E, E[:1]]))


def targets_for_the_wide_tile(T):
    """The fewest whole blocks of 128 targets plus one target, doubling from one block, for which the library says that the
    sum kernel takes its 128 x 64 tile (sd_spatial_time_tile: the launcher's own rule, two workgroups per compute unit)."""
    blocks = 1
    while engine.spatial_time_tile(T, blocks * SP_TILE + 1) != SP_WIDE:
        blocks *= 2
        assert blocks <= 1 << 16, 'the launcher never takes the wide tile'
    return blocks * SP_TILE + 1


@pytest.mark.parametrize('n,T,kind', [(5, SP_WIDE - 1, 'normal'), (17, SP_WIDE, 'rounded'), (33, SP_WIDE + 1, 'duplicated'),
                                      (5, 2 * SP_WIDE - 1, 'far'), (16, 2 * SP_WIDE, 'up470'), (15, 2 * SP_WIDE + 1, 'subnormal'),
                                      (5, 1, 'normal'), (2, 3, 'down470'), (70, SP_WIDE + 1, 'normal')])
def test_the_wide_time_tile(n, T, kind):
    """Enough targets (a list that repeats the sample curves) for the launcher to take the 128 x 64 tile, as the library
    itself reports; one target more than whole blocks, so the last block holds one.  70 curves: five chunks of sample curves
    and a second column tile of pass 1."""
    X = curves(T, n, kind)
    S, E = spatial_exact(X)
    m = targets_for_the_wide_tile(T)
    assert engine.spatial_time_tile(T, m) == SP_WIDE and engine.spatial_time_tile(T, n) == SP_NARROW
    tg = np.arange(m) % n
    tg[-1] = n - 1
    dS, dE = engine.spatial_sums(X, targets=tg, field=True)
    assert same(dS, S[tg]) and same(dE, E[tg])
    assert same(engine.spatial_sums(X, targets=tg), dS)            # without the field
    few = engine.spatial_sums(X, field=True)                        # the same curves on the narrow tile
    assert same(few[0], S) and same(few[1], E)


FORMS = [(65, 5, 'rounded'), (129, 17, 'duplicated'), (129, 17, 'far'), next(c for c in CASES if c[:2] == (257, 2 * SP_NARROW + 1))]


@pytest.mark.parametrize('n,T,kind', FORMS)
def test_forms(n, T, kind):
    """C- and F-contiguous X; all targets, a list, a permuted list with repeats; external targets equal to sample curves;
    with and without the field; the workspace at the floor, one block above it and recommended."""
    X, pick, S, E, dS, dE = case(n, T, kind)
    rng = np.random.default_rng(n + T)
    tg = rng.permutation(n)[:max(2, n // 3)]
    tg[-1] = tg[0]
    many = np.concatenate([rng.permutation(n), rng.permutation(n)[:n // 2 + 1]])    # more targets than curves: several blocks
    block = SP_TILE * 8 * (n + T)
    for M in (np.ascontiguousarray(X), np.asfortranarray(X)):
        cm = M.flags.f_contiguous and not M.flags.c_contiguous
        for t in (None, tg, many):
            m = n if t is None else len(t)
            want = (dS, dE) if t is None else (dS[t], dE[t])
            rec, floor = engine.spatial_workspace_bytes(T, n, curve_major=cm, m=m)
            assert rec == floor + (-(-m // SP_TILE) - 1) * block
            for ws in (None, floor, floor + block, rec):
                if ws is not None:                                  # the batches the size implies: whole blocks of 128 targets
                    per = engine.spatial_targets_per_batch(T, n, ws, curve_major=cm, m=m)
                    assert per == min(m, (1 + (ws - floor) // block) * SP_TILE)
                got = engine.spatial_sums(M, targets=t, ws_bytes=ws, field=True)
                assert same(got[0], want[0]) and same(got[1], want[1]), (cm, m, ws)
                assert same(engine.spatial_sums(M, targets=t, ws_bytes=ws), want[0])
            with pytest.raises(StatdepthHipError) as e:
                engine.spatial_sums(M, targets=t, ws_bytes=floor - 1)
            assert e.value.code == SD_ERR_WORKSPACE
    for t in (tg, many, np.arange(1)):
        xS, xE = engine.spatial_external_sums(X, X[:, t], field=True)
        assert same(xS, dS[t]) and same(xE, dE[t])
        assert same(engine.spatial_external_sums(X, X[:, t]), dS[t])
        floor = engine.spatial_workspace_bytes(T, n, m=len(t))[1]
        assert same(engine.spatial_external_sums(X, X[:, t], ws_bytes=floor), dS[t])
    assert engine.spatial_sums(X, targets=np.zeros(0, dtype=np.int64)).shape == (0,)
    empty = engine.spatial_sums(X, targets=np.zeros(0, dtype=np.int64), field=True)
    assert empty[0].shape == (0,) and empty[1].shape == (0, T)


def test_external_targets():
    """Columns of Q that are no sample curves equal the restatement; the depth refers to n + 1 curves."""
    n, T = 40, 9
    X = curves(T, n, 'normal')
    Q = np.concatenate([curves(T, 6, 'rounded', seed=1), X[:, [3, 3]], 2.0 * X[:, [0]]], axis=1)
    S, E = spatial_exact(X, Q=Q)
    dS, dE = engine.spatial_external_sums(X, Q, field=True)
    assert same(dS, S) and same(dE, E)
    ref = spatial_reference(X, Q=Q)
    depth = depth_of(dS, n + 1)
    err = max(abs(float(mpmath.mpf(float(d)) - r)) for d, r in zip(depth, ref))
    assert err <= depth_bound(n, T), err / depth_bound(n, T)
    inside = depth_of(engine.spatial_sums(X), n)                    # a sample curve as an external target: one curve more
    assert depth[6] == 1.0 - np.sqrt(dS[6]) / (n + 1) and depth[6] > inside[3] and dS[6] == engine.spatial_sums(X)[3]


@pytest.mark.parametrize('T', [2, 3, 8])
def test_against_the_l1_depth_of_the_point_cloud(T):
    """The curves as points of R^T: K5 computes the same depth (its unit vectors through a Newton reciprocal root, hence its
    tolerance of 1e-12); non-coincident data, where the two conventions agree."""
    n = 300
    X = curves(T, n, 'normal', seed=T)
    df = pd.DataFrame(X, columns=[f'c{i}' for i in range(n)])
    depth = FunctionalDepth([df], containment='spatial').to_numpy()
    cloud = engine.l1_depth(np.ascontiguousarray(X.T))
    assert depth.shape == cloud.shape and np.isfinite(cloud).all()
    assert np.abs(depth - cloud).max() <= 1e-12


@pytest.mark.parametrize('n,T', SHAPES_REF)
@pytest.mark.parametrize('kind', [k for k in KINDS if k != 'subnormal'])
def test_depth_against_the_reference(n, T, kind):
    X, pick, S, E, dS, dE = case(n, T, kind)
    assert normal_squares(X)
    depth = depth_of(dS[pick], n)
    ref = spatial_reference(X, pick)
    err = max(abs(float(mpmath.mpf(float(d)) - r)) for d, r in zip(depth, ref))
    print(f'{kind} n={n} T={T}: largest error {err / depth_bound(n, T):.4f} of the bound')
    assert err <= depth_bound(n, T)
    every = depth_of(dS, n)
    assert (every >= 0.0).all() and (every <= 1.0).all()
    if kind == 'far':
        assert abs(every[n - 1] - 1 / n) <= 1e-6 and every.argmin() == n - 1
    if kind == 'identical':
        assert (every == 1.0).all()


def test_public_api():
    """Labels, `to_compute` and order as for 'hmodal' on the same frame; the values are the engine's through the host
    formula; the result object is the usual one."""
    n, T = 37, 11
    X = curves(T, n, 'duplicated')
    for M in (X, np.asfortranarray(X)):
        df = pd.DataFrame(M, columns=[f'c{i}' for i in range(n)])
        res = FunctionalDepth([df], containment='spatial')
        hm = FunctionalDepth([df], containment='hmodal')
        assert list(res.index) == list(hm.index) == list(df.columns)
        S = engine.spatial_sums(X)
        assert np.array_equal(res.to_numpy(), 1.0 - np.sqrt(S) / n)
        cols = ['c30', 'c2', 'c17']
        part = FunctionalDepth([df], to_compute=cols, containment='spatial')
        assert list(part.index) == list(FunctionalDepth([df], to_compute=cols, containment='hmodal').index) == cols
        assert np.array_equal(part.to_numpy(), res[cols].to_numpy())
        assert list(res.ordered().index) == list(res.sort_values(ascending=False).index)
        assert res.deepest(1).iloc[0] == res.to_numpy().max() and res.outlying(1).iloc[0] == res.to_numpy().min()
    box = res.boxplot()
    assert set(box.outliers) <= set(df.columns)
    two = FunctionalDepth([pd.DataFrame(np.array([[0.0, 1.0], [3.0, 3.0]]))], containment='spatial')
    assert list(two) == [0.5, 0.5]
    same_curves = FunctionalDepth([pd.DataFrame(curves(4, 6, 'identical'))], containment='spatial')
    assert list(same_curves) == [1.0] * 6
