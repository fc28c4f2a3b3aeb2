"""The lens, spherical and beta-skeleton depth (K22) on the GPU: the counts equal the restatement
(tests/test_lens_depth_host.py) by np.array_equal, on the device's own matrix of squared distances and, up to 129 curves, on
the matrix in rational arithmetic, at every extent of the count kernel; the three forms agree; nothing depends on the target
list, the external form, the memory layout or the workspace size; the counts do not increase with kappa; and the public API
returns counts / C(n, 2)."""
import functools

import numpy as np
import pandas as pd
import pytest

from test_curve_dist_host import KINDS, curves, sqdist_exact
from test_lens_depth_host import LN_COLS, LN_JK, LN_TILE, lens_counts_np, lens_span, pairs_of, small_integers, two_ball_counts
from statdepth_amd import FunctionalDepth, PointcloudDepth, engine
from statdepth_amd._native import SD_ERR_WORKSPACE, StatdepthHipError

pytestmark = pytest.mark.gpu

WHOLE = 129                                                        # up to here every curve is restated, and on the exact matrix too
DRAWN = 16                                                         # targets restated above
KAPPAS = (0.0, 1.0, 0.5, -0.5, -1.0, 2 / 1.5 - 1)


def picked(n):
    """The targets restated: all up to 129 curves; above, 16 with the first and the last."""
    if n <= WHOLE:
        return np.arange(n)
    rest = np.random.default_rng(n).permutation(np.arange(1, n - 1))[:DRAWN - 2]
    return np.array(sorted({0, n - 1} | set(map(int, rest))))


@functools.lru_cache(maxsize=None)
def case(n, T, kind):
    """(X, the device's matrix D2, the targets restated), computed once per case."""
    X = curves(T, n, kind)
    D2 = engine.curve_sqdist(X)
    pick = picked(n)
    for a in (X, D2, pick):
        a.setflags(write=False)
    return X, D2, pick


@functools.lru_cache(maxsize=None)
def restated(n, T, kind, kappa):
    X, D2, pick = case(n, T, kind)
    G = lens_counts_np(D2, D2[pick], kappa)
    G.setflags(write=False)
    return G


# n one below, at and one above the sample curves of a chunk (16), of a tile (64) and the targets of a block (128): 129 is
# also two tiles plus one, with diagonal and off-diagonal tile pairs and a second block of targets; n = 2; T in {1, 3, 17}
EDGES = [(2, 1), (2, 3), (3, 17), (LN_JK - 1, 3), (LN_JK, 1), (LN_JK + 1, 17), (LN_COLS - 1, 3), (LN_COLS, 17), (LN_COLS + 1, 1),
         (LN_TILE - 1, 1), (LN_TILE, 3), (LN_TILE + 1, 17), (2 * LN_COLS + 1, 3), (3 * LN_COLS + 5, 3)]
CASES = sorted(set([(n, T, KINDS[i % len(KINDS)]) for i, (n, T) in enumerate(EDGES)] + [(LN_COLS + 1, 3, kind) for kind in KINDS]))


@pytest.mark.parametrize('n,T,kind', CASES)
def test_counts_equal_the_restatement(n, T, kind):
    X, D2, pick = case(n, T, kind)
    for kappa in KAPPAS:
        G = engine.lens_counts(X, kappa)
        assert G.shape == (n,) and G.dtype == np.int64
        want = restated(n, T, kind, kappa)
        assert np.array_equal(G[pick], want), (kappa, np.flatnonzero(G[pick] != want)[:5])
        assert (G >= n - 1).all() and (G <= pairs_of(n)).all()     # a target's own pairs count
        if kind == 'identical':
            assert (G == pairs_of(n)).all()
    if n <= WHOLE:
        exact = sqdist_exact(X)                                     # the device's matrix is the specified one
        assert np.array_equal(D2, exact)
        for kappa in (0.0, 1.0, 2 / 1.5 - 1):
            assert np.array_equal(engine.lens_counts(X, kappa), lens_counts_np(exact, exact, kappa))


def test_one_larger_case():
    n, T = 1025, 3
    X, D2, pick = case(n, T, 'rounded')
    assert len(pick) == DRAWN
    for kappa in (0.0, 1.0, 2 / 1.5 - 1):
        G = engine.lens_counts(X, kappa)
        assert np.array_equal(G[pick], restated(n, T, 'rounded', kappa)), kappa
        assert np.array_equal(engine.lens_counts(X, kappa, targets=pick), G[pick])


@pytest.mark.parametrize('n,T,kind', [(LN_TILE + 1, 17, 'rounded'), (LN_COLS + 1, 3, 'duplicated'), (LN_COLS + 1, 3, 'subnormal'),
                                      (LN_COLS + 1, 3, 'up470'), (LN_JK + 1, 17, 'normal')])
def test_the_general_form_equals_the_lens_and_the_sphere_form(n, T, kind):
    X = curves(T, n, kind)
    for kappa in (0.0, 1.0):
        assert np.array_equal(engine.lens_counts(X, kappa, algo=1), engine.lens_counts(X, kappa, algo=0))
    assert np.array_equal(engine.lens_counts(X, 0.5, algo=1), engine.lens_counts(X, 0.5))
    Q = curves(T, 5, kind, seed=1)
    for kappa in (0.0, 1.0):
        assert np.array_equal(engine.lens_external_counts(X, Q, kappa, algo=1), engine.lens_external_counts(X, Q, kappa))


def test_integer_data_gives_the_geometric_counts():
    X = small_integers(3, 11, 1)
    for kappa in (1.0, 0.5, 0.0, -0.5, -1.0):
        assert np.array_equal(engine.lens_counts(X, kappa), two_ball_counts(X, kappa))


@pytest.mark.parametrize('n,T,kind', [(LN_TILE + 1, 17, 'duplicated'), (3 * LN_COLS + 5, 3, 'rounded')])
def test_target_lists(n, T, kind):
    """Lists with repeats and permutations, more targets than curves (several blocks), one target, none."""
    X, D2, pick = case(n, T, kind)
    rng = np.random.default_rng(n + T)
    tg = rng.permutation(n)[:max(2, n // 3)]
    tg[-1] = tg[0]
    many = np.concatenate([rng.permutation(n), rng.permutation(n)[:n // 2 + 1]])
    for kappa in (0.0, 1.0, -0.5):
        G = engine.lens_counts(X, kappa)
        assert np.array_equal(G[pick], restated(n, T, kind, kappa))
        for t in (tg, many, np.array([n - 1])):
            assert np.array_equal(engine.lens_counts(X, kappa, targets=t), G[t])
    assert engine.lens_counts(X, 0.0, targets=np.zeros(0, dtype=np.int64)).shape == (0,)


def test_a_workgroup_that_walks_several_tiles():
    """Enough targets (a list that repeats the sample curves) for the launcher to give a workgroup two tiles of sample
    curves j, one target more than whole blocks; the same counts as with one tile each."""
    n, T = 2 * LN_COLS + 1, 3
    X, D2, pick = case(n, T, 'duplicated')
    m = LN_TILE * 1821 + 1
    assert lens_span(n, n) == 1 and lens_span(n, m) == 2
    tg = np.arange(m) % n
    tg[-1] = n - 1
    for kappa in (0.0, 1.0, 0.5):
        assert np.array_equal(engine.lens_counts(X, kappa, targets=tg), restated(n, T, 'duplicated', kappa)[tg]), kappa


def test_external_targets():
    """Columns of Q that are no sample curves equal the restatement on their own rows of distances; one equal to a sample
    curve gets that curve's count; one far outside lies in no lune but, at kappa = -1, in the slabs it projects into."""
    n, T = 70, 9
    X = curves(T, n, 'normal')
    far = 1e6 * (np.abs(X[:, [0]]) + 1.0)
    Q = np.concatenate([curves(T, 6, 'rounded', seed=1), X[:, [3, 3]], far, 2.0 * X[:, [0]]], axis=1)
    D2, A = engine.curve_sqdist(X), engine.curve_sqdist_external(X, Q)
    assert np.array_equal(A, sqdist_exact(np.concatenate([X, Q], axis=1), n + np.arange(Q.shape[1]))[:, :n])
    for kappa in KAPPAS:
        G = engine.lens_external_counts(X, Q, kappa)
        assert G.shape == (Q.shape[1],) and G.dtype == np.int64
        assert np.array_equal(G, lens_counts_np(D2, A, kappa)), kappa
        inside = engine.lens_counts(X, kappa)
        assert G[6] == G[7] == inside[3]
        if kappa >= 0.0:
            assert G[8] == 0


@pytest.mark.parametrize('n,T,kind', [(LN_TILE + 1, 17, 'duplicated'), (LN_COLS + 1, 3, 'far')])
def test_layouts_and_workspaces(n, T, kind):
    """C- and F-contiguous X; the workspace at the floor, one block above it and recommended, with external targets in
    several batches; one byte below the floor is refused."""
    X, D2, pick = case(n, T, kind)
    rng = np.random.default_rng(n)
    tg = rng.permutation(n)[:n // 2]
    ext = rng.integers(0, n, size=2 * LN_TILE + 45)                 # more than two blocks
    block = LN_TILE * 8 * n
    for kappa in (0.0, 2 / 1.5 - 1):
        want = restated(n, T, kind, kappa)
        for M in (np.ascontiguousarray(X), np.asfortranarray(X)):
            cm = M.flags.f_contiguous and not M.flags.c_contiguous
            for t in (None, tg):
                m = n if t is None else len(t)
                rec, floor = engine.lens_workspace_bytes(T, n, curve_major=cm, m=m)
                assert floor <= rec and rec == floor + (-(-m // LN_TILE) - 1) * block
                for ws in (None, floor, rec):
                    got = engine.lens_counts(M, kappa, targets=t, ws_bytes=ws)
                    assert np.array_equal(got, want if t is None else want[t]), (cm, m, ws)
                with pytest.raises(StatdepthHipError) as e:
                    engine.lens_counts(M, kappa, targets=t, ws_bytes=floor - 1)
                assert e.value.code == SD_ERR_WORKSPACE
        rec, floor = engine.lens_workspace_bytes(T, n, m=len(ext))
        assert rec == floor + 2 * block
        for ws, per in ((None, len(ext)), (floor, LN_TILE), (floor + block, 2 * LN_TILE), (rec, len(ext))):
            if ws is not None:
                assert engine.lens_targets_per_batch(T, n, ws, m=len(ext)) == per
            assert np.array_equal(engine.lens_external_counts(X, X[:, ext], kappa, ws_bytes=ws), want[ext]), ws
        with pytest.raises(StatdepthHipError) as e:
            engine.lens_external_counts(X, X[:, ext], kappa, ws_bytes=floor - 1)
        assert e.value.code == SD_ERR_WORKSPACE


@pytest.mark.parametrize('n,T,kind', [(LN_TILE + 1, 17, 'normal'), (LN_COLS + 1, 3, 'rounded'), (LN_COLS + 1, 3, 'subnormal')])
def test_counts_do_not_increase_with_kappa(n, T, kind):
    X = curves(T, n, kind)
    ks = np.sort(np.concatenate([np.linspace(-1.0, 1.0, 9), [2 / 1.5 - 1, np.nextafter(0.0, 1.0), np.nextafter(1.0, 0.0)]]))
    G = np.stack([engine.lens_counts(X, k) for k in ks])
    assert (np.diff(G, axis=0) <= 0).all()


def test_public_api():
    """FunctionalDepth and PointcloudDepth return counts / C(n, 2), labels and `to_compute` as elsewhere; d = 12 too."""
    n, T = 37, 12
    X = curves(T, n, 'duplicated')
    for M in (X, np.asfortranarray(X)):
        df = pd.DataFrame(M, columns=[f'c{i}' for i in range(n)])
        for containment, beta, kappa in (('lens', None, 0.0), ('spherical', None, 1.0), ('beta_skeleton', 1.5, 2.0 / 1.5 - 1.0),
                                         ('beta_skeleton', float('inf'), -1.0)):
            G = engine.lens_counts(X, kappa)
            assert np.array_equal(G, lens_counts_np(*[engine.curve_sqdist(X)] * 2, kappa))
            res = FunctionalDepth([df], containment=containment, beta=beta)
            assert list(res.index) == list(df.columns) and np.array_equal(res.to_numpy(), G / pairs_of(n))
            assert res.attrs['beta'] == (beta if beta is not None else 2.0 - kappa)
            cols = ['c30', 'c2', 'c17']
            part = FunctionalDepth([df], to_compute=cols, containment=containment, beta=beta)
            assert list(part.index) == cols and np.array_equal(part.to_numpy(), res[cols].to_numpy())
            assert res.deepest(1).iloc[0] == res.to_numpy().max() and res.outlying(1).iloc[0] == res.to_numpy().min()
            if beta is None:                                        # the same points as a cloud in R^12
                cloud = PointcloudDepth(df.T, containment=containment)
                assert list(cloud.index) == list(df.columns) and np.array_equal(cloud.to_numpy(), res.to_numpy())
                assert cloud.attrs['beta'] == res.attrs['beta']
                some = PointcloudDepth(df.T, to_compute=cols, containment=containment)
                assert list(some.index) == cols and np.array_equal(some.to_numpy(), res[cols].to_numpy())
    line = PointcloudDepth(pd.DataFrame({'x': [0.0, 1.0, 2.0, 3.0]}), containment='lens')       # d = 1: the segments that hold x
    assert list(line) == [3 / 6, 5 / 6, 5 / 6, 3 / 6]
    same = FunctionalDepth([pd.DataFrame(curves(4, 6, 'identical'))], containment='spherical')
    assert list(same) == [1.0] * 6
