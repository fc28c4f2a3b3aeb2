"""Halfspace (Tukey) depth over a fixed direction set (containment='halfspace', K10) without a GPU: the numpy restatement
of the definition against hand-computed cases, direction generation, the host-side validation, the C ABI's refusals, and
the missing device reported as such (no CPU fallback).

The restatement (`projections`, `halfspace_counts`, `halfspace_counts_sorted`, `halfspace_external`, `halfspace_sampled`,
`make_directions`) is imported by tests/test_halfspace_gpu.py as its oracle.
"""
import ctypes

import numpy as np
import pandas as pd
import pytest


# ---------------------------------------------------------------- numpy restatement of the definition
def projections(X, U):
    """k x len(X): z_r(x) = ((x_0 u_r0 + x_1 u_r1) + x_2 u_r2) + ..., every product and sum rounded to fp64 on its own."""
    X, U = np.asarray(X, dtype=np.float64), np.asarray(U, dtype=np.float64)
    Z = U[:, 0][:, None] * X[:, 0][None, :]
    for e in range(1, X.shape[1]):
        Z = Z + U[:, e][:, None] * X[:, e][None, :]
    return Z


def halfspace_counts(P, U, targets=None):
    """min over directions of min(#{i: z(p_i) >= z(q)}, #{i: z(p_i) <= z(q)}), q = P[t] itself and every tie counted."""
    Z = projections(P, U)
    targets = range(Z.shape[1]) if targets is None else targets
    out = []
    for t in targets:
        ge = (Z >= Z[:, [t]]).sum(axis=1)
        le = (Z <= Z[:, [t]]).sum(axis=1)
        out.append(min(ge.min(), le.min()))
    return np.array(out, dtype=np.int64)


def halfspace_counts_sorted(P, U, targets=None):
    """The same counts for sizes where n comparisons per (target, direction) are too many: positions in the sorted row
    (`searchsorted` left / right are the strict / non-strict counts).  test_sorted_form_equals_comparisons ties it to
    halfspace_counts."""
    Z = projections(P, U)
    n = Z.shape[1]
    best = np.full(n, n, dtype=np.int64)
    for z in Z:
        s = np.sort(z)
        le = np.searchsorted(s, z, side='right')
        ge = n - np.searchsorted(s, z, side='left')
        best = np.minimum(best, np.minimum(le, ge))
    return best if targets is None else best[np.asarray(targets, dtype=np.int64)]


def halfspace_external(F, Q, U):
    """Counts of each external point g inside F u {g}: n + 1 points, g counted once."""
    F = np.asarray(F, dtype=np.float64)
    return np.array([halfspace_counts(np.vstack([F, g]), U, [len(F)])[0] for g in np.asarray(Q, dtype=np.float64)],
                    dtype=np.int64)


def make_directions(k, seed, d):
    """What PointcloudDepth(directions=k, seed=seed) documents: normalised rows of a seeded standard normal draw."""
    if d == 1:
        return np.ones((1, 1))
    U = np.random.default_rng(seed).standard_normal((k, d))
    return U / np.linalg.norm(U, axis=1, keepdims=True)


def halfspace_sampled(P, targets, K, U):
    """The K-block estimator replaying _samplepointwisedepth's draws from the global numpy RNG: per target ss = n // K
    blocks of `rows.sample(n=ss)` with the target appended last; depth inside the block, mean over the blocks."""
    P = np.asarray(P, dtype=np.float64)
    n = len(P)
    ss = n // K
    rows = pd.Series(np.arange(n))
    out = []
    for tp in targets:
        vals = []
        for _ in range(ss):
            drawn = rows.sample(n=ss).to_numpy()
            blk = np.append(drawn[drawn != tp], tp)
            vals.append(halfspace_counts(P[blk], U, [len(blk) - 1])[0] / len(blk))
        out.append(np.mean(vals))
    return np.array(out)


# ---------------------------------------------------------------- the restatement against hand-computed cases
def test_collinear_points_d1():
    P = np.array([[3.0], [-1.0], [7.0], [0.0], [12.0]])               # sorted: -1 0 3 7 12
    assert halfspace_counts(P, [[1.0]]).tolist() == [3, 1, 2, 2, 1]
    P = np.arange(5, dtype=np.float64)[:, None]
    assert halfspace_counts(P, [[1.0]]).tolist() == [1, 2, 3, 2, 1]
    assert halfspace_counts(P, [[-1.0]]).tolist() == [1, 2, 3, 2, 1]  # one direction serves u and -u
    assert halfspace_counts_sorted(P, [[1.0]]).tolist() == [1, 2, 3, 2, 1]


def test_square_and_centre():
    P = np.array([[1, 1], [1, -1], [-1, 1], [-1, -1], [0, 0]], dtype=np.float64)
    U = np.array([[1, 0], [0, 1], [1, 1], [1, -1]], dtype=np.float64)
    assert halfspace_counts(P, U).tolist() == [1, 1, 1, 1, 3]
    # the axes alone do not separate a corner from its two neighbours
    assert halfspace_counts(P, U[:2]).tolist() == [2, 2, 2, 2, 3]


def test_ties_and_duplicates_count():
    P = np.array([[0.0], [0.0], [0.0], [1.0]])
    assert halfspace_counts(P, [[1.0]]).tolist() == [3, 3, 3, 1]      # le = 3, ge = 4 for the triple point
    assert halfspace_external(P, [[0.0], [5.0], [0.5]], [[1.0]]).tolist() == [4, 1, 2]


def test_sorted_form_equals_comparisons():
    rng = np.random.default_rng(0)
    for n, d, k in ((1, 1, 1), (2, 3, 4), (40, 2, 7), (300, 3, 5)):
        P = rng.integers(-3, 4, size=(n, d)).astype(np.float64)       # heavy ties
        U = rng.integers(-2, 3, size=(k, d)).astype(np.float64)
        U[~U.any(axis=1)] = 1.0
        assert np.array_equal(halfspace_counts_sorted(P, U), halfspace_counts(P, U))
        C = rng.normal(size=(n, d))
        V = make_directions(k, 1, d)
        tg = rng.permutation(n)[:5]
        assert np.array_equal(halfspace_counts_sorted(C, V, tg), halfspace_counts(C, V, tg))


def test_projection_is_the_unfused_feature_loop():
    """(x0 u0 + x1 u1) + x2 u2 with separately rounded products: 1 + 2^-53 + 2^-53 rounds to 1 step by step."""
    e = 2.0 ** -53
    assert projections([[1.0, e, e]], [[1.0, 1.0, 1.0]])[0, 0] == 1.0
    assert projections([[e, e, 1.0]], [[1.0, 1.0, 1.0]])[0, 0] == 1.0 + 2 * e


# ---------------------------------------------------------------- direction generation and validation (host only)
def test_direction_generation():
    from statdepth_amd.depth.calculations._pointcloud import _halfspace_directions
    U = _halfspace_directions(50, 7, 3)
    assert U.shape == (50, 3) and U.dtype == np.float64
    assert np.array_equal(U, _halfspace_directions(50, 7, 3))
    assert np.array_equal(U, make_directions(50, 7, 3))
    assert not np.array_equal(U, _halfspace_directions(50, 8, 3))
    assert np.allclose(np.linalg.norm(U, axis=1), 1.0, atol=1e-15)
    for k in (1, 5, 1000):
        assert _halfspace_directions(k, 0, 1).tolist() == [[1.0]]
    given = [[2.0, 0.0], [0.0, -3.0]]
    assert _halfspace_directions(given, 0, 2).tolist() == given       # used as given, not normalised
    assert _halfspace_directions(np.int64(4), 0, 2).shape == (4, 2)


def test_validation_errors_before_device_work():
    from statdepth_amd import PointcloudDepth
    rng = np.random.default_rng(2)
    good = pd.DataFrame(rng.normal(size=(10, 2)))
    for bad_value in (np.nan, np.inf, -np.inf):
        bad = good.copy()
        bad.iloc[3, 1] = bad_value
        with pytest.raises(ValueError, match='NaN or infinite'):
            PointcloudDepth(bad, containment='halfspace')
        with pytest.raises(ValueError, match='NaN or infinite'):
            PointcloudDepth(bad, containment='halfspace', K=2)
    with pytest.raises(ValueError, match='all-zero row'):
        PointcloudDepth(good, containment='halfspace', directions=[[1.0, 0.0], [0.0, 0.0]])
    with pytest.raises(ValueError, match='finite'):
        PointcloudDepth(good, containment='halfspace', directions=[[1.0, np.nan]])
    with pytest.raises(ValueError, match=r'\(k x 2\) array'):
        PointcloudDepth(good, containment='halfspace', directions=np.ones((4, 3)))
    with pytest.raises(ValueError, match=r'\(k x 2\) array'):
        PointcloudDepth(good, containment='halfspace', directions=np.ones((4, 3)), K=2)
    with pytest.raises(ValueError, match='positive number'):
        PointcloudDepth(good, containment='halfspace', directions=0)
    with pytest.raises(NotImplementedError, match='d <= 8'):
        PointcloudDepth(pd.DataFrame(rng.normal(size=(12, 9))), containment='halfspace')


def test_unknown_containment_keeps_its_message():
    from statdepth_amd import PointcloudDepth
    df = pd.DataFrame(np.random.default_rng(0).normal(size=(6, 2)))
    for kw in ({}, {"K": 2}, {"directions": 5, "seed": 1}):
        with pytest.raises(ValueError) as e:
            PointcloudDepth(df, containment='nonsense', **kw)
        assert str(e.value) == 'nonsense is not a valid containment measure. '


def test_new_parameters_are_keyword_only_with_defaults():
    import inspect
    from statdepth_amd import PointcloudDepth
    sig = inspect.signature(PointcloudDepth)
    assert list(sig.parameters) == ['data', 'to_compute', 'K', 'containment', 'quiet', 'device', 'directions', 'seed']
    for name in ('directions', 'seed'):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig.parameters['directions'].default == 1000 and sig.parameters['seed'].default == 0
    assert sig.parameters['containment'].default == 'simplex'


# ---------------------------------------------------------------- C ABI, no device needed
def _lib():
    from statdepth_amd import _native
    return _native, _native.load()


def test_abi_refusals_before_device_work():
    _native, lib = _lib()
    fake = ctypes.c_void_p(256)                  # never dereferenced: every refusal happens before device work
    out = ctypes.c_void_p(512)
    INV, UNS = _native.SD_ERR_INVALID, _native.SD_ERR_UNSUPPORTED

    def counts(P, n, d, U, k, tg, m, o):
        return lib.sd_halfspace_counts(P, n, d, U, k, tg, m, o, fake, 1 << 40, None)

    def pairwise(P, n, d, U, k, tg, m, o):
        return lib.sd_halfspace_pairwise_counts(P, n, d, U, k, tg, m, o, None)

    for fn in (counts, pairwise):
        assert fn(None, 10, 2, fake, 4, None, 10, out) == INV
        assert fn(fake, 10, 2, None, 4, None, 10, out) == INV
        assert fn(fake, 10, 2, fake, 4, None, 10, None) == INV
        assert fn(fake, 10, 2, fake, 4, None, 9, out) == INV                  # NULL targets, m != n
        assert fn(fake, 0, 2, fake, 4, None, 0, out) == INV
        assert fn(fake, 10, 0, fake, 4, None, 10, out) == INV
        assert fn(fake, 10, 2, fake, 0, None, 10, out) == INV                 # k = 0
        assert fn(fake, 10, 9, fake, 4, None, 10, out) == UNS                 # d = 9
        assert b"d in [1,8]" in lib.sd_last_error()
        assert fn(fake, 2**31, 1, fake, 1, fake, 1, out) == UNS               # n = 2^31
        assert b"2^31" in lib.sd_last_error()
    assert lib.sd_halfspace_external_counts(fake, 10, 2, fake, 4, None, 3, out, None) == INV
    assert lib.sd_halfspace_external_counts(fake, 10, 2, fake, 0, fake, 3, out, None) == INV
    assert lib.sd_halfspace_external_counts(fake, 10, 9, fake, 4, fake, 3, out, None) == UNS
    assert lib.sd_halfspace_external_counts(fake, 2**31, 1, fake, 1, fake, 1, out, None) == UNS
    assert lib.sd_halfspace_external_counts(fake, 2**31 - 1, 1, fake, 1, fake, 1, out, None) == UNS   # n + 1 points
    assert lib.sd_halfspace_subset_counts(fake, 10, 2, fake, 4, None, 3, 4, out, None) == INV
    assert lib.sd_halfspace_subset_counts(fake, 10, 2, fake, 4, fake, 3, 0, out, None) == INV
    assert lib.sd_halfspace_subset_counts(fake, 10, 2, fake, 0, fake, 3, 4, out, None) == INV
    assert lib.sd_halfspace_subset_counts(fake, 10, 9, fake, 4, fake, 3, 4, out, None) == UNS
    # beyond 1e14 projections and comparisons: k n (d + log2 n) for the ranking route, m n k d pairwise
    assert counts(fake, 2**30, 3, fake, 10**4, fake, 1, out) == UNS
    assert b"cap" in lib.sd_last_error()
    assert pairwise(fake, 10**6, 3, fake, 10**3, None, 10**6, out) == UNS
    assert lib.sd_halfspace_external_counts(fake, 10**7, 8, fake, 10**4, fake, 10**3, out, None) == UNS
    assert lib.sd_halfspace_subset_counts(fake, 10**7, 8, fake, 10**4, fake, 10**6, 10**4, out, None) == UNS
    # a workspace below the floor is refused by the launcher's first check, before any launch
    floor = lib.sd_halfspace_min_workspace_bytes(1000, 3, 8)
    assert lib.sd_halfspace_counts(fake, 1000, 3, fake, 8, None, 1000, out, fake, floor - 1, None) == _native.SD_ERR_WORKSPACE
    assert lib.sd_halfspace_counts(fake, 1000, 3, fake, 8, None, 1000, out, None, 0, None) == _native.SD_ERR_WORKSPACE


def test_workspace_sizes():
    _native, lib = _lib()
    for n, d, k in ((1, 1, 1), (1000, 3, 8), (10**6, 3, 1000), (2**31 - 1, 8, 5)):
        floor = lib.sd_halfspace_min_workspace_bytes(n, d, k)
        rec = lib.sd_halfspace_workspace_bytes(n, d, k)
        assert 28 * n <= floor <= rec
        assert floor <= 28 * n + 4 * (n // 2048 + 1) + 8 * 256         # one direction: about 28 bytes per point
    assert lib.sd_halfspace_workspace_bytes(10**6, 3, 1000) <= 256 << 20
    for bad in ((0, 3, 5), (10, 0, 5), (10, 3, 0), (2**31, 3, 5)):
        assert lib.sd_halfspace_workspace_bytes(*bad) == 0 and lib.sd_halfspace_min_workspace_bytes(*bad) == 0


def test_no_device_is_an_error_not_a_fallback():
    from statdepth_amd import PointcloudDepth
    from statdepth_amd.homogeneity import PointcloudHomogeneity
    _native, lib = _lib()
    if lib.sd_device_count() > 0:
        pytest.skip("a HIP device is visible: tests/test_halfspace_gpu.py covers this machine")
    rng = np.random.default_rng(1)
    df = pd.DataFrame(rng.normal(size=(12, 2)))
    with pytest.raises(RuntimeError, match='no HIP device'):
        PointcloudDepth(df, containment='halfspace')
    with pytest.raises(RuntimeError, match='no HIP device'):
        PointcloudDepth(df, containment='halfspace', K=2, directions=8)
    with pytest.raises(RuntimeError, match='no HIP device'):
        PointcloudHomogeneity(df, pd.DataFrame(rng.normal(size=(12, 2))), containment='halfspace').homogeneity()
