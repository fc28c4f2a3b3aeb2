"""Oja depth (containment='oja', K7) without a GPU: the reference's fixtures against a numpy restatement, the C ABI's
refusals, the host-side DepthDegeneracy checks, and the missing device reported as such (no CPU fallback).

The restatement (`oja_sums`, `oja_depths`, `oja_sampled`) is imported by tests/test_oja_gpu.py as its oracle.
"""
import ctypes
import math
from itertools import combinations

import numpy as np
import pandas as pd
import pytest
from scipy.spatial import ConvexHull

from conftest import assert_depths_close, depths_of, frame_df, golden_names, load_golden

HULL_MSG = ('Too many collinear points to compute depth of convex hull spanned by data. '
            'Try another depth method or remove collinearities.')


# ---------------------------------------------------------------- numpy restatement of _oja_depth (:175-205)
def _volume_sum(others, x):
    """sum over d-subsets S of `others` of |det[S - x]| / d! (itertools + np.linalg.det)."""
    others = np.asarray(others, dtype=np.float64)
    d = others.shape[1]
    combos = np.array(list(combinations(range(len(others)), d)), dtype=np.int64).reshape(-1, d)
    if len(combos) == 0:
        return 0.0
    A = others[combos] - np.asarray(x, dtype=np.float64)            # (C, d, d): rows are the translated points
    return float(np.abs(np.linalg.det(A)).sum()) / math.factorial(d)


def oja_sums(P, targets=None):
    """Volume sums of the default form: every OTHER row of P in the subsets."""
    P = np.asarray(P, dtype=np.float64)
    targets = range(len(P)) if targets is None else targets
    return np.array([_volume_sum(np.delete(P, t, axis=0), P[t]) for t in targets])


def oja2_rowwise_targets(P, targets):
    """oja_sums at d = 2 for clouds whose n^2 table of cross products does not fit: one row of it at a time."""
    out = []
    for t in targets:
        a = np.delete(P, t, axis=0) - P[t]
        s = 0.0
        for i in range(len(a)):
            s += np.abs(a[i, 0] * a[i + 1:, 1] - a[i, 1] * a[i + 1:, 0]).sum()
        out.append(s / 2.0)
    return np.array(out)


def oja_depths(P, targets=None):
    return oja_sums(P, targets) / ConvexHull(P).volume


def oja_sampled(P, targets, K):
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
            vals.append(_volume_sum(P[blk[:-1]], P[tp]) / ConvexHull(P[blk]).volume)
        out.append(np.mean(vals))
    return np.array(out)


def oja_external(F, g):
    """Depth of an external point g inside the intact F u {g}: subsets of F, hull of F u {g}."""
    F = np.asarray(F, dtype=np.float64)
    return _volume_sum(F, g) / ConvexHull(np.vstack([F, g])).volume


# ---------------------------------------------------------------- fixtures
@pytest.mark.parametrize("name", golden_names(kind="pointcloud_oja"))
def test_fixture_matches_restatement(name):
    fx = load_golden(name)
    df = frame_df(fx["input"])
    assert fx["index"] == fx["input"]["index"]
    assert_depths_close(oja_depths(df.to_numpy()), depths_of(fx), 1e-12)


def test_record_grid_reference_raises_on_flat_simplices():
    """The reference raises on the first flat (q, S) simplex; here those add their volume, 0 (DESIGN §4 difference 1)."""
    fx = load_golden("oja_rec_grid")
    assert fx["raises"] == "DepthDegeneracy"
    P = frame_df(fx["input"]).to_numpy()
    got = oja_depths(P)
    assert np.isfinite(got).all() and (got > 0).all()


def test_record_to_compute_reference_restricts_subsets():
    """The reference enumerates subsets among the to_compute points only; here among all other rows (difference 2)."""
    fx = load_golden("oja_rec_to_compute")
    df = frame_df(fx["input"])
    P = df.to_numpy()
    tc = fx["call"]["to_compute"]
    pos = [fx["input"]["index"].index(c) for c in tc]
    vol = ConvexHull(P).volume
    restricted = np.array([_volume_sum(P[[p for p in pos if p != t]], P[t]) for t in pos]) / vol
    assert_depths_close(restricted, depths_of(fx), 1e-12)
    full = oja_depths(P, pos)
    assert (full > restricted).all()


def test_record_sampled_reference_is_zero():
    """The reference's K-sampled Oja is identically 0 (one point in to_compute: no subsets); here the depth of the point
    inside its block (difference 3)."""
    fx = load_golden("oja_rec_k2")
    assert (depths_of(fx) == 0).all()
    df = frame_df(fx["input"])
    np.random.seed(fx["call"]["np_random_seed"])
    got = oja_sampled(df.to_numpy(), range(len(df)), 2)
    assert np.isfinite(got).all() and (got > 0).all()


@pytest.mark.parametrize("name", golden_names(kind="pointcloud_oja_error"))
def test_degenerate_sample_raises_reference_message(name):
    """The sample's hull fails (flat, NaN, d = 1): DepthDegeneracy with the reference's message, before any device work,
    exact and sampled."""
    from statdepth_amd import PointcloudDepth
    from statdepth_amd.depth import DepthDegeneracy
    fx = load_golden(name)
    assert fx["raises"] == "DepthDegeneracy" and fx["message"] == HULL_MSG
    df = frame_df(fx["input"])
    with pytest.raises(DepthDegeneracy) as e:
        PointcloudDepth(df, containment='oja')
    assert str(e.value) == HULL_MSG
    with pytest.raises(DepthDegeneracy) as e:
        PointcloudDepth(df, containment='oja', K=1)
    assert str(e.value) == HULL_MSG


def test_dimension_above_eight_is_not_implemented():
    from statdepth_amd import PointcloudDepth
    df = pd.DataFrame(np.random.default_rng(0).normal(size=(12, 9)))
    with pytest.raises(NotImplementedError, match='oja depth is implemented for d <= 8'):
        PointcloudDepth(df, containment='oja')
    with pytest.raises(NotImplementedError, match='oja depth is implemented for d <= 8'):
        PointcloudDepth(df, containment='oja', K=2)


def test_mahalanobis_stays_not_implemented():
    from statdepth_amd import PointcloudDepth
    df = pd.DataFrame(np.random.default_rng(0).normal(size=(6, 2)))
    with pytest.raises(NotImplementedError):
        PointcloudDepth(df, containment='mahalanobis')


# ---------------------------------------------------------------- C ABI, no device needed
def _lib():
    from statdepth_amd import _native
    return _native, _native.load()


def test_abi_refusals_before_device_work():
    _native, lib = _lib()
    fake = ctypes.c_void_p(256)                  # never dereferenced: every refusal happens before device work
    out = ctypes.c_void_p(512)
    assert lib.sd_oja_volume_sums(None, 10, 2, None, 10, out, None) == _native.SD_ERR_INVALID
    assert lib.sd_oja_volume_sums(fake, 10, 2, None, 10, None, None) == _native.SD_ERR_INVALID
    assert lib.sd_oja_external_volume_sums(fake, 10, 2, None, 3, out, None) == _native.SD_ERR_INVALID
    assert lib.sd_oja_subset_volume_sums(fake, 10, 2, None, 3, 4, out, None) == _native.SD_ERR_INVALID
    assert lib.sd_oja_volume_sums(fake, 10, 2, None, 9, out, None) == _native.SD_ERR_INVALID      # NULL targets, m != n
    for d in (0, 9):
        assert lib.sd_oja_volume_sums(fake, 20, d, None, 20, out, None) == _native.SD_ERR_UNSUPPORTED
        assert lib.sd_oja_external_volume_sums(fake, 20, d, fake, 2, out, None) == _native.SD_ERR_UNSUPPORTED
        assert lib.sd_oja_subset_volume_sums(fake, 20, d, fake, 2, 8, out, None) == _native.SD_ERR_UNSUPPORTED
    assert b"d in [1,8]" in lib.sd_last_error()
    # subset indices are 32-bit: 2^31 or more other points are refused even where the subset count is small
    assert lib.sd_oja_volume_sums(fake, 2**31 + 1, 1, fake, 1, out, None) == _native.SD_ERR_UNSUPPORTED
    assert lib.sd_oja_external_volume_sums(fake, 2**31, 1, fake, 1, out, None) == _native.SD_ERR_UNSUPPORTED
    assert b"2^31" in lib.sd_last_error()
    # C(10^6 - 1, 8) >= 2^62: not enumerable
    assert lib.sd_oja_volume_sums(fake, 10**6, 8, fake, 1, out, None) == _native.SD_ERR_OVERFLOW
    assert lib.sd_oja_external_volume_sums(fake, 10**6, 8, fake, 1, out, None) == _native.SD_ERR_OVERFLOW
    # enumerable, but m * C(n - 1, d) above the 1e14 cap
    assert math.comb(9999, 4) < 2**62 and 10**4 * math.comb(9999, 4) > 1e14
    assert lib.sd_oja_volume_sums(fake, 10**4, 4, None, 10**4, out, None) == _native.SD_ERR_UNSUPPORTED
    assert b"cap" in lib.sd_last_error()


def test_no_device_is_an_error_not_a_fallback():
    from statdepth_amd import PointcloudDepth
    from statdepth_amd.homogeneity import PointcloudHomogeneity
    _native, lib = _lib()
    if lib.sd_device_count() > 0:
        pytest.skip("a HIP device is visible: tests/test_oja_gpu.py covers this machine")
    rng = np.random.default_rng(1)
    df = pd.DataFrame(rng.normal(size=(12, 2)))
    with pytest.raises(RuntimeError, match='no HIP device'):
        PointcloudDepth(df, containment='oja')
    with pytest.raises(RuntimeError, match='no HIP device'):
        PointcloudDepth(df, containment='oja', K=2)
    with pytest.raises(RuntimeError, match='no HIP device'):
        PointcloudHomogeneity(df, pd.DataFrame(rng.normal(size=(12, 2))), containment='oja').homogeneity()
