"""Point-cloud depth drivers on the HIP engine.

Mirrors statdepth/depth/calculations/_pointcloud.py: `_pointwisedepth` (:14-66),
`_samplepointwisedepth` (:68-123), `_L1_depth` (:125-150) and `_oja_depth` (:175-205).  Oja depth is the
reference's quantity -- the summed volumes of the simplices the point spans with every d-subset of the other
points, over the volume of the sample's convex hull -- with the volume sums on the GPU (sd_oja_*) and the hull
(scipy's Qhull, as in the reference) on the host; DESIGN.md §3 K7 / §4 lists where it departs from the reference.
Mahalanobis depth (:152-173) is not provided: the reference's covariance is singular by construction.
Halfspace (Tukey) depth over a fixed direction set (containment='halfspace', sd_halfspace_*) is an extension the
reference does not have; DESIGN.md §3 K10 states its definition.  directions='exact' asks for the exact halfspace depth
(d = 2: sd_halfspace2_*; d = 1: the direction (1.0), which is exact already).
Projection depth (containment='projection', sd_projection_*: 1 / (1 + the Stahel-Donoho outlyingness) over the same kind
of direction set) is another extension; DESIGN.md §3 K12 states its definition bit for bit.
containment='simplex_exact' is the reference's simplex depth of a planar cloud counted by an angular sweep with exact signs
(sd_simplicial2_*): O(n log^2 n) per point where 'simplex' enumerates C(n - 1, 3) triangles.
"""
from typing import Union

import numpy as np
import pandas as pd
from scipy.special import binom

from ... import engine
from ._helper import DepthDegeneracy

__all__ = ['_pointwisedepth', '_samplepointwisedepth']


def _row_positions(data: pd.DataFrame, labels) -> np.ndarray:
    pos = data.index.get_indexer(list(labels))
    if (pos < 0).any():
        missing = [l for l, p in zip(labels, pos) if p < 0]
        raise KeyError(f'{missing} not in index')
    return pos.astype(np.int64)


_OJA_HULL_MESSAGE = ('Too many collinear points to compute depth of convex hull spanned by data. '
                     'Try another depth method or remove collinearities.')          # (:189)


def _hull_volume(P: np.ndarray) -> float:
    """ConvexHull(P).volume, the normaliser of Oja depth (:187-189): any failure of Qhull (d = 1, NaN / inf, a flat
    sample, fewer than d + 1 points) is the reference's DepthDegeneracy."""
    from scipy.spatial import ConvexHull
    try:
        return float(ConvexHull(P).volume)
    except Exception as e:                       # noqa: BLE001 -- the reference's bare except (:188)
        raise DepthDegeneracy(_OJA_HULL_MESSAGE) from e


def _oja_check_dim(d: int) -> None:
    if d > 8:
        raise NotImplementedError('oja depth is implemented for d <= 8')


def _halfspace_directions(directions, seed, d: int) -> np.ndarray:
    """The k x d fp64 direction array of containment='halfspace'.  An int k: the rows of
    `np.random.default_rng(seed).standard_normal((k, d))`, each divided by its norm (`np.linalg.norm`); d = 1 has one
    direction up to sign, [[1.0]], whatever k is.  An array is used as given: k x d, finite, no all-zero row."""
    if isinstance(directions, (int, np.integer)) and not isinstance(directions, bool):
        if directions < 1:
            raise ValueError('directions must be a positive number of directions or a (k x d) array')
        if d == 1:
            return np.ones((1, 1), dtype=np.float64)
        U = np.random.default_rng(seed).standard_normal((int(directions), d))
        return U / np.linalg.norm(U, axis=1, keepdims=True)
    U = np.array(directions, dtype=np.float64, ndmin=2)
    if U.ndim != 2 or U.shape[0] < 1 or U.shape[1] != d:
        raise ValueError(f'directions must be a (k x {d}) array for data with {d} columns, got shape {U.shape}')
    if not np.isfinite(U).all():
        raise ValueError('directions must be finite')
    if not U.any(axis=1).all():
        raise ValueError('directions must not contain an all-zero row')
    return np.ascontiguousarray(U)


def _halfspace_check(P: np.ndarray) -> None:
    d = P.shape[1]
    if d > 8:
        raise NotImplementedError('halfspace depth is implemented for d <= 8')
    if not np.isfinite(P).all():
        raise ValueError('halfspace depth does not accept NaN or infinite values')


def _halfspace_setup(P: np.ndarray, directions, seed):
    """Host checks of containment='halfspace', then the k x d direction array -- or None for the exact depth of a planar
    cloud (directions='exact', d = 2: no direction set, K11)."""
    _halfspace_check(P)
    d = P.shape[1]
    if not isinstance(directions, str):
        return _halfspace_directions(directions, seed, d)
    if directions != 'exact':
        raise ValueError(f"directions must be a positive number of directions, a (k x {d}) array or 'exact', "
                         f"got {directions!r}")
    if d == 1:
        return np.ones((1, 1), dtype=np.float64)         # one direction up to sign: exact already
    if d != 2:
        raise NotImplementedError("exact halfspace depth (directions='exact') is implemented for the plane "
                                  f"(d = 2; d = 1 is exact with any directions), got d = {d}")
    if P.size and np.abs(P).max() > 2.0 ** 500:          # the exact predicate's products must not overflow
        raise ValueError('exact halfspace depth needs coordinates of magnitude at most 2^500')
    return None


def _simplex_exact_check(P: np.ndarray) -> None:
    """Host checks of containment='simplex_exact': the plane, finite, |coordinate| <= 2^500."""
    d = P.shape[1]
    if d != 2:
        raise NotImplementedError("exact simplicial depth (containment='simplex_exact') is implemented for the plane "
                                  f"(d = 2), got d = {d}: use containment='simplex'")
    if not np.isfinite(P).all():
        raise ValueError('exact simplicial depth does not accept NaN or infinite values')
    if P.size and np.abs(P).max() > 2.0 ** 500:          # the exact predicate's products must not overflow
        raise ValueError('exact simplicial depth needs coordinates of magnitude at most 2^500')


_PROJECTION_MAX_BLOCK = 2048                             # members of a K-block: sd_projection_subset_outlyingness sorts it in LDS


def _projection_check(P: np.ndarray) -> None:
    if P.shape[1] > 8:
        raise NotImplementedError('projection depth is implemented for d <= 8')
    engine.projection_check('coordinates', P)            # finite, |x| <= 2^500: ValueError otherwise


def _projection_setup(P: np.ndarray, directions, seed) -> np.ndarray:
    """Host checks of containment='projection', then the k x d direction array (as for halfspace: an int with `seed`, or
    an array used as given)."""
    _projection_check(P)
    if isinstance(directions, str):
        if directions == 'exact':
            raise NotImplementedError("projection depth has no exact form: directions='exact' belongs to "
                                      "containment='halfspace'; give a number of directions or a (k x d) array")
        raise ValueError(f"directions must be a positive number of directions or a (k x {P.shape[1]}) array, "
                         f"got {directions!r}")
    U = _halfspace_directions(directions, seed, P.shape[1])   # finite, no all-zero row
    engine.projection_check('direction entries', U)
    return U


def _projection_depth(outlyingness: np.ndarray) -> np.ndarray:
    """1 / (1 + O) in numpy; O = inf gives 0.0."""
    return 1.0 / (1.0 + np.asarray(outlyingness, dtype=np.float64))


def _pointwisedepth(data: pd.DataFrame, to_compute: Union[list, pd.Index] = None, containment='simplex',
                    quiet=True, device=None, directions=1000, seed=0) -> pd.Series:
    n, d = data.shape
    if to_compute is None:
        to_compute = data.index                          # (:41-42)
    if containment == 'simplex':
        P = data.to_numpy(dtype=np.float64)
        counts = engine.pointcloud_simplex_counts(P, _row_positions(data, to_compute), device=device)
        depths = counts.astype(np.float64) / binom(n, d + 1)     # n INCLUDES the point (:38,56)
        return pd.Series(index=to_compute, data=depths)
    elif containment == 'simplex_exact':
        # the same depth for d = 2 with exact signs in place of the tolerance, by angular sweep
        P = data.to_numpy(dtype=np.float64)
        _simplex_exact_check(P)
        counts = engine.simplicial_exact_counts(P, _row_positions(data, to_compute), device=device)
        return pd.Series(index=to_compute, data=counts.astype(np.float64) / binom(n, 3))
    elif containment == 'l1':
        P = data.to_numpy(dtype=np.float64)
        depths = engine.l1_depth(P, _row_positions(data, to_compute), device=device)
        return pd.Series(index=to_compute, data=depths)          # (:150)
    elif containment in ('linf', 'linf_relax'):
        # An extension (the reference knows no such string and raises ValueError, :63-64): the L-infinity / box
        # containment SURVEY 8 P4 spells out with reference semantics -- the band depth of the points read as curves over
        # their coordinates, FunctionalDepth([data.T]).  'linf': the share of pairs of other points whose bounding box
        # contains the point (relax=False); 'linf_relax': the mean over the coordinates (relax=True).
        from ._functional import _univariate_depths
        depths = _univariate_depths(data.T, list(to_compute), 2, containment == 'linf_relax', device=device)
        return pd.Series(index=to_compute, data=depths)
    elif containment == 'oja':
        # (:175-205) with every other row in the subsets, also for a to_compute subset
        _oja_check_dim(d)
        P = data.to_numpy(dtype=np.float64)
        vol = _hull_volume(P)                                    # host first: a degenerate sample never reaches the GPU
        sums = engine.oja_volume_sums(P, _row_positions(data, to_compute), device=device)
        return pd.Series(index=to_compute, data=sums / vol)
    elif containment == 'halfspace':
        # An extension (no such string in the reference): min over the directions of min(#{p.u <= x.u}, #{p.u >= x.u}),
        # the point itself and ties counted, over n -- the random Tukey depth, an upper bound of the exact halfspace
        # depth for d >= 2 and exact for d = 1
        # directions='exact': the halfspace depth itself for d <= 2, seed unused
        P = data.to_numpy(dtype=np.float64)
        U = _halfspace_setup(P, directions, seed)
        if U is None:
            counts = engine.halfspace_exact_counts(P, _row_positions(data, to_compute), device=device)
        else:
            counts = engine.halfspace_counts(P, U, _row_positions(data, to_compute), device=device)
        return pd.Series(index=to_compute, data=counts.astype(np.float64) / n)
    elif containment == 'projection':
        # An extension (no such string in the reference): 1 / (1 + O), O = max over the directions of
        # |x.u - med(P.u)| / MAD(P.u), the Stahel-Donoho outlyingness over the direction set
        P = data.to_numpy(dtype=np.float64)
        U = _projection_setup(P, directions, seed)
        out = engine.projection_outlyingness(P, U, _row_positions(data, to_compute), device=device)
        return pd.Series(index=to_compute, data=_projection_depth(out))
    elif containment == 'mahalanobis':
        raise NotImplementedError(f'{containment} depth is outside the band-depth hot path this engine covers')
    else:
        raise ValueError(f'{containment} is not a valid containment measure. ')   # (:63-64)


def _block_depths(P: np.ndarray, blocks, containment: str, device=None, directions=None) -> np.ndarray:
    """Depth of each block's target (its LAST row) inside the block, every block in one launch."""
    width = max(len(b) for b in blocks)
    mem = np.full((len(blocks), width), -1, dtype=np.int32)
    for i, b in enumerate(blocks):
        mem[i, :len(b)] = b
    if containment == 'oja':                             # (:187-205) on the sample: the block's own hull
        _oja_check_dim(P.shape[1])
        vols = np.array([_hull_volume(P[np.asarray(b)]) for b in blocks], dtype=np.float64)
        return engine.oja_subset_volume_sums(P, mem, device=device) / vols
    if containment == 'halfspace':                       # the block, its target included, is the sample
        sizes = np.array([len(b) for b in blocks], dtype=np.float64)
        if directions is None:                           # directions='exact' in the plane
            return engine.halfspace_exact_subset_counts(P, mem, device=device).astype(np.float64) / sizes
        return engine.halfspace_subset_counts(P, mem, directions, device=device).astype(np.float64) / sizes
    if containment == 'projection':                      # med and MAD of the block, its target included
        return _projection_depth(engine.projection_subset_outlyingness(P, mem, directions, device=device))
    if containment == 'simplex':
        d = P.shape[1]
        sizes = np.array([len(b) for b in blocks], dtype=np.float64)
        counts = engine.pointcloud_simplex_subset_counts(P, mem, device=device).astype(np.float64)
        return counts / binom(sizes, d + 1)              # (:38,56) on the sample: its size INCLUDES the point
    if containment == 'simplex_exact':
        sizes = np.array([len(b) for b in blocks], dtype=np.float64)
        return engine.simplicial_exact_subset_counts(P, mem, device=device).astype(np.float64) / binom(sizes, 3)
    return engine.l1_subset_depth(P, mem, device=device)  # (:148-150) on the sample


def _samplepointwisedepth(data: pd.DataFrame, to_compute: pd.Index = None, K=2, containment='simplex',
                          quiet=True, device=None, directions=1000, seed=0) -> pd.Series:
    """K-block sampled point-cloud depth (:68-123).

    Same sampling rule and RNG consumption as the reference: `ss = n // K` (:107) and, per point, `ss`
    repetitions (:113 -- the loop bound is ss, not K) of a `data.sample(n=ss)` draw (:114) with the point
    appended when the draw missed it (:117-118; the reference's `DataFrame.append` is gone from pandas >= 2,
    so the reference itself cannot run this path any more).  The draws are made first -- rows by position, from
    the global numpy RNG exactly as `DataFrame.sample` consumes it -- and all len(to_compute) * ss
    (point, sample) pairs are evaluated in ONE launch (sd_pointcloud_simplex_subset_counts /
    sd_l1_subset_depth / sd_oja_subset_volume_sums / sd_halfspace_subset_counts / sd_halfspace2_subset_counts /
    sd_projection_subset_outlyingness / sd_simplicial2_subset_counts) instead of as many `_pointwisedepth` calls.
    Oja: the depth of the point inside its block -- the block's other rows in the subsets, the block's hull as the
    normaliser (the reference's is identically 0).  Halfspace: one direction set (directions, seed) for
    every block, or none (directions='exact'); neither takes anything from the global RNG.  Projection: one direction
    set as well; blocks of more than 2 048 rows (the n // K drawn rows and the point: n // K + 1 > 2048) are refused
    before anything is drawn.
    """
    if K == 1:
        return _pointwisedepth(data=data, to_compute=to_compute, containment=containment, device=device,
                               directions=directions, seed=seed)
    if containment == 'mahalanobis':
        raise NotImplementedError(f'{containment} depth is outside the band-depth hot path this engine covers')
    if containment not in ('simplex', 'simplex_exact', 'l1', 'oja', 'halfspace', 'projection'):
        raise ValueError(f'{containment} is not a valid containment measure. ')
    n, d = data.shape
    U = None
    if containment == 'simplex_exact':
        _simplex_exact_check(data.to_numpy(dtype=np.float64))
    if containment == 'halfspace':                       # host checks first: bad input never reaches the RNG or the GPU
        U = _halfspace_setup(data.to_numpy(dtype=np.float64), directions, seed)
    if containment == 'projection':
        U = _projection_setup(data.to_numpy(dtype=np.float64), directions, seed)
        if n // K + 1 > _PROJECTION_MAX_BLOCK:           # a block: n // K drawn rows, and the point where the draw missed it
            raise NotImplementedError(f'K-sampled projection depth takes blocks of at most {_PROJECTION_MAX_BLOCK} rows '
                                      f'(n // K drawn rows and the point itself), got {n // K + 1}: raise K')
    if to_compute is None:
        to_compute = data.index
    ss = n // K
    targets = _row_positions(data, to_compute)
    if ss == 0 or len(targets) == 0:                     # the reference's mean over no draws
        return pd.Series(index=to_compute, data=np.full(len(targets), np.nan))
    rows = pd.Series(np.arange(n))                       # `.sample` on it draws what `data.sample(axis=0)` draws
    blocks = []
    for tp in targets:
        for _ in range(ss):
            drawn = rows.sample(n=ss).to_numpy()
            blocks.append(np.append(drawn[drawn != tp], tp))          # others in draw order, the point last
    depth = _block_depths(data.to_numpy(dtype=np.float64), blocks, containment, device=device, directions=U)
    return pd.Series(index=to_compute, data=depth.reshape(len(targets), ss).mean(axis=1))
