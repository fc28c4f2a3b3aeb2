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
from dataclasses import dataclass
from typing import Callable, Optional, Union

import numpy as np
import pandas as pd
from scipy.special import binom

from ... import engine
from ._helper import DepthDegeneracy, _padded_members

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


def _oja_check(P: np.ndarray) -> None:
    if P.shape[1] > 8:
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
    """The k x d direction array of containment='halfspace' for a checked cloud -- or None for the exact depth of a planar
    cloud (directions='exact', d = 2: no direction set, K11)."""
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
    """The k x d direction array of containment='projection' for a checked cloud (as for halfspace: an int with `seed`, or
    an array used as given)."""
    if isinstance(directions, str):
        if directions == 'exact':
            raise NotImplementedError("projection depth has no exact form: directions='exact' belongs to "
                                      "containment='halfspace'; give a number of directions or a (k x d) array")
        raise ValueError(f"directions must be a positive number of directions or a (k x {P.shape[1]}) array, "
                         f"got {directions!r}")
    U = _halfspace_directions(directions, seed, P.shape[1])   # finite, no all-zero row
    engine.projection_check('direction entries', U)
    return U


@dataclass(frozen=True)
class _Family:
    """One point-cloud depth family.  rows / blocks / external: the engine function of each form, by name (looked up on
    `engine` when it is called).  depth(raw, N, d, vols): its raw output to depths; N is the size of each target's sample,
    the target included (n, the block lengths as a float array, n + 1 for an external point), vols the samples' hull
    volumes where `hull` asks for them.  check(P): the host check of a point array.  setup(P, directions, seed): the
    direction array of a checked cloud, or None for the `exact` kind.  max_block: the largest K-block the blocks form takes."""
    rows: str
    blocks: str
    external: Optional[str]
    depth: Callable
    check: Optional[Callable] = None
    setup: Optional[Callable] = None
    hull: bool = False
    max_block: Optional[int] = None
    exact: Optional['_Family'] = None


# the halfspace depth itself for d <= 2, seed unused; no external form
_HALFSPACE_EXACT = _Family('halfspace_exact_counts', 'halfspace_exact_subset_counts', None,
                           depth=lambda raw, N, d, vols: raw.astype(np.float64) / N)

_FAMILIES = {
    # (d+1)-subsets of the others whose simplex contains the point, over binom(N, d + 1): N INCLUDES the point (:38,56)
    'simplex': _Family('pointcloud_simplex_counts', 'pointcloud_simplex_subset_counts',
                       'pointcloud_simplex_external_counts',
                       depth=lambda raw, N, d, vols: raw.astype(np.float64) / binom(N, d + 1)),
    # the same depth for d = 2 with exact signs in place of the tolerance, by angular sweep
    'simplex_exact': _Family('simplicial_exact_counts', 'simplicial_exact_subset_counts',
                             'simplicial_exact_external_counts',
                             depth=lambda raw, N, d, vols: raw.astype(np.float64) / binom(N, 3),
                             check=_simplex_exact_check),
    'l1': _Family('l1_depth', 'l1_subset_depth', 'l1_external_depth',
                  depth=lambda raw, N, d, vols: raw),    # (:148-150)
    # (:175-205) with every other row of the sample in the subsets, also for a to_compute subset; the normaliser is the
    # hull of the sample the depth refers to: P, the block, or the intact F u {g}
    'oja': _Family('oja_volume_sums', 'oja_subset_volume_sums', 'oja_external_volume_sums',
                   depth=lambda raw, N, d, vols: raw / vols, check=_oja_check, hull=True),
    # An extension (no such string in the reference): min over the directions of min(#{p.u <= x.u}, #{p.u >= x.u}),
    # the point itself and ties counted, over N -- the random Tukey depth, an upper bound of the exact halfspace
    # depth for d >= 2 and exact for d = 1.  The sample, its target included, is what is counted.
    'halfspace': _Family('halfspace_counts', 'halfspace_subset_counts', 'halfspace_external_counts',
                         depth=_HALFSPACE_EXACT.depth, check=_halfspace_check, setup=_halfspace_setup,
                         exact=_HALFSPACE_EXACT),
    # An extension (no such string in the reference): 1 / (1 + O), O = max over the directions of
    # |x.u - med(S.u)| / MAD(S.u), the Stahel-Donoho outlyingness over the direction set; med and MAD
    # of the sample S, its target included; O = inf gives 0.0
    'projection': _Family('projection_outlyingness', 'projection_subset_outlyingness',
                          'projection_external_outlyingness',
                          depth=lambda raw, N, d, vols: 1.0 / (1.0 + np.asarray(raw, dtype=np.float64)),
                          check=_projection_check,
                          setup=_projection_setup, max_block=_PROJECTION_MAX_BLOCK),
}


def _family(containment) -> _Family:
    if containment == 'mahalanobis':
        raise NotImplementedError(f'{containment} depth is outside the band-depth hot path this engine covers')
    if not isinstance(containment, str) or containment not in _FAMILIES:
        raise ValueError(f'{containment} is not a valid containment measure. ')   # (:63-64)
    return _FAMILIES[containment]


def _host_side(fam: _Family, directions, seed, *arrays):
    """Everything a family refuses on the host: its check of every array, in order, then its directions from the first.
    Returns (the family -- its exact kind where the set-up gave no direction set --, the direction array or None)."""
    if fam.check is not None:
        for A in arrays:
            fam.check(A)
    U = None if fam.setup is None else fam.setup(arrays[0], directions, seed)
    return (fam.exact if U is None and fam.exact is not None else fam), U


def _hulls(fam: _Family, samples) -> Optional[np.ndarray]:
    """Hull volume of each target's sample (`samples()` yields them), on the host: a degenerate sample never reaches the
    GPU.  None for a family that does not ask for it."""
    return np.array([_hull_volume(S) for S in samples()], dtype=np.float64) if fam.hull else None


def _engine_call(fam: _Family, form: str, P, sel, U, **kw) -> np.ndarray:
    """The family's engine function of `form` ('rows', 'blocks', 'external') on the selector `sel` (row positions, the
    padded member matrix, the external points)."""
    f = getattr(engine, getattr(fam, form))
    if U is None:
        return f(P, sel, **kw)
    return f(P, U, sel, **kw) if form == 'rows' else f(P, sel, U, **kw)


def _pointwisedepth(data: pd.DataFrame, to_compute: Union[list, pd.Index] = None, containment='simplex',
                    quiet=True, device=None, directions=1000, seed=0) -> pd.Series:
    n, d = data.shape
    if to_compute is None:
        to_compute = data.index                          # (:41-42)
    if containment in ('linf', 'linf_relax'):
        # An extension (the reference knows no such string and raises ValueError, :63-64): the L-infinity / box
        # containment SURVEY 8 P4 spells out with reference semantics -- the band depth of the points read as curves over
        # their coordinates, FunctionalDepth([data.T]).  'linf': the share of pairs of other points whose bounding box
        # contains the point (relax=False); 'linf_relax': the mean over the coordinates (relax=True).
        from ._functional import _univariate_depths
        depths = _univariate_depths(data.T, list(to_compute), 2, containment == 'linf_relax', device=device)
        return pd.Series(index=to_compute, data=depths)
    P = data.to_numpy(dtype=np.float64)
    fam, U = _host_side(_family(containment), directions, seed, P)
    vols = _hulls(fam, lambda: [P])
    raw = _engine_call(fam, 'rows', P, _row_positions(data, to_compute), U, device=device)
    return pd.Series(index=to_compute, data=fam.depth(raw, n, d, vols))


def _lens_cloud_depths(data: pd.DataFrame, to_compute=None, K=None, containment='lens', device=None) -> pd.Series:
    """The lune depths with a fixed beta ('lens', 'spherical') of the rows `to_compute` of the n x d frame as points of
    R^d, any d >= 1: the share of the C(n, 2) pairs of points whose beta-lune holds the point.  The frame is the curve-major
    layout of FunctionalDepth's call with T = d, so nothing is transposed on the host: one upload, one device call
    (sd_lens_counts), one division.  Refused before anything is uploaded: `K`, NaN or infinite values, magnitudes above 2^480,
    fewer than 2 or more than 16 384 points, no column, and 'beta_skeleton', whose beta PointcloudDepth has no argument for."""
    from ._functional import METRIC_MAX_ABS, _lens_counts_to_depths

    def refuse(reason):
        raise ValueError(f'containment \'{containment}\' {reason}')

    if containment == 'beta_skeleton':
        refuse('needs a beta, which PointcloudDepth has no argument for: call FunctionalDepth([data.T], '
               'containment=\'beta_skeleton\', beta=...), whose curves are the points.')
    if K is not None:
        refuse('has no K-block estimator: K must be None.')
    P = data.to_numpy(dtype=np.float64)
    if P.ndim != 2 or P.shape[1] < 1:
        refuse('needs at least one column.')
    n, d = P.shape
    if n < 2:
        refuse(f'needs at least 2 points, got {n}.')
    if not np.isfinite(P).all():
        refuse('does not take NaN or infinite values (they have no distance): drop or fill them first.')
    if np.abs(P).max() > METRIC_MAX_ABS:
        refuse('takes values up to 2^480 in magnitude (a squared difference beyond would overflow): rescale the points.')
    if to_compute is None:
        to_compute = data.index
    return _lens_counts_to_depths(P.T, _row_positions(data, to_compute), to_compute, containment, None, device)


def _block_depths(P: np.ndarray, blocks, containment: str, device=None, directions=None) -> np.ndarray:
    """Depth of each block's target (its LAST row) inside the block, every block in one launch.  `directions`: the
    direction array of a family that has one; None there asks for its exact kind."""
    fam = _family(containment)
    if directions is None and fam.exact is not None:
        fam = fam.exact
    mem = _padded_members(blocks)
    sizes = np.array([len(b) for b in blocks], dtype=np.float64)
    vols = _hulls(fam, lambda: (P[np.asarray(b)] for b in blocks))
    return fam.depth(_engine_call(fam, 'blocks', P, mem, directions, device=device), sizes, P.shape[1], vols)


def _external_depths(F: np.ndarray, Q: np.ndarray, containment, directions=1000, seed=0) -> np.ndarray:
    """Depth of every external point Q[q] inside F u {Q[q]} (n + 1 points), one launch; `directions` and `seed` default
    to PointcloudDepth's."""
    n, d = F.shape
    fam, U = _host_side(_family(containment), directions, seed, F, Q)
    vols = _hulls(fam, lambda: (np.vstack([F, Q[[r]]]) for r in range(Q.shape[0])))
    return fam.depth(_engine_call(fam, 'external', F, Q, U), n + 1, d, vols)


def _samplepointwisedepth(data: pd.DataFrame, to_compute: pd.Index = None, K=2, containment='simplex',
                          quiet=True, device=None, directions=1000, seed=0) -> pd.Series:
    """K-block sampled point-cloud depth (:68-123).

    Same sampling rule and RNG consumption as the reference: `ss = n // K` (:107) and, per point, `ss`
    repetitions (:113 -- the loop bound is ss, not K) of a `data.sample(n=ss)` draw (:114) with the point
    appended when the draw missed it (:117-118; the reference's `DataFrame.append` is gone from pandas >= 2,
    so the reference itself cannot run this path any more).  The draws are made first -- rows by position, from
    the global numpy RNG exactly as `DataFrame.sample` consumes it -- and all len(to_compute) * ss
    (point, sample) pairs are evaluated in ONE launch (the family's blocks form) instead of as many `_pointwisedepth` calls.
    Oja: the depth of the point inside its block -- the block's other rows in the subsets, the block's hull as the
    normaliser (the reference's is identically 0).  Halfspace: one direction set (directions, seed) for
    every block, or none (directions='exact'); neither takes anything from the global RNG.  Projection: one direction
    set as well; blocks of more than 2 048 rows (the n // K drawn rows and the point: n // K + 1 > 2048) are refused
    before anything is drawn.
    """
    if K == 1:
        return _pointwisedepth(data=data, to_compute=to_compute, containment=containment, device=device,
                               directions=directions, seed=seed)
    fam = _family(containment)
    n = data.shape[0]
    P = data.to_numpy(dtype=np.float64)
    fam, U = _host_side(fam, directions, seed, P)        # host checks first: bad input never reaches the RNG or the GPU
    # a block: n // K drawn rows, and the point where the draw missed it
    if fam.max_block is not None and n // K + 1 > fam.max_block:
        raise NotImplementedError(f'K-sampled {containment} depth takes blocks of at most {fam.max_block} rows '
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
    depth = _block_depths(P, blocks, containment, device=device, directions=U)
    return pd.Series(index=to_compute, data=depth.reshape(len(targets), ss).mean(axis=1))
