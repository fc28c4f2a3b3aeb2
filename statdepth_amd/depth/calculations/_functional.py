"""Functional (band) depth drivers on the HIP engine.

Mirrors statdepth/depth/calculations/_functional.py: `_functionaldepth` (:17-97),
`_samplefunctionaldepth` (:99-196).  The per-target subset enumeration of
`_univariate_band_depth` (:198-255) and `_simplex_depth` (:257-286) is replaced by
calls into libstatdepth_hip (statdepth_amd.engine); the float normalisers stay here,
in fp64, written as the reference writes them.
"""
import math
import numbers
from itertools import combinations
from typing import List, Union

import numpy as np
import pandas as pd
from scipy.special import binom

from ... import engine
from ..._native import SD_ERR_OVERFLOW, StatdepthHipError
from ._containment import (_is_cloud_depth, _is_metric_depth, _is_order_depth, _is_rank_depth, _is_shape_depth,
                           _is_lens_depth, _is_projected_depth, _is_spatial_depth, _select_containment)
from ._helper import DepthDegeneracy, _band_depth_sum, _deep_check, _handle_depth_errors, _padded_members
from ._pointcloud import _halfspace_directions
from ._rank import _projected_depth_values, _rank_depth_values
from ._shape import _shape_depth_values

__all__ = ['_functionaldepth', '_samplefunctionaldepth', '_curve_distances', '_curve_projections']


# tests switch this off to compare the one-launch strict estimator with the block-by-block evaluation
_BATCH_STRICT_BLOCKS = True

def _positions(df: pd.DataFrame, labels) -> np.ndarray:
    """Column positions of `labels` (the reference addresses targets by label, :232)."""
    pos = df.columns.get_indexer(list(labels))
    if (pos < 0).any():
        missing = [l for l, p in zip(labels, pos) if p < 0]
        raise KeyError(f'{missing} not in columns')
    return pos.astype(np.int64)


def _require_unique_labels(df: pd.DataFrame) -> None:
    """Curves are addressed by column label (:232,248).  With duplicated labels the reference's label tuples collapse
    through a set (_helper.py:32) and `.loc` returns every column carrying a label, so bands silently merge curves, and
    any target whose own label is duplicated -- hence the default `to_compute=None` -- dies with a TypeError inside
    `_r2_containment` (tests/golden/g11_duplabels.json records this).  That accident is not reproduced: duplicated
    labels are refused up front."""
    if not df.columns.is_unique:
        dup = list(df.columns[df.columns.duplicated()].unique())
        raise ValueError(f'column labels must be unique to address curves; duplicated: {dup}')


def _univariate_depths(df: pd.DataFrame, cols, J: int, relax: bool, device=None, algo='auto') -> np.ndarray:
    """Band depth of columns `cols` of `df` (rows = timepoints): sum_j S_nj / binom(n, j).

    n = number of columns INCLUDING the target (:229) while bands come from the other
    n-1 (:235,243); S_nj = (sum_t contained j-bands)/T for relax (_containment.py:80
    `c/T`) or the number of j-bands containing the curve at every t (`c//T`).
    """
    X = df.to_numpy(dtype=np.float64, copy=False)      # keeps the frame's memory layout
    T, n = X.shape
    tg = _positions(df, cols)
    if relax:
        try:
            counts = engine.mbd_counts(X, tg, J=J, algo=algo, device=device).astype(np.float64) / T
        except StatdepthHipError as e:
            if e.code != SD_ERR_OVERFLOW:
                raise
            # T * C(n-1, J) beyond int64 (J >= 4 with ~10^5 curves): two-limb totals, exact big-integer normalisation
            wide = engine.mbd_counts_wide(X, tg, J=J, algo=algo, device=device)
            depth = np.zeros(len(tg), dtype=np.float64)
            for j in range(2, J + 1):
                den = T * math.comb(n, j)
                depth += np.array([int(v) / den for v in wide[:, j - 2]], dtype=np.float64)     # (:253), exact quotient
            return depth
    else:
        if J > 4:
            raise NotImplementedError('strict band depth (relax=False) is implemented for J <= 4')
        counts = engine.bd_strict_counts(X, tg, J=J, device=device).astype(np.float64)
    return _band_depth_sum(counts, n, J)               # (:253)


def _callable_band_depth(data: pd.DataFrame, curve, relax: bool, containment, J: int) -> float:
    """Generic enumerator for a user-supplied containment callable (:228-255).

    Not the hot path: arbitrary Python cannot run on the GPU, so the plug-in protocol
    of docs/index.md:124-148 is honoured on the host, one call per subset.
    """
    band_depth = 0
    n = data.shape[1]
    curvedata = data.loc[:, curve]
    data = data.drop(curve, axis=1)
    for j in range(2, J + 1):
        S_nj = 0
        for sequence in combinations(list(data.columns), j):
            S_nj += containment(data=data.loc[:, list(sequence)], curve=curvedata, relax=relax)
        band_depth += S_nj / binom(n, j)
    return band_depth


def _curves_tensor(data: List[pd.DataFrame]) -> np.ndarray:
    """list of n frames (T x d) -> (n, T, d) fp64."""
    return np.stack([np.asarray(df.to_numpy(dtype=np.float64)) for df in data])


def _componentwise_band_depth(data: List[pd.DataFrame], to_compute, J: int, relax: bool, device=None) -> pd.Series:
    """Multivariate band depth with the 'r2_enum' containment the reference declares and leaves unimplemented
    (_containment.py:83-103: every component treated as a real-valued function, contained iff all components are).

    Built as `_univariate_band_depth` (:238-253) with that predicate: bands from j-subsets of the n-1 other curves,
    sum_j S_nj / binom(n, j) with n INCLUDING the target (:229,253) -- so one feature (d = 1) gives the univariate depth.
    relax=True: one launch; J = 2 counts pairs through the 3^d state classes (sd_multi_band_counts), J = 3, 4 count
    j-subsets by inclusion-exclusion over the same classes (sd_multi_band_j_counts).  relax=False
    (contained at every timepoint in every component) is the strict univariate depth of the T*d component series.
    """
    f = [i for i in range(len(data))] if to_compute is None else to_compute
    P = _curves_tensor(data)
    n, T, d = P.shape
    tg = np.asarray(list(f), dtype=np.int64)
    if relax:
        if J > 4:
            raise NotImplementedError("'r2_enum' with relax=True is implemented for J <= 4")
        if J == 2:
            counts = engine.multi_band_counts(P, tg, device=device).astype(np.float64)[:, None] / T
        else:
            counts = engine.multi_band_j_counts(P, tg, J=J, device=device).astype(np.float64) / T
    else:
        if J > 4:
            raise NotImplementedError('strict band depth (relax=False) is implemented for J <= 4')
        X = P.reshape(n, T * d).T                        # rows = (timepoint, feature), columns = curves; no copy
        counts = engine.bd_strict_counts(X, tg, J=J, device=device).astype(np.float64)
    return pd.Series(index=f, data=_band_depth_sum(counts, n, J))


def _ranked_frame(data, J, containment: str, deep_check=False):
    """(frame, its T x n fp64 matrix) for a depth built on the pointwise ranks of univariate curves (the rank depths and
    the extremal depth), or the refusal they share, raised before anything is uploaded: one frame, J at its default,
    unique labels, at least 2 curves and 1 timepoint, no NaN."""
    def refuse(reason):
        raise ValueError(f'containment \'{containment}\' {reason}')

    if not isinstance(data, list):
        raise ValueError('data must be passed as a list.')
    if len(data) == 0:
        raise ValueError('No data passed.')
    if len(data) != 1:
        refuse('is defined for univariate data only (a list of one DataFrame whose columns are the curves).')
    if not isinstance(J, numbers.Integral) or isinstance(J, bool) or J != 2:
        refuse(f'has no band size: J must be left at its default 2, got {J!r}.')
    if deep_check:
        _deep_check(data)
    df = data[0]
    _require_unique_labels(df)
    X = df.to_numpy(dtype=np.float64, copy=False)      # keeps the frame's memory layout
    T, n = X.shape
    if n < 2:
        refuse(f'needs at least 2 curves, got {n}.')
    if T < 1:
        refuse('needs at least one timepoint.')
    if np.isnan(X).any():
        refuse('does not take NaN (a missing value has no rank): drop or fill them first.')
    return df, X


def _rank_depths(data, to_compute, J, containment: str, deep_check=False, device=None) -> pd.Series:
    """An integrated rank depth (containment in _containment.RANK_DEPTHS: 'fm', 'mei', 'mhi', 'half_region',
    'integrated_halfspace', 'infimal_halfspace') of the columns `to_compute` of the single frame in `data`: one device
    call for the integer records (sd_rank_depth_sums), the normalisation of _rank.py on the host.  Labels, `to_compute`
    and the result's order are those of 'r2'.  What cannot be computed is refused here, before anything is uploaded.
    The band-depth rule that J be below the number of timepoints does not apply: these depths have no J."""
    df, X = _ranked_frame(data, J, containment, deep_check)
    T, n = X.shape
    cols = df.columns if to_compute is None else to_compute
    records = engine.rank_depth_sums(X, _positions(df, cols), device=device)
    return pd.Series(index=cols, data=_rank_depth_values(records, n, T, containment))


PROJECTED_MAX_T = 2 ** 23          # timepoints of a projection: with |x|, |u| <= 2^500 no sum of T products overflows


def _projected_inputs(data, J, what: str, deep_check=False, directions=1000, seed=0):
    """(frame, its T x n fp64 matrix, U [k, T]) for the projections of univariate curves on a direction set, or the refusal,
    raised before anything is uploaded: what the rank depths refuse (_ranked_frame), infinite values, magnitudes above 2^500,
    2^23 or more timepoints; `directions` a positive int k (the rows of _halfspace_directions(k, seed, T): seeded unit
    vectors of R^T) or a k x T array used as given -- finite, no all-zero row, magnitudes of at most 2^500."""
    df, X = _ranked_frame(data, J, what, deep_check)
    T, n = X.shape
    if not np.isfinite(X).all():
        raise ValueError(f'containment \'{what}\' does not take infinite values: drop or clip them first.')
    engine.projection_check('values', X)                 # |x| <= 2^500: no projection or midpoint overflows
    if T >= PROJECTED_MAX_T:
        raise ValueError(f'containment \'{what}\' takes fewer than 2^23 timepoints, got {T}.')
    if isinstance(directions, str):
        if directions == 'exact':
            raise NotImplementedError(f"containment '{what}' has no exact form: give a number of directions or a "
                                      f"(k x {T}) array")
        raise ValueError(f"containment '{what}' takes a positive number of directions or a (k x {T}) array, "
                         f"got directions={directions!r}.")
    U = _halfspace_directions(directions, seed, T)       # finite, no all-zero row
    engine.projection_check('direction entries', U)
    return df, X, U


def _projected_depths(data, to_compute, J, containment: str, deep_check=False, device=None, directions=1000,
                      seed=0) -> pd.Series:
    """A random projection depth (containment in _containment.PROJECTED_DEPTHS) of the columns `to_compute` of the single
    frame in `data`: every curve is projected on the k directions (`directions`, `seed`: as for PointcloudDepth's
    'halfspace', in R^T) and a univariate depth of the projections is averaged or minimised over them -- 'rp_halfspace' the
    mean Tukey depth (the random projection depth), 'rp_fm' the mean of 1 - |1/2 - F_r|, 'random_tukey' the minimum Tukey
    depth, 'rp_projection' 1 / (1 + the largest |z - med| / MAD).  One device call for the records (sd_rp_depth_sums) or the
    outlyingness (sd_rp_outlyingness), the normalisation of _rank.py on the host.  Labels, `to_compute` and the result's
    order are those of 'r2'.  What cannot be computed is refused here, before anything is uploaded."""
    df, X, U = _projected_inputs(data, J, containment, deep_check, directions, seed)
    T, n = X.shape
    cols = df.columns if to_compute is None else to_compute
    call = engine.rp_outlyingness if containment == 'rp_projection' else engine.rp_depth_sums
    values = call(X, U, _positions(df, cols), device=device)
    return pd.Series(index=cols, data=_projected_depth_values(values, n, U.shape[0], containment))


def _curve_projections(data, directions=1000, seed=0, device=None) -> pd.DataFrame:
    """The projections of the columns of a frame (or of the single frame of a list) on the direction set: k rows, one
    column per curve under its label (engine.curve_projections)."""
    frames = data if isinstance(data, list) else [data]
    df, X, U = _projected_inputs(frames, 2, 'CurveProjections', directions=directions, seed=seed)
    return pd.DataFrame(engine.curve_projections(X, U, device=device), columns=df.columns)


EXTREMAL_MAX_T = 16384             # timepoints a curve's sort holds on the device (sd_extremal_counts)


def _extremal_depth(data, to_compute, J, containment: str, deep_check=False, device=None) -> pd.Series:
    """The extremal depth (Narisetty & Nair 2016; containment 'extremal') of the columns `to_compute` of the single frame
    in `data`: G / n, G the number of sample curves at least as extreme as the curve (sd_extremal_counts: the curve itself
    and its ties included), so the deepest curve has depth 1.  Labels, `to_compute` and the result's order are those of
    'r2'; the refusals are those of the rank depths, and more than 16 384 timepoints are not implemented."""
    df, X = _ranked_frame(data, J, containment, deep_check)
    T, n = X.shape
    if T > EXTREMAL_MAX_T:
        raise NotImplementedError(f'containment \'{containment}\' is implemented for up to {EXTREMAL_MAX_T} timepoints, '
                                  f'got {T}.')
    cols = df.columns if to_compute is None else to_compute
    G = engine.extremal_counts(X, _positions(df, cols), device=device)
    return pd.Series(index=cols, data=np.asarray(G, dtype=np.float64) / n)


def _shape_depths(data, to_compute, J, containment: str, deep_check=False, device=None) -> pd.Series:
    """The total variation depth ('tvd') or the modified shape similarity ('mss') of the columns `to_compute` of the single
    frame in `data` (Huang & Sun 2019; _shape.py): one device call for the sums (sd_tvd_sums), one division on the host.
    Labels, `to_compute` and the result's order are those of 'r2'; the refusals are those of the rank depths, and 'mss'
    also needs 2 timepoints and finite values (an infinite step has no weight).  All raised before anything is uploaded."""
    df, X = _ranked_frame(data, J, containment, deep_check)
    T, n = X.shape
    if containment == 'mss':
        if T < 2:
            raise ValueError(f'containment \'{containment}\' needs at least 2 timepoints, got {T}.')
        if not np.isfinite(X).all():
            raise ValueError(f'containment \'{containment}\' does not take infinite values (a step of infinite length '
                             'has no weight).')
    cols = df.columns if to_compute is None else to_compute
    sd_sum, shape = engine.tvd_sums(X, _positions(df, cols), device=device)
    return pd.Series(index=cols, data=_shape_depth_values(sd_sum, shape, n, T, containment))


METRIC_MAX_ABS = 2.0 ** 480         # |x| up to here: no squared L2 distance over fewer than 2^31 timepoints overflows


def _metric_frame(data, J, what: str, deep_check=False):
    """_ranked_frame for what is built on the L2 distances between curves: also no infinite value and none above 2^480 in
    magnitude (a squared difference would overflow).  `what` names the caller in the refusals."""
    def refuse(reason):
        raise ValueError(f'{what} {reason}')

    if not isinstance(data, list):
        raise ValueError('data must be passed as a list.')
    if len(data) == 0:
        raise ValueError('No data passed.')
    if len(data) != 1:
        refuse('is defined for univariate data only (a list of one DataFrame whose columns are the curves).')
    if not isinstance(J, numbers.Integral) or isinstance(J, bool) or J != 2:
        refuse(f'has no band size: J must be left at its default 2, got {J!r}.')
    if deep_check:
        _deep_check(data)
    df = data[0]
    _require_unique_labels(df)
    X = df.to_numpy(dtype=np.float64, copy=False)      # keeps the frame's memory layout
    T, n = X.shape
    if n < 2:
        refuse(f'needs at least 2 curves, got {n}.')
    if T < 1:
        refuse('needs at least one timepoint.')
    if not np.isfinite(X).all():
        refuse('does not take NaN or infinite values (they have no distance): drop or fill them first.')
    if np.abs(X).max() > METRIC_MAX_ABS:
        refuse('takes values up to 2^480 in magnitude (a squared difference beyond would overflow): rescale the curves.')
    return df, X


def _coincident_pairs(X: np.ndarray) -> int:
    """The pairs i < j of columns of X that are equal entry by entry (0.0 and -0.0 are equal): their distance is 0."""
    T, n = X.shape
    rows = np.ascontiguousarray(X.T) + 0.0               # -0.0 -> 0.0: equal values, equal bytes
    _, counts = np.unique(rows.view(np.dtype((np.void, 8 * T))).ravel(), return_counts=True)
    counts = counts.astype(object)
    return int((counts * (counts - 1) // 2).sum())


def _metric_depths(data, to_compute, J, containment: str, deep_check=False, device=None, quantile=0.15,
                   bandwidth=None) -> pd.Series:
    """The h-modal depth (Cuevas, Febrero & Fraiman 2006; containment 'hmodal') of the columns `to_compute` of the single
    frame in `data`: (1/n) sum_j exp(-||x - x_j||^2 / (2 h^2)) over all n curves, the curve itself included, in (0, 1].
    h is `bandwidth`, or the quantile `quantile` of the L2 distances over the pairs of curves i < j as an order statistic:
    h^2 = the k-th smallest squared distance, k = max(1, ceil(quantile n (n - 1) / 2)) (type 1; fda.usc's depth.mode
    interpolates, type 7, so its h differs slightly).  Three device calls at most: the selection (sd_curve_sqdist_select),
    the sums (sd_hmodal_sums), one division on the host.  The bandwidth used is in the result's attrs['bandwidth'].
    Labels, `to_compute` and the result's order are those of 'r2'.  Refused before anything is uploaded: what the rank
    depths refuse, infinite values or magnitudes above 2^480, a quantile outside (0, 1], a bandwidth that is not positive
    and finite, both given, and a quantile at which the distance is 0 because that share of the pairs coincides."""
    df, X = _metric_frame(data, J, f'containment \'{containment}\'', deep_check)
    T, n = X.shape
    default_q = isinstance(quantile, numbers.Real) and not isinstance(quantile, bool) and quantile == 0.15
    if bandwidth is not None:
        if not default_q:
            raise ValueError(f'containment \'{containment}\' takes bandwidth or quantile, not both: got bandwidth={bandwidth!r} '
                             f'and quantile={quantile!r}.')
        if not isinstance(bandwidth, numbers.Real) or isinstance(bandwidth, bool) or not 0.0 < bandwidth < math.inf:
            raise ValueError(f'containment \'{containment}\' takes a positive finite bandwidth, got {bandwidth!r}.')
        h = float(bandwidth)
        h2 = h * h
    else:
        if not isinstance(quantile, numbers.Real) or isinstance(quantile, bool) or not 0.0 < quantile <= 1.0:
            raise ValueError(f'containment \'{containment}\' takes a quantile in (0, 1], got {quantile!r}.')
        N = n * (n - 1) // 2
        k = max(1, math.ceil(quantile * N))
        same = _coincident_pairs(X)

        def refuse_zero(share):
            raise ValueError(f'containment \'{containment}\': the quantile {quantile!r} of the distances between the curves is 0, '
                             f'because {share} of the pairs of curves coincide; pass a larger quantile or a bandwidth.')

        if same >= k:
            refuse_zero(f'{same / N:.1%}')
    cols = df.columns if to_compute is None else to_compute
    targets = _positions(df, cols)
    M = engine.to_device_matrix(X, device)               # one upload for the selection and the sums
    if bandwidth is None:
        h2 = engine.curve_sqdist_select(M, k, device=device)
        if h2 == 0.0:                                    # differences so small that their squares underflow
            refuse_zero(f'at least {k / N:.1%}')
        h = math.sqrt(h2)
    g = 1.0 / (2.0 * h2) if h2 > 0.0 else math.inf       # (a given bandwidth whose square underflows)
    if not g < math.inf:
        raise ValueError(f'containment \'{containment}\': the bandwidth {h!r} is too small, 1 / (2 h^2) overflows.')
    S = engine.hmodal_sums(M, g, targets, device=device)
    depths = pd.Series(index=cols, data=np.asarray(S, dtype=np.float64) / n)
    depths.attrs['bandwidth'] = h
    return depths


def _spatial_depths(data, to_compute, J, containment: str, deep_check=False, device=None, quantile=0.15,
                    bandwidth=None) -> pd.Series:
    """The functional spatial depth (Chakraborty & Chaudhuri 2014; Sguera, Galeano & Lillo 2014; containment 'spatial') of
    the columns `to_compute` of the single frame in `data`: 1 - ||(1/n) sum_j (x - x_j) / ||x - x_j|| ||, the L2 norms as plain
    sums over the timepoints, the sum over the curves x_j at a nonzero distance from x (x itself and its exact copies add
    nothing and still count in n), in [0, 1].  One upload, one device call for the squared norms of the sums
    (sd_spatial_sums), a root and a division on the host.  Labels, `to_compute` and the result's order are those of 'r2'.
    Refused before anything is uploaded: what 'hmodal' refuses of the data, and `quantile` or `bandwidth`, which belong to
    'hmodal' (there is no bandwidth here)."""
    df, X = _metric_frame(data, J, f'containment \'{containment}\'', deep_check)
    T, n = X.shape
    default_q = isinstance(quantile, numbers.Real) and not isinstance(quantile, bool) and quantile == 0.15
    if bandwidth is not None or not default_q:
        raise ValueError(f'containment \'{containment}\' has no bandwidth: quantile and bandwidth belong to \'hmodal\' and must '
                         f'be left at their defaults, got quantile={quantile!r}, bandwidth={bandwidth!r}.')
    cols = df.columns if to_compute is None else to_compute
    targets = _positions(df, cols)
    M = engine.to_device_matrix(X, device)               # one upload
    S = engine.spatial_sums(M, targets, device=device)
    return pd.Series(index=cols, data=1.0 - np.sqrt(np.asarray(S, dtype=np.float64)) / n)


def _lens_kappa(containment: str, beta) -> tuple:
    """(beta, kappa = 2 / beta - 1) of a lune depth: 'lens' is beta = 2 and 'spherical' beta = 1, and both refuse a `beta`;
    'beta_skeleton' takes a real beta >= 1 or math.inf."""
    if containment != 'beta_skeleton':
        if beta is not None:
            raise ValueError(f'containment \'{containment}\' has its beta fixed ({2 if containment == "lens" else 1}): beta belongs '
                             f'to \'beta_skeleton\' and must be left at None, got {beta!r}.')
        beta = 2.0 if containment == 'lens' else 1.0
    elif not isinstance(beta, numbers.Real) or isinstance(beta, bool) or not beta >= 1:
        raise ValueError(f'containment \'beta_skeleton\' takes a real beta >= 1 or math.inf (beta=2 is the lens depth, beta=1 the '
                         f'spherical depth), got {beta!r}.')
    beta = float(beta)
    return beta, 2.0 / beta - 1.0


def _lens_counts_to_depths(X, targets, cols, containment: str, beta, device) -> pd.Series:
    """The tail shared by the curves and the point clouds: X (T x n, checked) goes up once, sd_lens_counts gives G, and the
    depth is G / C(n, 2)."""
    T, n = X.shape
    beta, kappa = _lens_kappa(containment, beta)
    if n > engine.LENS_MAX_N:
        raise ValueError(f'containment \'{containment}\' keeps the n x n matrix of distances on the device and takes at most '
                         f'{engine.LENS_MAX_N} curves or points, got {n}.')
    M = engine.to_device_matrix(X, device)               # one upload
    G = engine.lens_counts(M, kappa, targets, device=device)
    depths = pd.Series(index=cols, data=np.asarray(G, dtype=np.float64) / np.float64(n * (n - 1) // 2))
    depths.attrs['beta'] = beta
    return depths


def _lens_depths(data, to_compute, J, containment: str, deep_check=False, device=None, quantile=0.15, bandwidth=None,
                 beta=None) -> pd.Series:
    """The lune depths (containment in _containment.LENS_DEPTHS) of the columns `to_compute` of the single frame in `data`:
    the share of the C(n, 2) pairs of curves (x_i, x_j) whose beta-lune holds the curve x -- 'lens' (beta = 2; Liu & Modarres
    2011): ||x - x_i|| and ||x - x_j|| both at most ||x_i - x_j||; 'spherical' (beta = 1; Elmore, Hettmansperger & Xuan 2006): x in
    the ball with diameter x_i x_j; 'beta_skeleton' (Yang & Modarres 2018): any beta in [1, inf].  L2 norms as plain sums over
    the timepoints.  The curve's own pairs count, as in the papers.  One upload, one device call for the integer counts
    (sd_lens_counts), one division.  The beta used is in the result's attrs['beta'].  Labels, `to_compute` and the result's
    order are those of 'r2'.  Refused before anything is uploaded: what 'hmodal' refuses of the data, `quantile` or
    `bandwidth` (they belong to 'hmodal'), a `beta` with 'lens' or 'spherical', none or one below 1 with 'beta_skeleton', and
    more than 16 384 curves."""
    df, X = _metric_frame(data, J, f'containment \'{containment}\'', deep_check)
    default_q = isinstance(quantile, numbers.Real) and not isinstance(quantile, bool) and quantile == 0.15
    if bandwidth is not None or not default_q:
        raise ValueError(f'containment \'{containment}\' has no bandwidth: quantile and bandwidth belong to \'hmodal\' and must '
                         f'be left at their defaults, got quantile={quantile!r}, bandwidth={bandwidth!r}.')
    cols = df.columns if to_compute is None else to_compute
    return _lens_counts_to_depths(X, _positions(df, cols), cols, containment, beta, device)


def _curve_distances(data, to_compute=None, device=None) -> pd.DataFrame:
    """The L2 distances (the square roots of sd_curve_sqdist's matrix) of the columns `to_compute` (default: all) of a
    frame, or of the single frame of a list, to all of its columns: rows `to_compute`, columns the frame's labels."""
    frames = data if isinstance(data, list) else [data]
    df, X = _metric_frame(frames, 2, 'CurveDistances')
    rows = df.columns if to_compute is None else to_compute
    D2 = engine.curve_sqdist(X, _positions(df, rows), device=device)
    return pd.DataFrame(np.sqrt(D2), index=rows, columns=df.columns)


def _cloud_depth_values(records, n: int, T: int, containment: str, aggregate: str) -> np.ndarray:
    """The records [m, 2] of engine.multi_halfspace_sums (SH, MH: int64) or engine.multi_projection_sums (PS, OM: fp64) of
    curves among n at T timepoints -> the fp64 depths: one division each ('projection', 'inf': one addition as well)."""
    if containment == 'halfspace':
        R = np.asarray(records, dtype=np.int64).reshape(-1, 2)
        if aggregate == 'mean':
            return R[:, 0].astype(np.float64) / np.float64(np.int64(n) * np.int64(T))
        return R[:, 1].astype(np.float64) / np.float64(n)
    R = np.asarray(records, dtype=np.float64).reshape(-1, 2)
    if aggregate == 'mean':
        return R[:, 0] / np.float64(T)
    return 1.0 / (1.0 + R[:, 1])                         # OM = inf: 0.0


def _cloud_inputs(data, to_compute, what: str, projection: bool, deep_check=False, directions=1000, seed=0):
    """The validation and the labels shared by the depths of curves over time (_cloud_depths) and their directional
    outlyingness (_directional): (P [n, T, d], U [k, d], target positions, the result's index).  `what` names the caller in
    the refusals; `projection`: the values also pass engine.projection_check.  Nothing is uploaded here."""
    def refuse(reason):
        raise ValueError(f'{what} {reason}')

    if not isinstance(data, list):
        raise ValueError('data must be passed as a list.')
    if len(data) == 0:
        raise ValueError('No data passed.')
    if deep_check:
        _deep_check(data)
    if len(data) == 1:                                   # univariate: the columns are the curves
        df = data[0]
        _require_unique_labels(df)
        P = np.ascontiguousarray(df.to_numpy(dtype=np.float64).T)[:, :, None]
        index = df.columns if to_compute is None else to_compute
        targets = _positions(df, index)
    else:
        shape = np.shape(data[0])
        if len(shape) != 2 or any(np.shape(f) != shape for f in data):
            refuse(f'needs frames of one shape (timepoints x features), got {sorted(set(np.shape(f) for f in data))}.')
        P = _curves_tensor(data)
        index = [i for i in range(len(data))] if to_compute is None else to_compute
        targets = np.asarray(list(index), dtype=np.int64)
    n, T, d = P.shape
    if n < 2:
        refuse(f'needs at least 2 curves, got {n}.')
    if T < 1:
        refuse('needs at least one timepoint.')
    if d < 1:
        refuse('needs at least one feature.')
    if d > 8:
        refuse(f'is implemented for at most 8 features, got {d}.')
    if not np.isfinite(P).all():
        refuse('does not take NaN or infinite values: drop or fill them first.')
    if projection:
        engine.projection_check('coordinates', P)        # |x| <= 2^500: no projection or midpoint overflows
    if isinstance(directions, str):
        if directions != 'exact':
            refuse(f"takes a positive number of directions, a (k x {d}) array or 'exact', got directions={directions!r}.")
        if d != 1:
            raise NotImplementedError(f"{what} of curves with directions='exact' is implemented for "
                                      f"one feature (where the direction (1.0) is exact), got d = {d}")
        U = np.ones((1, 1), dtype=np.float64)
    else:
        U = _halfspace_directions(directions, seed, d)   # finite, no all-zero row
    if projection:
        engine.projection_check('direction entries', U)
    return P, U, targets, index


def _cloud_depths(data, to_compute, J, containment: str, deep_check=False, device=None, directions=1000, seed=0,
                  aggregate='mean') -> pd.Series:
    """The halfspace or the projection depth of curves over time (containment in _containment.CLOUD_DEPTHS): the depth of
    the point X(t) inside the cloud of all curves' points at t -- PointcloudDepth's 'halfspace' / 'projection' over the
    direction set (`directions`, `seed`), the same for every t -- averaged over t (aggregate='mean': the multivariate
    functional halfspace depth of Claeskens et al. 2014, resp. the mean of 1 / (1 + O_t)) or its infimum over t ('inf').
    One device call for the records (sd_multi_halfspace_sums / sd_multi_projection_sums), the normalisation on the host.
    A list of n >= 2 frames (T x d each): the curves are the frames, `to_compute` and the result's index are list
    positions, as for 'simplex'.  A list of one frame: its columns are the curves (d = 1, the direction [[1.0]]), labels
    and `to_compute` as for 'r2'.  What cannot be computed is refused here, before anything is uploaded."""
    def refuse(reason):
        raise ValueError(f'containment \'{containment}\' {reason}')

    if not isinstance(data, list):
        raise ValueError('data must be passed as a list.')
    if len(data) == 0:
        raise ValueError('No data passed.')
    if not isinstance(J, numbers.Integral) or isinstance(J, bool) or J != 2:
        refuse(f'has no band size: J must be left at its default 2, got {J!r}.')
    if aggregate not in ('mean', 'inf'):
        refuse(f"takes aggregate='mean' (the average over the timepoints) or 'inf' (their infimum), got {aggregate!r}.")
    P, U, targets, index = _cloud_inputs(data, to_compute, f'containment \'{containment}\'', containment == 'projection',
                                         deep_check=deep_check, directions=directions, seed=seed)
    n, T, d = P.shape
    sums = engine.multi_halfspace_sums if containment == 'halfspace' else engine.multi_projection_sums
    records = sums(P, U, targets, device=device)
    return pd.Series(index=index, data=_cloud_depth_values(records, n, T, containment, aggregate))


def _functionaldepth(data: List[pd.DataFrame], to_compute: Union[list, pd.Index] = None, J=2, containment='r2',
                     relax=False, deep_check=False, quiet=True, device=None, algo='auto', directions=1000, seed=0,
                     aggregate='mean', quantile=0.15, bandwidth=None, beta=None) -> pd.Series:
    if _is_lens_depth(containment):                      # as 'spatial', with `beta`
        return _lens_depths(data, to_compute, J, containment, deep_check=deep_check, device=device, quantile=quantile,
                            bandwidth=bandwidth, beta=beta)
    if _is_metric_depth(containment):                    # `relax` and `algo` have nothing to select
        return _metric_depths(data, to_compute, J, containment, deep_check=deep_check, device=device, quantile=quantile,
                              bandwidth=bandwidth)
    if _is_spatial_depth(containment):                   # as 'hmodal'; `quantile` and `bandwidth` are refused
        return _spatial_depths(data, to_compute, J, containment, deep_check=deep_check, device=device, quantile=quantile,
                               bandwidth=bandwidth)
    if _is_cloud_depth(containment):                     # multivariate too; `relax` and `algo` have nothing to select
        return _cloud_depths(data, to_compute, J, containment, deep_check=deep_check, device=device,
                             directions=directions, seed=seed, aggregate=aggregate)
    if _is_rank_depth(containment):                      # not a band depth: `relax` and `algo` have nothing to select
        return _rank_depths(data, to_compute, J, containment, deep_check=deep_check, device=device)
    if _is_projected_depth(containment):                 # as the rank depths, with `directions` and `seed`
        return _projected_depths(data, to_compute, J, containment, deep_check=deep_check, device=device,
                                 directions=directions, seed=seed)
    if _is_order_depth(containment):
        return _extremal_depth(data, to_compute, J, containment, deep_check=deep_check, device=device)
    if _is_shape_depth(containment):
        return _shape_depths(data, to_compute, J, containment, deep_check=deep_check, device=device)
    _handle_depth_errors(data=data, J=J, containment=containment, relax=relax, deep_check=deep_check)
    cdef = _select_containment(containment=containment)

    if len(data) == 1:                                   # real-valued case by assumption (:60-61)
        if cdef == 'simplex':
            cdef = 'r2'                                  # (:62-63)
        df = data[0]
        _require_unique_labels(df)
        cols = df.columns if to_compute is None else to_compute     # (:68-71)
        if cdef == 'r2':
            depths = _univariate_depths(df, cols, J, relax, device=device, algo=algo)
        elif cdef == 'r2_enum':
            raise NotImplementedError                    # _containment.py:103
        else:
            depths = [_callable_band_depth(df, col, relax, cdef, J) for col in cols]
        return pd.Series(index=cols, data=depths)        # (:78)

    # multivariate case (:79-95)
    if cdef == 'simplex':
        f = [i for i in range(len(data))] if to_compute is None else to_compute
        P = _curves_tensor(data)
        n, T, d = P.shape
        counts = engine.multi_simplex_counts(P, np.asarray(list(f), dtype=np.int64), relax=relax,
                                             device=device).astype(np.float64)
        if relax:
            counts = counts / T                          # _containment.py:136
        depths = counts / binom(n - 1, d + 1)            # (:278,286): n there = number of OTHERS
        return pd.Series(index=f, data=depths)
    if cdef == 'r2_enum':
        return _componentwise_band_depth(data, to_compute, J, relax, device)
    raise NotImplementedError('custom containment callables are only supported for univariate data')


def _sample_blocks(df: pd.DataFrame, orig: pd.DataFrame, ss: int, K: int):
    """The reference's block draws (:172-183), in draw order: for each target column of `orig`, K blocks of `ss` curves
    drawn without replacement from the pool `df` with the global numpy RNG (`df.sample(n=ss, axis=1)`, :176), the
    pool reset to `orig` -- it shrinks to the targets, as in the reference -- after each target.  Yields (target label,
    the drawn frame, member labels with the target appended where it was not drawn, :178)."""
    for col in orig.columns:
        for _ in range(K):
            t = df.sample(n=ss, axis=1)                  # (:176) global numpy RNG
            df = df.drop(t.columns, axis=1)              # (:177) without replacement across blocks
            members = list(t.columns)
            if col not in members:
                members.append(col)                      # (:178) force the target into the block
            yield col, t, members
        df = orig.copy()                                 # (:183) -- the pool shrinks to `cols`, as in the reference


def _samplefunctionaldepth(data: List[pd.DataFrame], K: int, to_compute: Union[list, pd.Index] = None, J=2,
                           containment='r2', relax=False, deep_check=False, quiet=True, device=None,
                           algo='auto') -> pd.Series:
    """K-block sampled band depth (:99-196).

    Block selection is host logic and consumes the global numpy RNG exactly as the
    reference does (`df.sample(n=ss, axis=1)`, :176), so `np.random.seed` reproduces the
    reference's blocks; each block's depth is one device call.
    """
    samples = []
    if (_is_rank_depth(containment) or _is_order_depth(containment) or _is_shape_depth(containment)
            or _is_cloud_depth(containment) or _is_metric_depth(containment) or _is_spatial_depth(containment)
            or _is_lens_depth(containment) or _is_projected_depth(containment)):
        raise ValueError(f'containment \'{containment}\' has no K-block estimator: K must be None.')
    _handle_depth_errors(data=data, J=J, containment=containment, relax=relax, deep_check=deep_check)
    cdef = _select_containment(containment=containment)
    if len(data) != 1:
        return pd.Series(dtype=np.float64)               # reference stub returns an empty list (:187-196)

    df = data[0]
    _require_unique_labels(df)
    cols = df.columns if to_compute is None else to_compute
    orig = df.loc[:, cols]                               # (:161)
    ss = df.shape[1] // K                                # (:162)
    if ss == 0:
        raise DepthDegeneracy(f'Block size {K} is too large, not enough functions to sample.')
    if cdef == 'simplex':
        cdef = 'r2'
    if cdef == 'r2_enum':
        raise NotImplementedError

    # every (target, block) pair in one launch: relax=True always; the reference's default relax=False for J = 2 (the
    # blocks' masks in LDS, or in the workspace when n / K runs into the thousands)
    batched = cdef == 'r2' and (relax or (J == 2 and _BATCH_STRICT_BLOCKS))
    blocks, block_targets = [], []           # column positions (in data[0]) of every block, in draw order
    full = data[0]
    depths = []
    for col, t, members in _sample_blocks(df, orig, ss, K):
        if batched:
            blocks.append(full.columns.get_indexer(members))
            block_targets.append(full.columns.get_loc(col))
            continue
        t = t.copy()
        t.loc[:, col] = orig.loc[:, col]
        if cdef == 'r2':
            depths.append(_univariate_depths(t, [col], J, relax, device=device, algo='pairwise')[0])
        else:
            depths.append(_callable_band_depth(t, col, relax, cdef, J))
        if len(depths) == K:
            samples.append(np.mean(depths))              # (:182)
            depths = []
    if len(orig.columns):
        df = orig                                        # (:183) the pool the reference's loop leaves behind
    if batched:
        # every (target, block) pair of the estimator in ONE launch
        mem = _padded_members(blocks)
        X = full.to_numpy(dtype=np.float64)
        T = X.shape[0]
        if relax:
            counts = engine.mbd_subset_counts(X, mem, np.asarray(block_targets, dtype=np.int32), J=J,
                                              device=device).astype(np.float64) / T
        else:
            counts = engine.bd_strict_subset_counts(X, mem, np.asarray(block_targets, dtype=np.int32),
                                                    device=device).astype(np.float64)[:, None]
        sizes = np.array([len(b) for b in blocks], dtype=np.float64)
        depth = _band_depth_sum(counts, sizes, J)        # (:253) n = block size including the target
        samples = [np.mean(depth[i * K:(i + 1) * K]) for i in range(len(orig.columns))]
    return pd.Series(index=df.columns, data=samples)     # (:186)
