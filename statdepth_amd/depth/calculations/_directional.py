"""Directional outlyingness of multivariate curves and the magnitude-shape plot (Dai & Genton 2018, 2019; K19).

No reference code.  The device gives, per curve, the Welford record (M_0 .. M_(d-1), Q) of its directional outlyingness
O_t over the timepoints (engine.multi_outlyingness_moments); this module turns the records into
    MO = M            the mean directional outlyingness, a vector in R^d: large for a magnitude outlier,
    VO = Q / T        its variation over time: large for a shape outlier,
    FO = |MO|^2 + VO  the total outlyingness,
and runs the outlier rule of the MS-plot on the points (MO, VO) in R^(d+1): robust Mahalanobis distances from the minimum
covariance determinant estimator (a small FAST-MCD, numpy only) against the F approximation of Hardin & Rocke (2005).
Everything below the device call is host-side numpy on n x (d + 1) numbers.
"""
import math
import numbers

import numpy as np
import pandas as pd
from scipy import stats

from ... import engine
from ._functional import _cloud_inputs

__all__ = ['DirectionalOutlyingnessResult', 'MSPlotOutlierResult', '_directional_outlyingness', '_ms_plot_outliers',
           '_fast_mcd', '_mcd_support_size', '_mcd_consistency', '_hardin_rocke', '_ms_cutoff']

_WHAT = 'DirectionalOutlyingness'


class DirectionalOutlyingnessResult:
    """The directional outlyingness of m curves among n, over T timepoints and d features.

    mean       DataFrame m x d (columns 'MO0' .. ): MO, the mean over time of the directional outlyingness
    variation  Series: VO, its variation over time
    total      Series: FO = |MO|^2 + VO
    centres    int64[T]: per timepoint the curve (position) whose point is the deepest of the cloud
    curves     float64[m, T, d]: the directional outlyingness itself (curves=True), else None
    points()   DataFrame: the MO columns and 'VO' -- the coordinates of the magnitude-shape plot
    """

    def __init__(self, mean, variation, total, centres, curves=None):
        self.mean, self.variation, self.total, self.centres, self.curves = mean, variation, total, centres, curves

    def points(self) -> pd.DataFrame:
        pts = self.mean.copy()
        pts['VO'] = self.variation.to_numpy()
        return pts

    def __repr__(self):
        return f'DirectionalOutlyingnessResult({self.mean.shape[0]} curves, d={self.mean.shape[1]}, T={len(self.centres)})'


class MSPlotOutlierResult:
    """What the outlier rule of the magnitude-shape plot returns.

    points     DataFrame n x (d + 1): (MO, VO) of every curve
    distances  Series: the squared robust Mahalanobis distance of every point (raw MCD, consistency factor applied)
    cutoff     the bound on the squared distance: (q m / (m - q + 1)) F_(q, m - q + 1; level), q = d + 1
    outliers   the labels of the curves above it, in the order of the data
    location, scatter, support   the raw MCD: mean, covariance times the consistency factor, the h points it rests on
    """

    def __init__(self, points, distances, cutoff, outliers, location, scatter, support):
        self.points, self.distances, self.cutoff, self.outliers = points, distances, cutoff, outliers
        self.location, self.scatter, self.support = location, scatter, support

    def __repr__(self):
        return f'MSPlotOutlierResult(outliers={list(self.outliers)!r}, cutoff={self.cutoff:.6g})'


def _directional_outlyingness(data, to_compute=None, directions=1000, seed=0, device=None, algo='auto',
                              curves=False) -> DirectionalOutlyingnessResult:
    P, U, targets, index = _cloud_inputs(data, to_compute, _WHAT, True, directions=directions, seed=seed)
    n, T, d = P.shape
    got = engine.multi_outlyingness_moments(P, U, targets, device=device, algo=algo, centres=True, curves=bool(curves))
    R = np.asarray(got[0], dtype=np.float64).reshape(-1, d + 1)
    index = pd.Index(index)
    with np.errstate(invalid='ignore', over='ignore'):                # (records of a timepoint with MAD 0: inf, NaN)
        vo = R[:, d] / np.float64(T)
        fo = (R[:, :d] * R[:, :d]).sum(axis=1) + vo
    mean = pd.DataFrame(R[:, :d].copy(), index=index, columns=[f'MO{e}' for e in range(d)])
    return DirectionalOutlyingnessResult(mean=mean, variation=pd.Series(vo, index=index, name='VO'),
                                         total=pd.Series(fo, index=index, name='FO'),
                                         centres=np.asarray(got[1], dtype=np.int64),
                                         curves=np.asarray(got[2], dtype=np.float64) if curves else None)


# ---------------------------------------------------------------- the minimum covariance determinant, raw
def _mcd_support_size(n: int, q: int) -> int:
    return (n + q + 1) // 2


def _mean_cov(S):
    """Mean and covariance of the rows of S with the divisor len(S) (the maximum-likelihood one, as FAST-MCD's C-step)."""
    mu = S.mean(axis=0)
    D = S - mu
    return mu, D.T @ D / np.float64(len(S))


def _c_step(Y, mu, C, h):
    """One concentration step: the h points nearest to (mu, C) in Mahalanobis distance (ties: the lower index), their mean
    and covariance.  None when the distances cannot be had (C singular to the solver, or not finite)."""
    D = Y - mu
    try:
        dist = np.einsum('ij,ij->i', D, np.linalg.solve(C, D.T).T)
    except np.linalg.LinAlgError:
        return None
    if not np.isfinite(dist).all():
        return None
    support = np.sort(np.argsort(dist, kind='stable')[:h])
    return (support,) + _mean_cov(Y[support])


def _shortest_window(x, h):
    """The length of the shortest interval that holds h of the values x: a scale that n - h outliers cannot move."""
    x = np.sort(x)
    return float((x[h - 1:] - x[:len(x) - h + 1]).min())


_MCD_FLOOR = 1e-12     # an eigenvalue at or below it, in coordinates of robust unit scale: a hyperplane
_REGULAR, _FLAT, _UNRESOLVED = 0, 1, 2


def _cov_state(C):
    """_REGULAR: the smallest eigenvalue of C lies above _MCD_FLOOR and above what rounding leaves of it (the computed
    value carries an absolute error of the order q eps times the LARGEST eigenvalue).  _FLAT: it does not, and the largest
    eigenvalue is small enough for that error to lie below the floor: a hyperplane.  _UNRESOLVED: it does not, but only
    because the points reach so far (a standard deviation of more than about 14 robust units) that fp64 cannot tell the
    smallest eigenvalue from 0: a subset that holds gross outliers, not a hyperplane."""
    lam = np.linalg.eigvalsh(C)
    if not np.isfinite(lam).all():
        return _UNRESOLVED
    noise = 16.0 * len(lam) * np.finfo(np.float64).eps * float(lam.max())
    if lam.min() > _MCD_FLOOR and lam.min() > noise:
        return _REGULAR
    return _FLAT if noise <= _MCD_FLOOR else _UNRESOLVED


def _fast_mcd(Y, h=None, seed=0, starts=500, keep=10, max_iter=200):
    """(location, covariance, support, determinant) of the raw minimum covariance determinant estimator of the rows of Y
    (n x q) on h points (default (n + q + 1) // 2): FAST-MCD of Rousseeuw & Van Driessen (1999) without its nested
    subsampling -- `starts` random (q + 1)-subsets (a subset in a hyperplane grows by random points until it spans),
    two C-steps each, the `keep` best by determinant iterated to convergence, the lowest determinant wins.  The covariance
    has the divisor h.  Deterministic for a given seed.

    ValueError when the winning h-subset is singular (then more than half of the points lie in a hyperplane).  Whether a
    covariance is singular is judged on a scale that outliers cannot move: the search runs on the coordinates divided by
    the length of their shortest window of h points (the MCD is affine equivariant, so the subsets rank as they do on Y),
    where a covariance with an eigenvalue of at most 1e-12 counts as singular however far the other n - h points lie
    (_cov_state).  A coordinate whose window has length 0 has h points in the hyperplane x_e = const.  A start that meets
    a singular h-subset ends there and competes with the determinant 0; one that meets a subset too wide for fp64 to
    resolve its smallest eigenvalue (it holds gross outliers) is left out, as is one whose distances are not finite."""
    Y = np.ascontiguousarray(np.asarray(Y, dtype=np.float64))
    if Y.ndim != 2:
        raise ValueError('the MCD takes an n x q array')
    n, q = Y.shape
    h = _mcd_support_size(n, q) if h is None else int(h)
    if not (q + 1 <= h <= n):
        raise ValueError(f'the MCD of {n} points in {q} dimensions needs q + 1 <= h <= n, got h = {h}')
    if not np.isfinite(Y).all():
        raise ValueError('the MCD takes finite points')

    def hyperplane():
        raise ValueError(f'more than half of the points lie in a hyperplane: the covariance of the {h} most concentrated '
                         f'of {n} points is singular, the robust distances are not defined')

    width = np.array([_shortest_window(Y[:, e], h) for e in range(q)])
    if not (width > 0.0).all() or not np.isfinite(width).all():
        hyperplane()                                                 # h points share a coordinate
    Z = (Y - np.median(Y, axis=0)) / width
    rng = np.random.default_rng(seed)
    cands = []                                                       # (determinant, (support, mu, C), singular)
    for _ in range(int(starts)):
        order = rng.permutation(n)
        size = q + 1
        mu, C = _mean_cov(Z[order[:size]])
        while _cov_state(C) == _FLAT and size < n:
            size += 1
            mu, C = _mean_cov(Z[order[:size]])
        state = _cov_state(C)
        if state == _FLAT:
            hyperplane()                                             # all n points
        step = None
        for _ in range(2):
            step = _c_step(Z, mu, C, h) if state == _REGULAR else None
            if step is None:
                break
            _, mu, C = step
            state = _cov_state(C)
            if state == _FLAT:
                break
        if step is not None and state != _UNRESOLVED:
            cands.append((0.0 if state == _FLAT else float(np.linalg.det(C)), step, state == _FLAT))
    if not cands:
        raise ValueError(f'the MCD of {n} points: no start out of {int(starts)} gave an h-subset that fp64 resolves')
    cands.sort(key=lambda c: (c[0], tuple(c[1][0])))
    best = None
    seen = set()
    for det, (support, mu, C), flat in cands:
        key = support.tobytes()
        if key in seen:
            continue
        seen.add(key)
        if len(seen) > keep:
            break
        for _ in range(int(max_iter)):
            step = None if flat else _c_step(Z, mu, C, h)
            state = _UNRESOLVED if step is None else _cov_state(step[2])
            if state == _UNRESOLVED:
                break
            new_det = 0.0 if state == _FLAT else float(np.linalg.det(step[2]))
            if np.array_equal(step[0], support) or not new_det < det:  # a C-step never raises the determinant: converged
                break
            support, mu, C, det, flat = step[0], step[1], step[2], new_det, state == _FLAT
        if best is None or det < best[0]:
            best = (det, support, flat)
    if best[2]:
        hyperplane()                                                 # the winner: an h-subset of determinant 0
    support = best[1]
    mu, C = _mean_cov(Y[support])                                    # in the coordinates of Y
    return mu, C, support, float(np.linalg.det(C))


# ---------------------------------------------------------------- consistency factor and cutoff
def _mcd_consistency(n: int, h: int, q: int):
    """(alpha, q_alpha, c_alpha): alpha = (n - h) / n, q_alpha the 1 - alpha quantile of chi2_q, and the factor
    c_alpha = (1 - alpha) / P(chi2_(q+2) <= q_alpha) that makes the raw MCD covariance consistent at the normal model."""
    alpha = (n - h) / n
    q_alpha = stats.chi2.ppf(1.0 - alpha, q)
    return alpha, q_alpha, (1.0 - alpha) / stats.chi2.cdf(q_alpha, q + 2)


def _hardin_rocke(n: int, h: int, q: int):
    """(m_asy, m): the degrees of freedom of the Wishart distribution that matches the MCD covariance on h of n points in
    q dimensions (Hardin & Rocke 2005): the asymptotic value and the one corrected for finite n by their simulation fit."""
    alpha, q_alpha, c_alpha = _mcd_consistency(n, h, q)
    c2 = -stats.chi2.cdf(q_alpha, q + 2) / 2.0
    c3 = -stats.chi2.cdf(q_alpha, q + 4) / 2.0
    c4 = 3.0 * c3
    b1 = c_alpha * (c3 - c4) / (1.0 - alpha)
    b2 = 0.5 + (c_alpha / q) * (c3 - (q_alpha / q) * (c2 + (1.0 - alpha) / 2.0))
    v1 = ((1.0 - alpha) * b1 ** 2 * (alpha * (c_alpha * q_alpha / q - 1.0) ** 2 - 1.0)
          - 2.0 * c3 * c_alpha ** 2 * (3.0 * (b1 - q * b2) ** 2 + (q + 2.0) * b2 * (2.0 * b1 - q * b2)))
    v2 = n * (b1 * (b1 - q * b2) * (1.0 - alpha)) ** 2 * c_alpha ** 2
    m_asy = 2.0 * v2 / (c_alpha ** 2 * v1)
    return m_asy, m_asy * math.exp(0.725 - 0.00663 * q - 0.078 * math.log(n))


def _ms_cutoff(n: int, q: int, level: float) -> float:
    """The bound on the squared robust distance of n points in q dimensions: (q m / (m - q + 1)) F_(q, m - q + 1; level)."""
    _, m = _hardin_rocke(n, _mcd_support_size(n, q), q)
    if not m - q + 1 > 0:
        raise ValueError(f'{n} curves are too few for the F approximation of the cutoff in {q} dimensions')
    return float(q * m / (m - q + 1.0) * stats.f.ppf(level, q, m - q + 1.0))


def _ms_plot_outliers(data, level=0.993, directions=1000, seed=0, mcd_seed=0, device=None) -> MSPlotOutlierResult:
    if not isinstance(level, numbers.Real) or isinstance(level, bool) or not 0.0 < level < 1.0:
        raise ValueError(f'MSPlotOutliers: level must lie in (0, 1), got {level!r}.')
    res = _directional_outlyingness(data, None, directions=directions, seed=seed, device=device)
    pts = res.points()
    Y = pts.to_numpy(dtype=np.float64)
    n, q = Y.shape
    bad = int((~np.isfinite(Y).all(axis=1)).sum())
    if bad:
        raise ValueError(f'MSPlotOutliers: the records of {bad} of {n} curves are not finite: at some timepoint a direction '
                         'sees more than half of the points at one place (its MAD is 0), so their outlyingness is infinite. '
                         'Use other directions or drop the timepoint.')
    h = _mcd_support_size(n, q)
    if h < q + 1 or n < q + 2:
        raise ValueError(f'MSPlotOutliers: {n} curves are too few for the MCD of points in {q} dimensions')
    cutoff = _ms_cutoff(n, q, float(level))
    mu, C, support, _ = _fast_mcd(Y, h, seed=mcd_seed)
    S = _mcd_consistency(n, h, q)[2] * C
    D = Y - mu
    dist = pd.Series(np.einsum('ij,ij->i', D, np.linalg.solve(S, D.T).T), index=pts.index, name='RMD2')
    return MSPlotOutlierResult(points=pts, distances=dist, cutoff=cutoff, outliers=pts.index[(dist > cutoff).to_numpy()],
                               location=mu, scatter=S, support=support)
