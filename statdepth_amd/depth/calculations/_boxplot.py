"""The functional boxplot on the HIP engine (K16; no counterpart in the reference, whose result objects stop at
`ordered` / `deepest` / `outlying`).

Sun & Genton (2011) draw it from the central regions of the modified band depth, Narisetty & Nair (2016) from the extremal
depth; any depth of the curves will do.  The host ranks the curves and gives each one byte, the device does the rest in
one call (engine.central_regions): the envelope of every region, the fence of the box region, how often each curve
leaves the fence, and the whiskers.

    order = argsort(-depth, stable)          ties: the earlier column is deeper
    region of the fraction a                 the first min(n, max(1, ceil(a n))) curves of that order
    envelope                                 pointwise min and max over the region
    fence                                    lower - F (upper - lower), upper + F (upper - lower) of the box region
    outlier                                  a curve below or above the fence at some timepoint
    whiskers                                 pointwise min and max over the curves that are not outliers
"""
import math

import numpy as np
import pandas as pd

from ... import engine
from .. import _plotting
from ._functional import _require_unique_labels

__all__ = ['_region_levels', 'FunctionalBoxplotResult']

MAX_REGIONS = 8                    # levels one call of sd_central_regions takes


def _region_levels(depth, alphas, n: int) -> np.ndarray:
    """uint8[n]: for ascending fractions `alphas` (L of them), the smallest l whose region holds curve i, else L."""
    depth = np.asarray(depth, dtype=np.float64)
    if depth.shape != (n,):
        raise ValueError('one depth per curve is needed')
    L = len(alphas)
    order = np.argsort(-depth, kind='stable')
    rank = np.empty(n, dtype=np.int64)
    rank[order] = np.arange(n)
    level = np.full(n, L, dtype=np.uint8)
    for l in range(L - 1, -1, -1):
        size = min(n, max(1, math.ceil(alphas[l] * n)))
        level[rank < size] = l
    return level


class FunctionalBoxplotResult:
    """What a functional boxplot consists of.

    median     the label of the deepest curve (ties: the earlier column)
    envelope   DataFrame on the frame's time index, columns 'lower' and 'upper': the region of `alpha` (the box)
    regions    {fraction: DataFrame like envelope} for `alpha` and every further fraction, ascending
    fence      DataFrame 'lower' / 'upper': the envelope inflated by `factor` times its pointwise width
    outside    DataFrame per curve label, int columns 'below' and 'above': timepoints at which the curve leaves the fence
    outliers   Index of the labels with any such timepoint, in column order
    whiskers   DataFrame 'lower' / 'upper': min and max over the curves that are not outliers
    depths     the depths the regions were built from, in column order
    """

    def __init__(self, data, depths, alpha, factor, median, envelope, regions, fence, outside, outliers, whiskers):
        self.data, self.depths, self.alpha, self.factor = data, depths, alpha, factor
        self.median, self.envelope, self.regions, self.fence = median, envelope, regions, fence
        self.outside, self.outliers, self.whiskers = outside, outliers, whiskers

    def __repr__(self):
        return (f'FunctionalBoxplotResult(alpha={self.alpha}, factor={self.factor}, median={self.median!r}, '
                f'outliers={list(self.outliers)!r})')

    def plot(self, return_plot=False, title=None, xaxis_title=None, yaxis_title=None, showlegend=False):
        '''Region band(s), whiskers, the median curve, and the outliers in red.'''
        return _plotting.boxplot_figure(self, title, xaxis_title, yaxis_title, return_plot, showlegend)


def _single_frame(data) -> pd.DataFrame:
    if isinstance(data, pd.DataFrame):
        return data
    if not isinstance(data, (list, tuple)) or len(data) == 0:
        raise ValueError('data must be a DataFrame whose columns are the curves, or a list holding one.')
    if len(data) != 1:
        raise ValueError('the functional boxplot is defined for univariate curves: exactly one DataFrame, '
                         f'got {len(data)}.')
    return data[0]


def _fractions(alpha, levels):
    """(ascending distinct fractions, position of alpha among them), or the refusal."""
    try:
        alpha = float(alpha)
        fr = sorted({alpha, *(float(a) for a in levels)})
    except (TypeError, ValueError) as e:
        raise ValueError('alpha and levels must be numbers in (0, 1].') from e
    if not all(0.0 < a <= 1.0 for a in fr):                      # NaN fails too
        raise ValueError(f'fractions must lie in (0, 1], got {fr}.')
    if len(fr) > MAX_REGIONS:
        raise ValueError(f'at most {MAX_REGIONS} distinct fractions are drawn at once, got {len(fr)}.')
    return fr, fr.index(alpha)


def _check_boxplot(data, alpha, factor, levels):
    """(frame, its T x n fp64 matrix, fractions, box) or the ValueError, before anything is uploaded."""
    df = _single_frame(data)
    fr, box = _fractions(alpha, levels)
    try:
        ok = math.isfinite(factor) and factor >= 0
    except TypeError:
        ok = False
    if not ok:
        raise ValueError(f'factor must be a finite number >= 0, got {factor!r}.')
    _require_unique_labels(df)
    X = df.to_numpy(dtype=np.float64, copy=False)                # keeps the frame's memory layout
    if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError('the functional boxplot needs at least one curve and one timepoint.')
    if np.isnan(X).any():
        raise ValueError('the functional boxplot does not take NaN in the data: drop or fill them first.')
    return df, X, fr, box


def _aligned_depths(df: pd.DataFrame, depths) -> pd.Series:
    """`depths` as a plain Series in column order; it must name every column exactly once and hold no NaN."""
    if not isinstance(depths, pd.Series):
        raise ValueError('depths must be a Series (or a depth result) indexed by the column labels.')
    d = pd.Series(np.asarray(depths, dtype=np.float64), index=depths.index)
    if not d.index.is_unique or len(d) != df.shape[1] or not d.index.isin(df.columns).all():
        raise ValueError('depths must cover every column of the data exactly once.')
    d = d.reindex(df.columns)
    if d.isna().any():
        raise ValueError('depths must not hold NaN.')
    return d


def _frame(index, pair) -> pd.DataFrame:
    return pd.DataFrame({'lower': pair[0], 'upper': pair[1]}, index=index)


def _central_region(data, depths, alpha=0.5, device=None) -> pd.DataFrame:
    """The envelope ('lower', 'upper' on the time index) of the deepest fraction `alpha` of the curves."""
    df, X, fr, box = _check_boxplot(data, alpha, 0.0, ())
    d = _aligned_depths(df, depths)
    level = _region_levels(d.to_numpy(), fr, X.shape[1])
    env, _, _, _ = engine.central_regions(X, level, L=1, box=None, device=device)
    return _frame(df.index, env[0])


def _functional_boxplot(df, X, fr, box, depths, factor, device=None) -> FunctionalBoxplotResult:
    """The boxplot of a checked frame (_check_boxplot) from `depths`."""
    d = _aligned_depths(df, depths)
    n = X.shape[1]
    level = _region_levels(d.to_numpy(), fr, n)
    env, fence, outside, whisker = engine.central_regions(X, level, L=len(fr), box=box, factor=float(factor), whiskers=True,
                                                          device=device)
    median = df.columns[int(np.argsort(-d.to_numpy(), kind='stable')[0])]
    regions = {a: _frame(df.index, env[l]) for l, a in enumerate(fr)}
    counts = pd.DataFrame({'below': outside[:, 0], 'above': outside[:, 1]}, index=df.columns)
    outliers = df.columns[(outside != 0).any(axis=1)]
    return FunctionalBoxplotResult(data=df, depths=d, alpha=fr[box], factor=float(factor), median=median,
                                   envelope=regions[fr[box]], regions=regions, fence=_frame(df.index, fence), outside=counts,
                                   outliers=outliers, whiskers=_frame(df.index, whisker))
