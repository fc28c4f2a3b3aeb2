"""Public factories and result objects (reference: statdepth/depth/depth.py).

`FunctionalDepth` (:362-402) and `PointcloudDepth` (:347-359) keep the reference's
signatures; `device=`, `algo=` and, for containment='halfspace' and 'projection', `directions=` and `seed=` are keyword-only additions.  `ProbabilisticDepth` is the
signature the reference documents (docs/index.md §5.1.3) and lists in `__all__` (:11) without
implementing it, plus `to_compute` and the keyword-only `device=`.  Result classes keep
the reference's method names and conventions (:14-65,178-185,337-341), including the
plotly views (:91-175,193-335; `_plotting.py`, host-side visualisation outside the hot path).
"""
import math
from typing import List

import numpy as np
import pandas as pd

from abc import ABC, abstractmethod
from .calculations._functional import _curve_distances, _curve_projections, _functionaldepth, _samplefunctionaldepth
from .calculations._helper import DepthDegeneracy   # noqa: F401
from .calculations._containment import _is_lens_depth
from .calculations._pointcloud import _lens_cloud_depths, _pointwisedepth, _samplepointwisedepth
from .calculations._uncertainty import _probabilistic_band_depth
from .calculations import _boxplot
from .calculations._boxplot import FunctionalBoxplotResult
from .calculations import _directional
from .calculations._directional import DirectionalOutlyingnessResult, MSPlotOutlierResult
from . import _plotting

__all__ = ['FunctionalDepth', 'PointcloudDepth', 'ProbabilisticDepth', 'FunctionalBoxplot', 'TotalVariationOutliers',
           'DirectionalOutlyingness', 'MSPlotOutliers', 'CurveDistances']


class AbstractDepth(ABC):
    """What every depth result can do (reference: statdepth/depth/abstract.py:3-18)."""

    @abstractmethod
    def ordered(self, ascending=False): ...

    @abstractmethod
    def deepest(self, n=1): ...

    @abstractmethod
    def outlying(self, n=1): ...


class _FunctionalDepthSeries(AbstractDepth, pd.Series):
    """The depth values as a Series that also remembers the data they were computed from (:14-65).

    Ordering conventions of the reference are kept: `ordered()` caches the FIRST ordering it is asked for
    (:25-27), `deepest`/`outlying` read the head/tail of a descending ordering (:29-46), `quartile` ignores
    its argument and returns the lower half (:55-56).  Ties are ordered by `Series.sort_values`'s default
    sort, like the reference.
    """

    def __init__(self, df: pd.DataFrame, depths: pd.Series):
        super().__init__(data=depths)
        # plain attributes (bypassing pandas' attribute machinery); a reference to the frame, not a copy (:19)
        for name, value in (('_orig_data', df), ('_depths', depths), ('_ordered_depths', None)):
            object.__setattr__(self, name, value)

    def _ranking(self, ascending=False) -> pd.Series:
        cached = self._ordered_depths
        if cached is None:
            cached = self._depths.sort_values(ascending=ascending)
            object.__setattr__(self, '_ordered_depths', cached)
        return cached

    @staticmethod
    def _slice(ranked: pd.Series, sel) -> pd.Series:
        return pd.Series(index=list(ranked.index[sel]), data=list(ranked.values[sel]))

    def ordered(self, ascending=False) -> pd.Series:
        return self._ranking(ascending)

    def deepest(self, n=1) -> pd.Series:
        return self._slice(self._ranking(False), slice(0, n))

    def outlying(self, n=1) -> pd.Series:
        return self._slice(self._ranking(False), slice(-n, None))

    # aliases (:48-65)
    def sorted(self, ascending=False):
        return self.ordered(ascending=ascending)

    def median(self):
        return self.deepest(n=1)

    def quartile(self, ratio=0.5):
        return self._depths.sort_values().head(int(self._depths.shape[0] * 0.5))

    def get_depths(self):
        return self._depths

    def depths(self):
        return self._depths

    def get_data(self):
        return self._orig_data


class _FunctionalDepthUnivariate(_FunctionalDepthSeries):
    '''Univariate curves are the COLUMNS of the frame (:178-185).'''

    def drop_outlying_data(self, n=1) -> pd.DataFrame:
        return self._orig_data.drop(self.outlying(n=n).index, axis=1)

    def get_deepest_data(self, n=1) -> pd.DataFrame:
        return self._orig_data.loc[:, self.deepest(n=n).index]

    def get_outlying_data(self, n=1) -> pd.DataFrame:
        return self._orig_data.loc[:, self.outlying(n=n).index]

    def plot_deepest(self, n=1, title=None, xaxis_title=None, yaxis_title=None, return_plot=False, showlegend=False):
        '''All curves, the n deepest in red (:141-157).'''
        return _plotting.curves_figure(self._orig_data, self.deepest(n=n).index, title, xaxis_title, yaxis_title,
                                       return_plot, showlegend)

    def plot_outlying(self, n=1, title=None, xaxis_title=None, yaxis_title=None, return_plot=False, showlegend=False):
        '''All curves, the n most outlying in red (:159-175).'''
        return _plotting.curves_figure(self._orig_data, self.outlying(n=n).index, title, xaxis_title, yaxis_title,
                                       return_plot, showlegend)

    def central_region(self, alpha=0.5, device=None) -> pd.DataFrame:
        '''The envelope ('lower' and 'upper' on the time index) of the deepest fraction `alpha` of the curves by these
        depths.  ValueError unless every column of the data has a depth (a result of `to_compute` or `K` has not).'''
        return _boxplot._central_region(self._orig_data, self._depths, alpha=alpha, device=device)

    def boxplot(self, alpha=0.5, factor=1.5, levels=(), device=None) -> FunctionalBoxplotResult:
        '''The functional boxplot of the data by these depths: FunctionalBoxplot(data, depths=self, ...).'''
        return FunctionalBoxplot(self._orig_data, self._depths, alpha=alpha, factor=factor, levels=levels, device=device)


class _PointwiseDepth(_FunctionalDepthSeries):
    '''Points are the ROWS of the frame (:337-341).'''

    def drop_outlying_data(self, n=1) -> pd.DataFrame:
        return self._orig_data.drop(self.outlying(n=n).index, axis=0)

    def get_deepest_data(self, n=1) -> pd.DataFrame:
        return self._orig_data.loc[self.deepest(n=n).index, :]

    def plot_depths(self, invert_colors=False, marker=None, return_plot=False, title='', xaxis_title=None,
                    yaxis_title=None):
        '''Points coloured by depth (:193-243).'''
        return _plotting.depth_coloured_figure(self._orig_data, self._depths, invert_colors, marker, return_plot, title,
                                               xaxis_title, yaxis_title)

    def plot_distribution(self, invert_colors=False, marker=None):
        '''Alias of plot_depths, shown at once (:343-344).'''
        return self.plot_depths(invert_colors=invert_colors, marker=marker)

    def plot_deepest(self, n=1, return_plot=False, title='', xaxis_title=None, yaxis_title=None):
        '''All points in blue, the n deepest in red (:309-321).'''
        return _plotting.points_figure(self._orig_data, self.deepest(n=n).index, return_plot, title, xaxis_title,
                                       yaxis_title)

    def plot_outlying(self, n=1, return_plot=False, title='', xaxis_title=None, yaxis_title=None):
        '''All points in blue, the n most outlying in red (:323-335).'''
        return _plotting.points_figure(self._orig_data, self.outlying(n=n).index, return_plot, title, xaxis_title,
                                       yaxis_title)


def PointcloudDepth(data: pd.DataFrame, to_compute: pd.Index = None, K=None, containment='simplex', quiet=True,
                    *, device=None, directions=1000, seed=0) -> _PointwiseDepth:
    """`directions` and `seed` belong to containment='halfspace' and containment='projection' (every other containment
    ignores them): an int k asks for k unit directions drawn from `np.random.default_rng(seed)`, a (k x d) array is used
    as given.  For 'halfspace' both give the directional depth, an upper bound of the halfspace depth once d >= 2, and
    'exact' gives the halfspace depth itself for d <= 2 (`seed` is ignored; d >= 3 raises NotImplementedError).  For
    'projection' they are the directions of the Stahel-Donoho outlyingness O = max |x.u - med| / MAD, depth =
    1 / (1 + O); there 'exact' raises NotImplementedError.
    containment='simplex_exact' is 'simplex' for planar data (d = 2; any other d raises NotImplementedError) counted by an
    angular sweep with exact orientation signs, O(n log^2 n) per point: the closed triangles of the other points that
    contain the point, over C(n, 3).  'simplex' itself keeps its enumeration and its tolerance.
    containment='lens' and 'spherical' are FunctionalDepth's lune depths of the rows as points of R^d, any d >= 1 (they need
    nothing of the data but Euclidean distances): the share of the C(n, 2) pairs of points whose lens (beta = 2), resp. whose
    ball with the pair as a diameter (beta = 1), holds the point; the beta is in the result's attrs['beta'].  ValueError for
    `K` other than None, NaN or infinite values, magnitudes above 2^480, fewer than 2 or more than 16 384 points.  This
    function has no `beta` argument, so 'beta_skeleton' is refused here with the call that computes it:
    FunctionalDepth([data.T], containment='beta_skeleton', beta=...), whose curves are the points."""
    if _is_lens_depth(containment):
        depth = _lens_cloud_depths(data=data, to_compute=to_compute, K=K, containment=containment, device=device)
        result = _PointwiseDepth(df=data, depths=depth)
        result.attrs['beta'] = depth.attrs['beta']
        return result
    if K is not None:
        depth = _samplepointwisedepth(data=data, to_compute=to_compute, K=K, containment=containment,
                                      device=device, directions=directions, seed=seed)
    else:
        depth = _pointwisedepth(data=data, to_compute=to_compute, containment=containment, device=device,
                                directions=directions, seed=seed)
    return _PointwiseDepth(df=data, depths=depth)


def FunctionalDepth(data: List[pd.DataFrame], to_compute=None, K=None, J=2, containment='r2', relax=False,
                    deep_check=False, quiet=True, *, device=None, algo='auto', directions=1000, seed=0, aggregate='mean',
                    quantile=0.15, bandwidth=None, beta=None):
    """Band depth of curves ('r2', 'r2_enum', 'simplex' or a callable), as in the reference.

    For univariate data (`data` a list of one frame whose columns are the curves) `containment` also names the integrated
    rank depths, all computed from the per-timepoint counts of curves strictly above and strictly below:
    'fm' (Fraiman-Muniz, 1 - |1/2 - F_t(x(t))| averaged over t with the "<=" empirical CDF, hence not symmetric under
    x -> -x), 'mei' and 'mhi' (modified epigraph and hypograph index: the mean proportion of curves at or above, resp. at
    or below the curve), 'half_region' (their minimum, the modified half-region depth), 'integrated_halfspace' and
    'infimal_halfspace' (mean and infimum over t of the univariate Tukey depth).  Labels, `to_compute` and the result
    object are those of 'r2'.  These are the integrated ("modified") forms, so `relax` is accepted and ignored -- there
    is no strict form to select -- and `algo` is ignored too.  ValueError for multivariate data, `K` other than None, `J`
    other than 2, NaN anywhere in the frame, or fewer than 2 curves.

    Under the same rules `containment` names the two depths of Huang & Sun (2019), which look at two consecutive timepoints
    at once: 'tvd', the total variation depth (mean over t of a (n - a) / n^2, a the number of curves at or below the curve,
    at most 1/4), and 'mss', the modified shape similarity (the squared phi coefficient of "at or below at t - 1" and "at or
    below at t" over the sample, averaged over the steps with the curve's own |increments| as weights; 1 where the curve is
    the highest at either timepoint).  'mss' also needs 2 timepoints and finite values.  `.boxplot()` and
    `.central_region()` of a 'tvd' result work as for any depth; TotalVariationOutliers runs the paper's outlier rule.

    containment='halfspace' and 'projection' take multivariate curves as well: a list of n >= 2 frames, each T x d with d <= 8
    (`to_compute` and the result's index are list positions, as for 'simplex'), or a list of one frame whose columns are the
    curves (d = 1).  The depth of a curve is PointcloudDepth's depth of its point X(t) inside the cloud of all curves' points
    at t, over one direction set for every t -- `directions` and `seed` mean what they mean there; 'exact' only for d = 1 --
    aggregated over t: aggregate='mean' averages (for 'halfspace' the multivariate functional halfspace depth of Claeskens,
    Hubert, Slaets & Vakili 2014), aggregate='inf' takes the infimum.  Every other containment ignores the three arguments.
    `relax` and `algo` are ignored; ValueError for `K` other than None, `J` other than 2, frames of unequal shape, NaN or
    infinite values, fewer than 2 curves, no timepoint or more than 8 features.

    containment='hmodal' (univariate data, under the rules of the rank depths) is the h-modal depth of Cuevas, Febrero &
    Fraiman (2006), built on the L2 distances between whole curves, not on pointwise order: (1/n) sum_j exp(-||x - x_j||^2 /
    (2 h^2)) over all n curves, the curve itself included, in (0, 1]; ||.||^2 is the plain sum of squared differences over the
    timepoints.  `bandwidth` gives h (positive, finite); otherwise h is the quantile `quantile` in (0, 1] (default 0.15) of
    the distances over the pairs of curves, taken as an order statistic: the k-th smallest, k = max(1, ceil(quantile n (n - 1)
    / 2)).  fda.usc's depth.mode interpolates between order statistics (type 7), so its h differs slightly.  The bandwidth
    used is the attribute `bandwidth` of the result.  ValueError also for infinite values or magnitudes above 2^480, for both
    `bandwidth` and a `quantile` other than the default, and where the quantile of the distances is 0 (that share of the
    pairs of curves coincides).  Every other containment but 'spatial' ignores the two arguments.

    containment='spatial' (univariate data, under the rules of 'hmodal') is the functional spatial depth of Chakraborty &
    Chaudhuri (2014) and Sguera, Galeano & Lillo (2014), fda.usc's depth.FSD: 1 - ||(1/n) sum_j (x - x_j) / ||x - x_j|| ||, the
    norm of the mean unit vector from the other curves to the curve, in [0, 1]; ||.|| is the root of the plain sum of squared
    differences over the timepoints (a uniform grid: the quadrature weight cancels).  A curve at distance 0 from x -- x itself,
    an exact copy of it, or one so close that every squared difference underflows -- adds nothing to the sum and still counts
    in n (the papers' sum over x_j != x), so n identical curves all have depth 1; PointcloudDepth's 'l1', the same depth for
    points, returns NaN for coincident points as its reference does.  The sum over the curves runs on the device in column
    order with one fused multiply-add per term (sd_spatial_sums), so a curve's depth does not depend on `to_compute`.
    ValueError for what 'hmodal' refuses of the data, for `K` other than None, `J` other than 2, and for a `quantile` or a
    `bandwidth` other than the default (they belong to 'hmodal'); `relax` and `algo` are ignored.

    containment='lens', 'spherical' and 'beta_skeleton' (univariate data, under the rules of 'hmodal') are the lune depths: the
    share of the C(n, 2) pairs of curves (x_i, x_j) whose beta-lune holds the curve x, i.e. ||x - (l x_i + (1 - l) x_j)|| <= l ||x_i -
    x_j|| and the same with i and j swapped, l = beta / 2.  'lens' is beta = 2 (Liu & Modarres 2011: both distances from x at
    most ||x_i - x_j||), 'spherical' is beta = 1 (Elmore, Hettmansperger & Xuan 2006: x in the ball with diameter x_i x_j);
    both refuse a `beta` other than None.  'beta_skeleton' (Yang & Modarres 2018) requires `beta`, a real number >= 1 or
    math.inf.  The test runs on the squared L2 distances between whole curves (CurveDistances' numbers, squared) as
    a + kappa b <= c and b + kappa a <= c with kappa = 2 / beta - 1, every product and sum rounded on its own; the counts are
    integers (sd_lens_counts) and the depth is count / C(n, 2).  The curve's own pairs count, as in the papers' sum over all
    pairs, and so do not depend on `to_compute`.  On data whose values are not exactly representable a pair at an exact right
    angle in the reals is judged by the rounded distances.  The beta used is in the result's attrs['beta'].  ValueError for
    what 'spatial' refuses and for more than 16 384 curves (the n x n matrix of distances is kept on the device).  Every other
    containment ignores `beta`.

    containment='rp_halfspace', 'rp_fm', 'random_tukey' and 'rp_projection' (univariate data, under the rules of the rank
    depths) are the random projection depths: every curve is projected on k directions of R^T, z_r = sum_t x(t) u_r(t) (the
    plain sum over the timepoints in order; fold quadrature weights or a smooth basis into the directions), and a univariate
    depth of the n projections is taken per direction.  'rp_halfspace' averages the univariate Tukey depth min(#<=, #>=) / n
    over the directions (the random projection depth of Cuevas, Febrero & Fraiman 2007, fda.usc's depth.RP), 'rp_fm' averages
    1 - |1/2 - F_r(z_r)| with the "<=" empirical CDF, 'random_tukey' takes the minimum of the Tukey depth (the random Tukey
    depth of Cuesta-Albertos & Nieto-Reyes 2008) and 'rp_projection' is 1 / (1 + O), O the largest |z_r - med_r| / MAD_r
    (PointcloudDepth's 'projection' rules for median, MAD and a MAD of 0).  `directions` is an int k -- k unit vectors drawn
    from `np.random.default_rng(seed)`, the direction set of PointcloudDepth's 'halfspace' in R^T -- or a (k x T) array used
    as given; 'exact' raises NotImplementedError.  The projections themselves are CurveProjections.  A point cloud with any
    number of features is a set of short curves: FunctionalDepth([df.T], containment='random_tukey', directions=U) is
    PointcloudDepth(df, containment='halfspace', directions=U) and 'rp_projection' is its 'projection', without their limit
    of 8 features.  ValueError for what the rank depths refuse, for infinite values, magnitudes above 2^500 and 2^23 or more
    timepoints; `relax`, `algo`, `aggregate`, `quantile`, `bandwidth` and `beta` are ignored."""
    if K is not None:
        depth = _samplefunctionaldepth(data=data, to_compute=to_compute, K=K, J=J, containment=containment,
                                       relax=relax, deep_check=deep_check, quiet=quiet, device=device, algo=algo)
    else:
        depth = _functionaldepth(data=data, to_compute=to_compute, J=J, containment=containment, relax=relax,
                                 deep_check=deep_check, quiet=quiet, device=device, algo=algo, directions=directions,
                                 seed=seed, aggregate=aggregate, quantile=quantile, bandwidth=bandwidth, beta=beta)
    if len(data) == 1:                                   # univariate by assumption (:399-400)
        result = _FunctionalDepthUnivariate(df=data[0], depths=depth)
        if 'beta' in depth.attrs:                        # the lune depths
            result.attrs['beta'] = depth.attrs['beta']
        if 'bandwidth' in depth.attrs:                   # 'hmodal': a plain attribute, as the result's other state
            object.__setattr__(result, 'bandwidth', depth.attrs['bandwidth'])
        return result
    return _FunctionalDepthSeries(df=data[0], depths=depth)   # multivariate (:401-402)


def CurveDistances(data, to_compute=None, device=None) -> pd.DataFrame:
    """The L2 distances between univariate curves: a DataFrame with one row per curve of `to_compute` (column labels;
    default: all) and one column per curve of `data` (a DataFrame whose columns are the curves, or a list of one), entry
    sqrt(sum_t (x(t) - y(t))^2) -- the plain sum over the timepoints, no quadrature weights.  The squares are accumulated on
    the device in time order with one fused multiply-add per timepoint (sd_curve_sqdist), so the matrix of all curves is
    exactly symmetric with a zero diagonal.  ValueError, before anything is uploaded: more than one frame, duplicate labels,
    fewer than 2 curves, no timepoint, NaN or infinite values, magnitudes above 2^480."""
    return _curve_distances(data, to_compute=to_compute, device=device)


def CurveProjections(data, directions=1000, seed=0, device=None) -> pd.DataFrame:
    """The projections of univariate curves on a set of directions of R^T: a DataFrame with one row per direction and one
    column per curve of `data` (a DataFrame whose columns are the curves, or a list of one) under its label, entry
    ((x(0) u(0) + x(1) u(1)) + x(2) u(2)) + ... over the timepoints in order, every product and every sum rounded to fp64
    (sd_curve_projections).  `directions` and `seed` as for FunctionalDepth's 'rp_halfspace': an int k asks for k seeded
    unit vectors, a (k x T) array is used as given.  These are the numbers the random projection depths rank.  ValueError,
    before anything is uploaded: more than one frame, duplicate labels, fewer than 2 curves, no timepoint, NaN or infinite
    values, magnitudes above 2^500, directions of the wrong width, non-finite or with an all-zero row."""
    return _curve_projections(data, directions=directions, seed=seed, device=device)


def FunctionalBoxplot(data, depths=None, *, alpha=0.5, factor=1.5, levels=(), device=None,
                      **depth_kwargs) -> FunctionalBoxplotResult:
    """The functional boxplot of univariate curves (Sun & Genton 2011): the envelope of the deepest fraction `alpha` of
    the curves, the fence `factor` times its pointwise width beyond it, the curves that leave the fence somewhere (the
    outliers) and the envelope of the others (the whiskers), all in one device call.

    data: a DataFrame whose columns are the curves, or a list of one.  depths: a Series or a depth result indexed by the
    column labels -- any depth, the user's own or a K-sampled one included.  depths=None computes
    FunctionalDepth([data], **depth_kwargs) with relax=True unless given: the modified band depth, the paper's choice;
    containment='extremal' gives the regions of Narisetty & Nair (2016) without their simultaneous-coverage calibration.
    levels: further fractions whose regions are returned (and drawn) beside `alpha`.  Curves of equal depth are ranked in
    column order.
    ValueError, before anything is uploaded: more than one frame, duplicate labels, NaN in the data or the depths, depths
    that do not cover every column exactly once, a fraction outside (0, 1], more than 8 distinct fractions, a negative or
    non-finite factor."""
    df, X, fr, box = _boxplot._check_boxplot(data, alpha, factor, levels)
    if depths is None:
        depth_kwargs.setdefault('relax', True)
        depths = FunctionalDepth([df], device=device, **depth_kwargs)
    else:
        if depth_kwargs:
            raise ValueError(f'depths are given: {sorted(depth_kwargs)} would have no effect.')
        depths = _boxplot._aligned_depths(df, depths)
    return _boxplot._functional_boxplot(df, X, fr, box, depths, factor, device=device)


class TotalVariationOutlierResult:
    """What the two-step outlier detection of Huang & Sun (2019) returns.

    mss                 Series: the modified shape similarity of every curve, in column order
    tvd                 Series: the total variation depth of the curves that are not shape outliers, among themselves
    shape_fence         Q1 - shape_factor * (Q3 - Q1) of mss
    shape_outliers      Index of the labels with mss below the fence, in column order
    boxplot             the FunctionalBoxplotResult of the other curves by tvd
    magnitude_outliers  its outliers
    outliers            the union, in column order
    """

    def __init__(self, mss, tvd, shape_fence, shape_outliers, boxplot, magnitude_outliers, outliers):
        self.mss, self.tvd, self.shape_fence, self.shape_outliers = mss, tvd, shape_fence, shape_outliers
        self.boxplot, self.magnitude_outliers, self.outliers = boxplot, magnitude_outliers, outliers

    def __repr__(self):
        return (f'TotalVariationOutlierResult(shape_outliers={list(self.shape_outliers)!r}, '
                f'magnitude_outliers={list(self.magnitude_outliers)!r})')


def TotalVariationOutliers(data, *, shape_factor=3.0, factor=1.5, alpha=0.5, device=None) -> TotalVariationOutlierResult:
    """Shape and magnitude outliers among univariate curves by the two-step procedure of Huang & Sun (2019).

    Step 1: the modified shape similarity of every curve (FunctionalDepth(containment='mss')); with Q1 and Q3 its quartiles
    (np.quantile), the curves with MSS < Q1 - shape_factor * (Q3 - Q1) are the shape outliers -- curves that stay inside
    the bulk but oscillate or cross the others the wrong way, which no pointwise depth and no fence sees.
    Step 2: FunctionalBoxplot of the remaining curves by their total variation depth (containment='tvd', `alpha` and
    `factor` as there); its outliers are the magnitude outliers.
    data: a DataFrame whose columns are the curves, or a list of one.  ValueError for what FunctionalBoxplot or 'mss'
    refuse (NaN, infinities, fewer than 2 timepoints, duplicate labels, ...), a negative or non-finite shape_factor, or
    fewer than 2 curves left after step 1."""
    df, _, _, _ = _boxplot._check_boxplot(data, alpha, factor, ())
    try:
        ok = math.isfinite(shape_factor) and shape_factor >= 0
    except TypeError:
        ok = False
    if not ok:
        raise ValueError(f'shape_factor must be a finite number >= 0, got {shape_factor!r}.')
    mss = pd.Series(FunctionalDepth([df], containment='mss', device=device).get_depths())
    q1, q3 = np.quantile(mss.to_numpy(), [0.25, 0.75])
    shape_fence = float(q1 - shape_factor * (q3 - q1))
    is_shape = (mss < shape_fence).to_numpy()
    shape_outliers = df.columns[is_shape]
    rest = df.loc[:, ~is_shape]
    if rest.shape[1] < 2:
        raise ValueError(f'{rest.shape[1]} curve(s) left after the shape outliers: the boxplot needs at least 2.')
    tvd = pd.Series(FunctionalDepth([rest], containment='tvd', device=device).get_depths())
    box = FunctionalBoxplot(rest, tvd, alpha=alpha, factor=factor, device=device)
    flagged = is_shape | df.columns.isin(box.outliers)
    return TotalVariationOutlierResult(mss=mss, tvd=tvd, shape_fence=shape_fence, shape_outliers=shape_outliers, boxplot=box,
                                       magnitude_outliers=box.outliers, outliers=df.columns[flagged])


def DirectionalOutlyingness(data, to_compute=None, *, directions=1000, seed=0, device=None, algo='auto',
                            curves=False) -> DirectionalOutlyingnessResult:
    """The directional outlyingness of multivariate curves (Dai & Genton 2018, 2019): why a curve is shallow.

    Per timepoint the Stahel-Donoho outlyingness of the curve's point inside the cloud of all curves' points (what
    containment='projection' turns into a depth, over the same `directions` and `seed`) is given a direction: the unit
    vector from the cloud's deepest point to the curve's point.  Its mean over time, MO in R^d, is large for a curve that is
    shifted (a magnitude outlier); its variation over time, VO, is large for a curve of another shape; FO = |MO|^2 + VO.
    One device call (sd_multi_outlyingness_moments), the three numbers per curve on the host.
    data, to_compute and the index of the result as for FunctionalDepth(containment='projection'): a list of n >= 2 frames
    (T x d, d <= 8; list positions), or a list of one frame whose columns are the curves (d = 1; labels).  ValueError for
    NaN, infinities, magnitudes above 2^500, frames of unequal shape or bad `directions`, before anything is uploaded.
    Where more than half of a cloud's points share a projection (a direction's MAD is 0) the records of the curves off
    that place are infinite or NaN, as the projection depth is 0 there.  curves=True keeps the m x T x d array itself."""
    return _directional._directional_outlyingness(data, to_compute, directions=directions, seed=seed, device=device,
                                                  algo=algo, curves=curves)


def MSPlotOutliers(data, *, level=0.993, directions=1000, seed=0, mcd_seed=0, device=None) -> MSPlotOutlierResult:
    """Magnitude and shape outliers among multivariate curves by the rule of the MS-plot (Dai & Genton 2018).

    The points Y = (MO, VO) of DirectionalOutlyingness(data, directions=, seed=) in R^q, q = d + 1; their raw minimum
    covariance determinant estimator on h = (n + q + 1) // 2 points (FAST-MCD in numpy, seeded by `mcd_seed`), scaled to
    consistency at the normal model; a curve is flagged when its squared robust distance exceeds
    (q m / (m - q + 1)) F_(q, m - q + 1; level) with m the degrees of freedom of Hardin & Rocke (2005).
    ValueError for what DirectionalOutlyingness refuses, a level outside (0, 1), records that are not finite (the message
    says how many curves and why), too few curves, or more than half of the points in a hyperplane."""
    return _directional._ms_plot_outliers(data, level=level, directions=directions, seed=seed, mcd_seed=mcd_seed,
                                          device=device)


def ProbabilisticDepth(data: pd.DataFrame, sigma2: pd.DataFrame, to_compute=None, K=None, J=2, relax=False, *,
                       device=None) -> _FunctionalDepthUnivariate:
    """Band depth (J = 2) of the univariate curves in the columns of `data` when every observation carries Gaussian
    noise of the variance at the same place in `sigma2` (the expected band depth of the random curves; zero variances
    give FunctionalDepth's values).  Same containment, normalisation, `to_compute` and `K` blocks as FunctionalDepth."""
    depth = _probabilistic_band_depth(data, sigma2, to_compute=to_compute, K=K, J=J, relax=relax, device=device)
    return _FunctionalDepthUnivariate(df=data, depths=depth)
