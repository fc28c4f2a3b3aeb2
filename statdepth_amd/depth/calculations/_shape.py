"""Total variation depth and modified shape similarity of univariate curves on the HIP engine (K17; Huang & Sun 2019, "A
decomposition of total variation depth for understanding functional outliers"; no counterpart in the reference).

The rank depths (_rank.py) and the extremal depth see one timepoint at a time: two curves with the same pointwise ranks get
the same depth however those ranks are ordered in time.  These two look at two consecutive timepoints at once.  For a curve
q among n curves at T timepoints, time-major Y[t][i], no NaN, the whole sample counted, q included:

    a_t = #{j : Y[t][j] <= Y[t][q]}                                     1 <= a_t <= n
    c_t = #{j : Y[s][j] <= Y[s][q] and Y[t][j] <= Y[t][q]},  s = t - 1   for t >= 1

    'tvd'   TVD(q) = (1/T) sum_t a_t (n - a_t) / n^2                     the total variation depth, at most 1/4
    'mss'   MSS(q) = sum_{t>=1} v_t S_t                                  the modified shape similarity, in [0, 1]
            S_t = (n c_t - a_s a_t)^2 / (a_s (n - a_s) a_t (n - a_t))    the squared phi coefficient of the 2 x 2 table of the
                                                                         indicators at s and t: Var(E[R_t | R_s]) / Var(R_t)
            v_t = |Y[t][q] - Y[t-1][q]| / sum_{u>=1} |Y[u][q] - Y[u-1][q]|

Where the denominator of S_t is 0 (a_s = n or a_t = n: the curve is the highest at s or at t) the numerator is 0 as well and
S_t = 1.  That is this project's convention, not the paper's: a curve on top of the sample at both timepoints keeps its
shape there.  A constant curve has no weights v_t and gets the plain mean of S_t.  MSS = 1 for a family of parallel curves.

The device returns per curve (engine.tvd_sums, called by _functional._shape_depths) the integer SD = sum_t a_t (n - a_t)
and three doubles SS = sum S_t, SN = sum |D_t| S_t, SW = sum |D_t| with D_t = Y[t][q] - Y[t-1][q]; `_shape_depth_values`
turns them into a depth with one fp64 division: SD / (n^2 T), and SN / SW (SS / (T - 1) where SW = 0).

The decomposition of the paper is TVD = shape part + magnitude part; its outlier rule (depth.TotalVariationOutliers) flags
a curve whose MSS lies below the lower fence of the MSS boxplot as a shape outlier, then draws the functional boxplot of
the others by TVD for the magnitude outliers.  `relax` is accepted and ignored, as for the rank depths.
"""
import numpy as np

from ._containment import SHAPE_DEPTHS

__all__ = ['_shape_depth_values']


def _shape_depth_values(sd_sum, shape, n: int, T: int, name: str) -> np.ndarray:
    """int64 sd_sum [m] and float64 shape [m, 3] = (SS, SN, SW) of curves among n at T timepoints -> the fp64 depths `name`."""
    if name not in SHAPE_DEPTHS:
        raise ValueError(f'{name!r} is not one of {list(SHAPE_DEPTHS)}')
    if name == 'tvd':
        SD = np.asarray(sd_sum, dtype=np.int64).reshape(-1)
        return SD.astype(np.float64) / np.float64(int(n) * int(n) * int(T))
    if T < 2:
        raise ValueError('\'mss\' needs at least 2 timepoints.')
    R = np.asarray(shape, dtype=np.float64).reshape(-1, 3)
    SS, SN, SW = R[:, 0], R[:, 1], R[:, 2]
    moving = SW > 0
    return np.where(moving, SN / np.where(moving, SW, 1.0), SS / np.float64(T - 1))
