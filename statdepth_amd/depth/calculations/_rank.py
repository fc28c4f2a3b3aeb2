"""Integrated rank depths of univariate curves on the HIP engine (K14; no counterpart in the reference, which has band
depths only for curves).

Everything comes from two integers per (curve, timepoint): A, the number of other curves strictly above, and B, the number
strictly below (ties in neither).  The device returns their record per curve (engine.rank_depth_sums, called by
_functional._rank_depths):

    SA = sum_t A    SB = sum_t B    SF = sum_t |2A - n|    SM = sum_t max(A, B)    MM = max_t max(A, B)

and `_rank_depth_values` turns a record into a depth: integer arithmetic, then one fp64 division.

    'fm'                    (2nT - SF) / (2nT)   Fraiman-Muniz: mean over t of 1 - |1/2 - F_t(x(t))|, F_t the empirical CDF
                                                 with "<=", F = (n - A) / n.  Because of the "<=" the depth is not symmetric
                                                 under x -> -x; that is the published definition.
    'mei'                   (nT - SB) / (nT)     modified epigraph index: mean proportion of curves at or above x
    'mhi'                   (nT - SA) / (nT)     modified hypograph index: mean proportion of curves at or below x
    'half_region'           min(mei, mhi)        modified half-region depth (Lopez-Pintado & Romo 2011)
    'integrated_halfspace'  (nT - SM) / (nT)     mean over t of the univariate Tukey depth min(#<=, #>=) / n
    'infimal_halfspace'     (n - MM) / n         its infimum over t

These are the integrated ("modified") forms: there is no strict variant to select, so `relax` is accepted and ignored.
"""
import numpy as np

from ._containment import PROJECTED_DEPTHS, RANK_DEPTHS

__all__ = ['_rank_depth_values', '_projected_depth_values']


def _rank_depth_values(records, n: int, T: int, name: str) -> np.ndarray:
    """int64 records [m, 5] = (SA, SB, SF, SM, MM) of curves among n at T timepoints -> the fp64 depths `name`."""
    if name not in RANK_DEPTHS:
        raise ValueError(f'{name!r} is not one of {list(RANK_DEPTHS)}')
    R = np.asarray(records, dtype=np.int64).reshape(-1, 5)
    SA, SB, SF, SM, MM = (R[:, k] for k in range(5))
    nT = np.int64(n) * np.int64(T)
    if name == 'fm':
        num, den = 2 * nT - SF, 2 * nT
    elif name == 'mei':
        num, den = nT - SB, nT
    elif name == 'mhi':
        num, den = nT - SA, nT
    elif name == 'half_region':
        num, den = nT - np.maximum(SA, SB), nT
    elif name == 'integrated_halfspace':
        num, den = nT - SM, nT
    else:
        num, den = np.int64(n) - MM, np.int64(n)
    return num.astype(np.float64) / np.float64(den)


# The random projection depths (K23) take the same record over the k rows of the curves' projections instead of the T
# timepoints, and K12's outlyingness over the same rows:
#
#     'rp_halfspace'   (nk - SM) / (nk)      mean over the directions of the univariate Tukey depth (Cuevas, Febrero & Fraiman 2007)
#     'rp_fm'          (2nk - SF) / (2nk)    mean over the directions of 1 - |1/2 - F_r|, i.e. 1 - SF / (2nk)
#     'random_tukey'   (n - MM) / n          minimum over the directions: the random Tukey depth (Cuesta-Albertos & Nieto-Reyes 2008)
#     'rp_projection'  1 / (1 + O)           O = max over the directions of |z_r - med_r| / mad_r (O = inf: 0.0)
_PROJECTED_AS_RANK = {'rp_halfspace': 'integrated_halfspace', 'rp_fm': 'fm', 'random_tukey': 'infimal_halfspace'}


def _projected_depth_values(values, n: int, k: int, name: str) -> np.ndarray:
    """The fp64 depths `name` of curves among n over k directions: from the int64 records [m, 5] of engine.rp_depth_sums,
    or for 'rp_projection' from the fp64 outlyingness [m] of engine.rp_outlyingness."""
    if name not in PROJECTED_DEPTHS:
        raise ValueError(f'{name!r} is not one of {list(PROJECTED_DEPTHS)}')
    if name == 'rp_projection':
        return 1.0 / (1.0 + np.asarray(values, dtype=np.float64).reshape(-1))
    return _rank_depth_values(values, n, k, _PROJECTED_AS_RANK[name])
