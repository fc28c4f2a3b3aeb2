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

from ._containment import RANK_DEPTHS

__all__ = ['_rank_depth_values']


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
