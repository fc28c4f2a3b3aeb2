"""Probabilistic depths on the HIP engine.

Mirrors statdepth/depth/calculations/_uncertainty.py: `probabilistic_normal_depth` (:123-139), the depth of n normal
distributions, and `probabilistic_poisson_depth` (:63-70), the depth of n Poisson curves with T rates each.  The
reference's sums are separated into pair terms: O(n^2) closed forms for the normal depth
(sd_prob_normal_sums) and O(n T lim) for the Poisson depth (sd_prob_poisson_sums), both on the GPU.  A custom `f` for
the normal depth is integrated on the host with scipy's quad, one call per (target, pair), as the reference does.
DESIGN.md §4 lists where this departs from the reference: finite sums where its factorials overflow to NaN, `to_compute`
honoured, and invalid parameters refused with ValueError.

`_probabilistic_band_depth` is the driver of `ProbabilisticDepth`, documented by the reference (docs/index.md §5.1.3)
but never implemented there: the expected J = 2 band depth of curves observed with independent Gaussian noise
(sd_prob_band_sums).
"""
import math
import operator
from itertools import combinations

import numpy as np
import pandas as pd
from scipy.integrate import quad
from scipy.stats import norm

from ... import engine
from ._functional import _positions, _require_unique_labels, _sample_blocks
from ._helper import DepthDegeneracy, _band_depth_sum, _handle_depth_errors, _padded_members

__all__ = ['probabilistic_normal_depth', 'probabilistic_poisson_depth']


def _normal_containment(z, parameters: list):
    """The reference's integrand (:96-99): (Phi_i(z) - Phi(z) Phi_j(z)) phi(z), parameters = [mu_i, sigma_i, mu_j,
    sigma_j, mu, sigma].  The default `f`: with it the depth runs on the GPU through the integral's closed form."""
    mu_i, sigma_i, mu_j, sigma_j, mu, sigma = parameters
    return (norm.cdf(z, mu_i, sigma_i) - norm.cdf(z, mu, sigma) * norm.cdf(z, mu_j, sigma_j)) * norm.pdf(z, mu, sigma)


def _quad_sums(mu: np.ndarray, sigma: np.ndarray, f) -> np.ndarray:
    """A custom integrand: one quad per (target, pair i < j of the others), as in _normal_depth (:101-121)."""
    n = len(mu)
    out = np.zeros(n)
    for k in range(n):
        s = 0.0
        for i, j in combinations([c for c in range(n) if c != k], 2):
            params = [mu[i], sigma[i], mu[j], sigma[j], mu[k], sigma[k]]
            s += quad(lambda x: f(x, params), -np.inf, np.inf)[0]
        out[k] = s
    return out


def probabilistic_normal_depth(means, stds, f=_normal_containment) -> pd.DataFrame:
    """Depth of each of n normal distributions N(means[k], stds[k]) among the others (:123-139).

    Returns pd.DataFrame({'means', 'stds', 'depths'}).  With the default `f` the depths come from the GPU; means must
    be finite and stds finite and positive (ValueError otherwise, where the reference returns NaN)."""
    if len(means) != len(stds):
        raise ValueError('Error, len(means) must equal len(stds)')
    mu = np.asarray(means, dtype=np.float64).reshape(-1)
    sg = np.asarray(stds, dtype=np.float64).reshape(-1)
    n = len(mu)
    if f is _normal_containment:
        if not np.isfinite(mu).all():
            raise ValueError('means must be finite')
        if not (np.isfinite(sg).all() and (sg > 0).all()):
            raise ValueError('stds must be finite and positive')
        sums = engine.prob_normal_sums(mu, sg) if n else np.zeros(0)
    else:
        sums = _quad_sums(mu, sg, f)
    with np.errstate(divide='ignore', invalid='ignore'):
        depths = sums / np.float64(math.comb(n, 2))                  # (:121); n = 1: 0 / 0
    return pd.DataFrame({'means': means, 'stds': stds, 'depths': list(depths)})


def probabilistic_poisson_depth(df: pd.DataFrame, to_compute=None, lim=1000, tol=10**-6) -> pd.Series:
    """Depth of each column of `df` (T timepoints x n curves of Poisson rates) among the other columns (:63-70).

    depth_f = sum over rows t, z = 1 .. lim - 1 and column pairs i < j other than f of P(X_f = z) P(X_i <= z)
    P(X_j >= z), divided by C(T, 2).  `to_compute` (column labels) selects the targets; each equals the full result at
    its label.  Rates must be finite and non-negative (ValueError otherwise).  `tol` is accepted and unused, as in the
    reference."""
    T, n = df.shape
    lim = operator.index(lim)
    lam = df.to_numpy(dtype=np.float64)
    if not (np.isfinite(lam).all() and (lam >= 0).all()):
        raise ValueError('Poisson rates must be finite and non-negative')
    if to_compute is None:
        labels, targets = df.columns, None
    else:
        labels = list(to_compute)
        pos = df.columns.get_indexer(labels)
        if (pos < 0).any():
            missing = [l for l, p in zip(labels, pos) if p < 0]
            raise KeyError(f'{missing} not in columns')
        targets = pos.astype(np.int64)
    m = n if targets is None else len(targets)
    sums = engine.prob_poisson_sums(lam, lim, targets) if m else np.zeros(0)
    with np.errstate(divide='ignore', invalid='ignore'):
        depths = np.float64(1.0) / np.float64(math.comb(T, 2)) * sums  # (:67); T < 2: 1 / 0 = inf
    return pd.Series(index=labels, data=depths)


def _probabilistic_band_depth(data: pd.DataFrame, sigma2: pd.DataFrame, to_compute=None, K=None, J=2, relax=False,
                              device=None) -> pd.Series:
    """Expected band depth (J = 2) of the columns of `data` (T timepoints x n curves) when X_c(t) ~ N(data[t, c],
    sigma2[t, c]) independently; a zero variance is a point mass.

    With p = P(min(X_j, X_k) <= X_i <= max(X_j, X_k)) for target i and a pair {j, k} of the other curves:
    depth_i = sum_{j<k} sum_t p / T / C(n, 2) (relax) or sum_{j<k} prod_t p / C(n, 2), n counting the target -- the
    containment and normalisation of FunctionalDepth, which it equals bit for bit when every variance is zero.  `K`
    draws FunctionalDepth's blocks (`_sample_blocks`, the same global numpy RNG draws) and averages the block depths."""
    _handle_depth_errors(data=[data], J=J, containment='r2', relax=relax, deep_check=False)
    _require_unique_labels(data)
    if J != 2:
        raise NotImplementedError('ProbabilisticDepth is implemented for J = 2 (J >= 3 needs trivariate orthant '
                                  'probabilities)')
    if not isinstance(sigma2, pd.DataFrame):
        raise ValueError('sigma2 must be a pd.DataFrame of variances with the index and columns of data')
    if not (sigma2.shape == data.shape and sigma2.index.equals(data.index) and sigma2.columns.equals(data.columns)):
        raise ValueError('sigma2 must have the same index and columns as data')
    mu = data.to_numpy(dtype=np.float64)
    var = sigma2.to_numpy(dtype=np.float64)
    if not np.isfinite(mu).all():
        raise ValueError('data must be finite (no NaN or inf)')
    if not np.isfinite(var).all():
        raise ValueError('sigma2 must be finite (no NaN or inf)')
    if (var < 0).any():
        raise ValueError('sigma2 holds variances: they must be non-negative')
    T, n = mu.shape
    cols = data.columns if to_compute is None else to_compute

    if K is None:
        tg = _positions(data, cols)
        sums = engine.prob_band_sums(mu, var, relax, tg, device=device)
        counts = sums / T if relax else sums             # as _univariate_depths normalises its counts
        return pd.Series(index=cols, data=_band_depth_sum(counts[:, None], n, 2))

    orig = data.loc[:, cols]
    ss = n // K
    if ss == 0:
        raise DepthDegeneracy(f'Block size {K} is too large, not enough functions to sample.')
    blocks, block_targets = [], []
    for col, _, members in _sample_blocks(data, orig, ss, K):
        blocks.append(data.columns.get_indexer(members))
        block_targets.append(data.columns.get_loc(col))
    if not blocks:
        return pd.Series(index=orig.columns, data=[], dtype=np.float64)
    mem = _padded_members(blocks)
    sums = engine.prob_band_sums(mu, var, relax, np.asarray(block_targets, dtype=np.int64), mem, device=device)
    counts = sums / T if relax else sums
    sizes = np.array([len(b) for b in blocks], dtype=np.float64)
    depth = _band_depth_sum(counts[:, None], sizes, 2)   # n = block size including the target
    return pd.Series(index=orig.columns, data=[np.mean(depth[i * K:(i + 1) * K]) for i in range(len(orig.columns))])
