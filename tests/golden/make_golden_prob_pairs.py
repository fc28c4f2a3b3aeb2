#!/usr/bin/env python3
"""Generate the single-pair fixtures of the probabilistic kernels (K8 prob_depth.hip, K9 prob_band.hip) with mpmath.

Unlike make_golden_prob.py this runs no reference code: every expected value is this project's own restatement of the
mathematical definition at 80+ digits.  Three files, each one JSON object with a `kind` of its own (pairs_band,
pairs_normal, pairs_poisson; the names do not begin with prob_, whose kinds test_fixture_kinds_are_new pins):

  pairs_band.json     K9: p = P(min(X_j, X_k) <= X_i <= max(X_j, X_k)) for one (target, pair, timepoint), by the
                      Drezner-Wesolowsky angle form (band_p_angle), plus one 6 x 4 strict case built from such values
  pairs_normal.json   K8 normal, n = 3: out[0] = Phi(h_1) - Phi2(0, h_2; rho_2) (normal_pair)
  pairs_poisson.json  K8 Poisson, n = 3, T = 1: out[f] = sum_z p_f(z) L_i(z) U_j(z) by exact summation (poisson_triple)

Inputs are float.hex() strings (the device and the reference read the same doubles), expected values 40-digit decimal
strings, next to the derived quantities the tests sort by.  The output is deterministic: a rerun rewrites the same bytes.

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_golden_prob_pairs.py
"""
import json
import math
import os
from concurrent.futures import ProcessPoolExecutor

import mpmath as mp

HERE = os.path.dirname(os.path.abspath(__file__))
DPS = 80                                     # working digits; raised where a difference cancels (band_p_angle)
DIGITS = 40                                  # digits of the stored strings
H_REGIME_A = 12.0 + 1e-9                     # |h| <= 12 up to the rounding of the constructed means
P_REGIME_A = 1e-290


def _s(v):
    return mp.nstr(v, DIGITS, strip_zeros=False, min_fixed=-1, max_fixed=0)


def _ncdf(x):
    if x < -1e100:                           # below 10^-(2e199): written as 0 (its digits cannot be printed)
        return mp.mpf(0)
    return mp.erfc(-x / mp.sqrt(2)) / 2


# ---------------------------------------------------------------- K9: the containment probability
def band_geometry(tr):
    """(h_j, h_k, rho) of a triple (mi, vi, mj, vj, mk, vk) of doubles, as mpf; h_c = 0 where s_c = 0."""
    mi, vi, mj, vj, mk, vk = (mp.mpf(v) for v in tr)
    sj, sk = mp.sqrt(vi + vj), mp.sqrt(vi + vk)
    hj = (mi - mj) / sj if sj else mp.mpf(0)
    hk = (mi - mk) / sk if sk else mp.mpf(0)
    rho = vi / (sj * sk) if sj and sk else mp.mpf(0)
    return hj, hk, rho


def _band_exact_branch(tr):
    """The zero-variance branches, or None: sigma_i = 0, and sigma_j = sigma_k = 0 < sigma_i."""
    mi, vi, mj, vj, mk, vk = (mp.mpf(v) for v in tr)
    if vi == 0:
        def ab(m, v):                        # P(X > mi), P(X < mi)
            if v == 0:
                return mp.mpf(m > mi), mp.mpf(m < mi)
            z = (m - mi) / mp.sqrt(v)
            return _ncdf(z), _ncdf(-z)
        (aj, bj), (ak, bk) = ab(mj, vj), ab(mk, vk)
        ej, ek = 1 - aj - bj if vj == 0 else mp.mpf(0), 1 - ak - bk if vk == 0 else mp.mpf(0)
        return aj * bk + bj * ak + ej + ek - ej * ek
    if vj == 0 and vk == 0:
        hj, hk, _ = band_geometry(tr)
        lo, hi = min(hj, hk), max(hj, hk)
        return _ncdf(-lo) - _ncdf(-hi) if hi > 0 else _ncdf(hi) - _ncdf(lo)
    return None


def band_p_angle(tr):
    """p by the Drezner-Wesolowsky angle form:  Phi(h_j) Phi(-h_k) + Phi(-h_j) Phi(h_k) - (1 / pi) int_0^asin(rho)
    exp((sin(th) h_j h_k - (h_j^2 + h_k^2) / 2) / cos^2(th)) d th, by mp.quad over 33 sub-intervals (16 uniform, 17
    halving towards asin(rho), where the integrand bends as rho -> 1).  The digits are raised until at least 45 survive
    the subtraction and the quadrature's own error estimate is below 1e-45 p."""
    dps = DPS
    while True:
        with mp.workdps(dps):
            p = _band_exact_branch(tr)
            if p is not None:
                return +p
            hj, hk, rho = band_geometry(tr)
            th = mp.asin(rho)
            hh, hs = hj * hk, (hj * hj + hk * hk) / 2
            f = lambda t: mp.exp((mp.sin(t) * hh - hs) / mp.cos(t) ** 2)
            pts = [th * i / 16 for i in range(16)] + [th * (1 - mp.mpf(2) ** -k) for k in range(5, 22)] + [th]
            integral, err = mp.quad(f, pts, error=True)
            a, b, c = _ncdf(hj) * _ncdf(-hk), _ncdf(-hj) * _ncdf(hk), integral / mp.pi
            p = a + b - c
            big = max(a, b, c)
            if p > 0 and dps - mp.log10(big / p) >= 45 and err / mp.pi <= mp.mpf(10) ** -45 * p:
                return +p
        dps += 40
        assert dps <= 400, tr


def band_p_line(tr, dps=DPS):
    """The second route, for |h| <= 12: int phi_i [F_j (1 - F_k) + F_k (1 - F_j)] over X_i, split at the means and at
    +-2, +-8 of every scale around them.  Needs sigma_i > 0."""
    with mp.workdps(dps):
        mi, vi, mj, vj, mk, vk = (mp.mpf(v) for v in tr)
        si = mp.sqrt(vi)

        def F(m, v, x):
            if v == 0:
                return mp.mpf(x >= m), mp.mpf(x < m)
            z = (x - m) / mp.sqrt(v)
            return _ncdf(z), _ncdf(-z)

        def f(x):
            (fj, gj), (fk, gk) = F(mj, vj, x), F(mk, vk, x)
            return mp.npdf(x, mi, si) * (fj * gk + fk * gj)
        scales = [si] + [mp.sqrt(v) for v in (vj, vk) if v > 0]
        pts = {mi, mj, mk}
        for c0 in (mi, mj, mk):
            for s in scales:
                for z in (-8, -2, 2, 8):
                    pts.add(c0 + z * s)
        return mp.quad(f, [-mp.inf] + sorted(pts) + [mp.inf])


def band_branch(tr):
    """The branch pb_prob takes, from the fp64 quantities the kernel forms."""
    mi, vi, mj, vj, mk, vk = tr
    if vi == 0.0:
        return "point_i"
    if vj == 0.0 and vk == 0.0:
        return "point_jk"
    si = math.sqrt(vi)
    g = [si * (1.0 / math.hypot(si, math.sqrt(v))) for v in (vj, vk)]
    rho = g[0] * g[1]
    return "gl6" if rho < 0.3 else "gl12" if rho < 0.75 else "gl20" if rho < 0.925 else "near1"


def special_triples():
    """tests/test_probabilistic_band_host.py's list (rho -> 1, |h| up to 35, h = 0, every zero-variance case, ties)."""
    r2 = math.sqrt(2.0)
    return [
        (0, 1, 0, 1, 0, 1), (0, 1e4, 0.3, 1e-4, -0.2, 1e-4), (0, 1e4, 0.3, 1e-4, 0.3, 1e-4),
        (0, 1e4, 250.0, 1e-4, -40.0, 1e-4), (35, 1, 0, 0, 0, 0), (35 * r2, 1, 0, 1, 0, 1), (-35 * r2, 1, 0, 1, 1, 1),
        (10, 1, 0, 1, 0.5, 1), (-8, 1, 0, 1, 0.5, 1), (5, 1, 0, 0.01, 0, 0.01), (0.5, 2, 0.5, 3, 0.5, 0.1),
        (0.5, 2, 0.5, 3, 1.5, 0.1), (0, 0, 1, 1, -1, 1), (0, 0, 1, 0, 0, 1), (0, 0, 0, 0, 0, 0), (0, 0, 1, 0, -1, 0),
        (0, 0, 1, 0, 2, 0), (0, 0, 0, 0, 2, 0), (0, 1, 1, 0, 2, 0), (0, 1, 1, 0, -2, 0), (0, 1, 0, 0, 0, 0),
        (0, 1, 30, 0, 31, 0), (0, 1, -30, 0, -29.5, 0), (3, 2, 0, 1e-6, 0.1, 3), (0, 1, 0.5, 0, 0.7, 1e-20),
        (0, 1e-6, 1, 1e6, -1, 1e6),
    ]


RHOS = [0.05, 0.2999, 0.3001, 0.5, 0.7499, 0.7501, 0.9, 0.9249, 0.9251, 0.95, 0.99, 1 - 1e-6, 1 - 1e-12]
HS = [(0, 0), (1, -1), (3, 3), (3, 3.001), (6, 6), (6, -6), (-8, -8.5), (10, 10), (10, 12), (12, 12), (12, -12)]
HS_UNEQUAL = [(1, -1), (3, 3.001), (6, -6), (10, 12)]
HS_TAIL = [(14, 14), (14.2, 14.2), (20, 20), (20, 21), (30, 31), (37, 38)]


def triple_for(rho, hj, hk, split=0.5):
    """sigma_i = 1, mu_i = 0 and s_j = rho^-split, s_k = rho^-(1 - split): rho = 1 / (s_j s_k), means -h s."""
    lr = math.log(rho)
    vj, vk = math.expm1(-2.0 * split * lr), math.expm1(-2.0 * (1.0 - split) * lr)
    return (0.0, 1.0, -hj * math.sqrt(1.0 + vj), vj, -hk * math.sqrt(1.0 + vk), vk)


def band_triples():
    out = [(f"special_{i:02d}", tuple(float(v) for v in tr)) for i, tr in enumerate(special_triples())]
    for rho in RHOS:
        for hj, hk in HS:
            out.append((f"grid_r{rho!r}_h{hj:g}_{hk:g}", triple_for(rho, hj, hk)))
        for hj, hk in HS_UNEQUAL:
            out.append((f"unequal_r{rho!r}_h{hj:g}_{hk:g}", triple_for(rho, hj, hk, split=0.3)))
    for rho in (0.5, 0.95):
        for hj, hk in HS_TAIL:
            out.append((f"tail_r{rho!r}_h{hj:g}_{hk:g}", triple_for(rho, hj, hk)))
    out.append(("tail_r0.95_h20_-21", triple_for(0.95, 20, -21)))
    out.append(("clamp_r0.5_h2e10_3e10", triple_for(0.5, 2e10, 3e10)))
    out.append(("clamp_r0.5_h2e10_-3e10", triple_for(0.5, 2e10, -3e10)))
    for rho in (0.95, 0.99):                     # h_j h_k = 199 and 201: either side of the near-1 branch's -100 cutoff
        for hh in (199.0, 201.0):
            out.append((f"cut_r{rho!r}_hh{hh:g}", triple_for(rho, math.sqrt(hh), math.sqrt(hh))))
    return out


def _band_entry(item):
    name, tr = item
    p = band_p_angle(tr)
    with mp.workdps(DPS):
        hj, hk, rho = band_geometry(tr)
        regime = "A" if max(abs(hj), abs(hk)) <= H_REGIME_A and p >= P_REGIME_A else "B"
        return {"name": name, "in": [float(v).hex() for v in tr], "hj": float(hj), "hk": float(hk), "rho": float(rho),
                "branch": band_branch(tr), "regime": regime, "p": _s(p)}


def strict_case():
    """6 timepoints x 4 curves for the strict product: at every t curve 0 lies at most 11.9 joint standard deviations
    above each of the others (and that far from the nearest), so its products fall below 1e-150; every factor is in
    regime A (asserted in build_band)."""
    import numpy as np
    rng = np.random.default_rng(20)
    T, n = 6, 4
    mu = rng.normal(0.0, 0.3, (T, n))
    var = rng.uniform(1.5, 1.7, (T, n))
    var[2, 1] = 40.0                             # one large variance: a target with rho near 1, a partner with small h
    mu[:, 0] = np.min(mu[:, 1:] + 11.9 * np.sqrt(var[:, :1] + var[:, 1:]), axis=1)
    return mu, var


def strict_items():
    mu, var = strict_case()
    T, n = mu.shape
    items = []
    for i in range(n):
        others = [c for c in range(n) if c != i]
        for a in range(len(others)):
            for b in range(a + 1, len(others)):
                j, k = others[a], others[b]
                for t in range(T):
                    items.append((f"strict_i{i}_j{j}_k{k}_t{t}",
                                  tuple(float(v) for v in (mu[t, i], var[t, i], mu[t, j], var[t, j], mu[t, k], var[t, k]))))
    return items


# ---------------------------------------------------------------- K8 normal: one pair term
def normal_pair(mu, sg):
    """out[0] of sd_prob_normal_sums for n = 3: Phi(h_1) - (Phi(h_2) / 2 + T(h_2, a_2)), h_m = (mu_0 - mu_m) / s_m,
    s_m = sqrt(sg_m^2 + sg_0^2), a_m = sg_0 / sqrt(2 sg_m^2 + sg_0^2), Owen's T by mp.quad (normal_depths_mp's form)."""
    with mp.workdps(DPS):
        m0, m1, m2 = (mp.mpf(v) for v in mu)
        s0, s1, s2 = (mp.mpf(v) for v in sg)
        h1 = (m0 - m1) / mp.sqrt(s1 ** 2 + s0 ** 2)
        h2 = (m0 - m2) / mp.sqrt(s2 ** 2 + s0 ** 2)
        a2 = s0 / mp.sqrt(2 * s2 ** 2 + s0 ** 2)
        t = mp.mpf(0)                            # T <= exp(-h^2 / 2) / 4: as _ncdf, 0 beyond |h| = 1e100
        if abs(h2) <= 1e100:
            t = mp.quad(lambda x: mp.exp(-h2 ** 2 * (1 + x ** 2) / 2) / (1 + x ** 2), mp.linspace(0, a2, 5)) / (2 * mp.pi)
        return _ncdf(h1) - (_ncdf(h2) / 2 + t), h1, h2, a2


NORMAL_H = [0.0] + [s * v for v in (1e-300, 1e-8, 0.5, 3.0, 6.0, 8.0, 12.0, 12.5, 20.0, 38.0, 39.0, 1e5) for s in (1, -1)]
NORMAL_RATIO = [1e-150, 1e-4, 0.5, 1.0, 10.0, 1e150]      # sigma_2 / sigma_0: a -> 1 ... a -> 0


def normal_cases():
    out = []
    for h in NORMAL_H:
        for r in NORMAL_RATIO:
            s0, s2 = 1.0, r
            s1 = 0.75
            out.append((f"h{h:g}_r{r:g}", (0.0, h * math.hypot(s1, s0), -h * math.hypot(s2, s0)), (s0, s1, s2)))
    big = 1e308
    out += [
        ("overflow_diff_pos", (big, 0.0, -big), (1.0, 1.0, 1.0)),          # mu_0 - mu_2 overflows: h_2 = +inf
        ("overflow_diff_neg", (-big, 0.0, big), (1.0, 1.0, 1.0)),
        ("overflow_double", (big, -big, -big), (1.5e308, 1.5e308, 1.5e308)),   # inf / inf without the scaling
        ("overflow_double_neg", (-big, big, big), (1.5e308, 1.5e308, 1.5e308)),
        ("overflow_hypot_only", (3e307, -3e307, 1e307), (1.4e308, 1.4e308, 1.2e308)),   # the difference is finite
        ("overflow_mixed_tiny", (8e307, -8e307, -8e307), (1e308, 1e-300, 1e308)),
        ("overflow_a_only", (1.0, 0.0, -1.0), (1.0, 1.0, 1.3e308)),         # sqrt(2) sigma_2 overflows
        ("below_scaling", (4e307, -4e307, -4e307), (4e307, 4e307, 4e307)),  # under the threshold: no scaling
        # both ends of the range in one pair: scaling the stds with the means would push them below the subnormals
        ("top_means_subnormal_stds_equal", (big, big, big), (1e-323, 1e-323, 1e-323)),
        ("top_means_subnormal_stds_apart", (big, -big, -big), (1e-323, 1e-323, 1e-323)),
        ("top_means_subnormal_stds_ratio", (big, big, big), (1e-320, 2e-320, 3e-320)),
        ("top_means_adjacent", (big, math.nextafter(big, 0.0), math.nextafter(big, math.inf)), (1e292, 1e292, 2e292)),
        ("top_std_subnormal_partner", (1.0, 0.0, -1.0), (1.3e308, 1e-320, 5e-324)),
        ("subnormal_std_top_partner", (1.0, 0.0, -1.0), (5e-324, 1e-320, 1.3e308)),
        ("subnormal_everything", (2e-320, -1e-320, 3e-320), (1e-320, 2e-320, 3e-320)),
        ("small_normal_stds", (3e-300, -1e-300, 1e-300), (1e-300, 2e-300, 3e-300)),   # below 2^-969, normal doubles
    ]
    return out


def _normal_entry(item):
    name, mu, sg = item
    v, h1, h2, a2 = normal_pair(mu, sg)
    fin = lambda x: float(x) if math.isfinite(float(x)) else str(float(x))     # "inf" / "-inf": beyond the fp64 range
    return {"name": name, "mu": [float(x).hex() for x in mu], "sigma": [float(x).hex() for x in sg],
            "h1": fin(h1), "h2": fin(h2), "a2": float(a2), "value": _s(v)}


# ---------------------------------------------------------------- K8 Poisson: one row, three columns
def poisson_triple(lam, lim):
    """out[f], f = 0, 1, 2, of sd_prob_poisson_sums for T = 1, n = 3: sum_{z=1}^{lim-1} p_f(z) L_i(z) U_j(z), i < j the
    other two columns.  p by the exact recurrence from e^-lam, L its running sum, U the upper tail summed from z until
    the terms are below 10^-(DPS + 10) of it (far past lim), never 1 - L."""
    with mp.workdps(DPS + 20):
        cols = []
        for l in lam:
            l = mp.mpf(l)
            if l == 0:
                cols.append(([mp.mpf(0)] * (lim + 1), [mp.mpf(1)] * (lim + 1), [mp.mpf(1)] + [mp.mpf(0)] * lim))
                continue
            top = max(lim, int(l)) + 1
            p = [mp.exp(-l)]
            tiny = mp.mpf(10) ** -(DPS + 30)
            while len(p) <= top or p[-1] > tiny * p[int(min(l, len(p) - 1))]:
                p.append(p[-1] * l / len(p))
            L, acc = [], mp.mpf(0)
            for z in range(lim + 1):
                acc += p[z]
                L.append(acc)
            U, acc = [None] * (lim + 1), mp.mpf(0)
            for z in range(len(p) - 1, -1, -1):
                acc += p[z]
                if z <= lim:
                    U[z] = acc
            cols.append((p, L, U))
        out = []
        for f in range(3):
            i, j = [c for c in range(3) if c != f]
            out.append(mp.fsum(cols[f][0][z] * cols[i][1][z] * cols[j][2][z] for z in range(1, lim)))
        return out


def poisson_cases():
    import numpy as np
    out = []
    # stirlerr's seams: z = 15/16, 35/36, 80/81, 500/501.  pp_dpois runs at the chunk starts (z = 1 mod 16) and at the
    # seeds of pp_tail (z = lim where lim > lam, z = lim - 1 otherwise), so lim sits on the seam and the rates around it
    for s in (15, 16, 35, 36, 80, 81, 500, 501):
        tag = f"stirlerr{s - s % 5}"
        for lim in (s, s + 1):
            out.append((f"{tag}_z{s}_lim{lim}", tag, (s - 0.5, s + 1.5, s + 0.25), lim))
    out += [("stirlerr15_bulk", "stirlerr15", (15.5, 16.5, 17.0), 40), ("stirlerr35_bulk", "stirlerr35", (33.0, 35.5, 36.5), 60),
            ("stirlerr80_bulk", "stirlerr80", (80.5, 81.0, 81.5), 120), ("stirlerr500_bulk", "stirlerr500", (497.0, 500.5, 513.0), 600)]
    # bd0's series switch |z - lam| = 0.1 (z + lam): lam = 9 z / 11 and 11 z / 9 at a seed z, and the doubles beside
    for z, lim, where in ((17, 40, "chunk"), (81, 100, "chunk"), (50, 50, "tail_up"), (49, 50, "tail_down")):
        for num, den in ((9, 11), (11, 9)):
            if (where == "tail_up" and num > den) or (where == "tail_down" and num < den):
                continue
            l = z * num / den
            out.append((f"bd0_{where}_z{z}_{num}_{den}", "bd0", (l, math.nextafter(l, 0.0), math.nextafter(l, math.inf)), lim))
    # pp_tail's branch lam = lim, and its 32-term re-seeds (tails of 80 to 250 terms)
    for lim in (33, 100, 600):
        out.append((f"tail_eq_lim{lim}", "tail", (float(lim), lim * (1 - 2.0 ** -40), lim * (1 + 2.0 ** -40)), lim))
    out.append(("tail_lam1e4_lim5000", "tail", (20.0, 30.0, 1e4), 5000))
    out.append(("tail_reseed_lim100", "tail", (99.0, 90.0, 97.5), 100))
    # the 16-z chunk edge of lim
    for lim in (16, 17, 18, 33, 34, 512):
        out.append((f"chunk_lim{lim}", "chunk", (lim / 2.0, lim - 1.0, lim + 3.0), lim))
    # rates at and near 0 (in column 0, where only out[0] becomes small)
    for name, l0 in (("zero", 0.0), ("denormal_min", 5e-324), ("1e-300", 1e-300), ("1e-8", 1e-8)):
        out.append((f"tiny_{name}", "tiny", (l0, 3.0, 5.0), 20))
    out += [("tiny_zero_mid", "tiny", (3.0, 0.0, 5.0), 20), ("tiny_zero_last", "tiny", (3.0, 5.0, 0.0), 20),
            ("tiny_all_zero", "tiny", (0.0, 0.0, 0.0), 20)]
    rng = np.random.default_rng(30)
    for r in range(8):
        lim = int(rng.integers(2, 600))
        lam = np.exp(rng.uniform(np.log(0.05), np.log(1.5 * lim), 3))
        out.append((f"random_{r}", "random", tuple(float(v) for v in lam), lim))
    return out


def _poisson_entry(item):
    name, seam, lam, lim = item
    return {"name": name, "seam": seam, "lam": [float(v).hex() for v in lam], "lim": lim,
            "values": [_s(v) for v in poisson_triple(lam, lim)]}


# ---------------------------------------------------------------- files
def build_band(pool_map=map):
    entries = list(pool_map(_band_entry, band_triples()))
    factors = list(pool_map(_band_entry, strict_items()))
    assert all(e["regime"] == "A" for e in factors), [e["name"] for e in factors if e["regime"] != "A"]
    mu, var = strict_case()
    return {"kind": "pairs_band", "digits": DIGITS, "entries": entries,
            "strict": {"mu": [[float(v).hex() for v in row] for row in mu], "var": [[float(v).hex() for v in row] for row in var],
                       "factors": factors}}


def build_normal(pool_map=map):
    return {"kind": "pairs_normal", "digits": DIGITS, "entries": list(pool_map(_normal_entry, normal_cases()))}


def build_poisson(pool_map=map):
    entries = list(pool_map(_poisson_entry, poisson_cases()))
    small = sum(1 for e in entries for v in e["values"] if 0 < mp.mpf(v) < mp.mpf("1e-290"))
    assert small <= 5, small
    return {"kind": "pairs_poisson", "digits": DIGITS, "entries": entries}


def dump(obj):
    """One entry per line: readable diffs, no whitespace inside an entry."""
    enc = lambda v: json.dumps(v, separators=(",", ":"), allow_nan=False)
    lines = ['{"kind":' + enc(obj["kind"]) + ',"digits":' + enc(obj["digits"]) + ',"entries":[']
    lines += [enc(e) + ("," if i + 1 < len(obj["entries"]) else "") for i, e in enumerate(obj["entries"])]
    if "strict" in obj:
        st = obj["strict"]
        lines.append('],"strict":{"mu":' + enc(st["mu"]) + ',"var":' + enc(st["var"]) + ',"factors":[')
        lines += [enc(e) + ("," if i + 1 < len(st["factors"]) else "") for i, e in enumerate(st["factors"])]
        lines.append("]}}")
    else:
        lines.append("]}")
    return "\n".join(lines) + "\n"


def main():
    with ProcessPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        pm = lambda fn, items: ex.map(fn, items, chunksize=4)
        for name, build in (("pairs_band", build_band), ("pairs_normal", build_normal), ("pairs_poisson", build_poisson)):
            text = dump(build(pm))
            with open(os.path.join(HERE, name + ".json"), "w") as f:
                f.write(text)
            print(f"wrote {name}: {len(text)} bytes", flush=True)


if __name__ == "__main__":
    main()
