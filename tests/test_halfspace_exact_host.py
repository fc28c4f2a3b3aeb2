"""Exact halfspace (Tukey) depth in the plane (directions='exact', K11) without a GPU: two numpy restatements of the
definition -- the L/R/S/O counts with a Dekker/Veltkamp two-product (no fma) and the angular sweep with
fractions.Fraction and a comparison sort -- against hand-computed cases and each other, the exact predicate against
rational arithmetic and against the rounded cross product, invariances, the host-side validation, the C ABI's refusals,
and the missing device reported as such (no CPU fallback).

The restatement (`exact_counts`, `exact_counts_sweep`, `exact_external`, `exact_sampled`, `sign_diff`,
`nearly_collinear_cloud`, `integer_cloud`) is imported by tests/test_halfspace_exact_gpu.py as its oracle.
"""
import ctypes
import functools
from fractions import Fraction

import numpy as np
import pandas as pd
import pytest

from test_halfspace_host import halfspace_counts, make_directions


# ---------------------------------------------------------------- numpy restatement of the definition
def two_product(a, b):
    """(p, e) with p = fl(a b) and p + e = a b exactly (Dekker's product over Veltkamp's split; no fma needed)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    p = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b                         # 2^27 + 1
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def sign_diff(a, b, c, d):
    """The exact sign of a b - c d: of p1 - p2 where the rounded products differ (rounding is monotone), else of the
    difference of the products' rounding errors (formed only there)."""
    a, b, c, d = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (a, b, c, d)))
    p1, p2 = a * b, c * d
    out = (p1 > p2).astype(np.int8) - (p1 < p2).astype(np.int8)
    eq = p1 == p2
    if eq.any():
        e1, e2 = two_product(a[eq], b[eq])[1], two_product(c[eq], d[eq])[1]
        out[eq] = (e1 > e2).astype(np.int8) - (e1 < e2).astype(np.int8)
    return out


def _count_one(P, q, extra, sign=sign_diff):
    V = P - np.asarray(q, dtype=np.float64)                            # one rounded subtraction per component
    nz = (V != 0.0).any(axis=1)
    c0 = int((~nz).sum()) + extra
    x, y = V[nz, 0], V[nz, 1]
    if len(x) == 0:
        return c0
    best = len(x)
    step = max(1, (1 << 20) // len(x))                                 # rows of the pair matrix at a time
    for j0 in range(0, len(x), step):
        xj, yj = x[j0:j0 + step], y[j0:j0 + step]
        C = sign(xj[:, None], y[None, :], yj[:, None], x[None, :])                 # cross(v_j, v_k)
        L, R = (C > 0).sum(axis=1), (C < 0).sum(axis=1)
        j, k = np.nonzero(C == 0)                                      # dot(v_j, v_k) matters on the line of v_j only
        D = sign(xj[j], x[k], -yj[j], y[k])
        S, O = np.bincount(j[D > 0], minlength=len(xj)), np.bincount(j[D < 0], minlength=len(xj))
        best = min(best, int(np.minimum.reduce([L + O, R + S, L + S, R + O]).min()))
    return c0 + best


def exact_counts(P, targets=None, sign=sign_diff):
    """c0 + min_j min(L_j + O_j, R_j + S_j, L_j + S_j, R_j + O_j): the definition as it stands.  sign: the predicate,
    sign_diff unless given (tests/test_planar_scale_host.py passes the rational sign_exact)."""
    P = np.asarray(P, dtype=np.float64)
    targets = range(len(P)) if targets is None else targets
    return np.array([_count_one(P, P[t], 0, sign) for t in targets], dtype=np.int64)


def exact_external(P, Q, sign=sign_diff):
    """Counts of each external point g inside P u {g}: n + 1 points, g adds one to c0."""
    P = np.asarray(P, dtype=np.float64)
    return np.array([_count_one(P, g, 1, sign) for g in np.asarray(Q, dtype=np.float64)], dtype=np.int64)


def _frac_cross(a, b):
    return a[0] * b[1] - a[1] * b[0]


def exact_counts_sweep(P, targets=None):
    """The sweep form in rational arithmetic: images in the half-plane y > 0 or (y = 0, x > 0) with their flip flags,
    sorted by angle, cuts at group boundaries, min(A, B) over the cuts."""
    P = np.asarray(P, dtype=np.float64)
    targets = range(len(P)) if targets is None else targets
    out = []
    for t in targets:
        V = P - P[t]
        c0, items = 0, []
        for vx, vy in V:
            if vx == 0.0 and vy == 0.0:
                c0 += 1
                continue
            f = vy < 0.0 or (vy == 0.0 and vx < 0.0)
            x, y = Fraction(float(vx)), Fraction(float(vy))
            items.append(((-x, -y) if f else (x, y), int(f)))
        if not items:
            out.append(c0)
            continue
        items.sort(key=functools.cmp_to_key(lambda a, b: -1 if _frac_cross(a[0], b[0]) > 0
                                            else (1 if _frac_cross(a[0], b[0]) < 0 else 0)))
        flags = np.array([f for _, f in items])
        t1, m = int(flags.sum()), len(items)
        best = min(t1, m - t1)                                         # the cut before everything
        f1 = 0
        for s in range(m):
            f1 += flags[s]
            if s == m - 1 or _frac_cross(items[s][0], items[s + 1][0]) != 0:
                A = (s + 1 - f1) + (t1 - f1)
                best = min(best, A, m - A)
        out.append(c0 + int(best))
    return np.array(out, dtype=np.int64)


def exact_sampled(P, targets, K):
    """The K-block estimator replaying _samplepointwisedepth's draws from the global numpy RNG (as
    test_halfspace_host.halfspace_sampled does), the exact depth inside each block."""
    P = np.asarray(P, dtype=np.float64)
    n = len(P)
    ss = n // K
    rows = pd.Series(np.arange(n))
    out = []
    for tp in targets:
        vals = []
        for _ in range(ss):
            drawn = rows.sample(n=ss).to_numpy()
            blk = np.append(drawn[drawn != tp], tp)
            vals.append(exact_counts(P[blk], [len(blk) - 1])[0] / len(blk))
        out.append(np.mean(vals))
    return np.array(out)


def nearly_collinear_cloud():
    """50 points a rounding error away from one line: where the rounded cross product gets signs wrong."""
    rng = np.random.default_rng(0)
    return np.outer(rng.normal(size=50), [0.1, 0.3]) + 0.7


def integer_cloud(n, seed):
    """Small integers: duplicates and collinear triples throughout."""
    return np.random.default_rng(seed).integers(-2, 3, size=(n, 2)).astype(np.float64)


def _all_pairs(P):
    """(ax, ay, bx, by) of every (target, j, k): the operands of the orientation predicate over a whole cloud."""
    V = P[None, :, :] - P[:, None, :]                                  # V[q, i] = p_i - p_q
    a, b = V[:, :, None, :], V[:, None, :, :]
    shape = np.broadcast_shapes(a.shape, b.shape)
    a, b = np.broadcast_to(a, shape).reshape(-1, 2), np.broadcast_to(b, shape).reshape(-1, 2)
    return a[:, 0], a[:, 1], b[:, 0], b[:, 1]


# ---------------------------------------------------------------- hand cases
def test_hand_cases():
    line = np.array([[i, 2.0 * i] for i in range(7)], dtype=np.float64)
    square = np.array([[1, 1], [1, -1], [-1, 1], [-1, -1], [0, 0]], dtype=np.float64)
    equal = np.full((5, 2), 0.25)
    for fn in (exact_counts, exact_counts_sweep):
        assert fn(line).tolist() == [1, 2, 3, 4, 3, 2, 1]
        assert fn(square).tolist() == [1, 1, 1, 1, 3]
        assert fn(equal).tolist() == [5, 5, 5, 5, 5]
        assert fn(square, [4, 0, 4]).tolist() == [3, 1, 3]
        assert fn(np.array([[2.0, 3.0]])).tolist() == [1]
    assert exact_external(square, [[0.0, 0.0], [9.0, 9.0], [1.0, 1.0], [0.5, 0.0]]).tolist() == [4, 1, 2, 2]


# ---------------------------------------------------------------- the two forms agree
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_counts_form_equals_sweep_form_on_integer_grids(seed):
    P = integer_cloud(40, seed)
    assert len(np.unique(P, axis=0)) < len(P)                          # duplicates are part of the case
    assert np.array_equal(exact_counts(P), exact_counts_sweep(P))


def test_counts_form_equals_sweep_form_on_the_nearly_collinear_cloud():
    P = nearly_collinear_cloud()
    assert np.array_equal(exact_counts(P), exact_counts_sweep(P))


# ---------------------------------------------------------------- the predicate
def test_two_product_sign_is_the_rational_sign():
    ax, ay, bx, by = _all_pairs(nearly_collinear_cloud())
    got = sign_diff(ax, by, ay, bx)
    sel = np.random.default_rng(1).permutation(len(ax))[:4000]         # Fractions are slow: a sample of the pairs ...
    rounded = ax * by - ay * bx
    sel = np.union1d(sel, np.flatnonzero(np.sign(rounded) != got)[:2000])   # ... and those the rounded form gets wrong
    for i in sel:
        exact = Fraction(float(ax[i])) * Fraction(float(by[i])) - Fraction(float(ay[i])) * Fraction(float(bx[i]))
        assert got[i] == (exact > 0) - (exact < 0)
    dots = sign_diff(ax, bx, -ay, by)
    for i in sel[:500]:
        exact = Fraction(float(ax[i])) * Fraction(float(bx[i])) + Fraction(float(ay[i])) * Fraction(float(by[i]))
        assert dots[i] == (exact > 0) - (exact < 0)


def test_rounded_cross_product_is_not_a_substitute():
    """On the nearly collinear cloud the sign of fl(fl(a0 b1) - fl(a1 b0)) differs from the exact sign, and counting with it
    changes depth counts: the GPU test on this cloud cannot pass with a rounded predicate."""
    P = nearly_collinear_cloud()
    ax, ay, bx, by = _all_pairs(P)
    exact = sign_diff(ax, by, ay, bx)
    rounded = np.sign(ax * by - ay * bx).astype(np.int8)
    assert (exact != rounded).sum() > 0

    def rounded_counts(P):
        out = []
        for q in P:
            V = P - q
            V = V[(V != 0.0).any(axis=1)]
            x, y = V[:, 0], V[:, 1]
            C = np.sign(x[:, None] * y[None, :] - y[:, None] * x[None, :])
            D = np.sign(x[:, None] * x[None, :] + y[:, None] * y[None, :])
            L, R = (C > 0).sum(axis=1), (C < 0).sum(axis=1)
            S, O = ((C == 0) & (D > 0)).sum(axis=1), ((C == 0) & (D < 0)).sum(axis=1)
            out.append(len(P) - len(V) + np.minimum.reduce([L + O, R + S, L + S, R + O]).min())
        return np.array(out)
    assert (rounded_counts(P) != exact_counts(P)).sum() > 0


# ---------------------------------------------------------------- against K10 and under exact maps
def test_exact_counts_never_exceed_directional_counts():
    for P in (np.random.default_rng(5).normal(size=(200, 2)), integer_cloud(40, 3), nearly_collinear_cloud()):
        exact = exact_counts(P)
        for k in (8, 200):
            assert (exact <= halfspace_counts(P, make_directions(k, 0, 2))).all()
    P = np.random.default_rng(5).normal(size=(200, 2))
    assert (exact_counts(P) < halfspace_counts(P, make_directions(8, 0, 2))).sum() == 160


def test_invariances_exact_in_fp64():
    rng = np.random.default_rng(7)
    for P in (rng.normal(size=(60, 2)), nearly_collinear_cloud()):
        want = exact_counts(P)
        rot = np.column_stack([-P[:, 1], P[:, 0]])                     # rotation by 90 degrees
        assert np.array_equal(exact_counts(rot), want)
        for s in (2.0 ** -40, 2.0 ** 13, -4.0):                        # power-of-two scaling (a point reflection too)
            assert np.array_equal(exact_counts(P * s), want)
    Z = integer_cloud(40, 4)
    want = exact_counts(Z)
    for shift in ([1000.0, -7.0], [2.0 ** 40, 2.0 ** 30]):
        assert np.array_equal(exact_counts(Z + np.array(shift)), want)


# ---------------------------------------------------------------- host validation (no device needed)
def test_validation_errors_before_device_work():
    from statdepth_amd import PointcloudDepth
    rng = np.random.default_rng(2)
    good = pd.DataFrame(rng.normal(size=(10, 2)))
    for bad_value in (np.nan, np.inf, -np.inf):
        bad = good.copy()
        bad.iloc[3, 1] = bad_value
        for kw in ({}, {"K": 2}):
            with pytest.raises(ValueError, match='NaN or infinite'):
                PointcloudDepth(bad, containment='halfspace', directions='exact', **kw)
    big = good.copy()
    big.iloc[0, 0] = 2.0 ** 501
    for kw in ({}, {"K": 2}):
        with pytest.raises(ValueError, match=r'2\^500'):
            PointcloudDepth(big, containment='halfspace', directions='exact', **kw)
        with pytest.raises(ValueError, match="or 'exact'"):
            PointcloudDepth(good, containment='halfspace', directions='exactly', **kw)
        with pytest.raises(ValueError, match="or 'exact'"):
            PointcloudDepth(good, containment='halfspace', directions='', **kw)
        with pytest.raises(NotImplementedError, match='implemented for the plane'):
            PointcloudDepth(pd.DataFrame(rng.normal(size=(10, 3))), containment='halfspace', directions='exact', **kw)
        with pytest.raises(NotImplementedError, match='d <= 8'):
            PointcloudDepth(pd.DataFrame(rng.normal(size=(12, 9))), containment='halfspace', directions='exact', **kw)


def test_engine_argument_checks_need_no_device_call():
    from statdepth_amd import engine
    assert engine.HALFSPACE2_ALGOS == {"auto": 0, "sweep": 1, "pairwise": 2}
    with pytest.raises(ValueError, match="'auto', 'sweep' or 'pairwise'"):
        engine._halfspace2_algo("rank")


# ---------------------------------------------------------------- C ABI, no device needed
def _lib():
    from statdepth_amd import _native
    return _native, _native.load()


def test_abi_refusals_before_device_work():
    _native, lib = _lib()
    fake = ctypes.c_void_p(256)                  # never dereferenced: every refusal happens before device work
    out = ctypes.c_void_p(512)
    INV, UNS = _native.SD_ERR_INVALID, _native.SD_ERR_UNSUPPORTED
    counts, external, subsets = lib.sd_halfspace2_counts, lib.sd_halfspace2_external_counts, lib.sd_halfspace2_subset_counts
    for algo in (0, 1, 2):
        assert counts(None, 10, None, 10, algo, out, None) == INV
        assert counts(fake, 10, None, 10, algo, None, None) == INV
        assert counts(fake, 0, None, 0, algo, out, None) == INV
        assert counts(fake, 10, None, 9, algo, out, None) == INV                  # NULL targets, m != n
        assert external(None, 10, fake, 3, algo, out, None) == INV
        assert external(fake, 10, None, 3, algo, out, None) == INV
        assert external(fake, 10, fake, 3, algo, None, None) == INV
        assert external(fake, 0, fake, 3, algo, out, None) == INV
        assert subsets(None, 10, fake, 3, 4, algo, out, None) == INV
        assert subsets(fake, 10, None, 3, 4, algo, out, None) == INV
        assert subsets(fake, 10, fake, 3, 4, algo, None, None) == INV
        assert subsets(fake, 10, fake, 3, 0, algo, out, None) == INV
        assert subsets(fake, 0, fake, 3, 4, algo, out, None) == INV
        assert counts(fake, 2**31, fake, 1, algo, out, None) == UNS               # 2^31 points
        assert b"2^31" in lib.sd_last_error()
        assert external(fake, 2**31, fake, 1, algo, out, None) == UNS
        assert external(fake, 2**31 - 1, fake, 1, algo, out, None) == UNS         # n + 1 points
        assert subsets(fake, 2**31, fake, 1, 4, algo, out, None) == UNS
    assert counts(fake, 10, None, 10, 3, out, None) == INV                        # unknown algo
    assert counts(fake, 10, None, 10, -1, out, None) == INV
    # the sweep asked for by name above its capacity
    assert counts(fake, 8193, fake, 1, 1, out, None) == UNS
    assert b"8192" in lib.sd_last_error()
    assert external(fake, 8193, fake, 1, 1, out, None) == UNS
    assert subsets(fake, 10**5, fake, 1, 8193, 1, out, None) == UNS
    # beyond 1e14 predicate evaluations on the route that would run: pairwise m n^2, sweep per target by capacity tier
    assert counts(fake, 10**5, None, 10**5, 0, out, None) == UNS                  # auto above the capacity: pairwise
    assert b"cap" in lib.sd_last_error()
    assert counts(fake, 10**5, None, 10**5, 2, out, None) == UNS
    assert counts(fake, 2 * 10**7, fake, 1, 2, out, None) == UNS                  # one target, n^2 = 4e14
    assert external(fake, 10**6, fake, 10**3, 0, out, None) == UNS
    assert subsets(fake, 10**6, fake, 10**7, 10**4, 0, out, None) == UNS
    assert subsets(fake, 10**6, fake, 2**30, 8192, 1, out, None) == UNS           # 2^30 blocks x 372 736 comparators
    assert external(fake, 8192, fake, 2**30, 0, out, None) == UNS


def test_no_device_is_an_error_not_a_fallback():
    from statdepth_amd import PointcloudDepth, engine
    _native, lib = _lib()
    if lib.sd_device_count() > 0:
        pytest.skip("a HIP device is visible: tests/test_halfspace_exact_gpu.py covers this machine")
    rng = np.random.default_rng(1)
    P = rng.normal(size=(12, 2))
    df = pd.DataFrame(P)
    with pytest.raises(RuntimeError, match='no HIP device'):
        PointcloudDepth(df, containment='halfspace', directions='exact')
    with pytest.raises(RuntimeError, match='no HIP device'):
        PointcloudDepth(df, containment='halfspace', directions='exact', K=2)
    for call in (lambda: engine.halfspace_exact_counts(P), lambda: engine.halfspace_exact_external_counts(P, P[:2]),
                 lambda: engine.halfspace_exact_subset_counts(P, [[0, 1, 2]])):
        with pytest.raises(RuntimeError, match='no HIP device'):
            call()
