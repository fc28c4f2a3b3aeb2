"""Oja volume sums (K7) without a GPU: exact references, a restatement of the kernel's arithmetic, and the tolerance.

`oja_exact` (integer arithmetic on the float64 inputs, any scale), `oja_exact_int` (numpy int64, integer clouds),
`oja_kernel_emulation` (the kernel's operations in Python floats, with mutant switches), `oja_tolerance` and the input
families below are imported by tests/test_oja_exact_gpu.py.  The checks here: the references agree with each other and
with tests/test_oja_host.py::_volume_sum, the faithful emulation stays inside `oja_tolerance` on every family the GPU
tests use, and every mutant of the emulation leaves it on one of them -- but for the sign of a row swap, which no
input can show because only |c . a_k| is summed; that one is asserted to change no bit.
"""
import math
from fractions import Fraction
from functools import lru_cache
from itertools import combinations, islice

import numpy as np
import pytest

from test_oja_host import oja_sums

U = 2.0 ** -53
PER_THREAD = 128                       # OJA_PER_THREAD
THREADS = 256                          # OJA_THREADS
SLICE = PER_THREAD * THREADS           # OJA_SLICE: 32 768 subsets per workgroup
D_COND = (3, 4, 5, 6, 8)
D_EQUI = (2, 3, 5, 8)
# others on either side of the first slice boundary, C(others, d) <= 32 768 < C(others + 1, d)
BOUNDARY = {1: (32768, 32769), 2: (256, 257), 3: (59, 60), 4: (31, 32), 5: (22, 23), 6: (19, 20), 7: (18, 19), 8: (17, 18)}


# ---------------------------------------------------------------- the three forms (point_select.h), on the host
def targets_of(P, selection=None):
    """[(others, x)] per target, the others in the order the kernel numbers them.  selection: None (every row), a list
    of rows, ('external', Q) or ('blocks', members) with members -1 padded at the end, others first, target last."""
    P = np.asarray(P, dtype=np.float64)
    if isinstance(selection, tuple) and selection[0] == 'external':
        return [(P, np.asarray(q, dtype=np.float64)) for q in np.atleast_2d(selection[1])]
    if isinstance(selection, tuple) and selection[0] == 'blocks':
        out = []
        for row in np.atleast_2d(selection[1]):
            row = np.asarray(row)
            neg = np.flatnonzero(row < 0)
            mem = row[:neg[0]] if len(neg) else row
            if len(mem) == 0:
                out.append((P[:0], P[0]))
            else:
                out.append((P[mem[:-1]], P[mem[-1]]))
        return out
    rows = range(len(P)) if selection is None else selection
    return [(np.delete(P, t, axis=0), P[t]) for t in rows]


def hadamard_sum(a):
    """H = sum over d-subsets S of prod_{s in S} ||a_s||_2 / d!: the elementary symmetric polynomial e_d of the norms.
    Every term is positive, so the float64 recurrence is accurate to a few u."""
    a = np.asarray(a, dtype=np.float64)
    d = a.shape[1]
    e = [1.0] + [0.0] * d
    for x in np.sqrt((a * a).sum(axis=1)).tolist():
        for k in range(d, 0, -1):
            e[k] += e[k - 1] * x
    return e[d] / math.factorial(d)


# ---------------------------------------------------------------- 1. exact references
def _det_int(M):
    """Determinant of a square matrix of Python ints (Bareiss, fraction free: every division is exact)."""
    n = len(M)
    M = [r[:] for r in M]
    sign, prev = 1, 1
    for k in range(n - 1):
        if M[k][k] == 0:
            for i in range(k + 1, n):
                if M[i][k] != 0:
                    M[k], M[i] = M[i], M[k]
                    sign = -sign
                    break
            else:
                return 0
        pk = M[k][k]
        rk = M[k]
        for i in range(k + 1, n):
            ri = M[i]
            f = ri[k]
            for j in range(k + 1, n):
                ri[j] = (ri[j] * pk - f * rk[j]) // prev
        prev = pk
    return sign * M[-1][-1]


def _exact_sum(a):
    """Fraction: sum over d-subsets of the rows of a (float64) of |det| / d!.  Every float64 is an integer times 2^-k."""
    no, d = a.shape
    if no < d:
        return Fraction(0)
    k = 0
    for v in a.ravel().tolist():
        den = Fraction(v).denominator
        k = max(k, den.bit_length() - 1)
    rows = [[int(Fraction(v) * (1 << k)) for v in r] for r in a.tolist()]
    total = 0
    for S in combinations(range(no), d):
        total += abs(_det_int([rows[s] for s in S]))
    return Fraction(total, (1 << (k * d)) * math.factorial(d))


def oja_exact(P, selection=None, scales=None):
    """(values, H): per target the exact sum_S |det[a_s]| / d! rounded once to float64, a_i = fl(x_i - x) formed in
    float64 as the kernel forms it, and the Hadamard sum H of the same a.

    scales (one positive number per axis): H is the scale-aware Hadamard sum prod(scales) * H(a / scales) instead.
    |det[a_s]| = prod(scales) |det[a_s / scales]| <= prod(scales) prod ||a_s / scales||, so it bounds the value like
    H, and it is the scale of the evaluation error when the axes of the cloud differ by the factors in `scales`:
    the axes are the rows of the matrix that oja_cofactor factors, M = diag(scales) N.  For a given order of the
    pivot rows the elimination of M is the elimination of N with row r of every intermediate carrying scales[r]
    (multipliers scales[r] / scales[p] times N's, U the scaled U of N): exactly for powers of two, and otherwise
    within the relative roundings that K_d already counts.  So |dM| <= g |L| |U| (see oja_k) is row by row scales[r]
    times the perturbation of N, and det, linear in each row, moves by prod(scales) times what the same pivot order
    costs on N: K u prod(scales) H(N), with the growth of that order on N in place of partial pivoting's 2^k.  The
    order that partial pivoting takes on M (largest axis first) is not N's own; K_d is kept as it is, its 2^k per
    column (up to 128 at d = 8) being the allowance for the growth of that order on a well-conditioned N."""
    vals, Hs = [], []
    for others, x in targets_of(P, selection):
        a = others - x
        vals.append(float(_exact_sum(a)))
        Hs.append(hadamard_sum(a) if scales is None else float(np.prod(scales)) * hadamard_sum(a / scales))
    return np.array(vals), np.array(Hs)


def _masks_by_popcount(d):
    by = [[] for _ in range(d + 1)]
    for m in range(1 << d):
        by[bin(m).count("1")].append(m)
    return by


def _abs_det_sum_int64(a):
    """Python int: sum over d-subsets of the rows of a (int64) of |det|.  Laplace expansion along the last row, by
    dynamic programming over column subsets: after r rows minors[mask] is the minor of rows 0..r-1 and the columns in
    mask.  Every intermediate is a minor, or a partial sum of at most d terms |entry| * |minor|, and is bounded by
    sqrt(d) * (max|a| * sqrt(d))^d (Hadamard); that bound is asserted to fit int64."""
    no, d = a.shape
    if no < d:
        return 0
    amax = max(1, int(np.abs(a).max()))
    assert math.sqrt(d) * (amax * math.sqrt(d)) ** d < 2.0 ** 62, \
        f"int64 Laplace expansion could overflow: max |coordinate difference| = {amax} at d = {d}"
    by = _masks_by_popcount(d)
    total = 0
    it = combinations(range(no), d)
    while True:
        chunk = list(islice(it, SLICE))
        if not chunk:
            break
        A = a[np.array(chunk, dtype=np.int64).reshape(-1, d)]             # (c, d, d): rows are the points
        minors = {0: np.ones(len(chunk), dtype=np.int64)}
        for r in range(d):
            new = {}
            for mask in by[r + 1]:
                acc = np.zeros(len(chunk), dtype=np.int64)
                pos = 0
                for j in range(d):
                    if mask >> j & 1:
                        term = A[:, r, j] * minors[mask ^ (1 << j)]
                        acc = acc + term if (r + pos) % 2 == 0 else acc - term
                        pos += 1
                new[mask] = acc
            minors = new
        total += sum(np.abs(minors[(1 << d) - 1]).tolist())
    return total


def oja_exact_int(P, selection=None):
    """(values, H) as `oja_exact`, for integer-valued P (and Q): the determinants in numpy int64."""
    P = np.asarray(P, dtype=np.float64)
    vals, Hs = [], []
    for others, x in targets_of(P, selection):
        a = others - x
        ai = a.astype(np.int64)
        assert np.array_equal(ai.astype(np.float64), a), "oja_exact_int takes integer-valued coordinates"
        d = a.shape[1]
        vals.append(float(Fraction(_abs_det_sum_int64(ai), math.factorial(d))))
        Hs.append(hadamard_sum(a))
    return np.array(vals), np.array(Hs)


# ---------------------------------------------------------------- 2. the tolerance
def oja_k(d):
    """K_d: |computed det - det| <= K_d u prod ||a_s||_2 per subset, to first order in u, from the operations of
    oja.hip (fp64, no contraction).  y is the last column, the others the prefix.

    d = 1: the value is |a|, no rounding: 0.
    d = 2: c = (-a_y, a_x) exactly; v = fl(c0 y0 + c1 y1): two products and one add, each term through at most two
           roundings: 2 u (|c0 y0| + |c1 y1|) <= 2 u ||c|| ||y||: 2.
    d = 3: c_i = fl(p q - r s): |dc_i| <= 2 u (|p q| + |r s|).  The vector (|p q| + |r s|)_i of a = |a_0|, b = |a_1| has
           squared norm sum_{i != j} a_i^2 b_j^2 + sum_{i != j} a_i b_i a_j b_j <= ||a||^2 ||b||^2 + (a . b)^2
           <= 2 ||a||^2 ||b||^2, so ||dc|| <= 2 sqrt(2) u ||a_0|| ||a_1||; the dot product of length 3 adds
           3 u ||c|| ||y||: 2 sqrt(2) + 3 < 6.
    d >= 4 (oja_cofactor): P M = L U, partial pivoting, M the d x (d - 1) prefix.
      * |L_ij| <= 1.  Column k of M is updated by the k eliminations before it, each at most doubling its largest
        entry, so row j of U has |U_jk| <= 2^j max|a_k| and sum_{j <= k} |L_ij| |U_jk| <= (2^(k+1) - 1) ||a_k||_inf:
        the growth of partial pivoting, 2^(d-2) in the last column.
      * The computed factors are exact for M + dM with |dM| <= g_(k+1) |L| |U| in column k (Higham, Accuracy and
        Stability, thm 9.3), g_n = n u; the back substitution L^T l = e_d is exact for L + dL, |dL| <= g_(d-1) |L|
        (thm 8.5), a further perturbation dL U of M.  Together column k of M moves by at most
        (k + 1 + d - 1) (2^(k+1) - 1) u ||a_k||_inf per entry, sqrt(d) times that in norm.
      * det is linear in each column and bounded by the product of the column norms (Hadamard), so the determinant
        moves by sqrt(d) sum_{k=0}^{d-2} (k + d) (2^(k+1) - 1) u prod ||a_s||.
      * prod takes d - 1 roundings and prod * l[i] one more: d u ||c|| ||y||; the final dot product of length d
        another d u ||c|| ||y||, and ||c|| ||y|| <= prod ||a_s||.
      K_d = sqrt(d) sum_{k=0}^{d-2} (k + d) (2^(k+1) - 1) + 2 d = 130, 439, 1 305, 3 562, 9 177 for d = 4 ... 8.
    Above a few hundred from d = 5 on because it carries the worst-case growth 2^k of partial pivoting in every
    column, which needs a matrix built for it; the emulation below measures about 1 on every family.  At d = 8 the
    bound is still 1e-12 H, and every mutant below misses it by orders of magnitude or by a NaN."""
    if d == 1:
        return 0.0
    if d == 2:
        return 2.0
    if d == 3:
        return 6.0
    return math.sqrt(d) * sum((k + d) * (2 ** (k + 1) - 1) for k in range(d - 1)) + 2 * d


def oja_tolerance(d, n_subsets, H):
    """K_d u H for the determinants plus (128 + 8 + 2 + slices) u H for the sums: a range of 128 added in order, the
    shuffle tree and the four wave sums of a workgroup, the fold over the slices and the division by d!."""
    slices = max(1, -(-int(n_subsets) // SLICE))
    return (oja_k(d) + PER_THREAD + 8 + 2 + slices) * U * np.asarray(H, dtype=np.float64)


# ---------------------------------------------------------------- the kernel's arithmetic, restated
MUTANTS = ('no_pivot', 'no_sign_flip', 'no_perm', 'abs_threshold', 'drop_last', 'wrap_prefix')


def _cofactor(A, d, mutant):
    """oja_cofactor<D>: A holds the d - 1 prefix rows (lists of d floats)."""
    if d == 1:
        return [1.0]
    if d == 2:
        return [-A[0][1], A[0][0]]
    if d == 3:
        return [A[0][1] * A[1][2] - A[0][2] * A[1][1],
                A[0][2] * A[1][0] - A[0][0] * A[1][2],
                A[0][0] * A[1][1] - A[0][1] * A[1][0]]
    C = d - 1
    M = [[A[j][r] for j in range(C)] for r in range(d)]
    perm = list(range(d))
    prod = 1.0
    for j in range(C):
        p = j
        best = abs(M[j][j])
        if mutant != 'no_pivot':
            for r in range(j + 1, d):
                if abs(M[r][j]) > best:
                    best = abs(M[r][j])
                    p = r
        if (best < 1e-12) if mutant == 'abs_threshold' else (best == 0.0):
            return [0.0] * d
        if p != j:
            if mutant != 'no_sign_flip':
                prod = -prod
            M[j], M[p] = M[p], M[j]
            perm[j], perm[p] = perm[p], perm[j]
        Mj = M[j]
        piv = Mj[j]
        prod *= piv
        for r in range(j + 1, d):
            Mr = M[r]
            f = Mr[j] / piv
            Mr[j] = f
            for k in range(j + 1, C):
                Mr[k] -= f * Mj[k]
    l = [0.0] * d
    l[d - 1] = 1.0
    for i in range(d - 2, -1, -1):
        s = 0.0
        for r in range(i + 1, d):
            s += M[r][i] * l[r]
        l[i] = -s
    c = [0.0] * d
    for i in range(d):
        c[i if mutant == 'no_perm' else perm[i]] = prod * l[i]
    return c


def _unrank(r, no, K):
    """The r-th K-subset of range(no) in lexicographic order."""
    idx, c0 = [], 0
    for p in range(K):
        kk = K - p
        c = c0
        while math.comb(no - c - 1, kk - 1) <= r:
            r -= math.comb(no - c - 1, kk - 1)
            c += 1
        idx.append(c)
        c0 = c + 1
    return idx


def _thread_range(a, no, d, first, left, mutant):
    """One thread of oja_kernel<D>: `left` subsets from rank `first`, summed in order."""
    acc = 0.0
    idx = _unrank(first, no, d)
    if mutant == 'drop_last':
        left -= 1
        if left == 0:
            return acc
    while True:
        try:
            c = _cofactor([a[idx[j]] for j in range(d - 1)], d, mutant)
        except ZeroDivisionError:                # Python raises where the device divides: 0/0 and x/0 poison the sum
            return math.nan
        k0 = idx[d - 1]
        run = min(no - k0, left)
        for j in range(run):
            y = a[k0 + j]
            v = c[0] * y[0]
            for e in range(1, d):
                v += c[e] * y[e]
            acc += abs(v)
        left -= run
        if left == 0 or d == 1:
            return acc
        i = 0
        for t in range(d - 1):
            if idx[t] != no - d + t:
                i = t
        for t in range(d - 1):
            if t == i:
                idx[t] += 1
            elif t > i:
                idx[t] = idx[t - 1] + (0 if mutant == 'wrap_prefix' else 1)
        idx[d - 1] = idx[d - 2] + 1


def _emulate(a, mutant=None):
    """Volume sum of the translated others a (no x d float64): ranges of 128, the workgroup's shuffle tree and wave
    sums, the slices folded in order, the division by d!."""
    a = np.asarray(a, dtype=np.float64)
    no, d = a.shape
    total = math.comb(no, d)
    if total == 0:
        return 0.0
    rows = a.tolist()
    out = 0.0
    for s in range(-(-total // SLICE)):
        acc = np.zeros(THREADS)
        for tid in range(THREADS):
            first = (s * THREADS + tid) * PER_THREAD
            if first >= total:
                break
            acc[tid] = _thread_range(rows, no, d, first, min(PER_THREAD, total - first), mutant)
        w = acc.reshape(THREADS // 64, 64)
        with np.errstate(invalid='ignore'):
            for o in (32, 16, 8, 4, 2, 1):
                w = w[:, :o] + w[:, o:2 * o]
            tot = 0.0
            for k in range(THREADS // 64):
                tot += float(w[k, 0])
            out += tot
    return out / float(math.factorial(d))


def oja_kernel_emulation(P, target, mutant=None):
    """sd_oja_volume_sums for one row of P, operation by operation in Python floats (IEEE binary64, no contraction).
    mutant: None, or one of MUTANTS."""
    assert mutant is None or mutant in MUTANTS
    (others, x), = targets_of(P, [target])
    return _emulate(others - x, mutant)


# ---------------------------------------------------------------- the input families of the GPU tests
def int_cloud(n, d, seed):
    """Integer coordinates in [-12, 12]."""
    return np.random.default_rng(seed).integers(-12, 13, size=(n, d)).astype(np.float64)


def three_targets(n):
    return [0, n // 2, n - 1]


def boundary_cloud(d, others):
    """The integer cloud of the slice-boundary GPU tests: others + 1 rows."""
    return int_cloud(others + 1, d, 1000 * d + others)


N_COND = 12
FAMILIES = ('normal', 'flat', 'collinear', 'pivot', 'outlier', 'duplicates', 'partial')
ZERO_FAMILIES = ('exactly_flat',)
_SEED_ORDER = ('normal', 'flat', 'collinear', 'pivot', 'outlier', 'duplicates', 'exactly_flat', 'partial')


def pivot_scales(d):
    """Axis r of the 'pivot' family is scaled by 2^(-40 e / (d - 1)), e = (r + 1) mod d."""
    return np.exp2(-40.0 * ((np.arange(d) + 1) % d) / (d - 1))


def conditioning_cloud(family, d):
    """The clouds of 3d: N_COND points."""
    rng = np.random.default_rng(7000 + 10 * d + _SEED_ORDER.index(family))
    n = N_COND
    P = rng.normal(size=(n, d))
    if family == 'normal':
        return P
    if family == 'flat':                         # the last coordinate a linear map of the others, plus 1e-9 noise
        P[:, -1] = P[:, :-1] @ rng.normal(size=d - 1) + 0.5 + 1e-9 * rng.normal(size=n)
        return P
    if family == 'collinear':                    # rows 1, 2, 3 on a line through row 0, up to rounding
        v = rng.normal(size=d)
        for row, t in ((1, 0.3), (2, 1.7), (3, -0.9)):
            P[row] = P[0] + t * v
        return P
    if family == 'pivot':                        # the largest scale sits on the last axis at every elimination step
        return P * pivot_scales(d)
    if family == 'partial':                      # every other point has a tiny first coordinate: seen from one of them,
        P[::2, 0] *= 2.0 ** -40                  # a prefix has a_0[0] near 2^-40 beside an a_1[0] near 1, and the
        return P                                 # diagonal entry is a pivot 12 orders too small, not a zero
    if family == 'outlier':                      # one point at 2^40 times the scale of the rest
        P[5] *= 2.0 ** 40
        return P
    if family == 'duplicates':                   # d distinct points: every simplex has two equal vertices and volume 0.
        return P[np.arange(n) % d]               # Two equal columns cancel only up to rounding (fl(fl(p / q) q) != p), so
                                                 # the kernel's sums are a few u H, not 0.0: held to the bound, not to == 0
    if family == 'exactly_flat':                 # in a coordinate hyperplane, two rows repeated: the translated last
                                                 # coordinate is exactly 0 and so is every product with it
        P[:, -1] = 0.75
        P[7] = P[2]
        P[9] = P[4]
        return P
    raise ValueError(family)


@lru_cache(maxsize=None)
def conditioning_case(family, d):
    """(P, exact values, H) for every target; computed once per session.  H is the Hadamard sum of the differences,
    for 'pivot' the scale-aware one of `oja_exact`: there the plain sum is C(n - 1, d) / d! times powers of the largest
    axis, 2^(20 d) times the volumes, and a bound in its units could only catch a NaN."""
    P = conditioning_cloud(family, d)
    want, H = oja_exact(P, scales=pivot_scales(d) if family == 'pivot' else None)
    for arr in (P, want, H):
        arr.setflags(write=False)
    return P, want, H


def normal_cloud(d, n=13):
    return np.random.default_rng(7500 + d).normal(size=(n, d))


def dyadic_cloud(d, n=13):
    """20-bit dyadic coordinates in [0, 1)."""
    return np.random.default_rng(7600 + d).integers(0, 2 ** 20, size=(n, d)).astype(np.float64) / 2.0 ** 20


def ratio(got, want, H):
    """|got - want| / (u H); NaN where got is not finite, 0 where H is 0 and the values agree."""
    got, want, H = (np.asarray(v, dtype=np.float64) for v in (got, want, H))
    with np.errstate(all='ignore'):
        r = np.abs(got - want) / (U * H)
    r = np.where((H == 0) & (got == want), 0.0, r)
    return np.where(np.isfinite(got), r, np.nan)


def outside(got, want, tol):
    """True where a value misses the bound; a NaN or an infinity misses every bound."""
    got = np.asarray(got, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        return ~np.isfinite(got) | ~(np.abs(got - want) <= tol)


# ---------------------------------------------------------------- checks: the references
@pytest.mark.parametrize("d", range(1, 9))
def test_exact_routes_agree_on_integer_clouds(d):
    """The two exact routes, bit for bit, in all three forms; and the float64 restatement to 1e-12."""
    n = {1: 20, 2: 14, 3: 12, 4: 11, 5: 10, 6: 10, 7: 10, 8: 11}[d]
    P = int_cloud(n, d, 10 + d)
    P[1] = P[0]
    a, Ha = oja_exact(P)
    b, Hb = oja_exact_int(P)
    assert np.array_equal(a, b) and np.array_equal(Ha, Hb)
    assert np.all(np.abs(a - oja_sums(P)) <= 1e-12 * np.maximum(1.0, a))
    Q = int_cloud(2, d, 30 + d)
    mem = np.full((3, n), -1, dtype=np.int32)
    mem[0] = np.random.default_rng(d).permutation(n)
    mem[1, :d + 2] = np.random.default_rng(d + 1).permutation(n)[:d + 2]
    for sel in (('external', Q), ('blocks', mem)):
        a, _ = oja_exact(P, sel)
        b, _ = oja_exact_int(P, sel)
        assert np.array_equal(a, b)
    assert b[2] == 0.0
    assert b[0] == oja_exact_int(P[mem[0]], [n - 1])[0][0]


@pytest.mark.parametrize("d", range(1, 9))
def test_exact_matches_restatement_on_the_uniform_and_grid_cases(d):
    """The clouds of test_oja_gpu.py: uniform [0, 1) and {0, 1, 2} grids."""
    n = {1: 30, 2: 25, 3: 18, 4: 14, 5: 12, 6: 11, 7: 11, 8: 12}[d]
    P = np.random.default_rng(100 + d).random((n, d))
    tg = three_targets(n)
    want = oja_sums(P, tg)
    got, H = oja_exact(P, tg)
    assert np.all(np.abs(got - want) <= 1e-12 * np.maximum(1.0, np.abs(want)))
    assert np.all(got <= H * (1 + 1e-12))                                   # Hadamard
    if d in (1, 2, 3, 5, 8):
        n = {1: 20, 2: 16, 3: 12, 5: 10, 8: 11}[d]
        G = np.random.default_rng(200 + d).integers(0, 3, size=(n, d)).astype(np.float64)
        G[1] = G[0]
        want = oja_sums(G)
        for got in (oja_exact(G)[0], oja_exact_int(G)[0]):
            assert np.all(np.abs(got - want) <= 1e-12 * np.maximum(1.0, np.abs(want)))


def test_exact_int_across_a_chunk_boundary():
    """The int route works in chunks of 32 768 subsets: C(299, 2) = 44 551 is two, against the d = 2 cross-product
    table (exact in float64 on integers).  The Hadamard sum of equal norms is the subset count times norm^d / d!."""
    P = int_cloud(300, 2, 5)
    a = np.delete(P, 0, axis=0) - P[0]
    M = np.abs(a[:, 0][:, None] * a[:, 1][None, :] - a[:, 1][:, None] * a[:, 0][None, :])
    assert oja_exact_int(P, [0])[0][0] == np.triu(M, 1).sum() / 2.0          # C(299, 2) = 44 551: two chunks
    assert hadamard_sum(np.ones((23, 5))) == pytest.approx(math.comb(23, 5) * 5 ** 2.5 / 120, rel=1e-13)


def test_exact_int_refuses_what_could_overflow():
    P = int_cloud(10, 8, 1) * 100.0                                           # (2400 sqrt 8)^8 ~ 4e30
    with pytest.raises(AssertionError, match="overflow"):
        oja_exact_int(P, [0])
    with pytest.raises(AssertionError, match="integer-valued"):
        oja_exact_int(int_cloud(6, 2, 1) * 0.5, [0])
    oja_exact_int(int_cloud(10, 8, 1), [0])                                   # |difference| <= 24: inside


def test_tolerance_constants():
    assert [oja_k(d) for d in (1, 2, 3)] == [0.0, 2.0, 6.0]
    assert [round(oja_k(d)) for d in (4, 5, 6, 7, 8)] == [130, 439, 1305, 3562, 9177]
    assert oja_tolerance(4, 35960, 2.0) == (oja_k(4) + 128 + 8 + 2 + 2) * U * 2.0
    assert oja_tolerance(2, 32768, 1.0) == (2 + 128 + 8 + 2 + 1) * U


# ---------------------------------------------------------------- checks: the emulation inside the bound
def _emulated(P, targets, mutant=None):
    return np.array([oja_kernel_emulation(P, t, mutant) for t in targets])


@pytest.mark.parametrize("d", D_COND)
@pytest.mark.parametrize("family", FAMILIES)
def test_emulation_inside_the_bound_conditioning(family, d):
    P, want, H = conditioning_case(family, d)
    got = _emulated(P, range(len(P)))
    r = ratio(got, want, H)
    print(f"emulation {family} d={d}: max |emulation - exact| = {np.nanmax(r):.3f} u H (bound {oja_k(d) + 139:.0f}), "
          f"{digits_checked(family, d):.1f} digits checked")
    assert not outside(got, want, oja_tolerance(d, math.comb(len(P) - 1, d), H)).any()


def digits_checked(family, d):
    """log10 of exact / tolerance, the smallest over the targets: how many leading digits of a value the bound holds
    the kernel to.  Zero or less: a kernel that returns 0.0 for that target passes."""
    P, want, H = conditioning_case(family, d)
    with np.errstate(divide='ignore'):
        return float(np.min(np.log10(want / oja_tolerance(d, math.comb(len(P) - 1, d), H))))


@pytest.mark.parametrize("d", D_COND)
@pytest.mark.parametrize("family", ('normal', 'pivot', 'partial'))
def test_bound_checks_digits(family, d):
    """The families meant to check values (not only survival) do: at least six digits of every target's sum, at every
    d.  'flat', 'outlier', 'collinear' and 'duplicates' are degenerate on purpose and check fewer, down to none
    (lists them); their figures are printed by test_emulation_inside_the_bound_conditioning."""
    digits = digits_checked(family, d)
    print(f"{family} d={d}: {digits:.1f} digits")
    assert digits >= 6.0


@pytest.mark.parametrize("d", D_COND)
@pytest.mark.parametrize("family", ZERO_FAMILIES)
def test_emulation_exact_zeros(family, d):
    P, want, H = conditioning_case(family, d)
    assert (want == 0.0).all()
    got = _emulated(P, range(len(P)))
    assert (got == 0.0).all()


# one slice and a few ranges per d (C(others, d) between 2 and 30 ranges): the integer family at the emulation's speed
INT_EMULATED = {1: 300, 2: 40, 3: 20, 4: 14, 5: 12, 6: 12, 7: 12, 8: 12}


@pytest.mark.parametrize("d", range(1, 9))
def test_emulation_inside_the_bound_integer_clouds(d):
    no = INT_EMULATED[d]
    P = int_cloud(no + 1, d, 40 + d)
    tg = three_targets(no + 1)
    want, H = oja_exact_int(P, tg)
    got = _emulated(P, tg)
    r = ratio(got, want, H)
    print(f"emulation integers d={d}: max |emulation - exact| = {np.nanmax(r):.3f} u H (bound {oja_k(d) + 139:.0f})")
    assert math.comb(no, d) > PER_THREAD
    assert not outside(got, want, oja_tolerance(d, math.comb(no, d), H)).any()


def test_emulation_across_slices():
    """d = 4, 32 others: 35 960 subsets, the second slice and the fold."""
    P = int_cloud(33, 4, 44)
    want, H = oja_exact_int(P, [0])
    got = _emulated(P, [0])
    assert not outside(got, want, oja_tolerance(4, 35960, H)).any()


@pytest.mark.parametrize("d", D_EQUI)
def test_emulation_equivariances_bitwise(d):
    P = normal_cloud(d)
    tg = three_targets(len(P))
    base = _emulated(P, tg)
    for k in (-60, 60):
        assert np.array_equal(_emulated(P * 2.0 ** k, tg), base * 2.0 ** (k * d))
    Q = dyadic_cloud(d)
    moved = _emulated(Q + 2.0 ** 13, tg)
    assert np.array_equal(moved, _emulated(Q, tg))
    want, H = oja_exact(Q, tg)
    assert not outside(moved, want, oja_tolerance(d, math.comb(len(Q) - 1, d), H)).any()
    want, H = oja_exact(P * 2.0 ** -60, tg)
    assert not outside(base * 2.0 ** (-60 * d), want, oja_tolerance(d, math.comb(len(P) - 1, d), H)).any()


# ---------------------------------------------------------------- checks: the mutants outside the bound
def _mutant_inputs(d_list=(4, 5)):
    """(label, P, targets, exact, H, subsets): inputs of the GPU tests themselves, the same arrays.  The one-slice
    integer clouds of test_slice_and_range_boundaries, then the conditioning families, then a scaled cloud of
    test_isotropic_scaling_is_exact."""
    for d in d_list:
        no = BOUNDARY[d][0]
        P = boundary_cloud(d, no)
        tg = three_targets(no + 1)
        want, H = oja_exact_int(P, tg)
        yield f"integers d={d}", P, tg, want, H, math.comb(no, d)
    for d in d_list:
        for family in FAMILIES:
            P, want, H = conditioning_case(family, d)
            yield f"{family} d={d}", P, list(range(len(P))), want, H, math.comb(len(P) - 1, d)
    for d in (5,):
        P = normal_cloud(d) * 2.0 ** -60
        tg = three_targets(len(P))
        want, H = oja_exact(P, tg)
        yield f"normal * 2^-60 d={d}", P, tg, want, H, math.comb(len(P) - 1, d)


def _killed_by(mutant):
    for label, P, tg, want, H, subsets in _mutant_inputs():
        got = _emulated(P, tg, mutant)
        tol = oja_tolerance(P.shape[1], subsets, H)
        if outside(got, want, tol).any():
            r = ratio(got, want, H)
            worst = "not finite" if np.isnan(r).any() else f"{np.max(r):.3g} u H"
            return f"{label}: {worst} (bound {np.max(tol / (U * H)):.0f} u H)"
    return None


@pytest.mark.parametrize("mutant", [m for m in MUTANTS if m != 'no_sign_flip'])
def test_mutant_is_caught(mutant):
    where = _killed_by(mutant)
    print(f"{mutant}: {where}")
    assert where is not None, f"{mutant} stays inside oja_tolerance on every input"


@pytest.mark.parametrize("d", (4, 5))
@pytest.mark.parametrize("family,mutant", [('pivot', 'no_perm'), ('partial', 'no_pivot')])
def test_family_alone_kills_its_mutant(family, mutant, d):
    """The families that guard the pivot search, the swap and `perm` do so on their own, and through the bound:
    the mutant's sums are finite (no zero pivot, no early exit on an exact 0) and outside `oja_tolerance`, at d = 4
    and at d = 5.  'pivot' in units of its scale-aware H; 'partial' makes a swap matter numerically, which row scaling
    alone never does (elimination without pivoting is as accurate on 'pivot' as with it)."""
    P, want, H = conditioning_case(family, d)
    tg = range(len(P))
    tol = oja_tolerance(d, math.comb(len(P) - 1, d), H)
    got = _emulated(P, tg, mutant)
    assert np.isfinite(got).all()
    miss = outside(got, want, tol)
    print(f"{mutant} on {family} d={d}: {int(miss.sum())} of {len(P)} targets outside, worst "
          f"{np.max(ratio(got, want, H)):.3g} u H (bound {oja_k(d) + 139:.0f})")
    assert miss.any()
    (others, x), = targets_of(P, [0])
    a = (others - x).tolist()
    for S in islice(combinations(range(len(a)), d - 1), 60):
        assert any(v != 0.0 for v in _cofactor([a[s] for s in S], d, mutant))
    assert not outside(_emulated(P, tg), want, tol).any()


def test_sign_mutant_is_equivalent():
    """'Sign not flipped on a row swap' cannot be caught by any input: the sign of the permutation multiplies every
    component of c, and the kernel sums |c . a_k|.  The mutant changes the sign of c for an odd number of swaps and no
    bit of any result; asserted here, so that a rewrite which makes the sign matter (signed partial sums, a Schur
    update that mixes old and new c) finds this test and adds the input that tells the two apart."""
    flipped = 0
    for d in (4, 5, 8):
        P, want, H = conditioning_case('pivot', d)
        (others, x), = targets_of(P, [0])
        a = (others - x).tolist()
        for S in islice(combinations(range(len(a)), d - 1), 40):
            c0 = _cofactor([a[s] for s in S], d, None)
            c1 = _cofactor([a[s] for s in S], d, 'no_sign_flip')
            assert c1 == c0 or c1 == [-v for v in c0]
            flipped += c1 != c0
        tg = three_targets(len(P))
        assert np.array_equal(_emulated(P, tg, 'no_sign_flip'), _emulated(P, tg))
    assert flipped > 0
