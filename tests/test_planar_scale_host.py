"""The exact planar depths (K11 exact halfspace, K13 exact simplicial) at the limits of their predicate and at the edges of
their sweep, without a GPU.

* `sign_exact`: the sign of a b - c d in Python integers, exact for every finite double.  The references of
  tests/test_halfspace_exact_host.py and tests/test_simplicial_exact_host.py take it as `sign=`; unlike their default
  `sign_diff` (Dekker's product, which underflows with the kernel's fma) it shares nothing with plane_sweep.h.
* witness clouds: the smallest clouds whose count changes when ONE non-collinear pair is taken for collinear, on a ladder of
  scales s = 2^-k, with operands of mixed magnitude and with subnormal coordinates.
* `kernel_sign_fma_only` / `kernel_sign`: Python restatements of hx_sign_diff as it was (two branches, the second by fma
  alone) and as it is (plane_sweep.h), the fma emulated by correctly rounding the rational value: the first reports the
  witness pair collinear for k >= 486 and changes the counts, the second equals sign_exact.
* star clouds: integer points on rays through the origin, whose multiplicities fix every group border of the sorted
  sequence; layouts per capacity tier of the sweep and closed forms of both counts, proved here against the references.

tests/test_planar_scale_gpu.py imports all of this as its oracle.
"""
import functools
import math
from fractions import Fraction
from math import comb

import numpy as np
import pytest

from test_halfspace_exact_host import (exact_counts, exact_counts_sweep, exact_external, integer_cloud,
                                       nearly_collinear_cloud, sign_diff)
from test_simplicial_exact_host import _brute_one, simplicial_brute, simplicial_counts, simplicial_external

U = 2.0 ** -52
LADDER = (0, 300, 484, 485, 486, 500, 511, 520, 537, 600, 1000, -300, -499)     # s = 2^-k
SCALES = (-499, 0, 490, 500, 700, 1000)                                          # P 2^-k


# ---------------------------------------------------------------- the rational sign
def _sign_int(a, b, c, d):
    """sign(a b - c d) of four Python floats over their exact integer ratios (the denominators are powers of two)."""
    (na, da), (nb, db), (nc, dc), (nd, dd) = (v.as_integer_ratio() for v in (a, b, c, d))
    v = na * nb * dc * dd - nc * nd * da * db
    return (v > 0) - (v < 0)


def _per_distinct_row(fn, a, b, c, d):
    """fn(a, b, c, d) -> int over arrays: evaluated once per distinct operand row."""
    rows, inv = np.unique(np.stack([a, b, c, d], axis=1), axis=0, return_inverse=True)
    return np.array([fn(*r) for r in rows.tolist()], dtype=np.int8)[np.asarray(inv).ravel()]


def sign_exact(a, b, c, d):
    """The sign of a b - c d, exact for every finite double (subnormals, zeros, products far outside the fp64 range).
    Pairs of products that are far apart are settled by an error bound: with both |fl(a b)|, |fl(c d)| in [2^-960, 2^1000]
    each rounded product is within 2^-53 of its value, relatively, so |fl(p1 - p2)| > 2^-50 (|p1| + |p2|) leaves no doubt.
    Integer operands below 2^30 in magnitude go through int64, where a b - c d is exact; everything else to Python
    integers."""
    arrs = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (a, b, c, d)))
    shape = arrs[0].shape
    a, b, c, d = (v.ravel() for v in arrs)
    with np.errstate(all="ignore"):
        p1, p2 = a * b, c * d
        m1, m2 = np.abs(p1), np.abs(p2)
        lo, hi = 2.0 ** -960, 2.0 ** 1000
        sure = (m1 >= lo) & (m1 <= hi) & (m2 >= lo) & (m2 <= hi) & (np.abs(p1 - p2) > 2.0 ** -50 * (m1 + m2))
        small = (np.abs(a) <= 2.0 ** 30) & (np.abs(b) <= 2.0 ** 30) & (np.abs(c) <= 2.0 ** 30) & (np.abs(d) <= 2.0 ** 30)
        small &= (a == np.rint(a)) & (b == np.rint(b)) & (c == np.rint(c)) & (d == np.rint(d)) & ~sure
    out = np.where(p1 > p2, 1, -1).astype(np.int8)
    if small.any():                                                    # integers below 2^30: a b - c d fits int64
        ai, bi, ci, di = (v[small].astype(np.int64) for v in (a, b, c, d))
        out[small] = np.sign(ai * bi - ci * di)
    rest = np.flatnonzero(~sure & ~small)
    if len(rest):
        out[rest] = _per_distinct_row(_sign_int, a[rest], b[rest], c[rest], d[rest])
    return out.reshape(shape)


def _as_sign(fn):
    """A scalar predicate as a `sign=` argument of the references."""
    def sign(a, b, c, d):
        arrs = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (a, b, c, d)))
        if arrs[0].size == 0:
            return np.zeros(arrs[0].shape, dtype=np.int8)
        return _per_distinct_row(fn, *(v.ravel() for v in arrs)).reshape(arrs[0].shape)
    return sign


# ---------------------------------------------------------------- hx_sign_diff restated (plane_sweep.h)
def _fl(x):
    """The Fraction x correctly rounded to fp64 (int / int is correctly rounded, subnormal results included)."""
    return x.numerator / x.denominator


def _fma(a, b, c):
    return _fl(Fraction(a) * Fraction(b) + Fraction(c))


def _cmp(x, y):
    return (x > y) - (x < y)


def kernel_sign_fma_only(a, b, c, d):
    """hx_sign_diff before the exponent branch: rounded products, else the fma errors wherever the products are equal."""
    p1, p2 = a * b, c * d
    if p1 != p2:
        return _cmp(p1, p2)
    return _cmp(_fma(a, b, -p1), _fma(c, d, -p2))


def kernel_sign(a, b, c, d):
    """hx_sign_diff as plane_sweep.h has it."""
    p1, p2 = a * b, c * d
    if p1 != p2:
        return _cmp(p1, p2)
    if abs(p1) >= 2.0 ** -900:
        return _cmp(_fma(a, b, -p1), _fma(c, d, -p2))
    z1, z2 = a == 0.0 or b == 0.0, c == 0.0 or d == 0.0
    if z1 or z2:
        if z1 and z2:
            return 0
        return (1 if (c < 0.0) != (d < 0.0) else -1) if z1 else (-1 if (a < 0.0) != (b < 0.0) else 1)
    (ma, ea), (mb, eb), (mc, ec), (md, ed) = (math.frexp(v) for v in (a, b, c, d))
    s1, s2 = (-1 if (ma < 0.0) != (mb < 0.0) else 1), (-1 if (mc < 0.0) != (md < 0.0) else 1)
    if s1 != s2:
        return s1
    de = (ea + eb) - (ec + ed)
    if de >= 2:
        return s1
    if de <= -2:
        return -s1
    ma = math.ldexp(ma, de)
    p1, p2 = ma * mb, mc * md
    if p1 != p2:
        return _cmp(p1, p2)
    return _cmp(_fma(ma, mb, -p1), _fma(mc, md, -p2))


# ---------------------------------------------------------------- witness clouds
def witness_pair(k):
    """(a, b, c, d) with a b - c d = u^2 s^2 > 0, s = 2^-k, and equal rounded products (except at k = 512)."""
    s = math.ldexp(1.0, -k)
    return (1.0 + U) * s, (1.0 + U) * s, s, (1.0 + 2.0 * U) * s


def mixed_pair():
    """a near 2^400, b near 2^-900 against c, d near 2^-250: a b - c d = u^2 2^-500 > 0, equal rounded products."""
    a, b, c, d = witness_pair(250)
    return math.ldexp(a, 650), math.ldexp(b, -650), c, d


def subnormal_pair():
    """b a subnormal: (1 + u) 2^499 times (1 + 2^-20) 2^-1054 against 2^-277 times (1 + u + 2^-20) 2^-278; the difference
    is u 2^-20 2^-555 > 0, equal rounded products."""
    beta = 2.0 ** -20
    return (1.0 + U) * 2.0 ** 499, (2.0 ** 20 + 1.0) * 2.0 ** -1074, 2.0 ** -277, (1.0 + U + beta) * 2.0 ** -278


def witness_clouds(pair, w):
    """(K11 cloud, K13 cloud), the origin row 0 the target of both.  v1 = (a, c) and v2 = -(d, b) have cross(v1, v2) =
    c d - a b < 0: not collinear, one closed halfplane through the origin misses both (count 1); taken for collinear they
    are opposite and every halfplane holds one of them (count 2).  With a third other w on the far side of the line, the
    triangle (v1, v2, w) misses the origin (count 0); taken for collinear the origin is on its edge (count 1)."""
    a, b, c, d = pair
    k11 = np.array([[0.0, 0.0], [a, c], [-d, -b]])
    return k11, np.vstack([k11, [w]])


def blind_to(pair):
    """sign_exact, except that the witness pair (a b against c d, in either order and with any signs) is reported
    collinear: what a predicate that loses this one difference computes."""
    want = (sorted(abs(v) for v in pair[:2]), sorted(abs(v) for v in pair[2:]))

    def sign(a, b, c, d):
        out = sign_exact(a, b, c, d)
        arrs = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (a, b, c, d)))
        a, b, c, d = (np.abs(v).ravel() for v in arrs)
        lo1, hi1, lo2, hi2 = np.minimum(a, b), np.maximum(a, b), np.minimum(c, d), np.maximum(c, d)
        hit = np.zeros(len(a), dtype=bool)
        for (l1, h1), (l2, h2) in (want, want[::-1]):
            hit |= (lo1 == l1) & (hi1 == h1) & (lo2 == l2) & (hi2 == h2)
        flat = out.ravel()
        flat[hit] = 0
        return flat.reshape(out.shape)
    return sign


def witness_cases():
    """name -> (pair, w): the ladder, the mixed magnitudes and the subnormal operand."""
    cases = {}
    for k in LADDER:
        s = math.ldexp(1.0, -k)
        cases[f"k{k}"] = (witness_pair(k), (s, -s))
    cases["mixed"] = (mixed_pair(), (0.0, -2.0 ** -250))
    cases["subnormal"] = (subnormal_pair(), (0.0, -2.0 ** -277))
    return cases


def assert_witness_discriminates(pair, w):
    """The counts of the witness clouds under the true sign and under the sign blind to the pair: (1, 2) and (0, 1)."""
    k11, k13 = witness_clouds(pair, w)
    assert _sign_int(*pair) == 1
    blind = blind_to(pair)
    assert exact_counts(k11, [0], sign=sign_exact).tolist() == [1] and exact_counts(k11, [0], sign=blind).tolist() == [2]
    assert simplicial_counts(k13, [0], sign=sign_exact).tolist() == [0]
    assert simplicial_counts(k13, [0], sign=blind).tolist() == [1]
    return k11, k13


# ---------------------------------------------------------------- clouds of the scaling tests
def continuous65():
    return np.random.default_rng(65).uniform(-1.0, 1.0, size=(65, 2))


def factor_cloud():
    """65 points of the grid of eighths in [-3/4, 3/4]^2: differences up to 12 eighths, so equal products with different
    factorisations (3 8 = 4 6 = 2 12), which reach the predicate's exponent branch with unequal exponent sums."""
    return np.random.default_rng(66).integers(-6, 7, size=(65, 2)) / 8.0


def scale_clouds():
    return {"nearly_collinear": nearly_collinear_cloud(), "integer40": integer_cloud(40, 40),
            "integer257": integer_cloud(257, 257), "continuous65": continuous65(), "factor65": factor_cloud()}


def scaled(P, kx, ky=None):
    """P with x times 2^-kx and y times 2^-ky, asserted exact: scaling back returns P, so nothing went subnormal."""
    ky = kx if ky is None else ky
    S = np.column_stack([np.ldexp(P[:, 0], -kx), np.ldexp(P[:, 1], -ky)])
    assert np.array_equal(np.column_stack([np.ldexp(S[:, 0], kx), np.ldexp(S[:, 1], ky)]), P)
    assert np.abs(S).max() <= 2.0 ** 500
    return S


@functools.lru_cache(maxsize=None)
def unit_scale_counts(name):
    """(K11 counts, K13 counts) of every row of scale_clouds()[name] by the rational sign; computed once, read-only."""
    P = scale_clouds()[name]
    out = exact_counts(P, sign=sign_exact), simplicial_counts(P, sign=sign_exact)
    for a in out:
        a.setflags(write=False)
    return out


# ---------------------------------------------------------------- star clouds
def _upper_directions(limit=9):
    """The primitive integer directions of the half-plane y > 0 or (y = 0, x > 0) with |x|, y <= limit, by angle."""
    dirs = [(x, y) for y in range(0, limit + 1) for x in range(-limit, limit + 1)
            if math.gcd(x, y) == 1 and (y > 0 or x > 0)]
    return sorted(dirs, key=functools.cmp_to_key(lambda p, q: -1 if p[0] * q[1] - p[1] * q[0] > 0 else 1))


def hx_tier(cnt_max):
    return 64 if cnt_max <= 64 else 512 if cnt_max <= 512 else 2048 if cnt_max <= 2048 else 8192


# Group starts of the sorted sequence per layout, position 0 first, and the number of vectors.  "full": cnt is the tier's
# capacity; "short": one run of 64 less (at tier 64: an odd count inside the only run).
_S512 = (0, 40, 62, 63, 64, 65, 128, 158, 400, 405, 412, 448)
_S2048 = _S512 + (512, 700, 1022, 1023, 1024, 1500, 1984)
_S8192 = _S2048 + (2048, 2100, 3264, 3840, 4500, 4501, 6000, 8000, 8128)
LAYOUTS = {
    (64, "full"): ((0, 10, 11, 30, 62, 63), 64),
    (64, "short"): ((0, 1, 2, 20, 36), 37),
    (512, "full"): (_S512, 512),
    (512, "short"): (_S512[:-1], 448),
    (2048, "full"): (_S2048, 2048),
    (2048, "short"): (_S2048[:-1], 1984),
    (8192, "full"): (_S8192, 8192),
    (8192, "short"): (_S8192[:-1], 8128),
}


class Star:
    """Ray i (direction dirs[i], by angle) carries pos[i] points j dirs[i], j = 1 .. pos[i], and neg[i] points -j dirs[i].
    The sorted sequence of the sweep is the groups i = 0, 1, ... in this order, group i of pos[i] + neg[i] elements, the
    neg ones carrying the flip flag.  `points`: the nonzero points, rows shuffled."""

    def __init__(self, tier, kind, seed=0):
        starts, cnt = LAYOUTS[tier, kind]
        sizes = np.diff(np.array(starts + (cnt,)))
        assert (sizes > 0).all()
        rng = np.random.default_rng(seed + tier)
        every = _upper_directions()
        pick = np.sort(rng.permutation(len(every))[:len(sizes)])
        self.dirs = [every[i] for i in pick]
        # only flipped, only unflipped, both, in turn (a group of one element cannot be both)
        self.pos = [int(s) if g % 3 == 0 else 0 if g % 3 == 1 else int(s) // 2 for g, s in enumerate(sizes)]
        self.neg = [int(s) - p for s, p in zip(sizes, self.pos)]
        pts = [(sg * j * dx, sg * j * dy) for (dx, dy), p, q in zip(self.dirs, self.pos, self.neg)
               for sg, c in ((1, p), (-1, q)) for j in range(1, c + 1)]
        self.points = rng.permutation(np.array(pts, dtype=np.float64))
        self.tier, self.kind, self.cnt = tier, kind, cnt

    def starts(self):
        """Group starts of the sorted sequence, from the multiplicities."""
        return [0] + np.cumsum(np.add(self.pos, self.neg))[:-1].tolist()

    def halfspace_count(self, c0):
        """K11: c0 + the fewest points strictly on one side of a line through the origin that passes between two
        neighbouring rays: the side counter-clockwise of the gap after ray i holds pos[j], j > i, and neg[j], j <= i."""
        best = self.cnt
        for i in range(len(self.pos)):
            A = sum(self.pos[i + 1:]) + sum(self.neg[:i + 1])
            best = min(best, A, self.cnt - A)
        return c0 + best

    def simplicial_count(self, dup=0):
        """K13: C(m, 3) - sum over direction classes of sum_{r < s} C(L + r, 2), m = cnt + dup others (dup duplicates of
        the origin), L the vectors strictly inside the half turn counter-clockwise of the class."""
        missing = 0
        for i in range(len(self.pos)):
            for s, L in ((self.pos[i], sum(self.pos[i + 1:]) + sum(self.neg[:i])),
                         (self.neg[i], sum(self.neg[i + 1:]) + sum(self.pos[:i]))):
                missing += sum(comb(L + r, 2) for r in range(s))
        return comb(self.cnt + dup, 3) - missing


def assert_layout(star):
    """What the layout is there for, asserted from the multiplicities."""
    st, cnt, tier = star.starts(), star.cnt, star.tier
    sizes = np.diff(st + [cnt]).tolist()
    assert st == list(LAYOUTS[tier, star.kind][0]) and cnt == len(star.points) and hx_tier(cnt) == tier
    kinds = {(p > 0, q > 0) for p, q in zip(star.pos, star.neg)}
    assert kinds == {(True, False), (False, True), (True, True)}       # unflipped only, flipped only, both
    assert len(np.unique(star.points, axis=0)) == cnt
    if star.kind == "full":
        assert cnt == tier and cnt % 64 == 0                           # at the capacity; the last group ends at cnt - 1
    elif tier > 64:
        assert cnt == tier - 64 and cnt % 64 == 0                      # one run short of it
    if tier == 64:
        if star.kind == "full":
            assert {62, 63} <= set(st)                                 # borders on bits 62 and 63: lane 63 reads all ones
        return
    assert {64, 65, 128} <= set(st)                                    # borders 63|64, 64|65, 127|128
    assert {62, 63} <= set(st)
    # a group that starts inside a run and covers at least three whole runs, small groups on both sides
    wide = [g for g, (s, z) in enumerate(zip(st, sizes)) if s % 64 and (s + z) // 64 - (s + 63) // 64 >= 3]
    assert any(0 < g < len(st) - 1 and sizes[g - 1] <= 64 and sizes[g + 1] <= 64 for g in wide)
    if tier == 8192:                                                   # two runs per lane: runs 2 t and 2 t + 1
        runs_with_start = {s // 64 for s in st}
        even_odd = [s for s in st if s % 64 == 0 and (s // 64) % 2 == 1]        # border between a lane's two runs
        odd_even = [s for s in st if s % 64 == 0 and (s // 64) % 2 == 0 and s]  # border between two lanes
        quiet = lambda s: all(s // 64 + o not in runs_with_start for o in (-2, -1, 1, 2))       # noqa: E731
        assert any(quiet(s) for s in even_odd) and any(quiet(s) for s in odd_even)
        assert {1022, 1023} <= set(st)                                 # bits 62 and 63 of a run in the middle


@functools.lru_cache(maxsize=None)
def star(tier, kind):
    s = Star(tier, kind)
    assert_layout(s)
    s.points.setflags(write=False)
    return s


def line_halfspace_counts(t, targets):
    """K11 counts of the points t[i] (1, 2) of a line: the target's multiplicity + min(points before it, points behind)."""
    t = np.asarray(t)
    return np.array([(t == t[p]).sum() + min((t < t[p]).sum(), (t > t[p]).sum()) for p in targets], dtype=np.int64)


def with_origin(points, at):
    """The points with the origin inserted as row `at`."""
    return np.insert(points, at, [0.0, 0.0], axis=0)


# ================================================================ tests
def _random_operands(rng, n):
    """Finite doubles over the whole exponent range, subnormals and zeros included."""
    x = np.ldexp(rng.uniform(0.5, 1.0, size=n), rng.integers(-1080, 1000, size=n)) * rng.choice([-1.0, 1.0], size=n)
    x[rng.random(n) < 0.05] = 0.0
    return x


def _adversarial_rows():
    """Operand rows with equal or nearly equal products: x y z w factored as (x y)(z w) against (x z)(y w), the last
    factor moved by one ulp either way or not at all, at scales down to where every product is zero; the witness pairs;
    zeros of both signs."""
    rng = np.random.default_rng(4)
    rows = []
    for _ in range(60):
        x, y, z, w = (float(v) for v in rng.integers(2 ** 12, 2 ** 13, size=4))
        for k in (0, 440, 460, 500, 530, 540, 700, 1040):
            for k1, k2 in ((k, k), (k + 20, k - 20), (2 * k, 0)):
                if 2 * k > 1040 and k2 == 0:
                    continue
                a, b = math.ldexp(x * y, -k1), math.ldexp(z * w, -k2)
                c, d = math.ldexp(x * z, -k), math.ldexp(y * w, -k)
                for dd in (d, math.nextafter(d, math.inf), math.nextafter(d, -math.inf)):
                    rows += [(a, b, c, dd), (-a, b, c, -dd), (c, dd, a, b), (a, -b, c, dd)]
    rows += [p for _, (p, _) in witness_cases().items()]
    rows += [(p[2], p[3], p[0], p[1]) for _, (p, _) in witness_cases().items()]
    tiny = 2.0 ** -1074
    rows += [(0.0, 3.0, 0.0, 5.0), (-0.0, 3.0, tiny, tiny), (tiny, tiny, 0.0, 1.0), (tiny, -tiny, -0.0, 1.0),
             (tiny, tiny, tiny, tiny), (tiny, 2 * tiny, tiny, tiny), (tiny, tiny, -tiny, tiny), (0.0, 0.0, -0.0, 0.0),
             (2.0 ** -600, 2.0 ** -600, 2.0 ** -1074, 2.0 ** -126), (2.0 ** -600, 2.0 ** -600, 2.0 ** -1074, 2.0 ** -127)]
    return rows


def _fraction_sign(a, b, c, d):
    v = Fraction(a) * Fraction(b) - Fraction(c) * Fraction(d)
    return (v > 0) - (v < 0)


def test_sign_exact_is_the_fraction_sign():
    rng = np.random.default_rng(1)
    a, b, c, d = (_random_operands(rng, 3000) for _ in range(4))
    keep = (np.abs(np.frexp(a)[1] + np.frexp(b)[1]) < 1020) & (np.abs(np.frexp(c)[1] + np.frexp(d)[1]) < 2200)
    adv = np.array(_adversarial_rows())
    a, b, c, d = (np.concatenate([v[keep], adv[:, i]]) for i, v in enumerate((a, b, c, d)))
    got = sign_exact(a, b, c, d)
    want = [_fraction_sign(*(float(v) for v in r)) for r in zip(a, b, c, d)]
    assert got.tolist() == want
    assert {-1, 0, 1} == set(want)
    # the shapes the references pass: a matrix of pairs, and nothing at all
    assert sign_exact(a[:7, None], b[None, :5], c[:7, None], d[None, :5]).shape == (7, 5)
    assert sign_exact(a[:0], b[:0], c[:0], d[:0]).shape == (0,)


def test_kernel_predicate_restated_is_exact():
    """hx_sign_diff as plane_sweep.h has it, restated with an emulated fma, against the rational sign: on operands over
    the whole exponent range whose products stay finite, and on the adversarial rows."""
    rng = np.random.default_rng(2)
    rows = _adversarial_rows()
    a, b, c, d = (_random_operands(rng, 3000) for _ in range(4))
    for r in zip(a, b, c, d):
        r = tuple(float(v) for v in r)
        if abs(math.frexp(r[0])[1] + math.frexp(r[1])[1]) < 1020 and abs(math.frexp(r[2])[1] + math.frexp(r[3])[1]) < 1020:
            rows.append(r)
    bad = [r for r in rows if kernel_sign(*r) != _sign_int(*r)]
    assert not bad, bad[:5]
    assert sum(kernel_sign_fma_only(*r) != _sign_int(*r) for r in rows) > 100     # what the rows are there to catch


def test_fma_only_predicate_loses_the_witness_from_k_486():
    """The two-branch predicate (rounded products, then fma errors) on the ladder: right up to k = 485; from 486 on
    e1 = u^2 s^2 is below half the smallest subnormal and the pair is reported collinear (at k = 512 a subnormal rounding
    separates the two products); from 538 on both products are zero.  The counts of the witness clouds follow the wrong
    sign -- and the predicate of plane_sweep.h gives the true ones."""
    signs = {k: kernel_sign_fma_only(*witness_pair(k)) for k in range(0, 1001)}
    assert all(signs[k] == 1 for k in range(0, 486))
    assert [k for k in range(486, 1001) if signs[k] != 0] == [512]
    assert all(kernel_sign_fma_only(*witness_pair(k)) == 1 for k in (-300, -499))
    assert kernel_sign_fma_only(*mixed_pair()) == 1 and kernel_sign_fma_only(*subnormal_pair()) == 1   # e1 is an fp64 number
    assert all(kernel_sign(*witness_pair(k)) == 1 for k in range(-499, 1001))
    old, new = _as_sign(kernel_sign_fma_only), _as_sign(kernel_sign)
    for name, (pair, w) in witness_cases().items():
        k11, k13 = witness_clouds(pair, w)
        lost = name.startswith("k") and int(name[1:]) >= 486
        # from k = 538 on every cross AND every dot is reported 0: no vector counts on any side, and K11's witness count
        # comes out as c0 = 1, the true value, by accident; K13's does not
        assert exact_counts(k11, [0], sign=old).tolist() == [2 if lost and int(name[1:]) < 538 else 1], name
        assert simplicial_counts(k13, [0], sign=old).tolist() == [1 if lost else 0], name
        assert exact_counts(k11, [0], sign=new).tolist() == [1], name
        assert simplicial_counts(k13, [0], sign=new).tolist() == [0], name


def test_dekker_sign_valid_range():
    """Where the default sign of the references, sign_diff (Dekker's product over Veltkamp's split), departs from the
    rational sign on the ladder: it is right for every s from 2^499 down to 2^-485 and reports the pair collinear from
    2^-486 on, exactly as the fma does -- so a reference built on it cannot see the loss."""
    rows = np.array([witness_pair(k) for k in LADDER]).T
    dekker = sign_diff(*rows)
    assert sign_exact(*rows).tolist() == [1] * len(LADDER)
    assert dekker.tolist() == [0 if k >= 486 else 1 for k in LADDER]


@pytest.mark.parametrize("name", list(witness_cases()))
def test_witness_clouds_discriminate(name):
    pair, w = witness_cases()[name]
    k11, k13 = assert_witness_discriminates(pair, w)
    # the other restatements in rational arithmetic agree with the rational-sign references
    assert exact_counts_sweep(k11).tolist() == exact_counts(k11, sign=sign_exact).tolist()
    assert simplicial_brute(k13).tolist() == simplicial_counts(k13, sign=sign_exact).tolist()
    g = np.zeros((1, 2))
    assert exact_external(k11[1:], g, sign=sign_exact).tolist() == [1]
    assert exact_external(k11[1:], g, sign=blind_to(pair)).tolist() == [2]
    assert simplicial_external(k13[1:], g, sign=sign_exact).tolist() == [0]
    assert simplicial_external(k13[1:], g, sign=blind_to(pair)).tolist() == [1]


def test_rational_references_agree_with_the_rational_restatements():
    for seed in (0, 1, 2):
        P = integer_cloud(40, seed)
        assert np.array_equal(exact_counts(P, sign=sign_exact), exact_counts_sweep(P))
        Z = integer_cloud(14, seed)
        assert np.array_equal(simplicial_counts(Z, sign=sign_exact), simplicial_brute(Z))
        Q = np.random.default_rng(100 + seed).integers(-3, 4, size=(5, 2)).astype(np.float64)
        assert np.array_equal(simplicial_external(Z, Q, sign=sign_exact), [_brute_one(Z - g) for g in Q])
        assert np.array_equal(exact_external(Z, Q, sign=sign_exact),
                              [exact_counts_sweep(np.vstack([Z, g]), [len(Z)])[0] for g in Q])
    P = nearly_collinear_cloud()
    assert np.array_equal(exact_counts(P, sign=sign_exact), exact_counts_sweep(P))
    assert np.array_equal(simplicial_counts(P[:16], sign=sign_exact), simplicial_brute(P[:16]))
    # at unit scale the Dekker sign is the rational sign: the references the other tests use stand
    assert np.array_equal(exact_counts(P), exact_counts(P, sign=sign_exact))
    assert np.array_equal(simplicial_counts(P), simplicial_counts(P, sign=sign_exact))


@pytest.mark.parametrize("k", [-499, 500, 1000])
def test_rational_references_are_scale_invariant(k):
    """P 2^-k has the counts of P (the rounded differences scale exactly), by the rational references themselves and by
    the rational sweep -- where the Dekker sign reports everything collinear."""
    P = nearly_collinear_cloud()
    h, s = unit_scale_counts("nearly_collinear")
    S = scaled(P, k)
    tg = [0, 7, 49]
    assert np.array_equal(exact_counts(S, tg, sign=sign_exact), h[tg])
    assert np.array_equal(simplicial_counts(S, tg, sign=sign_exact), s[tg])
    assert np.array_equal(exact_counts_sweep(S, tg), h[tg])
    if k == 1000:
        assert not np.array_equal(exact_counts(S, tg), h[tg])
    A = scaled(P, -400, 400)                                           # x 2^400, y 2^-400
    assert np.array_equal(exact_counts(A, tg, sign=sign_exact), h[tg])
    assert np.array_equal(simplicial_counts(A, tg, sign=sign_exact), s[tg])


def test_subnormal_grid_has_the_counts_of_the_integer_grid():
    P = integer_cloud(40, 40)
    S = np.ldexp(P, -1074)                                             # every coordinate a multiple of 2^-1074
    assert np.array_equal(np.ldexp(S, 1074), P)
    h, s = unit_scale_counts("integer40")
    assert np.array_equal(exact_counts(S, sign=sign_exact), h)
    assert np.array_equal(simplicial_counts(S, sign=sign_exact), s)
    assert np.array_equal(exact_counts(S, sign=_as_sign(kernel_sign)), h)
    assert not np.array_equal(exact_counts(S, sign=_as_sign(kernel_sign_fma_only)), h)


# ---------------------------------------------------------------- star clouds
@pytest.mark.parametrize("tier,kind", list(LAYOUTS))
def test_star_layouts(tier, kind):
    s = star(tier, kind)
    assert s.starts()[0] == 0 and len(s.points) == s.cnt
    assert np.abs(s.points).max() < 2.0 ** 20                          # integers: every difference and product is exact


@pytest.mark.parametrize("tier,kind", [k for k in LAYOUTS if k[0] <= 512])
def test_star_closed_forms(tier, kind):
    """The closed forms from the multiplicities equal the references with the rational sign: origin as a row (anywhere in
    the sample), as an external point, and with duplicates of the origin among the others; at the 64 tier also the
    brute-force enumeration and the rational sweep."""
    s = star(tier, kind)
    at = s.cnt // 3
    P = with_origin(s.points, at)
    assert exact_counts(P, [at], sign=sign_exact).tolist() == [s.halfspace_count(1)]
    assert simplicial_counts(P, [at], sign=sign_exact).tolist() == [s.simplicial_count()]
    g = np.zeros((1, 2))
    assert exact_external(s.points, g, sign=sign_exact).tolist() == [s.halfspace_count(1)]
    assert simplicial_external(s.points, g, sign=sign_exact).tolist() == [s.simplicial_count()]
    D = with_origin(with_origin(P, 0), len(P))                         # three rows at the origin
    assert exact_counts(D, [0], sign=sign_exact).tolist() == [s.halfspace_count(3)]
    assert simplicial_counts(D, [0], sign=sign_exact).tolist() == [s.simplicial_count(dup=2)]
    if tier == 64:
        assert exact_counts_sweep(P, [at]).tolist() == [s.halfspace_count(1)]
        assert simplicial_brute(P, [at]).tolist() == [s.simplicial_count()]
        assert _brute_one(D[1:]) == s.simplicial_count(dup=2)


def test_line_closed_forms():
    """Points t (1, 2) on one line through the origin: K11's count of a target is its own multiplicity plus the fewer of
    the points before and behind it."""
    t = np.arange(-20, 21)
    assert line_halfspace_counts(t, range(41)).tolist() == [1 + min(p, 40 - p) for p in range(41)]
    assert exact_counts(np.outer(t, [1.0, 2.0]), sign=sign_exact).tolist() == [1 + min(p, 40 - p) for p in range(41)]
    t = np.concatenate([t, t[[5, 5, 30]]])                             # duplicates of two targets
    want = line_halfspace_counts(t, range(len(t)))
    assert want[5] == 3 + 5 and want[30] == 2 + 10 and want[20] == 1 + 21
    assert exact_counts(np.outer(t, [1.0, 2.0]), sign=sign_exact).tolist() == want.tolist()
