"""The 45-bit key image of rank_bucket32_kernel taken from the mantissa of ONE fma.

The kernel computes v = fma(x, scale, off) with off = 2^38 + the core's offset.  For a core key v lies in [2^38, 2^39), where one
ulp is 2^-14 image: the 52-bit mantissa of v is the integer I = round(2^14 u), u = v - 2^38 being the 31-bit image with its
fraction.  With hi / lo the two words of v: bucket = bits 31 .. 44 = alignbit(hi, lo, 31) & 0x7FFF, local image = lo & 0x7FFFFFFF,
and the core test is hi - hi(2^38 + c0) < (c1 - c0) >> 18 (unsigned) -- exact because the core's bounds are multiples of 2^18.
Keys outside the core (and NaN) take the tail code as before; which side is read off v < 2^38 + c0.

Host tests: a model of that arithmetic (the fma in exact rationals), checked for the rounding, for monotonicity over runs of
adjacent doubles and for the core test.  GPU tests: totals == the oracle's rank-sort totals, and == the fp64 bucket kernel alone
(SD_RB_NO32=1), at E = 8, 20 and 22 keys per thread, 260 timepoints (more rows than CUs: the two-launch path is taken).
"""
import struct
from fractions import Fraction

import numpy as np
import pytest

VB = 2.0 ** 38
VB_HI = 0x42500000
CLIPPED = (1024 << 17, 15360 << 17)                                   # the core's images [c0, c1) under the three-piece map
UNCLIPPED = (1 << 18, 0x7FFC0000)                                     # ... of a light-tailed row
NANIMG = (16384 + 2) << 17
TSH = 30


def _bits(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def _fma(a, b, c):
    """fl(a * b + c), one rounding (Fraction -> float is correctly rounded, ties to even)."""
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        return a * b + c
    r = Fraction(a) * Fraction(b) + Fraction(c)
    try:
        return float(r)
    except OverflowError:
        return np.inf if r > 0 else -np.inf


def _words(v):
    w = _bits(v)
    return w >> 32, w & 0xFFFFFFFF


def _core(hi, core):
    c0, c1 = core
    return ((hi - (VB_HI + (c0 >> 18))) & 0xFFFFFFFF) < ((c1 - c0) >> 18)


class RowMap:
    """The kernel's per-row constants and the image of one key, step by step as the kernel computes it."""

    def __init__(self, lo, hi, core):
        self.lo, self.hi, self.core = lo, hi, core
        c0, c1 = core
        wc = hi - lo
        self.scale = (float(c1 - c0) - 64.0) / wc
        self.off = _fma(-lo, self.scale, VB + float(c0))
        self.mc = wc / 448.0

    def v(self, x):
        return _fma(x, self.scale, self.off)

    def image(self, x):
        """(bucket, local image)"""
        c0, c1 = self.core
        v = self.v(x)
        h, l = _words(v)
        if not _core(h, self.core):
            low = v < VB + float(c0)
            d = max((self.lo - x) if low else (x - self.hi), 0.0)
            tc = (_bits(d + self.mc) - _bits(self.mc)) >> TSH
            room = (c0 - 1) if low else 0x7FFFFEFF - c1
            tcc = min(tc, room)
            qt = (c0 - 1 - tcc) if low else (c1 + tcc)
            if x != x:
                qt = NANIMG
            h, l = qt >> 18, (qt << 14) & 0xFFFFFFFF
        return (((h << 32 | l) >> 31) & 0x7FFF), l & 0x7FFFFFFF


def _run(x, k):
    """x and its k neighbours on either side"""
    out = [x]
    a = b = x
    for _ in range(k):
        a, b = np.nextafter(a, -np.inf), np.nextafter(b, np.inf)
        out += [a, b]
    return sorted(out)


# ---------------------------------------------------------------------------------------------------------------------------
# host
# ---------------------------------------------------------------------------------------------------------------------------
def test_mantissa_is_the_rounded_45_bit_image():
    rng = np.random.default_rng(1)
    us = [Fraction(float(u)) for u in rng.uniform(0.0, 2.0 ** 31, size=3000)]
    us += [Fraction(int(k), 2 ** 40) for k in rng.integers(0, 2 ** 62, size=3000) >> rng.integers(0, 40, size=3000)]
    for q in (0, 1, 2 ** 17 - 1, 2 ** 17, 2 ** 18, 2 ** 27, 123456789, 2 ** 31 - 2):   # exact ties (to even, both parities) and a
        for f in (0, 1, 2, 8191, 8192, 16382, 16383):                                   # hair on either side of them
            base = Fraction(q) + Fraction(f, 2 ** 14)
            half = Fraction(1, 2 ** 15)
            us += [base, base + half, base + half - Fraction(1, 2 ** 70), base + half + Fraction(1, 2 ** 70), base + 3 * half]
    for u in us:
        v = float(u + 2 ** 38)                                        # the fma's single rounding
        assert 2.0 ** 38 <= v < 2.0 ** 39
        I = _bits(v) & (2 ** 52 - 1)
        assert I == round(u * 2 ** 14)                                # Fraction.__round__: half to even
        h, l = _words(v)
        assert ((h << 32 | l) >> 31) & 0x7FFF == (I >> 31) and (l & 0x7FFFFFFF) == I & (2 ** 31 - 1)
        assert I >> 31 <= 16384


@pytest.mark.parametrize("core", [CLIPPED, UNCLIPPED], ids=["clipped", "unclipped"])
def test_image_monotone_over_adjacent_doubles(core):
    """Bucket edges, both core bounds and both ends of the binade [2^38, 2^39), in rows at several offsets and scales (the
    offset's rounding grows with |lo| / range)."""
    rng = np.random.default_rng(2)
    c0, c1 = core
    for lo, hi in ((-3.0, 5.0), (1.0e6, 1.0e6 + 1.0), (-7.25e-3, 1.9e-3), (-1024.0, 1024.0), (1.0 / 3.0, 2.0e5 / 7.0)):
        m = RowMap(lo, hi, core)
        edges = [float(c0), float(c1), float(c1) - 64.0, 0.0, 2.0 ** 38 - 1.0, -(2.0 ** 38), 2.0 ** 31, float(c0) - 1.0]
        edges += [float(b << 17) for b in rng.integers(c0 >> 17, c1 >> 17, size=6)]
        edges += [float(rng.integers(c0, c1)) + float(rng.integers(0, 16384)) / 16384.0 + 2.0 ** -15 for _ in range(4)]
        for u in edges:
            xe = lo + (u - c0) / m.scale
            keys = [m.image(x) for x in _run(xe, 40)]
            assert all(a <= b for a, b in zip(keys, keys[1:])), (lo, hi, u)
            assert all(l < 2 ** 31 and b < 16384 for b, l in keys)
        # far apart as well: the pieces are ordered
        xs = np.sort(np.concatenate([rng.uniform(lo - 3 * (hi - lo), hi + 3 * (hi - lo), size=400), lo + (hi - lo) * rng.standard_cauchy(200),
                                     [lo, hi, -1e300, 1e300, lo - 1e12 * (hi - lo), hi + 1e12 * (hi - lo)]]))
        keys = [m.image(float(x)) for x in xs]
        assert all(a <= b for a, b in zip(keys, keys[1:]))
        if core is UNCLIPPED:                                          # the row's own extremes are core keys or one image outside
            assert m.image(lo)[0] in (1, 2) and m.image(hi)[0] == (c1 >> 17) - 1


@pytest.mark.parametrize("core", [CLIPPED, UNCLIPPED], ids=["clipped", "unclipped"])
def test_high_word_core_test_is_exact(core):
    """every double within 4 x 2^18 ulps of either bound"""
    c0, c1 = core
    for bound in (c0, c1):
        w0 = _bits(VB + float(bound))
        w = np.arange(w0 - (4 << 18), w0 + (4 << 18) + 1, dtype=np.uint64)
        hi = (w >> np.uint64(32)).astype(np.int64)
        I = (w & np.uint64(2 ** 52 - 1)).astype(np.int64)
        q = I >> 14
        want = (q >= c0) & (q < c1)
        got = ((hi - (VB_HI + (c0 >> 18))) & 0xFFFFFFFF) < ((c1 - c0) >> 18)
        assert (got == want).all()
        assert got.any() and not got.all()


def test_values_outside_the_binade_are_outside_the_core():
    vs = [np.nan, -np.nan, -0.0, 0.0, 5e-324, -5e-324, 2.2e-308, -2.2e-308, -1.0, -(2.0 ** 38) - float(1 << 20), -(2.0 ** 38.5),
          -1e300, -np.inf, np.inf, 2.0 ** 39, 2.0 ** 39 + 2.0 ** 30, 2.0 ** 37 + 2.0 ** 30, 2.0 ** 38, np.nextafter(2.0 ** 38 + 2.0 ** 18, 0.0),
          2.0 ** 38 + float(0x7FFC0000), 1e300]
    for core in (CLIPPED, UNCLIPPED):
        for v in vs + [np.nextafter(VB + float(core[0]), 0.0), VB + float(core[1])]:
            assert not _core(_words(v)[0], core), v
        for v in (VB + float(core[0]), np.nextafter(VB + float(core[1]), 0.0), VB + 2.0 ** 30):
            assert _core(_words(v)[0], core)
    m = RowMap(-1.0, 1.0, CLIPPED)
    assert m.v(-1e13) < 0.0 and m.image(-1e13) == (0, 0)              # v negative: the lowest tail image (clamped)
    assert m.image(1e13) == (0x7FFFFEFF >> 17, ((0x7FFFFEFF & 0x1FFFF) << 14))
    assert m.image(np.nan)[0] == 16386


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
T = 260
SIZES = [3100, 10000, 11264]                                          # E = 8, 20, 22


@pytest.fixture(scope="module")
def eng():
    from statdepth_amd import engine
    return engine


def _check(eng, oracle, xcheck, X):
    want = oracle.mbd_counts_ranksort(X, 2)
    got = eng.mbd_counts(X, None, 2, algo="rank")
    assert (got == want).all()
    with xcheck(SD_RB_NO32="1"):
        assert (eng.mbd_counts(X, None, 2, algo="rank") == want).all()


def _walks(n, seed):
    return np.random.default_rng(seed).normal(size=(T, n)).cumsum(axis=0)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_fma_image_walks(eng, oracle, xcheck, n):
    _check(eng, oracle, xcheck, _walks(n, 100 + n))


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_fma_image_extremes_on_the_core_ends(eng, oracle, xcheck, n):
    """Minimum and maximum on exactly representable values (power-of-two ranges, offsets where the map's offset is exact and
    where it is rounded), with equal keys and the adjacent doubles inside."""
    rng = np.random.default_rng(200 + n)
    X = _walks(n, 200 + n)
    ends = [(-1024.0, 1024.0), (0.0, 4096.0), (1.0e6, 1.0e6 + 512.0), (-3.0, 5.0), (-0.125, 0.125), (2.0 ** 40, 2.0 ** 40 + 2.0 ** 12)]
    for r, row in enumerate(X):
        a, b = ends[r % len(ends)]
        row[:] = a + (row - row.min()) * ((b - a) / (row.max() - row.min()))
        np.clip(row, a, b, out=row)
        free = rng.permutation(n)[:8]
        row[free] = [a, a, np.nextafter(a, np.inf), np.nextafter(np.nextafter(a, np.inf), np.inf), b, b, np.nextafter(b, -np.inf),
                     np.nextafter(np.nextafter(b, -np.inf), -np.inf)]
        assert row.min() == a and row.max() == b
    _check(eng, oracle, xcheck, X)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_fma_image_cauchy(eng, oracle, xcheck, n):
    """The clipped core with both tails; a few keys at 10^12 x scale on either side: v negative, or beyond the binade."""
    rng = np.random.default_rng(300 + n)
    X = rng.standard_cauchy(size=(T, n))
    for r, row in enumerate(X):
        far = rng.permutation(n)[:6]
        row[far] = np.array([1e12, -1e12, 3e12, -3e12, 1e12, -1e12]) * (1.0 + r)
        if r % 3 == 0:
            row[far[4:]] = [1e12 * (1.0 + r) * (1.0 + 2.0 ** -40), -1e12 * (1.0 + r) * (1.0 + 2.0 ** -40)]
    _check(eng, oracle, xcheck, X)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_fma_image_planted_pairs(eng, oracle, xcheck, n):
    """Pairs 2^-40, 2^-45 and 2^-50 of the range apart, anywhere and straddling a bucket edge of the unclipped map."""
    rng = np.random.default_rng(400 + n)
    X = _walks(n, 400 + n)
    c0, c1 = UNCLIPPED
    for row in X:
        order = np.argsort(row)
        lo, hi = row[order[0]], row[order[-1]]
        span = hi - lo
        cur = rng.permutation(order[10:-10])[:36]
        scale = (float(c1 - c0) - 64.0) / span
        k = 0
        for rel in (2.0 ** -40, 2.0 ** -45, 2.0 ** -50):
            for _ in range(3):                                        # anywhere
                row[cur[k + 1]] = row[cur[k]] + rel * span
                k += 2
            for b in rng.integers(200, 16000, size=3):                # either side of a bucket edge
                xe = lo + (float(int(b) << 17) - c0) / scale
                row[cur[k]], row[cur[k + 1]] = xe - 0.5 * rel * span, xe + 0.5 * rel * span
                k += 2
    _check(eng, oracle, xcheck, X)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_fma_image_rounded_with_duplicated_curves(eng, oracle, xcheck, n):
    rng = np.random.default_rng(500 + n)
    X = np.round(_walks(n, 500 + n), 1)
    src = rng.choice(n, size=n // 100, replace=False)
    X[:, (src + 1) % n] = X[:, src]
    _check(eng, oracle, xcheck, X)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_fma_image_nan_constant_and_signed_zero_rows(eng, oracle, xcheck, n):
    rng = np.random.default_rng(600 + n)
    X = _walks(n, 600 + n)
    for r in range(0, T, 4):
        k = r % 16
        if k == 0:
            X[r, rng.integers(0, n)] = np.nan                         # one NaN
        elif k == 4:
            X[r] = 1.5                                                # all equal
        elif k == 8:
            X[r, rng.permutation(n)[: n // 3]] = 0.0                  # +-0.0 among the values
            X[r, rng.permutation(n)[: n // 3]] = -0.0
        else:
            X[r] = np.where(rng.random(n) < 0.5, 0.0, -0.0)           # nothing but +-0.0
    _check(eng, oracle, xcheck, X)
