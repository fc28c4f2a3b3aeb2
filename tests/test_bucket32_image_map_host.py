"""Host model of the bucket-local key images of rank_bucket32_kernel (no GPU).

The kernel computes u = fma(x, scale, off) with 0 < u < 2^31 for a core key, q = trunc(u), the bucket q >> 17 and the local
image (q mod 2^17) << 14 | trunc(2^14 (u - q)).  These checks pin the arithmetic the kernel relies on: the fraction's 14 bits
are exact in fp64 (they equal floor(2^14 u) - 2^14 q), the bucket is the top 14 bits of the 45-bit image floor(2^14 u), the
local image stays below 2^31, and (bucket, local image) is non-decreasing over adjacent doubles.
"""
import numpy as np

CORE = float(0x7FFFFE00 - 256) - 64.0


def _images(u):
    q = np.trunc(u)
    fr = np.trunc((u - q) * 16384.0)
    qi = q.astype(np.int64)
    return qi >> 17, ((qi & 0x1FFFF) << 14) | fr.astype(np.int64), qi


def _row_map(row):
    lo, hi = row.min(), row.max()
    scale = CORE / (hi - lo)
    return lambda x: x * scale + (256.0 - lo * scale)


def test_fraction_bits_are_exact():
    rng = np.random.default_rng(1)
    u = np.concatenate([rng.uniform(256.0, 2.0 ** 31 - 512, size=200000),
                        np.arange(256, 2 ** 31 - 512, 2 ** 17 - 3, dtype=np.float64) + 1.0 - 2.0 ** -22])
    b, loc, q = _images(u)
    full = np.array([int(v * 16384.0) for v in u[:2000]], dtype=object)          # exact: 2^14 u is a double below 2^45
    assert all(int(f) == (int(qq) << 14) + (int(l) & 0x3FFF) for f, qq, l in zip(full, q[:2000], loc[:2000]))
    assert ((u - np.trunc(u)) * 16384.0 == np.ldexp(u - np.trunc(u), 14)).all()
    assert (loc >= 0).all() and (loc < 2 ** 31).all()
    assert (b == np.floor(u * 16384.0).astype(np.int64) >> 31).all()              # the bucket: top 14 bits of 45
    assert (b < 16384).all()


def test_bucket_and_local_image_monotone_over_adjacent_doubles():
    rng = np.random.default_rng(2)
    row = rng.normal(size=10000).cumsum()
    f = _row_map(row)
    x = np.sort(rng.choice(row, size=3000))
    for k in range(6):                                                 # runs of adjacent doubles from each of them
        xs = np.sort(np.concatenate([x, np.nextafter(x, np.inf), np.nextafter(x, -np.inf)]))
        b, loc, _ = _images(f(xs))
        key = b * 2 ** 31 + loc
        assert (np.diff(key) >= 0).all()
        x = np.nextafter(x, np.inf)
    b, loc, _ = _images(f(np.sort(row)))
    assert (np.diff(b * 2 ** 31 + loc) >= 0).all()


def test_near_pairs_resolved_and_unresolved():
    """Pairs 2^-38 x range apart share a 31-bit image about every other time and never a 45-bit one; pairs 2^-46 x range
    apart mostly share the 45-bit image too."""
    rng = np.random.default_rng(3)
    row = rng.normal(size=10000).cumsum()
    f = _row_map(row)
    span = row.max() - row.min()
    a = rng.choice(row, size=4000)
    b1, l1, q1 = _images(f(a))
    b2, l2, q2 = _images(f(a + span * 2.0 ** -38))
    assert (q1 == q2).mean() > 0.5
    assert ((b1 != b2) | (l1 != l2)).all()
    b3, l3, _ = _images(f(a + span * 2.0 ** -46))
    assert ((b1 == b3) & (l1 == l3)).mean() > 0.3


def test_tail_images_keep_the_old_order():
    """A tail key's local image is its 31-bit image's low 17 bits << 14: below every core key of a shared bucket when it is
    below the core, and the NaN image (bucket 16 386) is 0."""
    c0 = 1024 << 17
    qt = np.arange(c0 - 4000, c0, dtype=np.int64)
    loc_t = (qt & 0x1FFFF) << 14
    b_c, loc_c, _ = _images(np.linspace(c0, c0 + 10.0, 1000))
    assert ((qt >> 17).max() < b_c.min()) or (loc_t.max() < loc_c.min())
    nan_img = (16384 + 2) << 17
    assert nan_img >> 17 == 16386 and ((nan_img << 14) & 0x7FFFFFFF) == 0
