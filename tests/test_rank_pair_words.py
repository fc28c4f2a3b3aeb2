"""rank_bucket32_kernel's scatter with ONE 4-byte LDS read per key (round 10).

Behind the prefix sum, histogram word k of a row without a bucket of 64 keys is the PAIR WORD of buckets 2k and 2k + 1,

    count(2k) | count(2k + 1) << 8 | base(2k) << 16,

and a key reads it with its KEY WORD, 8 * (bucket & 1) | (4 * (bucket >> 1)) << 5 | slot << 24, whose low five bits are all that
v_bfe_u32 uses of an offset or a width: count = bfe(pair, key, 8), base = (pair >> 16) + bfe(pair, 0, key).  A crowded row (a
bucket of 64 keys or more) keeps the two bases of a word as halfwords and the scatter of two halfword reads; which of the two a
row takes is decided per row, so one workgroup may use both.

Host test: a model of the encoding and its decode.  GPU tests: sd_mbd_counts (engine.mbd_counts) against the oracle's rank-sort
totals, exactly; the oracle alone decides.  T = 256 timepoints is the fewest rows the two-launch path takes on 256 CUs, n = 3 073
the smallest n of the path (6 keys per thread).  Rows with hand-placed keys are checked on the host against the model of the key
image in test_bucket32_fma_image.py: the buckets meant are the buckets hit.
"""
import numpy as np
import pytest

from test_bucket32_fma_image import UNCLIPPED, RowMap

T = 256
NB = 16384
SIZES = [3073, 10000]                                                 # 6 and 20 keys per thread


# ---------------------------------------------------------------------------------------------------------------------------
# host: the words
# ---------------------------------------------------------------------------------------------------------------------------
def _bfe(src, offset, width):
    """v_bfe_u32: five bits of the offset and of the width are read"""
    return (src >> (offset & 31)) & ((1 << (width & 31)) - 1)


def _perm(s0, s1, sel):
    """v_perm_b32: byte i of the result is byte sel[i] of the eight bytes s0:s1 (selectors 0 .. 7 only)"""
    both = (s0 << 32) | s1
    return sum(((both >> (8 * ((sel >> (8 * i)) & 0xFF))) & 0xFF) << (8 * i) for i in range(4))


def key_word(b, slot):
    return ((b & 1) << 3) | ((b >> 1) << 7) | (slot << 24)


def pair_word(base, c0, c1):
    """from the histogram word of two 16-bit counters, as the prefix sum builds it"""
    return _perm(base, c0 | (c1 << 16), 0x05040200)


def decode(pw, kw):
    return (pw >> 16) + _bfe(pw, 0, kw), _bfe(pw, kw, 8)


def test_pair_word_model():
    counts = (0, 1, 2, 15, 16, 62, 63)
    seen = 0
    for c0 in counts:
        for c1 in counts:
            for base in (0, 1, 3, 4, 11263 - c0 - c1):
                pw = pair_word(base, c0, c1)
                assert pw == c0 | (c1 << 8) | (base << 16) and pw < 2 ** 30
                for b in (0, 1, 2, 3, 8190, 8191, NB - 4, NB - 3, NB - 1):
                    for slot in (0, 1, 62, 63, 255):
                        kw = key_word(b, slot)
                        assert kw < 2 ** 32
                        assert _bfe(kw, 5, 16) == 4 * (b >> 1)        # the byte offset of the key's histogram word
                        assert kw >> 22 == 4 * slot and kw >> 24 == slot
                        assert (_bfe(kw, 7, 14) << 1) | ((kw >> 3) & 1) == b
                        assert _bfe(kw << 1, 0, 5) == 16 * (b & 1)    # the half of the raw counter word its slot is read from
                        want = (base + c0, c1) if b & 1 else (base, c0)
                        assert decode(pw, kw) == want
                        seen += 1
    assert seen == 7 * 7 * 5 * 9 * 5
    # the dummy counter of the NaN image (bucket NB + 2) is word NB / 2 + 1, an even bucket
    kw = key_word(NB + 2, 200)
    assert _bfe(kw, 5, 16) == 4 * (NB // 2 + 1) and kw & 31 == 0 and kw >> 24 == 200


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    from statdepth_amd import engine
    return engine


def _walks(n, seed, rows=T):
    return np.random.default_rng(seed).normal(size=(rows, n)).cumsum(axis=0)


def _check(eng, oracle, X):
    want = oracle.mbd_counts_ranksort(X, 2)
    got = eng.mbd_counts(X, None, 2, algo="rank")
    assert got.shape == want.shape
    assert (got == want).all()


def _at(lo, hi, bucket, f):
    """the value whose image lies the fraction f into `bucket` of an unclipped row (core buckets 2 .. NB - 3)"""
    return lo + ((bucket - 2) + f) * (hi - lo) / 16380.0


def _placed_row(rng, n, lo, hi, groups):
    """A row with minimum lo and maximum hi whose keys are all placed by hand: `groups` = [(bucket, count)] with distinct
    fractions inside a bucket, the rest spread evenly (distinct buckets' worth apart) over the core, away from every bucket
    within 3 of a group.  The even spread, in a random order of the curves, keeps every thread's keys all over the range,
    so the row is not clipped.  Returns the row and the buckets the spread may have touched."""
    vals = [lo, hi]
    for b, c in groups:
        vals += [_at(lo, hi, b, 0.1 + 0.8 * (j + 0.5) / c) for j in range(c)]
    rest = n - len(vals)
    taken = np.zeros(NB, dtype=bool)
    for b, _ in groups:
        taken[max(b - 3, 0): b + 4] = True
    taken[:6] = True                                                  # the ends belong to lo, hi and the groups there
    taken[NB - 7:] = True
    free = np.flatnonzero(~taken)
    pick = free[np.linspace(0, len(free) - 1, rest).astype(np.int64)] if rest <= len(free) else rng.choice(free, size=rest)
    vals += [_at(lo, hi, int(b), f) for b, f in zip(pick, rng.uniform(0.2, 0.8, size=rest))]
    row = np.array(vals)
    assert len(row) == n and row.min() == lo and row.max() == hi
    return row[rng.permutation(n)], set(int(b) for b in pick)


def _assert_buckets(row, lo, hi, groups, spread):
    """the model of the image: the groups' buckets hold exactly their keys, the buckets named empty hold none"""
    m = RowMap(lo, hi, UNCLIPPED)
    near = set()
    for b, _ in groups:
        near.update(range(b - 1, b + 3))
    # every key that can lie in or next to a group's bucket, through the exact model (the others through their placement)
    approx = 2 + (row - lo) * (16380.0 / (hi - lo))
    cand = row[(np.abs(approx[:, None] - np.array(sorted(near), dtype=float)[None, :]) < 3.0).any(axis=1)]
    hist = {}
    for x in cand:
        b = m.image(float(x))[0]
        hist[b] = hist.get(b, 0) + 1
    want = dict(groups)
    for b in near:
        if 2 <= b <= NB - 3:
            assert hist.get(b, 0) == want.get(b, 0) + (b == NB - 3) + (b == 2 and m.image(lo)[0] == 2), (b, hist.get(b, 0))
    assert not (near & spread)


@pytest.mark.gpu
def test_parity_and_neighbours(eng, oracle):
    """In every row, at three places of the histogram that move with the row: a key alone in an even bucket (odd partner
    empty), a key alone in an odd bucket (even partner empty), a pair of buckets both occupied, an odd bucket followed by
    an occupied even bucket of the next word (its own even partner empty), and keys in the first and the last core bucket."""
    n = 3073
    rng = np.random.default_rng(1001)
    ends = [(-1024.0, 1024.0), (0.0, 4096.0), (-3.0, 5.0), (1.0e6, 1.0e6 + 512.0)]
    X = np.empty((T, n))
    for r in range(T):
        lo, hi = ends[r % len(ends)]
        groups = [(2, 2), (NB - 3, 1)]
        for w in (1000 + 14 * r, 6001 + 22 * r, 12000 + 2 * (r % 61)):
            w &= ~1
            groups += [(w, 1),                                        # even alone: w + 1 empty
                       (w + 11, 1),                                   # odd alone: w + 10 empty
                       (w + 20, 2), (w + 21, 3),                      # both buckets of a word
                       (w + 31, 2), (w + 32, 1)]                      # odd, then the even bucket of the next word; w + 30, w + 33 empty
        row, spread = _placed_row(rng, n, lo, hi, groups)
        if r % 16 == 0:
            _assert_buckets(row, lo, hi, groups, spread)
        X[r] = row
    _check(eng, oracle, X)


def _count_rows(n, count_of_row, seed):
    """walks in which one bucket of every row holds count_of_row(r) distinct values (an unclipped row's bucket 3000 + 5 r)"""
    rng = np.random.default_rng(seed)
    X = np.empty((T, n))
    for r in range(T):
        c = count_of_row(r)
        b = 3000 + 5 * r
        row, spread = _placed_row(rng, n, -8.0, 8.0, [(b, c)])
        if r % 64 == 0:
            _assert_buckets(row, -8.0, 8.0, [(b, c)], spread)
        X[r] = row
    return X


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_bucket_of_63_keys(eng, oracle, n):
    """the largest count a pair word carries: the member pass and its long-bucket loop run, in an even and in an odd bucket"""
    _check(eng, oracle, _count_rows(n, lambda r: 63, 2000 + n))


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_bucket_of_64_keys(eng, oracle, n):
    """the same rows with 64 keys in the bucket, every fourth of them: crowded, today's words, handed to the second launch"""
    _check(eng, oracle, _count_rows(n, lambda r: 64 if r % 4 == 0 else 63, 2000 + n))


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_closed_form_on_pair_words(eng, oracle, n):
    """values rounded to 0.1 with 1 % duplicated curves: buckets of 16 .. 63 equal keys read through the pair words"""
    rng = np.random.default_rng(3000 + n)
    X = np.round(_walks(n, 3000 + n), 1)
    src = rng.choice(n, size=n // 100, replace=False)
    X[:, (src + 1) % n] = X[:, src]
    _check(eng, oracle, X)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_closed_form_on_a_crowded_row(eng, oracle, n):
    """300 curves share one value in every third row of quantised data: closed form with a count the pair word cannot hold"""
    rng = np.random.default_rng(3500 + n)
    X = np.round(_walks(n, 3500 + n) * 4.0, 1)
    for r in range(0, T, 3):
        X[r, rng.choice(n, size=300, replace=False)] = X[r, rng.integers(n)]
        assert np.unique(X[r], return_counts=True)[1].max() >= 300
    _check(eng, oracle, X)


def _crowded(rng, row, kind):
    """a crowded version of a walk's row: 300 equal keys among quantised values (closed form), or 64 distinct values in
    one bucket of a continuous row (handed over)"""
    n = len(row)
    if kind == 0:
        row = np.round(row, 1)
        row[rng.choice(n, size=300, replace=False)] = row[rng.integers(n)]
        return row
    lo, hi = row.min(), row.max()
    inner = np.flatnonzero((row > lo) & (row < hi))
    # (a hundredth of an unclipped row's bucket: one bucket under a clipped map's finer core as well)
    row[rng.choice(inner, size=64, replace=False)] = [_at(lo, hi, 5000, 0.5 + 0.01 * j / 64) for j in range(64)]
    return row


@pytest.mark.gpu
@pytest.mark.parametrize("crowded_first", [True, False], ids=["crowded_then_plain", "plain_then_crowded"])
def test_two_formats_in_one_workgroup(eng, oracle, crowded_first):
    """T = 520: with a grid of 512 workgroups rows r and r + 512 share one.  Eight of them take a crowded row and a plain
    walk, in either order: a word format must not leak from one row into the next."""
    n, rows = 3073, 520
    rng = np.random.default_rng(4000 + crowded_first)
    X = _walks(n, 4000, rows=rows) + 3.0 * rng.normal(size=(rows, n))
    for k in range(8):
        r = k if crowded_first else 512 + k
        X[r] = _crowded(rng, X[r].copy(), k // 4)
    _check(eng, oracle, X)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_empty_slots_land_on_the_dummy(eng, oracle, n, sign):
    """Data of one sign: a key slot beyond n read as 0 would lie below (above) every curve; its image goes to the dummy word
    behind S, its pair-word read to the dummy counter."""
    X = sign * (np.abs(_walks(n, 5000 + n)) + 1.0)
    assert (sign * X > 0).all()
    _check(eng, oracle, X)

