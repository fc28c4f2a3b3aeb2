"""rank_bucket32_kernel: the member pass's second quad read where it lies, the histogram's words from the image words (round 11).

The member pass counts, among the eight window positions from the 16-byte boundary at or below a bucket's base, the bucket's
own positions [off, off + cnt), off = base & 3.  The second quad of the window is read unconditionally, through the first
one's address: what it holds beyond the bucket -- keys of the next buckets, the sentinels behind the keys, the padding behind
those -- must not count.  The histogram's word b >> 1 and half b & 1 of a key's bucket b are taken from the two words of the
45-bit image directly (the low 14 bits of the high word, bit 31 of the low one), the increment 1 << 16 * parity is
0xFFFF * parity + 1, and the parity stays in bit 31 of the image a key stores.

A member word packed by the scatter (base, position mask, count and a long-bucket flag laid out for the member pass) was built
and measured as well and is NOT in the kernel: it was slower (DESIGN S3, round 11), so there is no model of it here.

Host test: a model of the words that are.  GPU tests: sd_mbd_counts (engine.mbd_counts) against the oracle's rank-sort totals,
exactly; the oracle alone decides.  T = 256 timepoints is the fewest rows the two-launch path takes on 256 CUs; n = 3 073 ..
3 076 are every n mod 4 at the smallest n of the path, 10 000 is the headline's class.  Rows with hand-placed keys are checked
on the host against the model of the key image in test_bucket32_fma_image.py: the buckets meant are the buckets hit, at the
offsets meant.
"""
import numpy as np
import pytest

from test_bucket32_fma_image import NANIMG, UNCLIPPED, VB_HI, RowMap
from test_rank_pair_words import _at, _crowded, _walks, key_word

T = 256
NB = 16384
SIZES = [3073, 3074, 3075, 3076, 10000]
R32_PAD = 12


# ---------------------------------------------------------------------------------------------------------------------------
# host: the words
# ---------------------------------------------------------------------------------------------------------------------------
def image_words(b, local):
    """the two words of 2^38 + image for a key of bucket b with the 31-bit bucket-local image `local`"""
    image = (b << 31) | local
    return VB_HI + (image >> 32), image & 0xFFFFFFFF


def from_image_words(vh, q):
    """what the histogram phase makes of them: the atomic's byte offset, its increment, the key word, the stored image"""
    off4 = (vh << 2) & 0xFFFC
    par = q >> 31
    return off4, ((par * 0xFFFF) & 0xFFFFFF) + 1, (off4 << 5) | (par << 3), q


def test_histogram_words_from_the_image_words():
    for b in (0, 1, 2, 3, 1023, 1024, 8190, 8191, 8192, NB - 3, NB - 2, NB - 1, NB + 2):
        for local in (0, 1, 0x3FFF, 0x12345678, 0x7FFFFFFF):
            vh, q = image_words(b, local)
            off4, one, kw, stored = from_image_words(vh, q)
            assert off4 == 4 * (b >> 1) and one == 1 << (16 * (b & 1))
            assert kw == key_word(b, 0)                               # round 10's key word, bit for bit
            # the parity in bit 31 of the stored image: the same bit for every key of the bucket, so that the 32-bit
            # difference of two of its images has the sign of the 31-bit one
            assert stored >> 31 == (b & 1) and stored & 0x7FFFFFFF == local
            for other in (0, 1, local, 0x7FFFFFFF):
                y = image_words(b, other)[1]
                assert (((y - stored) & 0xFFFFFFFF) >> 31 == 1) == (other < local)
    # the NaN image as the tail code gives it: bucket NB + 2, word NB / 2 + 1, an even bucket
    vh, q = NANIMG >> 18, (NANIMG << 14) & 0xFFFFFFFF
    assert from_image_words(vh, q)[:3] == (4 * (NB // 2 + 1), 1, key_word(NB + 2, 0))


def test_second_quad_stays_inside_the_keys_block():
    """for every n of the path and every base the window's second quad ends inside the dummy_pos(n) + 4 words of S"""
    for n in list(range(3073, 3081)) + [4096, 4097, 9999, 10000, 10240, 11261, 11264]:
        al4 = (n + 3) & ~3
        words = al4 + R32_PAD + 4
        for base in (0, 1, 2, 3, 4, n - 5, n - 4, n - 3, n - 2, n - 1):
            assert 4 * (base >> 2) + 7 <= al4 + 3 < words


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    from statdepth_amd import engine
    return engine


def _check(eng, oracle, X):
    want = oracle.mbd_counts_ranksort(X, 2)
    got = eng.mbd_counts(X, None, 2, algo="rank")
    assert got.shape == want.shape
    assert (got == want).all()


def _offset_row(rng, n, lo, hi, groups, check):
    """A row with minimum lo and maximum hi whose keys are all placed by hand.  `groups` = [(bucket, count, off, f0, f1)] in
    ascending buckets: `count` keys at distinct fractions in [f0, f1] of `bucket`, whose first sorted position is `off` mod 4
    (off None: wherever it falls).  Up to three single keys in buckets of their own, 12 .. 16 below a group, shift it there.
    The rest of the row is spread evenly over the buckets away from every group, in a random order of the curves, so that
    every thread's keys lie all over the range and the row is not clipped.  With `check` the exact model of the image says
    which bucket every key near a group lies in."""
    assert all(groups[i][0] + 40 <= groups[i + 1][0] for i in range(len(groups) - 1)) and groups[0][0] >= 60
    taken = np.zeros(NB, dtype=bool)
    for b, *_ in groups:
        taken[b - 20: b + 6] = True
    taken[:6] = True
    taken[NB - 7:] = True
    free = np.flatnonzero(~taken)
    placed = sum(g[1] for g in groups)
    rest = n - 2 - placed - 3 * len(groups)
    assert 0 < rest <= len(free)
    pick = free[np.linspace(0, len(free) - 1, rest).astype(np.int64)]
    assert len(np.unique(pick)) == rest
    last = max(g[0] for g in groups if g[2] is not None)
    spare = [int(b) for b in free[~np.isin(free, pick)] if last + 10 < b < NB - 10]   # above every group that is given an offset
    shims = []
    for b, c, off, f0, f1 in groups:
        base = 1 + int((pick < b).sum()) + sum(g[1] for g in groups if g[0] < b) + len(shims)   # lo, the spread, groups, shims
        s = 0 if off is None else (off - base) % 4
        shims += [b - 12 - 2 * j for j in range(s)]
    fill = spare[:3 * len(groups) - len(shims)]                         # the keys the shims did not take: above every group
    assert len(fill) == 3 * len(groups) - len(shims)
    vals = [lo, hi]
    for b, c, off, f0, f1 in groups:
        vals += [_at(lo, hi, b, f0 + (f1 - f0) * (j + 0.5) / c) for j in range(c)]
    vals += [_at(lo, hi, b, 0.5) for b in shims + fill]
    vals += [_at(lo, hi, int(b), f) for b, f in zip(pick, rng.uniform(0.2, 0.8, size=rest))]
    row = np.array(vals)
    assert len(row) == n and row.min() == lo and row.max() == hi
    if check:
        m = RowMap(lo, hi, UNCLIPPED)
        approx = 2 + (row - lo) * (16380.0 / (hi - lo))
        srt = np.sort(row)
        for b, c, off, f0, f1 in groups:
            near = row[np.abs(approx - b) < 3.0]
            hit = [x for x in near if m.image(float(x))[0] == b]
            extra = (b == NB - 3) + (b == 2 and m.image(lo)[0] == 2)
            assert len(hit) == c + extra, (b, len(hit))
            base = int(np.searchsorted(srt, min(hit)))
            assert off is None or base % 4 == off, (b, base, off)
            assert all(m.image(float(x))[0] != b for x in row[(np.abs(approx - b) >= 3.0) & (np.abs(approx - b) < 6.0)])
    return row[rng.permutation(n)]


def _tile(rows, ends):
    """T rows from a few placed ones: row r is placed row r mod len(rows) (each was built for its own ends)"""
    return np.stack([rows[r % len(rows)] for r in range(T)])


ENDS = [(-1024.0, 1024.0), (0.0, 4096.0), (-3.0, 5.0), (1.0e6, 1.0e6 + 512.0)]


def _placed_matrix(n, seed, groups_of_row, nrows=16):
    rng = np.random.default_rng(seed)
    rows = []
    for k in range(nrows):
        lo, hi = ENDS[k % len(ENDS)]
        rows.append(_offset_row(rng, n, lo, hi, groups_of_row(k), check=(k % 4 == 0)))
    return _tile(rows, ENDS)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_either_side_of_the_second_quad_and_of_the_long_loop(eng, oracle, n):
    """At every off = base & 3: buckets with cnt + off = 4 and 5 (the second quad holds none / one of its keys) and with
    cnt + off = 8 and 9 (the window holds all of it / the long loop takes one key), and the row's last bucket -- three keys
    ending at position n - 1, so that the second quad is the sentinels' or, for n a multiple of 4, lies wholly behind the keys."""
    def groups(k):
        g = []
        b = 300 + 37 * k
        for off in range(4):
            for total in (4, 5, 8, 9):
                if total - off >= 1:
                    g.append((b, total - off, off, 0.1, 0.9))
                    b += 60 + (k % 3)
        g.append((NB - 3, 2, None, 0.1, 0.6))
        return g
    _check(eng, oracle, _placed_matrix(n, 100 + n, groups))


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_bucket_of_63_keys_at_off_3(eng, oracle, n):
    """the largest bucket of the member pass starting on a quad's last word: 66 window positions, 15 turns of the long loop;
    at off = 0 .. 2 in other rows"""
    _check(eng, oracle, _placed_matrix(n, 200 + n, lambda k: [(3000 + 45 * k, 63, 3 if k % 2 == 0 else k % 4, 0.05, 0.95),
                                                               (9000 + 45 * k, 62, 3, 0.05, 0.95)], nrows=8))


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("next_is", ["smaller", "larger"])
def test_second_quad_wholly_the_next_buckets(eng, oracle, n, next_is):
    """A bucket that ends with its first quad (cnt + off = 4, 3, 2) followed at once by a bucket of 9 keys: the second quad
    read unconditionally holds four keys of the NEXT bucket, whose bucket-local images are all smaller (larger) than the
    bucket's own.  Only the bucket's own positions may count."""
    f_own, f_next = ((0.6, 0.9), (0.05, 0.4)) if next_is == "smaller" else ((0.05, 0.4), (0.6, 0.9))

    def groups(k, shift):
        # (shift: the nine keys put behind each earlier group move this one's base; asked for so that it ends up at off)
        return [(500 + 41 * k + 70 * i, cnt, (off - shift * i) % 4, f_own[0], f_own[1])
                for i, (off, cnt) in enumerate(((0, 4), (1, 3), (2, 2), (3, 1), (0, 3), (1, 1)))]

    rng = np.random.default_rng(300 + n)
    rows = []
    for k in range(8):
        lo, hi = ENDS[k % len(ENDS)]
        row = _offset_row(rng, n, lo, hi, groups(k, 9), check=False)
        # nine keys of the bucket behind each group's, taken from the top of the spread (above every group)
        top = np.argsort(row)[-(2 + 9 * 6):-2]
        gs = groups(k, 0)
        row[top] = [_at(lo, hi, b + 1, f_next[0] + (f_next[1] - f_next[0]) * (j + 0.5) / 9) for b, *_ in gs for j in range(9)]
        assert row.min() == lo and row.max() == hi
        if k % 4 == 0:
            m = RowMap(lo, hi, UNCLIPPED)
            srt = np.sort(row)
            img = [m.image(float(x)) for x in srt]
            for b, cnt, off, *_ in gs:
                own = [i for i, im in enumerate(img) if im[0] == b]
                nxt = [i for i, im in enumerate(img) if im[0] == b + 1]
                assert len(own) == cnt and own[0] % 4 == off and len(nxt) == 9 and nxt[0] == own[-1] + 1
                # the second quad of the window: positions 4 .. 7 from the quad of the base, all of them the next bucket's
                q0 = 4 * (own[0] // 4)
                assert all(q0 + 4 + p in nxt for p in range(4)) or cnt + off < 4
                cmp = [(img[i][1] < img[own[0]][1]) for i in nxt]
                assert all(cmp) if next_is == "smaller" else not any(cmp)
        rows.append(row)
    _check(eng, oracle, _tile(rows, ENDS))


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_empty_slots_with_data_of_one_sign(eng, oracle, n, sign):
    """a key slot beyond n carries the word of one key at position 0 and the NaN image: read as a curve it would lie below
    (above) every curve"""
    X = sign * (np.abs(_walks(n, 6000 + n)) + 1.0)
    assert (sign * X > 0).all()
    _check(eng, oracle, X)


def _special_row(rng, row, kind):
    n = len(row)
    if kind == "closed":                                              # quantised: buckets of 16 .. 63 equal keys, one value per bucket
        row = np.round(rng.normal(scale=n / 750.0, size=n), 1)         # about 30 keys on the central levels
        c = np.unique(row, return_counts=True)[1].max()
        assert 16 <= c <= 63
        return row
    if kind == "ties":                                                # a few pairs of equal values in a continuous row: the fold's list
        j = rng.choice(n, size=12, replace=False)
        row[j[:6]] = row[j[6:]]
        return row
    return _crowded(rng, row, 0 if kind == "crowded_closed" else 1)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [3073, 10000])
@pytest.mark.parametrize("special_first", [True, False], ids=["special_then_plain", "plain_then_special"])
def test_word_formats_side_by_side_in_one_workgroup(eng, oracle, n, special_first):
    """T = 520: with a grid of 512 workgroups rows r and r + 512 share one.  Eight of them take a closed-form row (member
    words read by the closed form), a row with tied keys (the fold), a crowded row in closed form or a crowded row handed
    over (base | count << 14) next to a plain walk, in either order: a word format must not leak from one row into the next."""
    rows = 520
    rng = np.random.default_rng(7000 + n + special_first)
    X = _walks(n, 7000 + n, rows=rows) + 3.0 * rng.normal(size=(rows, n))
    kinds = ["closed", "ties", "crowded_closed", "crowded_handed_over"]
    for k in range(8):
        r = k if special_first else 512 + k
        X[r] = _special_row(rng, X[r].copy(), kinds[k % 4])
    _check(eng, oracle, X)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [3073, 10000])
def test_ties_duplicates_and_a_nan_row(eng, oracle, n):
    """values rounded to 0.1 with duplicated curves and one row with a NaN: its image goes to the dummy counter (word
    NB / 2 + 1 of the histogram, from the image words directly) and the row to the second launch"""
    rng = np.random.default_rng(n + 8000)
    X = np.round(_walks(n, n + 8000), 1)
    dup = rng.choice(n, size=n // 100, replace=False)
    X[:, dup] = X[:, rng.choice(n, size=n // 100, replace=False)]
    X[T // 2, rng.integers(n)] = np.nan
    _check(eng, oracle, X)
