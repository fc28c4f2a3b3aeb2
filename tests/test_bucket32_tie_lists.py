"""Keys whose 32-bit images coincide on the two-launch rank path (rank_bucket32_kernel + rank_bucket_kernel's SEL form).

Such keys (two values closer than range / 2^31, or equal values) go on a per-workgroup list of at most 64 entries, and the
first launch settles that list among itself in fp64 at the end of the workgroup.  The inputs here are config-2-sized rows
(10 000 curves) in which keys are planted so that every workgroup lists a known number of them, including exactly 64 (the
last list that is settled in place) and 65 (the list overflows and the workgroup hands all its rows to the second launch).
Row r is ranked by workgroup r mod G, G = min(rows, 2 x CUs), so every workgroup gets two rows.
Every curve's totals are compared with the oracle's rank-sort totals and with the fp64 bucket kernel alone (SD_RB_NO32=1).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 10000


@pytest.fixture(scope="module")
def eng():
    from statdepth_amd import engine
    return engine


def _grid():
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return 2 * cus


def _up(x, k=1):
    """x moved k ulps up: a different double with the same 32-bit image."""
    for _ in range(k):
        x = np.nextafter(x, np.inf)
    return x


def _plant(row, rng, groups):
    """Overwrite curves of `row` with tied groups; `groups` lists their sizes.  Each group takes the value of a random curve
    (away from the row's extremes) and its members sit 0 - 2 ulps above it or on it exactly.  Returns the curves used."""
    k = sum(groups)
    order = np.argsort(row)
    cur = rng.choice(order[10:-10], size=k, replace=False)
    i = 0
    for g in groups:
        x = row[cur[i]]
        for m in range(1, g):
            row[cur[i + m]] = _up(x, int(rng.integers(0, 3)))
        i += g
    return cur


def _check(eng, oracle, xcheck, X):
    want = oracle.mbd_counts_ranksort(X, 2)
    got = eng.mbd_counts(X, None, 2, algo="rank")
    assert (got == want).all()
    with xcheck(SD_RB_NO32="1"):
        assert (eng.mbd_counts(X, None, 2, algo="rank") == want).all()


def test_bucket32_tie_lists_few_per_row(eng, oracle, xcheck):
    """Random walks (their own image coincidences included) with a pair, a group of equal values and a triple planted in every
    row; the second row of each workgroup reuses one curve of the first, so a curve is settled twice into one block."""
    G = _grid()
    rng = np.random.default_rng(51)
    X = rng.normal(size=(2 * G, N)).cumsum(axis=0)
    for w in range(G):
        cur = _plant(X[w], rng, [2, 2, 3])
        X[w, cur[3]] = X[w, cur[2]]                                   # the second pair: equal doubles
        cur2 = _plant(X[w + G], rng, [2, 3])
        X[w + G, cur[0]] = _up(X[w + G, cur2[0]])                    # curve cur[0] is listed in both rows
    _check(eng, oracle, xcheck, X)


@pytest.mark.parametrize("per_wg", [64, 65, "mixed"])
def test_bucket32_tie_lists_at_capacity(eng, oracle, xcheck, per_wg):
    """Rows of distinct integers (no coincidences of their own) with exactly 64 listed keys per workgroup (settled in place),
    65 (every workgroup hands its rows over) or 64 and 65 on alternate workgroups."""
    G = _grid()
    rng = np.random.default_rng(52 if per_wg == "mixed" else per_wg)
    X = np.stack([rng.permutation(N).astype(np.float64) - N // 2 for _ in range(2 * G)])
    for w in range(G):
        k = per_wg if per_wg != "mixed" else 64 + (w & 1)
        _plant(X[w], rng, [2] * 16)                                   # 32 keys
        _plant(X[w + G], rng, [2] * 16 if k == 64 else [2] * 15 + [3])   # 32 or 33
    _check(eng, oracle, xcheck, X)


def test_bucket32_tie_lists_signed_zero_and_bucket_edges(eng, oracle, xcheck):
    """Groups of +0.0 / -0.0 (equal) with the smallest denormal (larger, same image), equal doubles, and pairs a hair either
    side of a bucket edge of the row's linear map (16 384 buckets over the image range [256, 2^31 - 512))."""
    G = _grid()
    rng = np.random.default_rng(53)
    X = np.stack([rng.permutation(N).astype(np.float64) - N // 2 for _ in range(2 * G)])
    for r in range(2 * G):
        row = X[r]
        z = rng.choice(np.flatnonzero(np.abs(row) > 50), size=3, replace=False)
        row[z[0]], row[z[1]], row[z[2]] = 0.0, -0.0, 5e-324
        if r % 3 == 0:
            row[np.flatnonzero(row == 7.0)[0]] = -0.0                 # a third zero in some rows
        lo, hi = row.min(), row.max()
        scale = ((0x7FFFFE00 - 256) - 64.0) / (hi - lo)
        eps = (hi - lo) * 1e-10                                       # under half an image
        free = rng.permutation(np.flatnonzero(np.abs(row) > 50))
        i = 0
        for b in rng.choice(np.arange(200, 16000), size=6, replace=False):
            xe = lo + (b * 2.0 ** 17 - 256) / scale                   # where image b << 17 starts
            for v in (xe - eps, xe + eps, xe, _up(xe)):
                row[free[i]] = v
                i += 1
        for _ in range(3):                                            # equal doubles
            row[free[i + 1]] = row[free[i]]
            i += 2
    _check(eng, oracle, xcheck, X)
