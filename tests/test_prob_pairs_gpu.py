"""The probabilistic kernels one pair at a time (K8 prob_depth.hip, K9 prob_band.hip) against the 40-digit fixtures of
tests/golden/make_golden_prob_pairs.py, and their tile, chunk and block edges against the fp64 oracles.

K9: p of a single (target, pair, timepoint) to a relative bound where |h| <= 12 (regime A), per branch of pb_prob; the
project's 5e-15 absolute beyond (regime B), with the list of entries that come back exactly 0; the strict product end to
end; 64 / 65 others (tile edges).  K8 normal: one pair term to an absolute bound, finite for every finite input (means and
stds at the top of the fp64 range included); the 2 048-partner chunk edge.  K8 Poisson: the seams of stirlerr, bd0 and
pp_tail at rtol 1e-12; the 256-column block edge.

B_A and B_N are 4 x the worst error measured on an MI355X, the margin covering a device erfc / exp /
sin / asin that moves by an ulp between ROCm releases; their ceilings (3e-12, 1e-12) are what the rest of the suite
already grants and are asserted as well.  Each branch of pb_prob is also held to 4 x its own worst (B_BRANCH), so that a
loss of digits in an accurate branch shows.  Every test prints its worst error beside its bound.
"""
import math

import mpmath as mp
import numpy as np
import pytest

from test_prob_pairs_host import band_fx, normal_fx, poisson_fx, ref_and_error, unhex  # noqa: F401 -- fixtures
from test_probabilistic_band_host import band_sums
from test_probabilistic_host import normal_sums, poisson_sums

pytestmark = pytest.mark.gpu

B_A = 1.31e-12                   # K9 regime A, relative: 4 x 3.261e-13 (near-1 branch, rho = 1 - 1e-12, h = 3, 3.001)
B_A_CEILING = 3e-12              # the strict product of 33 factors is granted 1e-10: 3e-12 per factor
# 4 x the worst of each branch: 2.659e-14, 3.468e-14, 1.844e-14, 3.261e-13, 2.131e-16, 2.508e-16; none above B_A
B_BRANCH = {"gl6": 1.07e-13, "gl12": 1.39e-13, "gl20": 7.4e-14, "near1": B_A, "point_i": 8.6e-16, "point_jk": 1.01e-15}
B_N = 3.7e-16                    # K8 normal pair term, absolute: 4 x 9.015e-17 (h = 0.30, 0.11 at a = 0.64)
B_N_CEILING = 1e-12              # the engine tests' tolerance
U = 2.0 ** -53
# regime B entries that return exactly 0 although p >= 2^-1022 (the near-1 branch's exp(-100) cutoffs)
ZERO_LIST = ["tail_r0.95_h14.2_14.2", "tail_r0.95_h20_20", "cut_r0.95_hh201", "cut_r0.99_hh201"]


@pytest.fixture(scope="module")
def eng():
    from statdepth_amd import engine
    return engine


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---------------------------------------------------------------- K9: single probabilities
def _band_single(eng, e):
    mi, vi, mj, vj, mk, vk = unhex(e["in"])
    mu, var = np.array([[mi, mj, mk]]), np.array([[vi, vj, vk]])
    r, s = eng.prob_band_sums(mu, var, True), eng.prob_band_sums(mu, var, False)
    assert np.array_equal(_bits(r), _bits(s)), (e["name"], r, s)       # T = 1: the sum and the product are the same p
    return float(r[0])


def test_band_regime_a(eng, band_fx):
    """|h| <= 12 and p >= 1e-290: relative error <= B_A on every branch, and <= 4 x the branch's own measured worst."""
    assert B_A <= B_A_CEILING and max(B_BRANCH.values()) <= B_A
    worst = {}
    bad = []
    for e in band_fx["entries"] + band_fx["strict"]["factors"]:
        if e["regime"] != "A":
            continue
        got = _band_single(eng, e)
        _, _, rel = ref_and_error(got, e["p"])
        if not (np.isfinite(got) and rel <= B_BRANCH[e["branch"]]):
            bad.append((e["name"], e["branch"], got, e["p"], rel))
        if rel > worst.get(e["branch"], (-1.0, ""))[0]:
            worst[e["branch"]] = (rel, e["name"])
    for branch in ("gl6", "gl12", "gl20", "near1", "point_i", "point_jk"):
        print(f"K9 regime A {branch}: worst relative error {worst[branch][0]:.3e} at {worst[branch][1]} (bound {B_BRANCH[branch]:.2e})")
    assert not bad, bad


def test_band_regime_b(eng, band_fx):
    """Beyond |h| = 12 or below 1e-290: a probability, within the project's 5e-15 absolute; the entries that come back
    exactly 0 where p is a normal double are the listed ones."""
    worst, zeros, count = 0.0, [], 0
    for e in band_fx["entries"]:
        if e["regime"] != "B":
            continue
        count += 1
        got = _band_single(eng, e)
        w, d, rel = ref_and_error(got, e["p"])
        assert np.isfinite(got) and 0.0 <= got <= 1.0, (e["name"], got)
        worst = max(worst, d)
        assert d <= 5e-15, (e["name"], got, e["p"])
        if got == 0.0 and mp.mpf(e["p"]) >= mp.mpf(2) ** -1022:
            zeros.append(e["name"])
        print(f"K9 regime B {e['name']} ({e['branch']}): p = {e['p'][:12]}..{e['p'][-5:]} got {got:.6e} relative error {rel:.2e}")
    print(f"K9 regime B: {count} entries, worst absolute error {worst:.2e} (bound 5e-15); exactly 0: {zeros}")
    assert zeros == ZERO_LIST


def test_band_strict_end_to_end(eng, band_fx):
    """n = 4, T = 6, every factor in regime A: the strict sums against the products of the fixture's factors (relative
    6 B_A + 8 u: six factors, five products, two additions, the conversion of the reference), the relax sums against their
    sums (B_A + 24 u: 18 positive terms)."""
    st = band_fx["strict"]
    mu, var = np.array([unhex(r) for r in st["mu"]]), np.array([unhex(r) for r in st["var"]])
    with mp.workdps(50):
        prod, tot = {}, {}
        for f in st["factors"]:
            key = f["name"].rsplit("_t", 1)[0]
            prod[key] = prod.get(key, mp.mpf(1)) * mp.mpf(f["p"])
            tot[key] = tot.get(key, mp.mpf(0)) + mp.mpf(f["p"])
        want_s = [mp.nstr(mp.fsum(v for k, v in prod.items() if k.startswith(f"strict_i{i}_")), 40) for i in range(4)]
        want_r = [mp.nstr(mp.fsum(v for k, v in tot.items() if k.startswith(f"strict_i{i}_")), 40) for i in range(4)]
    assert float(want_s[0]) < 1e-150
    for relax, want, bound in ((False, want_s, 6 * B_A + 8 * U), (True, want_r, B_A + 24 * U)):
        got = eng.prob_band_sums(mu, var, relax)
        rels = [ref_and_error(g, w)[2] for g, w in zip(got, want)]
        print(f"K9 {'relax' if relax else 'strict'} 6 x 4: sums {got}, worst relative error {max(rels):.3e} (bound {bound:.2e})")
        assert np.isfinite(got).all() and max(rels) <= bound, (got, want, rels)


# ---------------------------------------------------------------- K9: tile edges
def _noisy(T, n, seed, zero_frac=0.1):
    rng = np.random.default_rng(seed)
    mu = rng.normal(0, 1, (T, n))
    sd = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), (T, n)))
    sd[rng.random((T, n)) < zero_frac] = 0.0
    return mu, sd * sd


def _worst_rel(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and np.isfinite(got).all() and (want > 0).all()
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300)))


@pytest.mark.parametrize("T", [4, 5])
@pytest.mark.parametrize("n", [65, 66, 129, 130])
def test_band_tile_edges(eng, n, T):
    """64 and 65 others (one full tile; a second tile of one position and a diagonal tile without a pair), 128 and 129;
    T at and past the 4-timepoint chunk.  Against band_sums at the existing tolerances."""
    mu, var = _noisy(T, n, seed=1000 * n + T)
    tg = np.array([0, 63, 64, n - 1])
    for relax, tol in ((True, 1e-13), (False, 1e-10)):
        r = _worst_rel(eng.prob_band_sums(mu, var, relax, tg), band_sums(mu, var, relax, tg))
        print(f"K9 n={n} T={T} {'relax' if relax else 'strict'}: worst relative error {r:.2e} (bound {tol:.0e})")
        assert r <= tol


@pytest.mark.parametrize("bs", [64, 65])
def test_band_members_block_edge(eng, bs):
    """`members` blocks of exactly 64 and 65 positions, full (no -1), one of them listing its target."""
    mu, var = _noisy(5, 150, seed=70 + bs)
    rng = np.random.default_rng(71 + bs)
    tg = np.array([3, 149, 64, 0])
    mem = np.stack([rng.choice(150, bs, replace=False) for _ in tg]).astype(np.int32)
    if tg[1] not in mem[1]:
        mem[1, bs - 1] = tg[1]                           # the target in the last position of its block
    for relax, tol in ((True, 1e-13), (False, 1e-10)):
        r = _worst_rel(eng.prob_band_sums(mu, var, relax, tg, mem), band_sums(mu, var, relax, tg, mem))
        print(f"K9 members bs={bs} {'relax' if relax else 'strict'}: worst relative error {r:.2e} (bound {tol:.0e})")
        assert r <= tol


# ---------------------------------------------------------------- K8 normal
def test_normal_pair_terms(eng, normal_fx):
    """n = 3: out[0] is one pair term Phi(h_1) - Phi2(0, h_2; rho_2).  Absolute error <= B_N, every output finite."""
    assert B_N <= B_N_CEILING
    worst, where, bad = 0.0, "", []
    for e in normal_fx["entries"]:
        got = eng.prob_normal_sums(np.array(unhex(e["mu"])), np.array(unhex(e["sigma"])))
        _, d, _ = ref_and_error(got[0], e["value"]) if np.isfinite(got[0]) else (0.0, float("inf"), 0.0)
        if not (np.isfinite(got).all() and d <= B_N):
            bad.append((e["name"], got, e["value"], d))
        if d > worst:
            worst, where = d, e["name"]
        if e["name"].startswith(("overflow", "below", "top", "sub", "small")):
            print(f"K8 normal {e['name']}: got {got[0]!r} want {e['value'][:20]} error {d:.2e}")
    print(f"K8 normal pair terms: worst absolute error {worst:.3e} at {where} (bound {B_N:.1e})")
    assert not bad, bad


def test_normal_scaling_keeps_the_bits(eng):
    """h and a are ratios: means and stds scaled by a power of two into the ranges where the kernel rescales them (the
    largest beyond 2^1020; every std below 2^-969, still a normal double) give the bits of the unscaled call, and the
    public API accepts them."""
    from statdepth_amd import probabilistic_normal_depth
    rng = np.random.default_rng(81)
    mu, sg = rng.normal(0, 1.5, 9), np.exp(rng.uniform(-2, 2, 9))
    base = eng.prob_normal_sums(mu, sg)
    top = 2.0 ** (1023 - math.frexp(max(np.max(np.abs(mu)), np.max(sg)))[1])   # the largest input in [2^1022, 2^1023)
    for scale in (top, top / 4, top / 16, 2.0 ** -900, 2.0 ** -960, 2.0 ** -1000):
        got = eng.prob_normal_sums(mu * scale, sg * scale)
        assert np.array_equal(_bits(got), _bits(base)), (scale, got, base)
    d = probabilistic_normal_depth(mu * top, sg * top)["depths"].to_numpy(dtype=float)
    assert np.array_equal(_bits(d), _bits(base / np.float64(math.comb(9, 2))))


@pytest.mark.parametrize("n", [2048, 2049, 4097])
def test_normal_chunk_edges(eng, n):
    """One chunk exactly, a second (third) chunk holding one partner, that partner as the target; targets in reverse."""
    rng = np.random.default_rng(n)
    mu = rng.normal(0, 5, n)
    sg = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), n))
    tg = np.array([t for t in (0, 2047, 2048, n - 1) if t < n])
    c = math.comb(n, 2)
    want = normal_sums(mu, sg, tg) / c
    for order in (tg, tg[::-1].copy()):
        got = eng.prob_normal_sums(mu, sg, order) / c
        w = want if order is tg else want[::-1]
        err = float(np.max(np.abs(got - w)))
        print(f"K8 normal n={n} targets {list(order)}: worst |error| / C(n, 2) = {err:.2e} (bound 1e-12)")
        assert np.isfinite(got).all() and err <= 1e-12


# ---------------------------------------------------------------- K8 Poisson
def test_poisson_seams(eng, poisson_fx):
    """T = 1, n = 3: rtol 1e-12 where the value is at least 1e-290, exactly 0 where it is 0, finite and <= 1e-289 for
    the (at most 5) values in between."""
    worst, small, bad = {}, 0, []
    for e in poisson_fx["entries"]:
        got = eng.prob_poisson_sums(np.array([unhex(e["lam"])]), e["lim"])
        for f in range(3):
            w, d, rel = ref_and_error(got[f], e["values"][f]) if np.isfinite(got[f]) else (0.0, 0.0, float("inf"))
            if mp.mpf(e["values"][f]) == 0:
                if got[f] != 0.0:
                    bad.append((e["name"], f, got[f], "want exactly 0"))
            elif mp.mpf(e["values"][f]) >= mp.mpf("1e-290"):
                if rel > worst.get(e["seam"], (-1.0, ""))[0]:
                    worst[e["seam"]] = (rel, f"{e['name']}[{f}]")
                if not rel <= 1e-12:
                    bad.append((e["name"], f, got[f], e["values"][f], rel))
            else:
                small += 1
                if not (np.isfinite(got[f]) and 0.0 <= got[f] <= 1e-289):
                    bad.append((e["name"], f, got[f], e["values"][f]))
    for seam in sorted(worst):
        print(f"K8 Poisson {seam}: worst relative error {worst[seam][0]:.3e} at {worst[seam][1]} (bound 1e-12)")
    assert small <= 5, small
    assert not bad, bad


@pytest.mark.parametrize("n", [256, 257, 513])
def test_poisson_block_edges(eng, n):
    """One column block exactly, a second (third) block of one column; lim - 1 = 17 is one z past the 16-z chunk."""
    rng = np.random.default_rng(n)
    lam = np.exp(rng.uniform(np.log(0.05), np.log(40.0), size=(2, n)))
    lam[1, n - 1] = 0.0
    tg = np.array([t for t in (0, 255, 256, n - 1) if t < n])
    got, want = eng.prob_poisson_sums(lam, 18, tg), poisson_sums(lam, 18, tg)
    r = _worst_rel(got, want)
    print(f"K8 Poisson n={n}: worst relative error {r:.2e} (bound 1e-12)")
    assert r <= 1e-12
    assert np.array_equal(got, eng.prob_poisson_sums(lam, 18)[tg])
