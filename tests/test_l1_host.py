"""L1 (spatial) depth (K5, sd_l1_*) without a GPU: a 50-digit restatement of the definition, the error bound of its fp64
evaluation, a numpy emulation of the kernel's arithmetic, the C oracle against the restatement and against closed forms,
and the C ABI's refusals.

`l1_reference`, `l1_errors`, `l1_tolerance`, `l1_emulated`, the clouds (`normal_cloud`, `base_cloud`, `scaled`,
`mixed_cloud`, `unit_pairs`, `line_points`, `cross_polytope`) and `reference_case` are imported by tests/test_l1_gpu.py.
"""
import ctypes
import functools

import mpmath
import numpy as np
import pytest

U = 2.0 ** -53                                   # unit roundoff of fp64
_MP = mpmath.mp.clone()                          # a context of its own: the global precision stays as it is
_MP.dps = 50


# ---------------------------------------------------------------- the definition at 50 digits
def _mp_depth(x, others, N):
    """1 - || sum_y (y - x)/||y - x|| || / N over the rows `others`; NaN for a coincident or non-finite row."""
    if not (np.isfinite(x).all() and np.isfinite(others).all()):
        return _MP.nan                           # inf/inf, or NaN itself
    xs = [_MP.mpf(float(v)) for v in x]          # exact: every double is an mpf
    e = [_MP.mpf(0)] * len(xs)
    for y in others:
        df = [_MP.mpf(float(v)) - xc for v, xc in zip(y, xs)]
        s = _MP.fsum(df, squared=True)
        if s == 0:
            return _MP.nan                       # 0/0
        r = 1 / _MP.sqrt(s)
        e = [ec + dc * r for ec, dc in zip(e, df)]
    return 1 - _MP.sqrt(_MP.fsum(e, squared=True)) / N


def l1_reference(P, targets=None, Q=None, blocks=None):
    """depth = 1 - || sum_{y != x} (y - x)/||y - x|| || / N at 50 digits, on the exact doubles of P (and Q), in the three
    forms of DESIGN.md, "Point clouds: the three forms":
      rows      l1_reference(P, targets)       x = P[t] inside P (targets=None: every row); N = n
      external  l1_reference(P, Q=Q)           x = Q[q] inside P u {Q[q]}; N = n + 1
      blocks    l1_reference(P, blocks=B)      B[q]: row indices, others first, target last (entries from the first -1
                                               on are padding); N = members; a block without members gives NaN
    A coincident other (0/0) and a non-finite coordinate (inf/inf) give NaN.  Returns an object array of mpf."""
    P = np.asarray(P, dtype=np.float64)
    n = len(P)
    out = []
    if Q is not None:
        for q in np.asarray(Q, dtype=np.float64):
            out.append(_mp_depth(q, P, n + 1))
    elif blocks is not None:
        for b in blocks:
            b = [int(i) for i in b]
            if -1 in b:
                b = b[:b.index(-1)]
            out.append(_mp_depth(P[b[-1]], P[b[:-1]], len(b)) if b else _MP.nan)
    else:
        for t in (range(n) if targets is None else targets):
            out.append(_mp_depth(P[t], np.delete(P, t, axis=0), n))
    res = np.empty(len(out), dtype=object)
    res[:] = out
    return res


def l1_errors(got, ref):
    """|got_i - ref_i| as doubles, the difference formed at 50 digits; NaN where both are NaN (anything else about NaN
    is an assertion error)."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape
    out = np.empty(len(ref))
    for i, (g, r) in enumerate(zip(got, ref)):
        assert np.isnan(g) == bool(_MP.isnan(r)), (i, g, r)
        out[i] = np.nan if np.isnan(g) else float(abs(_MP.mpf(float(g)) - r))
    return out


def l1_tolerance(n, d):
    """Worst-case forward error of the fp64 evaluation of the depth of one point inside a sample of n points in R^d, for
    the oracle's arithmetic and the kernel's alike: sqrt(d) * (n + d/2 + 10) * u, u = 2^-53.

    Each component of a unit vector (y - x)/||y - x|| carries at most (d/2 + 7) u: the squared distance s, d products and
    d - 1 sums of positive terms on differences good to u each, has relative error <= (d + 2) u, its inverse root half of
    that, (d/2 + 1) u; r = 1/sqrt(s) itself adds 3 u (an unfused Newton step at convergence; an IEEE sqrt and division
    add less); the product (y - x) * r adds u, the difference y - x adds u, and one more u covers the second-order
    terms.  The n - 1 components, of magnitude <= 1, are summed in index order: every partial sum is below n and is
    rounded once, n u per component after the division by n.  A component of e/n is therefore within
    (d/2 + 7 + n) u, and sqrt(d) takes the bound from a component to the norm; the last three u are the norm's own
    squares, root and division and the final subtraction."""
    return np.sqrt(d) * (n + d / 2 + 10) * U


# ---------------------------------------------------------------- the kernel's arithmetic in numpy
GUARD_LO, GUARD_HI = 1e-280, 1e280               # l1_depth.hip: squared distances outside take the IEEE path


def _seed24(s):
    """1/sqrt(s) rounded to 24 significant bits: the ASSUMED accuracy of v_rsq_f64 (relative error <= 2^-24); nobody has
    measured the instruction's on the device."""
    m, ex = np.frexp(1.0 / np.sqrt(s))
    return np.ldexp(np.round(m * 2.0 ** 24) / 2.0 ** 24, ex)


def _emulated_one(x, Y, N, newton_steps):
    with np.errstate(all="ignore"):
        s = np.zeros(len(Y))
        for c in range(len(x)):
            df = x[c] - Y[:, c]
            s = s + df * df
        fast = (s > GUARD_LO) & (s < GUARD_HI)
        r = _seed24(np.where(fast, s, 1.0))
        for _ in range(newton_steps):
            r = r * (1.5 - (0.5 * s) * (r * r))
        r = np.where(fast, r, 1.0 / np.sqrt(s))
        terms = (Y - x) * r[:, None]
        e = np.cumsum(terms, axis=0)[-1] if len(Y) else np.zeros(len(x))       # cumsum adds in index order
        q = 0.0
        for c in range(len(x)):
            q = q + e[c] * e[c]
        return 1.0 - np.sqrt(q) / N


def l1_emulated(P, targets=None, newton_steps=2, blocks=None):
    """l1_depth_kernel's operations one by one in fp64 numpy (no fused multiply-add, as the library is built): the seed
    of `_seed24`, `newton_steps` steps r <- r (1.5 - (0.5 s)(r r)), the IEEE path outside the guard, sums in index order.
    Rows form, or the blocks form (lists of rows, others first, target last)."""
    P = np.asarray(P, dtype=np.float64)
    if blocks is not None:
        return np.array([_emulated_one(P[b[-1]], P[list(b[:-1])].reshape(-1, P.shape[1]), len(b), newton_steps)
                         for b in blocks])
    tg = range(len(P)) if targets is None else targets
    return np.array([_emulated_one(P[t], np.delete(P, t, axis=0), len(P), newton_steps) for t in tg])


# ---------------------------------------------------------------- the clouds both files use
D_ALL = (1, 2, 3, 4, 5, 6, 7, 8, 9, 33, 64)      # every compiled instantiation, and the generic form's middle and limit
N_ALL = 257                                      # two workgroups of targets, the second with one live lane
SHIFT = 480                                      # 2^-960 ~ 1e-289 and 2^960 ~ 1e289: outside the guard, normal, finite


def normal_cloud(n, d, seed):
    return np.random.default_rng(seed).standard_normal((n, d))


def base_cloud():
    return normal_cloud(300, 3, 5300)


def scaled(P, k):
    """P * 2^k, exactly."""
    return np.ldexp(P, k)


def mixed_cloud():
    """Rows 0-99 of the base cloud times 2^-480, rows 100-199 as they are, rows 200-299 times 2^480."""
    P = base_cloud()
    P[:100] = scaled(P[:100], -SHIFT)
    P[200:] = scaled(P[200:], SHIFT)
    return P


def pick_targets(n, seed, always=()):
    """16 rows: `always`, the first and the last row, the rest drawn."""
    rng = np.random.default_rng(seed)
    tg = list(dict.fromkeys([*always, 0, n - 1]))
    for t in rng.permutation(n):
        if len(tg) == 16:
            break
        if int(t) not in tg:
            tg.append(int(t))
    return np.array(sorted(tg))


@functools.lru_cache(maxsize=None)
def _reference_case(name, d):
    if name == "normal":
        P = normal_cloud(N_ALL, d, 5000 + d)
        tg = pick_targets(N_ALL, d, always=(255, 256))
    elif name == "base":
        P, tg = base_cloud(), pick_targets(300, 77)
    else:
        assert name == "mixed"
        P, tg = mixed_cloud(), pick_targets(300, 78, always=(50, 99, 100, 150, 199, 200, 250))
    return P, tg, l1_reference(P, tg)


def reference_case(name, d=3):
    """(P, targets, reference at the targets) of the cases both files compare: 'normal' (n = 257 in R^d), 'base' (the
    300 x 3 cloud, whose depths are also those of its power-of-two multiples) and 'mixed'.  The reference is computed
    once; P and the targets are the caller's own copies."""
    P, tg, ref = _reference_case(name, d)
    return P.copy(), tg.copy(), ref


def unit_pairs(d, pairs=4096, seed=0):
    """2 * pairs points: rows 2i and 2i + 1 are N(0,1)^d times 10^U(-145, 145), one factor per pair."""
    rng = np.random.default_rng(5400 + 100 * seed + d)
    X = rng.standard_normal((pairs, 2, d)) * 10.0 ** rng.uniform(-145, 145, size=(pairs, 1, 1))
    return X.reshape(2 * pairs, d)


def pair_limit(oracle, P):
    """(limit, the oracle's own maximum) of |depth - 0.5| for the two-point samples [2i, 2i + 1] of P: the oracle's
    maximum plus 4 u.  r within 3 u enters the depth halved, and the kernel's (y - x) * r and norm round at most 2.5 u
    more than the oracle's (y - x)/||y - x||."""
    worst = max(abs(oracle.l1_depth(P[i:i + 2], [1])[0] - 0.5) for i in range(0, len(P), 2))
    return worst + 4 * U, worst


def line_points(n, seed):
    """n sorted distinct points on a line."""
    x = np.sort(np.random.default_rng(seed).standard_normal(n))
    assert (np.diff(x) > 0).all()
    return x[:, None]


def line_depths(n):
    """d = 1, sorted distinct points: n - 1 - i unit vectors +1 and i unit vectors -1."""
    i = np.arange(n)
    return 1.0 - np.abs((n - 1 - i) - i) / n


def cross_polytope(d, a=0.7):
    """(P, row of the centre): 0 and +- a e_c; the vertices come in opposite pairs, the centre's sum is 0 exactly."""
    V = np.zeros((2 * d, d))
    V[np.arange(d), np.arange(d)] = a
    V[d + np.arange(d), np.arange(d)] = -a
    return np.vstack([V[:d], np.zeros((1, d)), V[d:]]), d


# ---------------------------------------------------------------- the oracle against the reference
@pytest.mark.parametrize("d", D_ALL)
def test_oracle_vs_reference_every_d(oracle, d):
    P, tg, ref = reference_case("normal", d)
    err = l1_errors(oracle.l1_depth(P, tg), ref)
    print(f"d={d}: oracle max |error| = {err.max() / U:.2f} u, bound {l1_tolerance(N_ALL, d) / U:.0f} u")
    assert err.max() <= l1_tolerance(N_ALL, d)


@pytest.mark.parametrize("shift", [-SHIFT, SHIFT])
def test_oracle_vs_reference_scaled(oracle, shift):
    """Scaling by a power of two changes no depth: the reference is that of the unscaled cloud, and the oracle's bits are
    those it gives the unscaled cloud."""
    P, tg, ref = reference_case("base")
    got = oracle.l1_depth(scaled(P, shift), tg)
    assert np.array_equal(got, oracle.l1_depth(P, tg))
    assert l1_errors(got, ref).max() <= l1_tolerance(300, 3)


def test_oracle_vs_reference_mixed_scales(oracle):
    P, tg, ref = reference_case("mixed")
    err = l1_errors(oracle.l1_depth(P, tg), ref)
    print(f"mixed: oracle max |error| = {err.max() / U:.2f} u")
    assert err.max() <= l1_tolerance(300, 3)


def test_reference_three_forms_agree():
    """The external and the blocks form of the reference are the rows form of the constructed cloud; N counts the target."""
    P = normal_cloud(12, 2, 5100)
    rows = l1_reference(P)
    ext = l1_reference(P[:-1], Q=P[-1:])
    assert ext[0] == rows[-1]
    blk = l1_reference(P, blocks=[list(range(12)), [3, 5, 1, -1, -1], [4], [], [-1, -1], [2, 7, 2]])
    assert blk[0] == rows[-1]
    assert blk[1] == l1_reference(P[[3, 5, 1]], [2])[0]
    assert blk[2] == 1                                               # no others: ||0|| / 1
    assert all(_MP.isnan(b) for b in blk[3:])                        # two empty blocks, one coincident other
    assert _MP.isnan(l1_reference(P, Q=P[4:5])[0])
    # the divisor is the sample size, not the number of others: 4 collinear points, an end point sees three units
    line = np.array([[0.0], [1.0], [3.0], [4.0]])
    assert [float(v) for v in l1_reference(line)] == [0.25, 0.75, 0.75, 0.25]


# ---------------------------------------------------------------- closed forms
def test_closed_forms(oracle):
    x = line_points(513, 5200)
    assert np.array_equal(oracle.l1_depth(x), line_depths(513))       # +-1 exactly, integer sums
    assert l1_errors(line_depths(513)[::37], l1_reference(x, range(0, 513, 37))).max() <= U
    for d in (2, 5, 9, 64):
        P, c = cross_polytope(d)
        assert oracle.l1_depth(P, [c])[0] == 1.0
        assert l1_reference(P, [c])[0] == 1
    for d in (1, 3):
        P = normal_cloud(2, d, 5210 + d)
        half = np.array([0.5, 0.5])                                   # two points: one unit vector, 1 - 1/2
        assert l1_errors(half, l1_reference(P)).max() <= 1e-49
        assert np.abs(oracle.l1_depth(P) - half).max() <= (0.0 if d == 1 else l1_tolerance(2, d))


# ---------------------------------------------------------------- the emulation, and what test (g) can tell apart
def test_emulation_is_the_oracle_to_rounding(oracle):
    for d in (1, 3, 9):
        P, tg, ref = reference_case("normal", d)
        assert l1_errors(l1_emulated(P, tg), ref).max() <= l1_tolerance(N_ALL, d)
    P, tg, ref = reference_case("mixed")
    assert l1_errors(l1_emulated(P, tg), ref).max() <= l1_tolerance(300, 3)
    P = base_cloud()
    P[7] = P[3]
    got = l1_emulated(P, [3, 7, 8])
    assert np.isnan(got[:2]).all() and np.isfinite(got[2])


@pytest.mark.parametrize("d", [1, 3, 8, 64])
def test_unit_pair_limit_discriminates(oracle, d):
    """The limit of test_l1_gpu.py's unit-vector test on the emulated kernel: two Newton steps pass, one fails -- given a
    seed good to 2^-24 (`_seed24`), which is an assumption about v_rsq_f64, not a measurement."""
    P = unit_pairs(d, pairs=1024)
    blocks = [[i, i + 1] for i in range(0, len(P), 2)]
    limit, worst = pair_limit(oracle, P)
    two = np.abs(l1_emulated(P, newton_steps=2, blocks=blocks) - 0.5).max()
    one = np.abs(l1_emulated(P, newton_steps=1, blocks=blocks) - 0.5).max()
    print(f"d={d}: oracle {worst / U:.1f} u, limit {limit / U:.1f} u, two steps {two / U:.1f} u, one step {one / U:.1f} u")
    assert two <= limit
    assert one > limit


# ---------------------------------------------------------------- C ABI, no device needed
def test_abi_refusals_before_device_work():
    from statdepth_amd import _native
    lib = _native.load()
    fake = ctypes.c_void_p(256)                  # never dereferenced: every refusal happens before device work
    out = ctypes.c_void_p(512)
    INV, UNS = _native.SD_ERR_INVALID, _native.SD_ERR_UNSUPPORTED

    def rows(P, n, d, o, sel=fake, m=3):
        return lib.sd_l1_depth(P, n, d, sel, m, o, None)

    def external(P, n, d, o, sel=fake, m=3):
        return lib.sd_l1_external_depth(P, n, d, sel, m, o, None)

    def blocks(P, n, d, o, sel=fake, m=3, bs=4):
        return lib.sd_l1_subset_depth(P, n, d, sel, m, bs, o, None)

    for fn in (rows, external, blocks):
        assert fn(fake, 10, 65, out) == UNS
        assert b"d <= 64" in lib.sd_last_error()
        assert fn(None, 10, 3, out) == INV
        assert fn(fake, 10, 3, None) == INV
        assert fn(fake, 0, 3, out) == INV
        assert fn(fake, 10, 0, out) == INV
        assert fn(fake, 10, -1, out) == INV
    assert rows(fake, 10, 3, out, sel=None, m=9) == INV               # NULL targets, m != n
    assert external(fake, 10, 3, out, sel=None) == INV
    assert external(fake, 10, 3, out, m=-1) == INV
    assert blocks(fake, 10, 3, out, sel=None) == INV
    assert blocks(fake, 10, 3, out, bs=0) == INV
    assert blocks(fake, 10, 3, out, m=-1) == INV
