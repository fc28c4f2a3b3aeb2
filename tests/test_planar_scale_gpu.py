"""The exact planar depths on the GPU (K11 sd_halfspace2_*, K13 sd_simplicial2_*) against references that share nothing
with plane_sweep.h (tests/test_planar_scale_host.py): the rational sign, closed forms, and invariances.

* the predicate at its scale limits, through the smallest clouds that turn one sign into a count: the witness pair on the
  ladder s = 2^-k down to where every product is zero and up to the host's limit, operands of mixed magnitude, a subnormal
  operand, a grid of subnormals;
* whole clouds scaled by exact powers of two (isotropic, anisotropic), shifted, and with signed zeros: the counts of the
  unscaled cloud by the rational sign;
* star clouds: group borders of the sorted sequence placed on run edges, groups over several runs, the two-runs-per-lane
  scans of the 8192 tier, at and one run below every tier's capacity, against closed forms;
* K11 on one line of 2 048 points.

Every case runs through both kernels (sweep, pairwise) and through the rows, external and block forms."""
import numpy as np
import pytest

from test_halfspace_exact_host import exact_counts, exact_external, integer_cloud, nearly_collinear_cloud
from test_planar_scale_host import (LAYOUTS, SCALES, assert_witness_discriminates, hx_tier, line_halfspace_counts,
                                    scale_clouds, scaled, sign_exact, star, unit_scale_counts, with_origin,
                                    witness_cases)
from test_simplicial_exact_host import simplicial_counts, simplicial_external

pytestmark = pytest.mark.gpu

ALGOS = ("sweep", "pairwise")


@pytest.fixture(scope="module")
def eng():
    from statdepth_amd import engine
    return engine


def _block_of(n, t, extra=()):
    """members of one block holding every row of an n-point cloud, row t last; `extra`: further, shorter blocks."""
    blocks = [[i for i in range(n) if i != t] + [t]] + [list(b) for b in extra]
    mem = np.full((len(blocks), n), -1, dtype=np.int32)
    for i, b in enumerate(blocks):
        mem[i, :len(b)] = b
    return mem


def _three_forms(eng, P, t, algo, blocks=True):
    """(K11 counts, K13 counts) of row t of P from the rows form, the external form (row t taken out of the sample and
    passed as an external point: the same n points, the same others) and the block form."""
    P = np.ascontiguousarray(P)
    rest, g = np.delete(P, t, axis=0), P[t:t + 1].copy()
    h = [eng.halfspace_exact_counts(P, [t], algo=algo)[0], eng.halfspace_exact_external_counts(rest, g, algo=algo)[0]]
    s = [eng.simplicial_exact_counts(P, [t], algo=algo)[0], eng.simplicial_exact_external_counts(rest, g, algo=algo)[0]]
    if blocks:
        mem = _block_of(len(P), t)
        h.append(eng.halfspace_exact_subset_counts(P, mem, algo=algo)[0])
        s.append(eng.simplicial_exact_subset_counts(P, mem, algo=algo)[0])
    return [int(v) for v in h], [int(v) for v in s]


# ---------------------------------------------------------------- the predicate at its scale limits
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("name", list(witness_cases()))
def test_witness_counts(eng, name, algo):
    """One non-collinear pair whose rounded products are equal: K11 counts 1 (2 if the pair is taken for collinear), K13
    counts 0 (1 if it is).  A predicate that leaves the difference to fma(a, b, -p) alone loses it from k = 486 on."""
    pair, w = witness_cases()[name]
    k11, k13 = assert_witness_discriminates(pair, w)                   # (1, 2) and (0, 1) by the rational reference
    h, _ = _three_forms(eng, k11, 0, algo)
    _, s = _three_forms(eng, k13, 0, algo)
    assert h == [1, 1, 1] and s == [0, 0, 0]
    for P in (k11, k13):                                               # every row a target
        assert np.array_equal(eng.halfspace_exact_counts(P, algo=algo), exact_counts(P, sign=sign_exact))
        assert np.array_equal(eng.simplicial_exact_counts(P, algo=algo), simplicial_counts(P, sign=sign_exact))


@pytest.mark.parametrize("algo", ALGOS)
def test_grid_of_subnormals(eng, algo):
    """Every coordinate a multiple of 2^-1074: every product of two differences is zero in fp64, and the counts are those
    of the integer grid."""
    P = integer_cloud(40, 40)
    S = np.ldexp(P, -1074)
    assert np.array_equal(np.ldexp(S, 1074), P) and np.abs(S).max() < 2.0 ** -1022
    h, s = unit_scale_counts("integer40")
    assert np.array_equal(eng.halfspace_exact_counts(S, algo=algo), h)
    assert np.array_equal(eng.simplicial_exact_counts(S, algo=algo), s)
    for t in (0, 17, 39):
        assert _three_forms(eng, S, t, algo) == ([h[t]] * 3, [s[t]] * 3)


# ---------------------------------------------------------------- scaling
def _check_against_unit_scale(eng, name, S, algo):
    h, s = unit_scale_counts(name)
    assert np.array_equal(eng.halfspace_exact_counts(S, algo=algo), h)
    assert np.array_equal(eng.simplicial_exact_counts(S, algo=algo), s)
    for t in (1, len(S) - 1):
        assert _three_forms(eng, S, t, algo) == ([h[t]] * 3, [s[t]] * 3)


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("k", SCALES)
@pytest.mark.parametrize("name", list(scale_clouds()))
def test_power_of_two_scaling(eng, name, k, algo):
    """P 2^-k: the rounded differences scale exactly (no input goes subnormal: asserted), so the counts are those of P,
    taken from the rational sign at unit scale."""
    _check_against_unit_scale(eng, name, scaled(scale_clouds()[name], k), algo)


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("name", list(scale_clouds()))
def test_anisotropic_scaling(eng, name, algo):
    """x 2^400, y 2^-400: both products of a cross keep their value, and the dot of two collinear vectors keeps its sign."""
    _check_against_unit_scale(eng, name, scaled(scale_clouds()[name], -400, 400), algo)


# ---------------------------------------------------------------- shift and signed zero
@pytest.mark.parametrize("algo", ALGOS)
def test_shifted_clouds(eng, algo):
    for name in ("integer40", "integer257"):                           # + 2^52: the differences stay exact integers
        P = scale_clouds()[name]
        S = P + 2.0 ** 52
        assert np.array_equal(S - 2.0 ** 52, P)
        h, s = unit_scale_counts(name)
        assert np.array_equal(eng.halfspace_exact_counts(S, algo=algo), h)
        assert np.array_equal(eng.simplicial_exact_counts(S, algo=algo), s)
    S = nearly_collinear_cloud() + 1e6                                 # rounded data: the reference on the same data
    assert not np.array_equal(S - 1e6, nearly_collinear_cloud())
    assert np.array_equal(eng.halfspace_exact_counts(S, algo=algo), exact_counts(S, sign=sign_exact))
    assert np.array_equal(eng.simplicial_exact_counts(S, algo=algo), simplicial_counts(S, sign=sign_exact))


@pytest.mark.parametrize("algo", ALGOS)
def test_negative_zero(eng, algo):
    P = integer_cloud(40, 40)
    N = np.where(P == 0.0, -0.0, P)
    assert np.signbit(N[P == 0.0]).all() and (P == 0.0).sum() > 8
    h, s = unit_scale_counts("integer40")
    assert np.array_equal(eng.halfspace_exact_counts(N, algo=algo), h)
    assert np.array_equal(eng.simplicial_exact_counts(N, algo=algo), s)
    Q = np.array([[0.0, 0.0], [-0.0, -0.0], [0.0, -0.0], [1.0, -0.0], [1.0, 0.0]])
    for X in (P, N):
        got = eng.halfspace_exact_external_counts(X, Q, algo=algo)
        assert np.array_equal(got, exact_external(P, np.abs(Q), sign=sign_exact))
        got = eng.simplicial_exact_external_counts(X, Q, algo=algo)
        assert np.array_equal(got, simplicial_external(P, np.abs(Q), sign=sign_exact))


# ---------------------------------------------------------------- star clouds: group and run edges of the sweep
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("tier,kind", list(LAYOUTS))
def test_star_clouds(eng, tier, kind, algo):
    """The origin inside a star cloud whose group borders sit where LAYOUTS puts them (asserted from the multiplicities
    by test_planar_scale_host.star), against the closed forms.  K13's others are the star in every form, so every form
    runs at the layout's tier; K11's sample holds the origin too in the rows and block forms, which therefore run where
    that still fits the tier."""
    s = star(tier, kind)
    pts = s.points.copy()                                              # (torch wants a writable array)
    g = np.zeros((1, 2))
    at = s.cnt // 3
    P = with_origin(pts, at)
    rng = np.random.default_rng(tier)
    small = rng.permutation(s.cnt)[:4].tolist()                        # a second, short block: ragged members
    small_P = np.vstack([pts[small], g])
    mem = _block_of(len(P), at, extra=[[i + (i >= at) for i in small] + [at]])
    # K13: others = the star
    assert hx_tier(len(P) - 1) == tier and hx_tier(len(pts)) == tier and hx_tier(mem.shape[1] - 1) == tier
    want = s.simplicial_count()
    assert eng.simplicial_exact_counts(P, [at], algo=algo).tolist() == [want]
    assert eng.simplicial_exact_external_counts(pts, g, algo=algo).tolist() == [want]
    assert eng.simplicial_exact_subset_counts(P, mem, algo=algo).tolist() == \
        [want, simplicial_counts(small_P, [4], sign=sign_exact)[0]]
    # K11: the sample is the star (external) or the star and the origin (rows, block)
    want = s.halfspace_count(1)
    assert hx_tier(len(pts)) == tier
    assert eng.halfspace_exact_external_counts(pts, g, algo=algo).tolist() == [want]
    if len(P) <= tier:
        assert kind == "short" and hx_tier(len(P)) == tier
        assert eng.halfspace_exact_counts(P, [at], algo=algo).tolist() == [want]
        assert eng.halfspace_exact_subset_counts(P, mem, algo=algo).tolist() == \
            [want, exact_counts(small_P, [4], sign=sign_exact)[0]]
        D = with_origin(with_origin(P, 0), len(P))                     # two duplicates of the target
        assert hx_tier(len(D)) == tier
        assert eng.halfspace_exact_counts(D, [0], algo=algo).tolist() == [s.halfspace_count(3)]
        assert eng.simplicial_exact_counts(D, [0], algo=algo).tolist() == [s.simplicial_count(dup=2)]
    else:
        assert kind == "full" and len(pts) == tier


# ---------------------------------------------------------------- K11 on one line
@pytest.mark.parametrize("algo", ALGOS)
def test_halfspace_on_one_line(eng, algo):
    """2 048 points on one line through the origin: one group holds all 2 047 vectors, and the only cuts are before and
    behind it.  The target at position p counts 1 + min(p, 2047 - p); with duplicates of targets on the line, the
    target's multiplicity instead of the 1."""
    t = np.arange(-1024, 1024)
    tg = np.array([0, 1, 2, 63, 64, 65, 511, 1023, 1024, 1025, 1500, 1983, 1984, 2045, 2046, 2047])
    want = np.array([1 + min(int(p), 2047 - int(p)) for p in tg], dtype=np.int64)
    assert np.array_equal(line_halfspace_counts(t, tg), want)
    assert np.array_equal(eng.halfspace_exact_counts(np.outer(t, [1.0, 2.0]), tg, algo=algo), want)
    t = np.concatenate([t, t[[64, 64, 1500]]])                         # 2 051 points: the next tier
    assert np.array_equal(eng.halfspace_exact_counts(np.outer(t, [1.0, 2.0]), tg, algo=algo), line_halfspace_counts(t, tg))
