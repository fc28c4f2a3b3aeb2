"""L1 (spatial) depth on the GPU (K5, l1_depth_kernel<D>): every compiled instantiation, squared distances on both sides
of the fast path's guard (and subnormal, and infinite), the accuracy of the fast path on single unit vectors, closed
forms, coincident and non-finite points, independence of a target's value from the rest of the call, and the external and
blocks forms with several workgroups of targets.  The kernel is compared with the 50-digit restatement of
tests/test_l1_host.py at 16 targets per case and with the C oracle at every target, both within `l1_tolerance`, the
worst-case bound of the fp64 evaluation (6e-14 ... 4e-13 here)."""
import numpy as np
import pytest

from test_l1_host import (D_ALL, GUARD_HI, GUARD_LO, N_ALL, SHIFT, U, cross_polytope, l1_errors, l1_reference,
                          l1_tolerance, line_depths, line_points, normal_cloud, pair_limit, pick_targets, reference_case,
                          scaled, unit_pairs)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from statdepth_amd import engine
    return engine


def _against_oracle(got, want, tol):
    """Every target: NaN where the oracle has NaN, otherwise within tol (a number, or one per target).  Returns the
    largest difference."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    diff = np.abs(got[ok] - want[ok])
    assert np.all(diff <= np.broadcast_to(tol, want.shape)[ok]), float(diff.max() / U)
    return float(diff.max()) if diff.size else 0.0


def _against_reference(label, got, ref, tol):
    err = l1_errors(got, ref)
    worst = np.nanmax(err)
    print(f"{label}: max |kernel - reference| = {worst / U:.2f} u (bound {np.max(tol) / U:.0f} u)")
    assert np.all(err[~np.isnan(err)] <= np.broadcast_to(tol, err.shape)[~np.isnan(err)]), worst / U
    return worst


# ---------------------------------------------------------------- (a) every instantiation
@pytest.mark.parametrize("d", D_ALL)
def test_every_instantiation(eng, oracle, d):
    """d = 1 ... 8 are the compiled l1_depth_kernel<D>, 9, 33 and 64 the generic form; n = 257: two workgroups."""
    P, tg, ref = reference_case("normal", d)
    got = eng.l1_depth(P)
    tol = l1_tolerance(N_ALL, d)
    _against_oracle(got, oracle.l1_depth(P), tol)
    _against_reference(f"normal d={d}", got[tg], ref, tol)


# ---------------------------------------------------------------- (b) - (e) scale
@pytest.mark.parametrize("shift", [-SHIFT, SHIFT])
def test_every_pair_on_the_ieee_path(eng, oracle, shift):
    """The 300 x 3 cloud times 2^-480 (s ~ 1e-289: below the guard, normal) and times 2^480 (above it): the depths are
    those of the unscaled cloud."""
    P0, tg, ref = reference_case("base")
    P = scaled(P0, shift)
    df = P[tg][:, None, :] - P[None, :, :]
    s = (df * df).sum(axis=2)
    s = s[s > 0]
    assert ((s < GUARD_LO) & (s > 1e-300)).all() if shift < 0 else ((s > GUARD_HI) & np.isfinite(s)).all()
    got = eng.l1_depth(P)
    tol = l1_tolerance(300, 3)
    _against_oracle(got, oracle.l1_depth(P), tol)
    _against_reference(f"scaled 2^{shift}", got[tg], ref, tol)


def test_mixed_scales_in_one_cloud(eng, oracle):
    """Rows times 2^-480, 1 and 2^480, a hundred each: the lanes of one wave take different branches for the same
    streamed point."""
    P, tg, ref = reference_case("mixed")
    got = eng.l1_depth(P)
    tol = l1_tolerance(300, 3)
    _against_oracle(got, oracle.l1_depth(P), tol)
    _against_reference("mixed", got[tg], ref, tol)
    assert np.array_equal(eng.l1_depth(P, tg), got[tg])


def test_subnormal_squared_distances(eng, oracle):
    """The cloud times 2^-525: every s is a subnormal (about 24 significant bits, so the fp64 formula itself is 2e-9 off
    the true depth and the oracle, which forms the same bits of s, is the reference).  A flushed subnormal would be
    s = 0 and a NaN."""
    P = scaled(reference_case("base")[0], -525)
    df = P[:16, None, :] - P[None, :, :]
    s = (df * df).sum(axis=2)
    assert ((s[s > 0] < np.finfo(np.float64).tiny) & (s[s > 0] > 1e-320)).all()
    got = eng.l1_depth(P)
    assert not np.isnan(got).any()
    _against_oracle(got, oracle.l1_depth(P), l1_tolerance(300, 3))


def test_overflowing_squared_distances(eng, oracle):
    """The cloud times 2^600: every s is +inf, every unit vector 0, every depth 1.0."""
    P = scaled(reference_case("base")[0], 600)
    assert np.isfinite(P).all()
    got = eng.l1_depth(P)
    assert (got == 1.0).all()
    assert (oracle.l1_depth(P) == 1.0).all()


# ---------------------------------------------------------------- (f) the guard's two edges
@pytest.mark.parametrize("c,edge", [(0.5e-140, GUARD_LO), (1e140, GUARD_HI)])
def test_guard_edges_on_a_line(eng, c, edge):
    """d = 1, points k c, k = -20 ... 20: squared distances (j c)^2 on both sides of the guard's edge, the depth the
    closed form of sorted points on a line."""
    x = (np.arange(-20, 21) * c)[:, None]
    df = x - x.T
    s = (df * df)[df != 0]
    inside = (s > GUARD_LO) & (s < GUARD_HI)
    assert inside.any() and (~inside).any()
    assert (np.abs(np.log10(s / edge)) < 4).all()
    got = eng.l1_depth(x)
    assert np.abs(got - line_depths(41)).max() <= l1_tolerance(41, 1)


# ---------------------------------------------------------------- (g) unit vectors have unit length
@pytest.mark.parametrize("d", [1, 3, 8, 64])
def test_unit_vectors_have_unit_length(eng, oracle, d):
    """4096 blocks of two points, pair i drawn as N(0,1)^d times 10^U(-145, 145): the sample is two points, the sum one
    unit vector, the depth 1 - ||(y - x) r|| / 2 = 0.5 in exact arithmetic, so |depth - 0.5| is half the error of one
    unit vector's length: the fast path (v_rsq_f64 + two unfused Newton steps) with nothing summed over it.

    Limit: the oracle's own max |depth - 0.5| on the same pairs + 4 * 2^-53 (`pair_limit`).  In the numpy emulation of
    the kernel (test_l1_host.py::test_unit_pair_limit_discriminates) two Newton steps stay at or below 2 u and one step
    reaches 22 - 23 u, IF v_rsq_f64 is good to 2^-24: that accuracy is an assumption, not measured on an MI355X.

    Measured on an MI355X, max |depth - 0.5| in u = 2^-53, kernel / oracle: d = 1: 1 / 0, d = 3: 2 / 1, d = 8: 2 / 2,
    d = 64: 3 / 3 -- the emulation's figures with two steps, so the seed is at least good enough for two steps to
    converge.  The same run's max |kernel - reference| on the clouds of the tests above: 6.0 u over the eleven d of
    test_every_instantiation (at d = 2), 3.1 u at either scale of test_every_pair_on_the_ieee_path, 29.1 u in
    test_mixed_scales_in_one_cloud (the oracle's own error on that cloud is the same 29.1 u)."""
    P = unit_pairs(d)
    members = np.arange(len(P), dtype=np.int32).reshape(-1, 2)
    got = eng.l1_subset_depth(P, members)
    limit, worst = pair_limit(oracle, P)
    mine = np.abs(got - 0.5).max()
    print(f"unit pairs d={d}: kernel max |depth - 0.5| = {mine / U:.2f} u, oracle {worst / U:.2f} u, limit {limit / U:.2f} u")
    assert np.isfinite(got).all()
    assert mine <= limit


# ---------------------------------------------------------------- (h) closed forms
def test_line_closed_form(eng):
    x = line_points(513, 5200)
    assert np.abs(eng.l1_depth(x) - line_depths(513)).max() <= l1_tolerance(513, 1)


@pytest.mark.parametrize("d", [2, 5, 9, 64])
def test_cross_polytope_centre(eng, d):
    """The vertices +- a e_c give (+- a) * r with the same r: the centre's sum is 0 whatever r is."""
    P, c = cross_polytope(d)
    assert eng.l1_depth(P, [c])[0] == 1.0
    assert eng.l1_depth(P)[c] == 1.0


# ---------------------------------------------------------------- (i) coincident and non-finite points
def test_coincident_rows(eng, oracle):
    P = reference_case("base")[0]
    P[7] = P[9] = P[3]
    got = eng.l1_depth(P)
    assert np.array_equal(np.flatnonzero(np.isnan(got)), [3, 7, 9])
    tol = l1_tolerance(300, 3)
    _against_oracle(got, oracle.l1_depth(P), tol)
    tg = pick_targets(300, 79, always=(2, 4, 8, 10))
    tg = tg[~np.isin(tg, (3, 7, 9))]
    _against_reference("coincident rows", got[tg], l1_reference(P, tg), tol)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_one_non_finite_coordinate(eng, oracle, bad):
    """NaN spreads; an infinite coordinate makes s = inf and the unit vector inf * 0 (the reference's inf/inf)."""
    P = reference_case("base")[0]
    P[130, 1] = bad
    assert np.isnan(eng.l1_depth(P)).all()
    assert np.isnan(oracle.l1_depth(P)).all()


# ---------------------------------------------------------------- (j) independence from the call
def test_value_does_not_depend_on_the_call(eng):
    """What distributed.sharded_pointcloud relies on: a target's bits are those of the all-rows call wherever it stands
    in the list of targets."""
    P = normal_cloud(600, 3, 5500)
    full = eng.l1_depth(P)
    rng = np.random.default_rng(5501)
    for tg in (rng.permutation(600), rng.integers(0, 600, size=700), np.arange(300, 600), [599], [0, 0, 599, 0]):
        assert np.array_equal(eng.l1_depth(P, tg), full[np.asarray(tg)])


# ---------------------------------------------------------------- (k) many targets in the other two forms
@pytest.mark.parametrize("d", [3, 9])
def test_external_many_targets(eng, oracle, d):
    P = normal_cloud(300, d, 5600 + d)
    Q = normal_cloud(600, d, 5610 + d)
    same = np.arange(0, 600, 43)
    Q[same] = P[same // 2]                                           # a sample point itself: 0/0
    far = np.arange(5, 600, 61)
    Q[far] += 1e6
    got = eng.l1_external_depth(P, Q)
    assert np.array_equal(np.flatnonzero(np.isnan(got)), same)
    tol = l1_tolerance(301, d)
    want = np.array([oracle.l1_depth(np.vstack([P, q]), [300])[0] for q in Q])
    _against_oracle(got, want, tol)
    some = np.array(sorted({0, 43, 5, 66, 255, 256, 599, *range(100, 109)}))
    _against_reference(f"external d={d}", got[some], l1_reference(P, Q=Q[some]), tol)


@pytest.mark.parametrize("d", [3, 9])
def test_blocks_many_targets(eng, oracle, d):
    P = normal_cloud(300, d, 5600 + d)
    rng = np.random.default_rng(5620 + d)
    sizes = rng.integers(1, 301, size=600)
    sizes[:3] = (300, 1, 2)
    blocks = [rng.choice(300, size=k, replace=False) for k in sizes] + [np.array([], dtype=int), np.array([17])]
    members = np.full((len(blocks), 300), -1, dtype=np.int32)
    for i, b in enumerate(blocks):
        members[i, :len(b)] = b
    got = eng.l1_subset_depth(P, members)
    assert np.isnan(got[600]) and got[601] == 1.0 and got[1] == 1.0
    want = np.array([oracle.l1_depth(P[b], [len(b) - 1])[0] if len(b) else np.nan for b in blocks])
    tol = np.array([l1_tolerance(max(len(b), 1), d) for b in blocks])
    _against_oracle(got, want, tol)
    some = np.array([0, 1, 2, 255, 256, 511, 512, 599, 600, 601, *range(300, 306)])
    _against_reference(f"blocks d={d}", got[some], l1_reference(P, blocks=[blocks[i] for i in some]), tol[some])
