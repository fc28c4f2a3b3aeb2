"""Oja depth on the GPU (K7, sd_oja_*): the reference's fixtures through PointcloudDepth, the engine against the numpy
restatement of tests/test_oja_host.py, translation, bitwise determinism, multi-launch scale, the K-sampled estimator
and point-cloud homogeneity."""
import numpy as np
import pandas as pd
import pytest

from conftest import assert_depths_close, depths_of, frame_df, golden_names, load_golden
from test_oja_host import oja2_rowwise_targets as _oja2_rowwise_targets
from test_oja_host import oja_depths, oja_external, oja_sampled, oja_sums

pytestmark = pytest.mark.gpu
TOL = 1e-12


@pytest.fixture(scope="module")
def eng():
    from statdepth_amd import engine
    return engine


def _cloud(n, d, seed):
    return np.random.default_rng(seed).random((n, d))


# ---------------------------------------------------------------- the reference's values through the public API
@pytest.mark.parametrize("name", golden_names(kind="pointcloud_oja"))
def test_golden_oja_api(name):
    from statdepth_amd import PointcloudDepth
    fx = load_golden(name)
    df = frame_df(fx["input"])
    got = PointcloudDepth(df, containment='oja')
    assert list(got.index) == fx["index"]
    assert_depths_close(got.to_numpy(), depths_of(fx), TOL)


# ---------------------------------------------------------------- engine vs the restatement
@pytest.mark.parametrize("d", range(1, 9))
def test_engine_every_target_and_subsets(eng, d):
    n = {1: 30, 2: 25, 3: 18, 4: 14, 5: 12, 6: 11, 7: 11, 8: 12}[d]
    P = _cloud(n, d, 100 + d)
    want = oja_sums(P)
    assert_depths_close(eng.oja_volume_sums(P), want, TOL)
    tg = [n - 1, 0, 3, 3]
    assert_depths_close(eng.oja_volume_sums(P, tg), want[tg], TOL)


@pytest.mark.parametrize("d", [1, 2, 3, 5, 8])
def test_engine_duplicates_and_integer_grids(eng, d):
    """Coincident points and integer grids: flat simplices add 0, nothing raises, nothing is NaN."""
    rng = np.random.default_rng(200 + d)
    n = {1: 20, 2: 16, 3: 12, 5: 10, 8: 11}[d]
    P = rng.integers(0, 3, size=(n, d)).astype(np.float64)
    P[1] = P[0]
    got = eng.oja_volume_sums(P)
    assert np.isfinite(got).all()
    assert_depths_close(got, oja_sums(P), TOL)


def test_translation_invariance(eng):
    """Y = X + 1e4: the device translates by the target before any product (the oracle on Y - 1e4 is exact)."""
    for d, n in ((2, 40), (3, 20), (5, 12), (8, 11)):
        X = _cloud(n, d, 300 + d)
        Y = X + 1e4
        want = oja_sums(Y - 1e4)
        got = eng.oja_volume_sums(Y)
        assert np.all(np.abs(got - want) <= 1e-9 * np.abs(want)), (d, got, want)


# ---------------------------------------------------------------- determinism, bitwise
@pytest.mark.parametrize("n,d", [(300, 2), (60, 3), (14, 8)])
def test_bitwise_determinism(eng, n, d):
    P = _cloud(n, d, 400 + d)
    a = eng.oja_volume_sums(P)
    assert np.array_equal(a, eng.oja_volume_sums(P))
    for t in (0, n // 2, n - 1):
        assert np.array_equal(eng.oja_volume_sums(P, [t]), a[[t]])
    perm = np.random.default_rng(n).permutation(n)
    assert np.array_equal(eng.oja_volume_sums(P, perm), a[perm])


def test_to_compute_equals_full_depth_subset():
    from statdepth_amd import PointcloudDepth
    df = pd.DataFrame(_cloud(20, 2, 500), index=[f"p{i}" for i in range(20)])
    s = ["p7", "p2", "p19", "p0"]
    part = PointcloudDepth(df, to_compute=s, containment='oja')
    full = PointcloudDepth(df, containment='oja')
    assert list(part.index) == s
    assert np.array_equal(part.to_numpy(), full.loc[s].to_numpy())


# ---------------------------------------------------------------- scale: several launches, several slices per target
def _oja2_rowwise(P):
    """d = 2 volume sums by an O(n^2)-per-target cross-product table."""
    out = np.empty(len(P))
    for t in range(len(P)):
        a = np.delete(P, t, axis=0) - P[t]
        M = np.abs(a[:, 0][:, None] * a[:, 1][None, :] - a[:, 1][:, None] * a[:, 0][None, :])
        out[t] = np.triu(M, 1).sum() / 2.0
    return out


def test_scale_d2_n700_every_target(eng):
    P = _cloud(700, 2, 600)
    got = eng.oja_volume_sums(P)                # C(699, 2) = 243 951 per target: 8 slices each
    want = _oja2_rowwise(P)
    assert np.all(np.abs(got - want) <= 1e-11 * want)


def test_scale_d3_n150_20_targets(eng):
    P = _cloud(150, 3, 700)
    tg = np.random.default_rng(7).choice(150, 20, replace=False)
    got = eng.oja_volume_sums(P, tg)
    want = []
    for t in tg:
        a = np.delete(P, t, axis=0) - P[t]
        cr = np.cross(a[:, None, :], a[None, :, :])                  # (i, j) -> a_i x a_j
        det = np.einsum('ijc,kc->ijk', cr, a)                         # a_k . (a_i x a_j) = det[a_i, a_j, a_k]
        i, j, k = np.ogrid[:149, :149, :149]
        want.append(np.abs(det[(i < j) & (j < k)]).sum() / 6.0)
    want = np.array(want)
    assert np.all(np.abs(got - want) <= 1e-11 * want)


def test_launch_split_does_not_change_bits(eng):
    """n = 2100, d = 2, every target: 68 slices of 32 768 subsets per target, 142 800 (target, slice) units in two
    evaluation-bounded launches, the split falling inside target 1927.  That target alone, and its neighbours, agree
    bit for bit with the all-target call."""
    P = _cloud(2100, 2, 800)
    many = eng.oja_volume_sums(P)
    for t in (0, 1926, 1927, 1928, 2099):
        assert np.array_equal(eng.oja_volume_sums(P, [t]), many[[t]])
    tg = [0, 1927, 2099]
    want = _oja2_rowwise_targets(P, tg)
    assert np.all(np.abs(many[tg] - want) <= 1e-11 * want)


def test_global_memory_path_and_lds_boundary(eng):
    """no * d * 8 bytes above 64 KB read the others from global memory (n = 4 200, d = 2); n = 4 097 puts exactly 64 KB
    in LDS.  Both against the row-wise oracle."""
    for n, tg in ((4200, [0, 2100, 4199]), (4097, [0, 4096])):
        P = _cloud(n, 2, 850 + n)
        want = _oja2_rowwise_targets(P, tg)
        got = eng.oja_volume_sums(P, tg)
        assert np.all(np.abs(got - want) <= 1e-11 * want), n


def test_target_beyond_4096_slices_split_across_launches(eng):
    """n = 65 537, d = 2: C(65 536, 2) = 2^31 - 2^15 subsets per target = 65 535 slices of 32 768 (global-memory path).
    Targets [17, 30 000, 5] are 196 605 (target, slice) units; a launch holds 131 072, so target 5 is cut after its
    second slice.  Target 5 alone (one launch) agrees bit for bit, and with the row-wise oracle."""
    P = _cloud(65537, 2, 860)
    three = eng.oja_volume_sums(P, [17, 30000, 5])
    alone = eng.oja_volume_sums(P, [5])
    assert np.array_equal(alone, three[[2]])
    want = _oja2_rowwise_targets(P, [5])
    assert np.all(np.abs(alone - want) <= 1e-10 * want)


# ---------------------------------------------------------------- sampled (K) and external forms
def test_sampled_k2_replays_the_draws():
    from statdepth_amd import PointcloudDepth
    df = pd.DataFrame(_cloud(24, 2, 900), index=[f"q{i}" for i in range(24)])
    tc = ["q3", "q0", "q23", "q11"]
    np.random.seed(11)
    got = PointcloudDepth(df, to_compute=tc, K=2, containment='oja')
    np.random.seed(11)
    want = oja_sampled(df.to_numpy(), [df.index.get_loc(c) for c in tc], 2)
    assert list(got.index) == tc
    assert_depths_close(got.to_numpy(), want, TOL)


def test_reference_test_input_api():
    """tests/test_statdepth.py::test_pointcloud_oja of the reference: exact and K=2 return Series.  Its input is
    generate_noisy_pointcloud(n=20, d=2), unseeded there; the oja_rec_k2 fixture holds that generator's output (seed 48)."""
    from statdepth_amd import PointcloudDepth
    df = frame_df(load_golden("oja_rec_k2")["input"])
    bd = PointcloudDepth(df, containment='oja')
    for s in (bd, bd.ordered(), bd.median(), bd.deepest(n=2), bd.outlying(n=2)):
        assert isinstance(s, pd.Series)
    assert bd.deepest(n=1).index[0] == bd.idxmax()                   # an outlyingness: "deepest" = the largest value
    assert isinstance(PointcloudDepth(df, K=2, containment='oja'), pd.Series)


def test_engine_external_and_subset_forms(eng):
    F = _cloud(13, 3, 1000)
    Q = _cloud(5, 3, 1001)
    got = eng.oja_external_volume_sums(F, Q)
    want = np.array([oja_sums(np.vstack([F, q]), [len(F)])[0] for q in Q])
    assert_depths_close(got, want, TOL)
    mem = np.array([[0, 4, 7, 9, 2, -1], [1, 2, 3, 5, 6, 8], [3, -1, -1, -1, -1, -1], [-1] * 6], dtype=np.int32)
    got = eng.oja_subset_volume_sums(F, mem)
    want = [oja_sums(F[[0, 4, 7, 9, 2]], [4])[0], oja_sums(F[[1, 2, 3, 5, 6, 8]], [5])[0], 0.0, 0.0]
    assert_depths_close(got, want, TOL)


# ---------------------------------------------------------------- homogeneity (DESIGN §4 difference 4)
def _hom_restated(F, G, method, K=None):
    """P1..P4 of _pointcloudhomogeneity with g evaluated inside the intact F u {g}; with K the draws are replayed in the
    order the product makes them."""
    Fx, Gx = F.to_numpy(), G.to_numpy()

    def depths(X):
        return oja_depths(X) if K is None else oja_sampled(X, range(len(X)), K)

    def ext(host, pts):
        if K is None:
            return np.array([oja_external(host, p) for p in pts])
        return np.array([oja_sampled(np.vstack([host, p]), [len(host)], K)[0] for p in pts])
    Fd, Gd = depths(Fx), depths(Gx)
    Fmed, Gmed = Fd.max(), Gd.max()                                     # median() = deepest(n=1) = the largest value
    if method in ('p1', 'p2'):
        v = ext(Fx, Gx[[np.argmax(Gd)]])[0]
        return v / Fmed if method == 'p1' else 1 - abs(v - Fmed)
    p3 = ext(Fx, Gx).max() / Gmed
    if method == 'p3':
        return p3
    p1FF = ext(Fx, Fx[[np.argmax(Fd)]])[0] / Fmed
    p1GG = ext(Gx, Gx[[np.argmax(Gd)]])[0] / Gmed
    return abs(p3 - p1FF) * abs(p3 - p1GG)


@pytest.mark.parametrize("K", [None, 2])
@pytest.mark.parametrize("method", ["p1", "p2", "p3", "p4"])
def test_pointcloud_homogeneity_oja(method, K):
    from statdepth_amd.homogeneity import PointcloudHomogeneity
    rng = np.random.default_rng(31)
    F = pd.DataFrame(rng.normal(size=(13, 2)), index=[f"f{i}" for i in range(13)])
    G = pd.DataFrame(rng.normal(size=(13, 2)) * 0.8 + 0.2, index=[f"g{i}" for i in range(13)])
    np.random.seed(5)
    got = PointcloudHomogeneity(F, G, method=method, K=K, containment='oja').homogeneity()
    np.random.seed(5)
    want = _hom_restated(F, G, method, K)
    assert_depths_close([got], [want], TOL)
