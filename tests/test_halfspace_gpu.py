"""Halfspace (Tukey) depth on the GPU (K10, sd_halfspace_*): counts EQUAL to the numpy restatement of
tests/test_halfspace_host.py -- smallest shapes, heavy ties, continuous data across the ranking route's tile and merge
boundaries, target lists, external and block forms, workspace independence, the public API, the K-sampled estimator,
point-cloud homogeneity and translation invariance."""
import functools

import numpy as np
import pandas as pd
import pytest

from test_halfspace_host import (halfspace_counts, halfspace_counts_sorted, halfspace_external, halfspace_sampled,
                                 make_directions)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from statdepth_amd import engine
    return engine


@functools.lru_cache(maxsize=None)
def _continuous(n, d, k):
    """(P, U, every point's count by the restatement), computed once per shape and not modified."""
    P = np.random.default_rng(1000 * d + n).normal(size=(n, d))
    U = make_directions(k, n, d)
    want = halfspace_counts_sorted(P, U)
    want.setflags(write=False)
    return P, U, want


def _integer_cloud(n, d, k, seed):
    rng = np.random.default_rng(seed)
    P = rng.integers(-3, 4, size=(n, d)).astype(np.float64)
    P[n // 2:n // 2 + n // 8] = P[:n // 8]                             # duplicated points
    U = rng.integers(-2, 3, size=(k, d)).astype(np.float64)
    U[~U.any(axis=1)] = 1.0
    return P, U


# ---------------------------------------------------------------- smallest shapes
@pytest.mark.parametrize("d", [1, 2, 3, 8])
@pytest.mark.parametrize("n", [1, 2, 3])
def test_smallest_shapes(eng, n, d):
    P = np.random.default_rng(10 * n + d).normal(size=(n, d))
    for U in (make_directions(5, n, d), np.eye(d)[:1]):
        want = halfspace_counts(P, U)
        assert np.array_equal(eng.halfspace_counts(P, U), want)
        assert np.array_equal(eng.halfspace_counts(P, U, algo="pairwise"), want)
        assert np.array_equal(eng.halfspace_external_counts(P, P[:1] + 0.25, U), halfspace_external(P, P[:1] + 0.25, U))


def test_univariate_is_the_exact_halfspace_depth(eng):
    x = np.array([3.0, -1.0, 7.0, 0.0, 12.0, 3.0])
    got = eng.halfspace_counts(x[:, None], [[1.0]])
    assert got.tolist() == [4, 1, 2, 2, 1, 4]                          # min(#{<= x}, #{>= x}), the pair of 3s tied
    assert eng.halfspace_counts(np.arange(5.0)[:, None], [[1.0]]).tolist() == [1, 2, 3, 2, 1]


def test_square_and_centre(eng):
    P = np.array([[1, 1], [1, -1], [-1, 1], [-1, -1], [0, 0]], dtype=np.float64)
    U = np.array([[1, 0], [0, 1], [1, 1], [1, -1]], dtype=np.float64)
    assert eng.halfspace_counts(P, U).tolist() == [1, 1, 1, 1, 3]


# ---------------------------------------------------------------- heavy ties, duplicated points
@pytest.mark.parametrize("d", [2, 3])
def test_integer_data_heavy_ties(eng, d):
    P, U = _integer_cloud(257, d, 12, 40 + d)
    want = halfspace_counts(P, U)
    assert np.array_equal(eng.halfspace_counts(P, U), want)
    assert np.array_equal(eng.halfspace_counts(P, U, algo="pairwise"), want)


def test_integer_data_ties_across_merge_tiles(eng):
    """n = 4 500: three sort tiles and two merge passes; runs of equal projections hundreds long cross the tile borders,
    so the ends of a run are found by the rank kernel's searches over the whole sorted row."""
    P, U = _integer_cloud(4500, 2, 6, 44)
    assert np.array_equal(eng.halfspace_counts(P, U), halfspace_counts_sorted(P, U))
    one = np.zeros((2500, 3))                                          # every projection equal: le = ge = n everywhere
    assert eng.halfspace_counts(one, U[:, :1] * np.ones((1, 3))).tolist() == [2500] * 2500


# ---------------------------------------------------------------- continuous data, the ranking route's boundaries
# One sort tile holds 2 048 values: n <= 2 048 is sorted by hs_tile_sort_kernel alone, n = 2 049 is the first size with a
# merge pass (a second run of one value); 4 096 / 4 097 are two full tiles / a third run that waits a pass unpaired.
@pytest.mark.parametrize("n,d,k", [(1025, 3, 65), (4097, 8, 33), (20000, 3, 17),
                                   (2047, 2, 3), (2048, 2, 3), (2049, 2, 3), (4096, 2, 3)])
def test_continuous_data(eng, n, d, k):
    P, U, want = _continuous(n, d, k)
    assert np.array_equal(eng.halfspace_counts(P, U), want)


def test_ranking_and_pairwise_kernels_agree(eng):
    """n = 5 000 (two slices of 4 096 sample points per workgroup row), k = 300 (two chunks of 256 directions)."""
    P, U, want = _continuous(5000, 3, 300)
    tg = np.array([0, 4999, 4096, 4095, 17])
    assert np.array_equal(eng.halfspace_counts(P, U, tg, algo="pairwise"), want[tg])
    assert np.array_equal(eng.halfspace_counts(P, U, tg), want[tg])


# ---------------------------------------------------------------- target lists
def test_to_compute_subsets_and_permuted_targets(eng):
    P, U, want = _continuous(1025, 3, 65)
    perm = np.random.default_rng(3).permutation(1025)
    assert np.array_equal(eng.halfspace_counts(P, U, perm), want[perm])
    tg = [1024, 0, 7, 7, 512]
    assert np.array_equal(eng.halfspace_counts(P, U, tg), want[tg])
    assert np.array_equal(eng.halfspace_counts(P, U, [5]), want[[5]])
    assert eng.halfspace_counts(P, U, []).shape == (0,)
    with pytest.raises(IndexError):
        eng.halfspace_counts(P, U, [1025])


# ---------------------------------------------------------------- external targets and blocks
def test_external_targets(eng):
    rng = np.random.default_rng(50)
    F = rng.normal(size=(300, 3))
    Q = np.vstack([rng.normal(size=(4, 3)), F[[17]], [[50.0, 50.0, 50.0]]])     # one duplicates a sample point
    U = make_directions(40, 5, 3)
    want = halfspace_external(F, Q, U)
    assert np.array_equal(eng.halfspace_external_counts(F, Q, U), want)
    assert want[5] == 1                                                # far outside: only itself on its side
    # inside F u {g} a copy of sample point 17 has one more point on both sides than point 17 has inside F
    assert want[4] == halfspace_counts(F, U, [17])[0] + 1
    Fi, Ui = _integer_cloud(257, 2, 9, 51)
    Qi = np.vstack([Fi[:3], [[0.0, 0.0], [9.0, -9.0]]])
    assert np.array_equal(eng.halfspace_external_counts(Fi, Qi, Ui), halfspace_external(Fi, Qi, Ui))


def test_external_many_sample_slices_and_direction_chunks(eng):
    P, U, _ = _continuous(5000, 3, 300)
    Q = np.vstack([P[[4999]], P[:2] * 0.5])
    assert np.array_equal(eng.halfspace_external_counts(P, Q, U), halfspace_external(P, Q, U))


def test_subset_blocks_of_unequal_size(eng):
    F = np.random.default_rng(60).normal(size=(13, 3))
    U = make_directions(20, 6, 3)
    mem = np.array([[0, 4, 7, 9, 2, -1], [1, 2, 3, 5, 6, 8], [3, -1, -1, -1, -1, -1], [-1] * 6, [5, 5, 12, 5, -1, -1]],
                   dtype=np.int32)
    want = [halfspace_counts(F[[0, 4, 7, 9, 2]], U, [4])[0], halfspace_counts(F[[1, 2, 3, 5, 6, 8]], U, [5])[0], 1, 0,
            halfspace_counts(F[[5, 5, 12, 5]], U, [3])[0]]
    assert eng.halfspace_subset_counts(F, mem, U).tolist() == want
    with pytest.raises(IndexError):
        eng.halfspace_subset_counts(F, [[0, 13]], U)


# ---------------------------------------------------------------- workspace independence
def test_workspace_floor_gives_the_same_counts(eng):
    """The recommended workspace ranks all 9 directions in one chunk; the floor one direction per chunk; a budget in
    between chunks of 2 with a last chunk of 1."""
    P, U, want = _continuous(4097, 3, 9)
    rec, floor = eng.halfspace_workspace_bytes(4097, 3, 9)
    assert floor < rec
    eng.release_workspace()                                            # so the floor call really gets a floor-sized buffer
    assert np.array_equal(eng.halfspace_counts(P, U, workspace_budget=0), want)
    per_direction = (rec - floor) // 8
    assert np.array_equal(eng.halfspace_counts(P, U, workspace_budget=floor + per_direction + 64), want)
    assert np.array_equal(eng.halfspace_counts(P, U), want)


def test_floor_sized_buffer_through_the_abi(eng):
    """sd_halfspace_counts given exactly sd_halfspace_min_workspace_bytes, and one byte less (refused)."""
    import torch
    from statdepth_amd import _native
    lib = _native.load()
    P, U, want = _continuous(2049, 2, 3)
    dev = torch.device("cuda", torch.cuda.current_device())
    Pd, Ud = torch.from_numpy(P.copy()).to(dev), torch.from_numpy(U.copy()).to(dev)
    out = torch.empty(2049, dtype=torch.int64, device=dev)
    floor = lib.sd_halfspace_min_workspace_bytes(2049, 2, 3)
    ws = torch.empty(floor, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    args = (Pd.data_ptr(), 2049, 2, Ud.data_ptr(), 3, None, 2049, out.data_ptr(), ws.data_ptr())
    assert lib.sd_halfspace_counts(*args, floor - 1, stream) == _native.SD_ERR_WORKSPACE
    assert lib.sd_halfspace_counts(*args, floor, stream) == _native.SD_OK
    assert np.array_equal(out.cpu().numpy(), want)


# ---------------------------------------------------------------- public API
def test_pointcloud_depth_api():
    from statdepth_amd import PointcloudDepth
    P = np.random.default_rng(70).normal(size=(120, 3))
    df = pd.DataFrame(P, index=[f"p{i}" for i in range(120)])
    got = PointcloudDepth(df, containment='halfspace', directions=64, seed=3)
    want = halfspace_counts(P, make_directions(64, 3, 3)) / 120
    assert list(got.index) == list(df.index)
    assert np.array_equal(got.to_numpy(), want)
    assert got.deepest(n=1).index[0] == df.index[int(np.argmax(want))]
    tc = ["p7", "p2", "p119", "p0"]
    part = PointcloudDepth(df, to_compute=tc, containment='halfspace', directions=64, seed=3)
    assert list(part.index) == tc and np.array_equal(part.to_numpy(), got.loc[tc].to_numpy())
    U = [[1.0, 0.0, 0.0], [0.0, 2.0, -1.0]]
    assert np.array_equal(PointcloudDepth(df, containment='halfspace', directions=U).to_numpy(),
                          halfspace_counts(P, U) / 120)
    default = PointcloudDepth(df, containment='halfspace')                          # directions=1000, seed=0
    assert np.array_equal(default.to_numpy(), halfspace_counts(P, make_directions(1000, 0, 3)) / 120)
    d1 = PointcloudDepth(df.iloc[:, :1], containment='halfspace', directions=7)     # d = 1: the direction (1.0)
    assert np.array_equal(d1.to_numpy(), halfspace_counts(P[:, :1], [[1.0]]) / 120)


def test_sampled_k2_replays_the_draws():
    from statdepth_amd import PointcloudDepth
    P = np.random.default_rng(80).normal(size=(24, 2))
    df = pd.DataFrame(P, index=[f"q{i}" for i in range(24)])
    tc = ["q3", "q0", "q23", "q11"]
    np.random.seed(11)
    got = PointcloudDepth(df, to_compute=tc, K=2, containment='halfspace', directions=32, seed=9)
    after = np.random.random()                                         # the blocks consumed the global RNG, nothing else did
    np.random.seed(11)
    want = halfspace_sampled(P, [df.index.get_loc(c) for c in tc], 2, make_directions(32, 9, 2))
    assert list(got.index) == tc
    assert np.array_equal(got.to_numpy(), want)
    assert after == np.random.random()
    np.random.seed(11)
    l1 = PointcloudDepth(df, to_compute=tc, K=2, containment='l1')
    assert np.random.random() == after and len(l1) == 4               # the same draws as any other containment
    k1 = PointcloudDepth(df, to_compute=tc, K=1, containment='halfspace', directions=32, seed=9)
    assert np.array_equal(k1.to_numpy(), halfspace_counts(P, make_directions(32, 9, 2),
                                                          [df.index.get_loc(c) for c in tc]) / 24)


@pytest.mark.parametrize("method", ["p1", "p3"])
def test_pointcloud_homogeneity_halfspace(method):
    """P1 and P3 as their host composition: depths of F and G, the points of G as external targets inside F u {g}."""
    from statdepth_amd.homogeneity import PointcloudHomogeneity
    rng = np.random.default_rng(31)
    F = pd.DataFrame(rng.normal(size=(40, 2)), index=[f"f{i}" for i in range(40)])
    G = pd.DataFrame(rng.normal(size=(40, 2)) * 0.8 + 0.2, index=[f"g{i}" for i in range(40)])
    got = PointcloudHomogeneity(F, G, method=method, containment='halfspace').homogeneity()
    U = make_directions(1000, 0, 2)
    Fx, Gx = F.to_numpy(), G.to_numpy()
    Fd, Gd = halfspace_counts(Fx, U) / 40, halfspace_counts(Gx, U) / 40
    ext = halfspace_external(Fx, Gx, U) / 41
    # median() = deepest(n=1): the first of the largest values in pandas' descending sort order
    g_star = pd.Series(Gd).sort_values(ascending=False).index[0]
    want = ext[g_star] / Fd.max() if method == 'p1' else ext.max() / Gd.max()
    assert got == want


# ---------------------------------------------------------------- invariance
def test_translation_by_integers_on_integer_data(eng):
    """Integer data, integer directions and an integer shift: every projection is an exact integer, moved by the same
    amount for every point of a direction, so the counts are equal."""
    P, U = _integer_cloud(600, 3, 16, 90)
    base = eng.halfspace_counts(P, U)
    assert np.array_equal(base, halfspace_counts(P, U))
    for shift in ([5.0, -2.0, 11.0], [-1000.0, 0.0, 3.0]):
        assert np.array_equal(eng.halfspace_counts(P + np.array(shift), U), base)
    from statdepth_amd import PointcloudDepth
    a = PointcloudDepth(pd.DataFrame(P), containment='halfspace', directions=U)
    b = PointcloudDepth(pd.DataFrame(P + np.array([7.0, 7.0, -4.0])), containment='halfspace', directions=U)
    assert np.array_equal(a.to_numpy(), b.to_numpy())
