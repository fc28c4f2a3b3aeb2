"""Projection depth on the GPU (K12, sd_projection_*): outlyingness and depth EQUAL, bit for bit, to the numpy restatement
of tests/test_projection_host.py (np.array_equal on float64, infinities included, no tolerance anywhere) -- smallest
shapes, the sort's tile and merge boundaries, ties and zero MADs, workspace independence, target lists, the external and
the blocks form, the two routes against each other, integer shifts, and the public API."""
import functools

import numpy as np
import pandas as pd
import pytest

from test_halfspace_host import make_directions
from test_projection_host import (depth_of, projection_external, projection_outlyingness, projection_sampled)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from statdepth_amd import engine
    return engine


@functools.lru_cache(maxsize=None)
def _continuous(n, d, k):
    """(P, U, every point's outlyingness by the restatement), computed once per shape and not modified."""
    P = np.random.default_rng(2000 * d + n).normal(size=(n, d))
    U = make_directions(k, n, d)
    want = projection_outlyingness(P, U)
    want.setflags(write=False)
    return P, U, want


def _integer_cloud(n, d, k, seed):
    """K10's integer cloud: small integer coordinates, duplicated points, integer directions."""
    rng = np.random.default_rng(seed)
    P = rng.integers(-3, 4, size=(n, d)).astype(np.float64)
    P[n // 2:n // 2 + n // 8] = P[:n // 8]                             # duplicated points
    U = rng.integers(-2, 3, size=(k, d)).astype(np.float64)
    U[~U.any(axis=1)] = 1.0
    return P, U


def _blocks(rows):
    width = max(len(r) for r in rows)
    mem = np.full((len(rows), max(width, 1)), -1, dtype=np.int32)
    for i, r in enumerate(rows):
        mem[i, :len(r)] = r
    return mem


def _block_want(P, U, rows):
    return np.array([projection_outlyingness(P[np.asarray(r)], U, [len(r) - 1])[0] if len(r) else 0.0 for r in rows])


# ---------------------------------------------------------------- smallest shapes
@pytest.mark.parametrize("d", [1, 2, 3, 8])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_smallest_shapes(eng, n, d):
    P = np.random.default_rng(10 * n + d).normal(size=(n, d))
    Q = np.vstack([P[:1] + 0.25, P[-1:], P.mean(axis=0, keepdims=True)])
    for U in (make_directions(5, n, d), np.eye(d)[:1]):
        assert np.array_equal(eng.projection_outlyingness(P, U), projection_outlyingness(P, U))
        assert np.array_equal(eng.projection_external_outlyingness(P, Q, U), projection_external(P, Q, U))


def test_hand_computed_cases(eng):
    one = [[1.0]]
    assert eng.projection_outlyingness([[0.0], [1.0], [2.0], [3.0], [10.0]], one).tolist() == [2.0, 1.0, 0.0, 1.0, 8.0]
    assert np.array_equal(eng.projection_outlyingness([[0.0], [1.0], [3.0], [10.0]], one),
                          np.array([4 / 3, 2 / 3, 2 / 3, 16 / 3]))
    assert eng.projection_outlyingness([[5.0], [5.0], [5.0], [5.0], [9.0]], one).tolist() == [0.0, 0.0, 0.0, 0.0, np.inf]
    assert eng.projection_outlyingness([[7.0]], one).tolist() == [0.0]
    assert eng.projection_external_outlyingness([[0.0], [1.0], [2.0], [3.0]], [[10.0], [2.0], [-1.0]], one).tolist() == \
        [8.0, 0.0, 2.0]


# ---------------------------------------------------------------- the sort's boundaries
# One sort tile holds 2 048 values: n <= 2 048 is sorted by the tile sort alone, 2 049 is the first size with a merge pass;
# at n = 4 096 the two middle values sit in different sort tiles before the merge; 4 097 has a run that waits a pass.
@pytest.mark.parametrize("n,d,k", [(2047, 2, 3), (2048, 2, 3), (2049, 2, 3), (4096, 2, 3), (4097, 2, 3),
                                   (1025, 3, 65), (20000, 3, 17)])
def test_continuous_data_across_sort_boundaries(eng, n, d, k):
    P, U, want = _continuous(n, d, k)
    got = eng.projection_outlyingness(P, U)
    assert got.dtype == np.float64 and np.array_equal(got, want)


# ---------------------------------------------------------------- ties
@pytest.mark.parametrize("n,d,k", [(257, 2, 12), (257, 3, 12), (4500, 2, 6)])
def test_integer_cloud_with_duplicated_points(eng, n, d, k):
    P, U = _integer_cloud(n, d, k, 40 + d + n)
    want = projection_outlyingness(P, U)
    assert np.isfinite(want).any()
    assert np.array_equal(eng.projection_outlyingness(P, U), want)
    Q = np.vstack([P[:3], np.zeros((1, d)), np.full((1, d), 9.0)])
    assert np.array_equal(eng.projection_external_outlyingness(P, Q, U), projection_external(P, Q, U))


def test_mostly_identical_rows_have_zero_mad(eng):
    """60 % of the rows identical: the MAD is 0 in every direction, the duplicates sit on every median (O = 0), every other
    point is off the median in some direction (O = inf, depth 0)."""
    rng = np.random.default_rng(7)
    n = 500
    P = rng.normal(size=(n, 3))
    same = rng.permutation(n)[:300]
    P[same] = [0.5, -1.25, 2.0]
    U = make_directions(16, 1, 3)
    got = eng.projection_outlyingness(P, U)
    assert np.array_equal(got, projection_outlyingness(P, U))
    other = np.setdiff1d(np.arange(n), same)
    assert (got[same] == 0.0).all() and np.isinf(got[other]).all()
    assert depth_of(got)[other].tolist() == [0.0] * len(other)


def test_flat_coordinate_direction_contributes_nothing(eng):
    rng = np.random.default_rng(8)
    P = rng.normal(size=(300, 3))
    P[:, 1] = 4.0                                                      # flat in coordinate 1
    axis = np.array([[0.0, 1.0, 0.0]])
    assert eng.projection_outlyingness(P, axis).tolist() == [0.0] * 300
    U = make_directions(9, 2, 3)
    both = np.vstack([U[:4], axis, U[4:]])
    got = eng.projection_outlyingness(P, both)
    assert np.array_equal(got, eng.projection_outlyingness(P, U))
    assert np.array_equal(got, projection_outlyingness(P, both))


# ---------------------------------------------------------------- workspace independence
def test_workspace_floor_gives_the_same_bits(eng):
    """The recommended workspace takes all 70 directions in one chunk, the floor one direction per chunk, a budget in
    between chunks of 3 with a last chunk of 1."""
    P, U, want = _continuous(4097, 3, 70)
    Q = np.vstack([P[:3] * 0.5, P[[4096]]])
    want_ext = projection_external(P, Q, U)
    rec, floor = eng.projection_workspace_bytes(4097, 3, 70)
    assert floor < rec
    per_direction = (rec - floor) // 69
    for budget in (0, floor + 2 * per_direction + 64, None):
        eng.release_workspace()                                        # so the call really gets a buffer of that size
        assert np.array_equal(eng.projection_outlyingness(P, U, workspace_budget=budget), want)
        assert np.array_equal(eng.projection_external_outlyingness(P, Q, U, workspace_budget=budget), want_ext)


def test_floor_sized_buffer_through_the_abi(eng):
    """sd_projection_outlyingness given exactly sd_projection_min_workspace_bytes, and one byte less (refused)."""
    import torch
    from statdepth_amd import _native
    lib = _native.load()
    P, U, want = _continuous(2049, 2, 3)
    dev = torch.device("cuda", torch.cuda.current_device())
    Pd, Ud = torch.from_numpy(P.copy()).to(dev), torch.from_numpy(U.copy()).to(dev)
    out = torch.empty(2049, dtype=torch.float64, device=dev)
    floor = lib.sd_projection_min_workspace_bytes(2049, 2, 3)
    ws = torch.empty(floor, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    args = (Pd.data_ptr(), 2049, 2, Ud.data_ptr(), 3, None, 2049, out.data_ptr(), ws.data_ptr())
    assert lib.sd_projection_outlyingness(*args, floor - 1, stream) == _native.SD_ERR_WORKSPACE
    assert lib.sd_projection_outlyingness(*args, floor, stream) == _native.SD_OK
    assert np.array_equal(out.cpu().numpy(), want)


# ---------------------------------------------------------------- target lists
def test_target_lists(eng):
    P, U, want = _continuous(1025, 3, 65)
    perm = np.random.default_rng(3).permutation(1025)
    assert np.array_equal(eng.projection_outlyingness(P, U, perm), want[perm])
    tg = [1024, 0, 7, 7, 512]
    assert np.array_equal(eng.projection_outlyingness(P, U, tg), want[tg])
    assert np.array_equal(eng.projection_outlyingness(P, U, [5]), want[[5]])
    assert eng.projection_outlyingness(P, U, []).shape == (0,)
    with pytest.raises(IndexError):
        eng.projection_outlyingness(P, U, [1025])


# ---------------------------------------------------------------- external targets
@pytest.mark.parametrize("n", [300, 301])
def test_external_targets(eng, n):
    rng = np.random.default_rng(50 + n)
    F = rng.normal(size=(n, 3))
    U = np.vstack([make_directions(39, 5, 3), [[1.0, 0.0, 0.0]]])
    x = F[:, 0]
    med_x = np.sort(x)[(n - 1) // 2] if n % 2 else (np.sort(x)[n // 2 - 1] + np.sort(x)[n // 2]) * 0.5
    Q = np.vstack([[[-60.0, 70.0, 80.0]], [[60.0, -70.0, -80.0]],     # beyond every projection on the axis, both sides
                   F[[17]],                                            # equal to a sample point
                   [[med_x, F[3, 1], F[3, 2]]]])                       # on F's median along the last direction
    want = projection_external(F, Q, U)
    assert np.array_equal(eng.projection_external_outlyingness(F, Q, U), want)
    axis = U[-1:]
    assert np.array_equal(eng.projection_external_outlyingness(F, Q, axis), projection_external(F, Q, axis))
    many = rng.normal(size=(100, 3)) * 1.5                             # 100 external points in one call
    assert np.array_equal(eng.projection_external_outlyingness(F, many, U), projection_external(F, many, U))


def test_external_targets_across_a_merge_pass(eng):
    P, U, _ = _continuous(2049, 2, 3)
    Q = np.vstack([P[[2048]], P[:2] * 0.5, [[40.0, -40.0]], P[[1000]]])
    assert np.array_equal(eng.projection_external_outlyingness(P, Q, U), projection_external(P, Q, U))


# ---------------------------------------------------------------- blocks
def test_blocks_of_every_width(eng):
    rng = np.random.default_rng(60)
    F = rng.normal(size=(2100, 3))
    U = make_directions(5, 6, 3)
    rows = [list(rng.permutation(2100)[:w]) for w in (1, 2, 3, 255, 256, 257, 2047, 2048)]
    rows += [[], [5, 5, 12, 5], [7]]                                   # an empty block, repeated members
    mem = _blocks(rows)
    assert mem.shape == (11, 2048) and (mem[0, 1:] == -1).all()       # ragged, trailing -1 padding
    assert np.array_equal(eng.projection_subset_outlyingness(F, mem, U), _block_want(F, U, rows))
    with pytest.raises(IndexError):
        eng.projection_subset_outlyingness(F, [[0, 2100]], U)


def test_blocks_with_ties_and_many_directions(eng):
    """Integer data (zero MADs, infinities) and 300 directions: two direction launches folded into out."""
    P, U = _integer_cloud(257, 2, 300, 61)
    rng = np.random.default_rng(62)
    rows = [list(rng.permutation(257)[:w]) for w in (4, 9, 64, 130, 257)]
    got = eng.projection_subset_outlyingness(P, _blocks(rows), U)
    assert np.array_equal(got, _block_want(P, U, rows))


def _all_rows_target_last(n):
    """n blocks of n members: block t = every other row in order, then row t."""
    mem = np.empty((n, n), dtype=np.int32)
    idx = np.arange(n, dtype=np.int32)
    for t in range(n):
        mem[t, :t] = idx[:t]
        mem[t, t:n - 1] = idx[t + 1:]
        mem[t, n - 1] = t
    return mem


@pytest.mark.parametrize("n,d,k", [(2048, 2, 3), (2047, 2, 3), (1025, 3, 65), (257, 8, 9)])
def test_block_of_all_rows_equals_the_rows_form(eng, n, d, k):
    """'all rows, the target last' through the LDS sort and selection = the rows form through the global sort, for EVERY
    target (n = 2 048: a 16 MB member array, one full LDS tile per block)."""
    P, U, want = _continuous(n, d, k)
    got = eng.projection_subset_outlyingness(P, _all_rows_target_last(n), U)
    assert np.array_equal(got, eng.projection_outlyingness(P, U))
    assert np.array_equal(got, want)


def test_all_small_blocks_equal_the_rows_form(eng):
    P, U, want = _continuous(40, 3, 7)
    rows = [[i for i in range(40) if i != t] + [t] for t in range(40)]
    assert np.array_equal(eng.projection_subset_outlyingness(P, _blocks(rows), U), want)


def test_block_above_one_sort_tile_is_refused(eng):
    from statdepth_amd import _native
    P = np.zeros((2100, 2))
    mem = np.arange(2049, dtype=np.int32)[None, :]
    with pytest.raises(_native.StatdepthHipError) as e:
        eng.projection_subset_outlyingness(P, mem, np.eye(2))
    assert e.value.code == _native.SD_ERR_UNSUPPORTED and '2048' in str(e.value)


# ---------------------------------------------------------------- invariance
def test_integer_shift_on_integer_data(eng):
    """Integer data, directions and shift: every projection, median, deviation and MAD is computed exactly and moves (or
    stays) with the shift, so the quotients are the same bits."""
    P, U = _integer_cloud(600, 3, 16, 90)
    base = eng.projection_outlyingness(P, U)
    assert np.array_equal(base, projection_outlyingness(P, U))
    for shift in ([5.0, -2.0, 11.0], [-1000.0, 0.0, 3.0]):
        assert np.array_equal(eng.projection_outlyingness(P + np.array(shift), U), base)


# ---------------------------------------------------------------- public API
def test_pointcloud_depth_api():
    from statdepth_amd import PointcloudDepth
    P = np.random.default_rng(70).normal(size=(120, 3))
    df = pd.DataFrame(P, index=[f"p{i}" for i in range(120)])
    got = PointcloudDepth(df, containment='projection', directions=64, seed=3)
    want = depth_of(projection_outlyingness(P, make_directions(64, 3, 3)))
    assert list(got.index) == list(df.index)
    assert np.array_equal(got.to_numpy(), want)
    assert got.deepest(n=1).index[0] == df.index[int(np.argmax(want))]
    tc = ["p7", "p2", "p119", "p0"]
    part = PointcloudDepth(df, to_compute=tc, containment='projection', directions=64, seed=3)
    assert list(part.index) == tc and np.array_equal(part.to_numpy(), got.loc[tc].to_numpy())
    U = [[1.0, 0.0, 0.0], [0.0, 2.0, -1.0]]
    assert np.array_equal(PointcloudDepth(df, containment='projection', directions=U).to_numpy(),
                          depth_of(projection_outlyingness(P, U)))
    default = PointcloudDepth(df, containment='projection')                         # directions=1000, seed=0
    assert np.array_equal(default.to_numpy(), depth_of(projection_outlyingness(P, make_directions(1000, 0, 3))))
    d1 = PointcloudDepth(df.iloc[:, :1], containment='projection', directions=7)    # d = 1: the direction (1.0)
    assert np.array_equal(d1.to_numpy(), depth_of(projection_outlyingness(P[:, :1], [[1.0]])))
    flat = pd.DataFrame([[5.0], [5.0], [5.0], [5.0], [9.0]])
    assert PointcloudDepth(flat, containment='projection').to_numpy().tolist() == [1.0, 1.0, 1.0, 1.0, 0.0]


def test_sampled_k2_replays_the_draws():
    from statdepth_amd import PointcloudDepth
    P = np.random.default_rng(80).normal(size=(40, 2))
    df = pd.DataFrame(P, index=[f"q{i}" for i in range(40)])
    tc = ["q3", "q0", "q39", "q11"]
    np.random.seed(11)
    got = PointcloudDepth(df, to_compute=tc, K=2, containment='projection', directions=32, seed=9)
    after = np.random.random()                                         # the blocks consumed the global RNG, nothing else did
    np.random.seed(11)
    want = projection_sampled(P, [df.index.get_loc(c) for c in tc], 2, make_directions(32, 9, 2))
    assert list(got.index) == tc
    assert np.array_equal(got.to_numpy(), want)
    assert after == np.random.random()


def test_pointcloud_homogeneity_projection():
    """P1 as its host composition: depths of F and G, G's deepest point as an external target inside F u {g}."""
    from statdepth_amd.homogeneity import PointcloudHomogeneity
    rng = np.random.default_rng(31)
    F = pd.DataFrame(rng.normal(size=(40, 2)), index=[f"f{i}" for i in range(40)])
    G = pd.DataFrame(rng.normal(size=(40, 2)) * 0.8 + 0.2, index=[f"g{i}" for i in range(40)])
    got = PointcloudHomogeneity(F, G, method='p1', containment='projection').homogeneity()
    U = make_directions(1000, 0, 2)
    Fx, Gx = F.to_numpy(), G.to_numpy()
    Fd, Gd = depth_of(projection_outlyingness(Fx, U)), depth_of(projection_outlyingness(Gx, U))
    ext = depth_of(projection_external(Fx, Gx, U))
    # median() = deepest(n=1): the first of the largest values in pandas' descending sort order
    g_star = pd.Series(Gd).sort_values(ascending=False).index[0]
    assert got == ext[g_star] / Fd.max()
