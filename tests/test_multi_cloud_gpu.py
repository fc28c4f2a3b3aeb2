"""Halfspace and projection depth of multivariate curves over time on the GPU (K18, sd_multi_halfspace_sums and
sd_multi_projection_sums): the records EQUAL, bit for bit, the numpy restatement of tests/test_multi_cloud_host.py on both
routes (np.array_equal on int64 and float64, infinities included, no tolerance anywhere) -- n across the padding, the wave
and the route edges, every kind of d, k and T, workspace independence, degenerate clouds, target lists, the anchors to the
point-cloud depths and to K14, and the public API."""
import functools

import numpy as np
import pandas as pd
import pytest

from test_halfspace_host import make_directions
from test_multi_cloud_host import depths_from_records, multi_halfspace_records, multi_projection_records

pytestmark = pytest.mark.gpu

ROUTES = ("lds", "global")


@pytest.fixture(scope="module")
def eng():
    from statdepth_amd import engine
    return engine


@functools.lru_cache(maxsize=None)
def _case(n, T, d, k, seed=0):
    """(P, U, halfspace records, projection records) of a continuous sample, computed once per shape and not modified."""
    P = np.random.default_rng(1000 * n + 10 * T + d + seed).normal(size=(n, T, d))
    U = make_directions(k, n + T, d)
    H, O = multi_halfspace_records(P, U), multi_projection_records(P, U)
    for A in (P, U, H, O):
        A.setflags(write=False)
    return P, U, H, O


def _check(eng, P, U, H=None, O=None, targets=None, algos=ROUTES, ws=(None, None)):
    """Both families on every route of `algos` against the restatement (H, O: its records of ALL curves, when in hand)."""
    H = multi_halfspace_records(P, U, targets) if H is None else (H if targets is None else H[np.asarray(targets)])
    O = multi_projection_records(P, U, targets) if O is None else (O if targets is None else O[np.asarray(targets)])
    for algo in algos:
        got = eng.multi_halfspace_sums(P, U, targets, algo=algo, ws_bytes=ws[0])
        assert got.dtype == np.int64 and np.array_equal(got, H), (algo, "halfspace")
        got = eng.multi_projection_sums(P, U, targets, algo=algo, ws_bytes=ws[1])
        assert got.dtype == np.float64 and np.array_equal(got, O), (algo, "projection")


# ---------------------------------------------------------------- n across padding and wave edges, and across the route edge
@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 1000])
def test_n_across_padding_and_wave_edges(eng, n):
    _check(eng, *_case(n, 3, 3, 5), algos=ROUTES + ("auto",))


@pytest.mark.parametrize("n", [2048, 2049, 3072, 3073, 5000, 6144, 6145])
def test_n_around_the_powers_of_two_of_the_sort(eng, n):
    """The LDS sort runs the network of the next power of two and leaves out the pairs that reach past n: full networks,
    one key more than a full network, and sizes where several pairs of a thread fall away."""
    _check(eng, *_case(n, 2, 2, 3))


def test_n_at_the_capacity_and_one_above(eng):
    from statdepth_amd._native import SD_ERR_UNSUPPORTED, StatdepthHipError
    cap = eng.multi_cloud_lds_capacity()
    _check(eng, *_case(cap, 2, 2, 3), algos=ROUTES + ("auto",))
    P, U, H, O = _case(cap + 1, 2, 2, 3)
    _check(eng, P, U, H, O, algos=("auto", "global"))               # auto takes the global route above the capacity
    for f in (eng.multi_halfspace_sums, eng.multi_projection_sums):
        with pytest.raises(StatdepthHipError) as e:
            f(P, U, algo="lds")
        assert e.value.code == SD_ERR_UNSUPPORTED and str(cap) in str(e.value)


# ---------------------------------------------------------------- dimensions, directions, timepoints
@pytest.mark.parametrize("k", [1, 7])
@pytest.mark.parametrize("d", [1, 2, 3, 8])
def test_dimensions_and_directions(eng, d, k):
    _check(eng, *_case(130, 2, d, k))


def test_directions_across_slices_and_chunks(eng):
    """k = 70: three slices of 32 directions on the LDS route; at the floor one direction per chunk on the global route."""
    P, U, H, O = _case(100, 2, 3, 70)
    _check(eng, P, U, H, O)
    floors = (eng.multi_halfspace_workspace_bytes(100, 2, 3, 70, algo="global")[1],
              eng.multi_projection_workspace_bytes(100, 2, 3, 70, algo="global")[1])
    _check(eng, P, U, H, O, algos=("global",), ws=floors)


@pytest.mark.parametrize("T", [1, 2])
def test_few_timepoints(eng, T):
    _check(eng, *_case(77, T, 3, 5))


def test_more_timepoints_than_a_launch_has_workgroups(eng):
    _check(eng, *_case(64, 700, 2, 3), algos=("lds",))
    P, U, H, O = _case(64, 700, 2, 3)
    _check(eng, P[:, :40], U, algos=("global",))                     # the global route: one launch chain per timepoint


# ---------------------------------------------------------------- workspace independence
@pytest.mark.parametrize("algo", ROUTES)
def test_recommended_floor_and_between_give_identical_records(eng, algo):
    n, T, d, k = 200, 9, 3, 40
    P, U, H, O = _case(n, T, d, k)
    (hr, hf), (pr, pf) = (eng.multi_halfspace_workspace_bytes(n, T, d, k, algo=algo),
                          eng.multi_projection_workspace_bytes(n, T, d, k, algo=algo))
    assert hf < hr and pf < pr
    for frac in (0.0, 0.4, 1.0):                                    # lds: 1, 4 (batches of 4, 4, 1) and 9 timepoints per batch
        ws = (int(hf + frac * (hr - hf)), int(pf + frac * (pr - pf)))
        _check(eng, P, U, H, O, algos=(algo,), ws=ws)
    from statdepth_amd._native import SD_ERR_WORKSPACE, StatdepthHipError
    with pytest.raises(StatdepthHipError) as e:
        eng.multi_halfspace_sums(P, U, algo=algo, ws_bytes=hf - 1)
    assert e.value.code == SD_ERR_WORKSPACE


# ---------------------------------------------------------------- degenerate clouds
def _integer_curves(n, T, d, k, seed):
    rng = np.random.default_rng(seed)
    P = rng.integers(-3, 4, size=(n, T, d)).astype(np.float64)
    U = rng.integers(-2, 3, size=(k, d)).astype(np.float64)
    U[~U.any(axis=1)] = 1.0
    return P, U


def test_integer_coordinates_so_projections_tie(eng):
    P, U = _integer_curves(150, 4, 3, 9, seed=1)
    H = multi_halfspace_records(P, U)
    assert H[:, 1].max() > 1                                         # ties: not every curve is alone on a side somewhere
    _check(eng, P, U, H)


def test_duplicated_curves(eng):
    P, U, _, _ = _case(90, 3, 2, 6)
    P = P.copy()
    P[45:60] = P[:15]
    P[60:70] = P[0]
    H, O = multi_halfspace_records(P, U), multi_projection_records(P, U)
    assert np.array_equal(H[45:60], H[:15]) and np.array_equal(O[60:70], np.repeat(O[:1], 10, axis=0))
    _check(eng, P, U, H, O)


def test_one_timepoint_where_all_points_coincide(eng):
    """MAD = 0 and every numerator 0: O = 0, the term of PS is 1.0; every point is tied with all: h = n."""
    n, T = 70, 3
    P, U, _, _ = _case(n, T, 3, 5)
    Q = P.copy()
    Q[:, 1, :] = [0.5, -2.0, 3.0]
    H, O = multi_halfspace_records(Q, U), multi_projection_records(Q, U)
    one = multi_halfspace_records(Q[:, 1:2], U), multi_projection_records(Q[:, 1:2], U)
    assert (one[0] == n).all() and np.array_equal(one[1], np.tile([1.0, 0.0], (n, 1)))
    _check(eng, Q, U, H, O)
    _check(eng, Q[:, 1:2], U, *one)


def test_collinear_cloud(eng):
    rng = np.random.default_rng(5)
    s = rng.integers(-20, 21, size=(120, 3, 1)).astype(np.float64)
    P = s * np.array([1.0, -2.0, 0.5])                               # every cloud on one line through the origin
    U = np.vstack([make_directions(4, 5, 3), [[2.0, 1.0, 0.0]], [[1.0, 0.0, 0.0]]])     # one direction sees the line as a point
    O = multi_projection_records(P, U)
    _check(eng, P, U, None, O)


def test_one_curve_at_a_million_times_the_scale(eng):
    P, U, _, _ = _case(50, 4, 3, 8)
    P = P.copy()
    P[17] *= 1e6
    H, O = multi_halfspace_records(P, U), multi_projection_records(P, U)
    assert H[17, 1] == 1 and O[17, 1] > 1e5
    _check(eng, P, U, H, O)


# ---------------------------------------------------------------- targets
def test_subset_permutation_and_repeated_targets(eng):
    P, U, H, O = _case(65, 3, 3, 5)
    rng = np.random.default_rng(2)
    for tg in (np.array([64, 3, 17]), rng.permutation(65), np.array([5, 5, 0, 64, 5, 0]), np.array([7])):
        _check(eng, P, U, H, O, targets=tg)
    assert eng.multi_halfspace_sums(P, U, np.array([], dtype=np.int64)).shape == (0, 2)
    with pytest.raises(IndexError):
        eng.multi_projection_sums(P, U, [65])


# ---------------------------------------------------------------- anchors to shipped code
@pytest.mark.parametrize("name", ["halfspace", "projection"])
def test_one_timepoint_is_the_point_cloud_depth(name):
    from statdepth_amd import FunctionalDepth, PointcloudDepth
    P = np.round(np.random.default_rng(11).normal(size=(60, 1, 3)), 1)
    frames = [pd.DataFrame(P[i]) for i in range(60)]
    want = PointcloudDepth(pd.DataFrame(P[:, 0, :]), containment=name, directions=50, seed=3).to_numpy()
    for aggregate in ("mean", "inf"):
        got = FunctionalDepth(frames, containment=name, directions=50, seed=3, aggregate=aggregate).to_numpy()
        assert np.array_equal(got, want), aggregate


def test_one_frame_is_the_integrated_and_the_infimal_halfspace_depth():
    from statdepth_amd import FunctionalDepth
    X = np.round(np.random.default_rng(14).normal(size=(25, 80)), 1)        # T = 25, n = 80, ties in every row
    df = pd.DataFrame(X, columns=[f"c{i}" for i in range(80)])
    for aggregate, k14 in (("mean", "integrated_halfspace"), ("inf", "infimal_halfspace")):
        got = FunctionalDepth([df], containment="halfspace", aggregate=aggregate)
        want = FunctionalDepth([df], containment=k14)
        assert list(got.index) == list(want.index) and np.array_equal(got.to_numpy(), want.to_numpy()), k14


# ---------------------------------------------------------------- the public API
@pytest.mark.parametrize("aggregate", ["mean", "inf"])
@pytest.mark.parametrize("name", ["halfspace", "projection"])
def test_functional_depth(name, aggregate):
    from statdepth_amd import FunctionalDepth
    n, T, d = 40, 12, 3
    P = np.random.default_rng(40).normal(size=(n, T, d))
    P[3] += 4.0                                                      # an outlying curve
    frames = [pd.DataFrame(P[i]) for i in range(n)]
    U = make_directions(30, 7, d)
    R = (multi_halfspace_records if name == "halfspace" else multi_projection_records)(P, U)
    got = FunctionalDepth(frames, containment=name, directions=30, seed=7, aggregate=aggregate)
    assert np.array_equal(got.to_numpy(), depths_from_records(R, n, T, name, aggregate))
    assert list(got.index) == list(range(n))
    if aggregate == "mean":                                          # (the infimum is tied at its floor for most curves)
        assert got.outlying(1).index[0] == 3
    part = FunctionalDepth(frames, to_compute=[3, 0], containment=name, directions=30, seed=7, aggregate=aggregate)
    assert list(part.index) == [3, 0] and np.array_equal(part.to_numpy(), got.to_numpy()[[3, 0]])
