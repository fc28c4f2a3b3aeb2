"""Random projection depths of curves (K23) on the device: the projections bit for bit against the numpy loop, the records
against K14's numpy restatement on the numpy projections, the outlyingness against K12's, both against the shipped d <= 8
point-cloud kernels, the API, and the caller-memory contract of the three compute entry points.

Every comparison is exact (np.array_equal, the projections as uint64 views): the definition fixes every rounding, so the
shapes are the smallest that reach every path of the tile kernel -- one value, a full tile (16 x 128 x 64), one past it and
one short of it in every dimension, several tiles with tails, many panels -- and of the two routes of the stage it feeds."""
import functools

import numpy as np
import pandas as pd
import pytest

import workspace_contract
from statdepth_amd import CurveProjections, FunctionalDepth, PointcloudDepth, _native
from statdepth_amd.depth.calculations._pointcloud import _halfspace_directions
from test_projection_host import locscale, outlyingness
from test_rank_depths_host import records_np
from workspace_contract import POISONS, ContractProxy, Memory

pytestmark = pytest.mark.gpu

SHAPES = [(1, 2, 1), (16, 128, 64), (17, 129, 65), (15, 127, 63), (37, 300, 70), (1000, 257, 3)]
KINDS = ['gaussian', 'tenths', 'signed_zeros', 'subnormal', 'big_x_small_u', 'small_x_big_u']
BIG_N = (3, 16390, 2)                                    # above the image route: auto takes the sort route


@pytest.fixture(scope='module')
def eng():
    from statdepth_amd import engine
    return engine


# ---------------------------------------------------------------------------------------------------- data and references
def projections_np(X, U):
    """The definition: z = X[0] * u[0]; for t in 1 .. T-1: z = z + X[t] * u[t], per direction, every operation rounded."""
    Z = np.empty((U.shape[0], X.shape[1]), dtype=np.float64)
    with np.errstate(under='ignore'):
        for r, u in enumerate(U):
            z = X[0] * u[0]
            for t in range(1, X.shape[0]):
                z = z + X[t] * u[t]
            Z[r] = z
    return Z


@functools.lru_cache(maxsize=None)
def case(shape, kind):
    """(X [T, n], U [k, T], Z [k, n]) of a shape and a kind of data; computed once, never written to."""
    T, n, k = shape
    rng = np.random.default_rng([T, n, k, KINDS.index(kind)])
    X = rng.normal(size=(T, n))
    U = rng.normal(size=(k, T))
    if kind == 'tenths':
        X, U = np.round(X, 1), np.round(U, 1)            # exact zeros and ties among the sums
        U[~U.any(axis=1)] = 0.1
    elif kind == 'signed_zeros':
        X = np.round(X, 1)
        X[:, 0] = -0.0                                   # every term -0.0 * u: the sum keeps the sign of its first terms
        X[:, n - 1] = 0.0
        U[0] = -np.abs(U[0])                             # (-0.0) * (-u) = +0.0, (+0.0) * (-u) = -0.0
        if k > 1:
            U[k - 1] = np.abs(U[k - 1])
    elif kind == 'subnormal':
        few = np.round(X[::3] * 16.0)
        few[few == 0.0] = 1.0
        X = X * 2.0 ** -1060                             # subnormal entries: every product rounds in the subnormal range
        X[::3] = few * 2.0 ** -1074                      # ... and some of a few units in the last place
    elif kind == 'big_x_small_u':
        X = np.clip(X / 4.0, -1.0, 1.0) * 2.0 ** 500
        U = np.clip(U / 4.0, -1.0, 1.0) * 2.0 ** -500
        X[0, 0], U[0, 0] = 2.0 ** 500, 2.0 ** -500
    elif kind == 'small_x_big_u':
        X = np.clip(X / 4.0, -1.0, 1.0) * 2.0 ** -500
        U = np.clip(U / 4.0, -1.0, 1.0) * 2.0 ** 500
        X[0, 0], U[0, 0] = -2.0 ** -500, 2.0 ** 500
    for A in (X, U):
        A.setflags(write=False)
    Z = projections_np(X, U)
    Z.setflags(write=False)
    return X, U, Z


@functools.lru_cache(maxsize=None)
def depth_case(shape, majority=False):
    """Data for the records and the outlyingness: values on a grid of tenths, a few curves duplicated (ties in every
    direction); majority: more than half the curves are one curve (a MAD of 0 in every direction).  With K14's and K12's
    references on the numpy projections."""
    T, n, k = shape
    rng = np.random.default_rng([T, n, k, 23])
    X = np.round(rng.normal(size=(T, n)), 1)
    U = rng.normal(size=(k, T))
    if majority:
        same = rng.permutation(n)[:n // 2 + 1]
        X[:, same] = X[:, same[:1]]
    else:
        for j in range(0, n - 1, 7):
            X[:, j + 1] = X[:, j]
    Z = projections_np(X, U)
    O = np.zeros(n)
    for z in Z:
        med, mad = locscale(z)
        O = np.maximum(O, outlyingness(z, med, mad))
    out = (X, U, Z, records_np(Z), O)
    for A in out:
        A.setflags(write=False)
    return out


def target_lists(n):
    rng = np.random.default_rng(n)
    return [None, np.sort(rng.permutation(n)[:max(1, n // 3)]), rng.permutation(n), np.array([n - 1, 0, n - 1, n // 2, 0, n - 1])]


def three_sizes(sizes):
    rec, floor = sizes
    assert 0 < floor <= rec
    return [floor, (floor + rec) // 2 // 8 * 8 if rec - floor >= 16 else rec, rec]


def bits(A):
    return np.ascontiguousarray(A, dtype=np.float64).view(np.uint64)


# ---------------------------------------------------------------------------------------------------- 1. projections
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_projections_bit_for_bit(eng, shape, kind):
    X, U, Z = case(shape, kind)
    assert np.isfinite(Z).all()
    time_major = eng.curve_projections(np.ascontiguousarray(X), U)
    curve_major = eng.curve_projections(np.asfortranarray(X), U)
    assert time_major.shape == Z.shape and time_major.dtype == np.float64
    assert np.array_equal(bits(time_major), bits(curve_major)), 'the two layouts of one X differ'
    assert np.array_equal(bits(time_major), bits(Z)), 'differs from the numpy loop'


def test_the_signed_zero_data_has_both_zeros():
    """The case is what it claims: sums that are -0.0 and sums that are +0.0, in the reference itself."""
    X, U, Z = case((17, 129, 65), 'signed_zeros')
    assert (Z[0, 0] == 0.0 and not np.signbit(Z[0, 0])) and (Z[0, 128] == 0.0 and np.signbit(Z[0, 128]))
    assert np.signbit(Z[64, 0]) and not np.signbit(Z[64, 128])
    assert (case((37, 300, 70), 'subnormal')[0] != 0).all() and np.abs(case((37, 300, 70), 'subnormal')[0]).max() < 2.0 ** -1022


# ---------------------------------------------------------------------------------------------------- 2. records
@pytest.mark.parametrize('shape', SHAPES + [BIG_N], ids=str)
def test_records_equal_k14_on_the_numpy_projections(eng, shape):
    X, U, Z, R, _ = depth_case(shape)
    T, n, k = shape
    assert (np.sort(Z, axis=1)[:, 1:] == np.sort(Z, axis=1)[:, :-1]).any(axis=1).all() or n == 2, 'ties in every direction'
    algos = ('auto', 'image', 'sort') if n <= 16384 else ('auto', 'sort')
    lists = target_lists(n)
    for algo in algos:
        sizes = eng.rp_depth_workspace_bytes(T, n, k, algo)
        for i, ws in enumerate(three_sizes(sizes)):
            for tg in (lists if i == 0 else lists[:2]):
                got = eng.rp_depth_sums(X, U, tg, algo=algo, ws_bytes=ws)
                want = R if tg is None else R[tg]
                assert got.dtype == np.int64 and np.array_equal(got, want), (algo, ws, sizes, tg)
        assert np.array_equal(eng.rp_depth_sums(np.asfortranarray(X), U, lists[1], algo=algo), R[lists[1]]), algo
    if n > 16384:
        assert eng.rp_depth_workspace_bytes(T, n, k, 'auto') == eng.rp_depth_workspace_bytes(T, n, k, 'sort')
        with pytest.raises(_native.StatdepthHipError) as e:
            eng.rp_depth_sums(X, U, algo='image')
        assert e.value.code == _native.SD_ERR_UNSUPPORTED


def test_records_below_the_floor_are_refused(eng):
    X, U, _, _, _ = depth_case((37, 300, 70))
    for algo in ('image', 'sort'):
        with pytest.raises(_native.StatdepthHipError) as e:
            eng.rp_depth_sums(X, U, algo=algo, ws_bytes=eng.rp_depth_workspace_bytes(37, 300, 70, algo)[1] - 8)
        assert e.value.code == _native.SD_ERR_WORKSPACE


# ---------------------------------------------------------------------------------------------------- 3. outlyingness
@pytest.mark.parametrize('majority', [False, True], ids=['ties', 'majority'])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_outlyingness_equals_k12_on_the_numpy_projections(eng, shape, majority):
    X, U, Z, _, O = depth_case(shape, majority)
    T, n, k = shape
    if majority and n > 2:
        assert np.isinf(O).any() and (O == 0.0).sum() >= n // 2 + 1
    lists = target_lists(n)
    for i, ws in enumerate(three_sizes(eng.rp_outlyingness_workspace_bytes(T, n, k))):
        for tg in (lists if i == 0 else lists[:2]):
            got = eng.rp_outlyingness(X, U, tg, ws_bytes=ws)
            assert np.array_equal(bits(got), bits(O if tg is None else O[tg])), (ws, tg)
    assert np.array_equal(bits(eng.rp_outlyingness(np.asfortranarray(X), U)), bits(O))
    with pytest.raises(_native.StatdepthHipError) as e:
        eng.rp_outlyingness(X, U, ws_bytes=eng.rp_outlyingness_workspace_bytes(T, n, k)[1] - 8)
    assert e.value.code == _native.SD_ERR_WORKSPACE


# ---------------------------------------------------------------------------------------------------- 4. the d <= 8 kernels
@functools.lru_cache(maxsize=None)
def cloud(d, n=300):
    rng = np.random.default_rng([d, n])
    P = np.round(rng.normal(size=(n, d)), 1)             # ties
    U = np.array([[1.0], [-1.0], [0.5]]) if d == 1 else _halfspace_directions(64, d, d)
    return P, U


@pytest.mark.parametrize('d', [1, 2, 5, 8])
def test_short_curves_are_the_point_cloud_kernels(eng, d):
    P, U = cloud(d)
    n = len(P)
    X = np.ascontiguousarray(P.T)
    tg = np.array([5, 0, n - 1, 5])
    assert np.array_equal(n - eng.rp_depth_sums(X, U)[:, 4], eng.halfspace_counts(P, U))
    assert np.array_equal(n - eng.rp_depth_sums(P.T, U, tg, algo='sort')[:, 4], eng.halfspace_counts(P, U, tg))
    assert np.array_equal(bits(eng.rp_outlyingness(X, U)), bits(eng.projection_outlyingness(P, U)))
    assert np.array_equal(bits(eng.rp_outlyingness(P.T, U, tg)), bits(eng.projection_outlyingness(P, U, tg)))
    df = pd.DataFrame(P, index=[f'p{i}' for i in range(n)])
    for curves, points in (('random_tukey', 'halfspace'), ('rp_projection', 'projection')):
        a = FunctionalDepth([df.T], containment=curves, directions=U)
        b = PointcloudDepth(df, containment=points, directions=U)
        assert list(a.index) == list(b.index) == list(df.index)
        assert np.array_equal(bits(a.to_numpy()), bits(b.to_numpy())), (curves, points)


def test_nine_features(eng):
    P, U = cloud(9)
    df = pd.DataFrame(P)
    Z = projections_np(np.ascontiguousarray(P.T), U)
    R = records_np(Z)
    for points in ('halfspace', 'projection'):
        with pytest.raises(NotImplementedError):
            PointcloudDepth(df, containment=points, directions=U)
    got = FunctionalDepth([df.T], containment='random_tukey', directions=U)
    assert np.array_equal(got.to_numpy(), (len(P) - R[:, 4]) / np.float64(len(P)))
    O = np.zeros(len(P))
    for z in Z:
        med, mad = locscale(z)
        O = np.maximum(O, outlyingness(z, med, mad))
    got = FunctionalDepth([df.T], containment='rp_projection', directions=U)
    assert np.array_equal(bits(got.to_numpy()), bits(1.0 / (1.0 + O)))


# ---------------------------------------------------------------------------------------------------- 5. API
NAMES = ('rp_halfspace', 'rp_fm', 'random_tukey', 'rp_projection')


@pytest.fixture(scope='module')
def frame():
    X = depth_case((37, 300, 70))[0][:, :40]
    return pd.DataFrame(np.array(X), columns=[f'c{i}' for i in range(40)])


@pytest.mark.parametrize('name', NAMES)
def test_labels_order_and_seed(frame, name):
    full = FunctionalDepth([frame], containment=name, directions=50, seed=3)
    assert list(full.index) == list(frame.columns) and full.to_numpy().dtype == np.float64
    assert ((full.to_numpy() >= 0.0) & (full.to_numpy() <= 1.0)).all()
    pick = ['c7', 'c0', 'c39', 'c7']
    part = FunctionalDepth([frame], containment=name, directions=50, seed=3, to_compute=pick)
    assert list(part.index) == pick
    assert np.array_equal(part.to_numpy(), full.to_numpy()[[7, 0, 39, 7]])
    again = FunctionalDepth([frame], containment=name, directions=50, seed=3)
    other = FunctionalDepth([frame], containment=name, directions=50, seed=4)
    assert np.array_equal(again.to_numpy(), full.to_numpy()) and not np.array_equal(other.to_numpy(), full.to_numpy())
    fortran = pd.DataFrame(np.asfortranarray(frame.to_numpy()), columns=frame.columns)
    assert np.array_equal(FunctionalDepth([fortran], containment=name, directions=50, seed=3).to_numpy(), full.to_numpy())
    with pytest.raises(KeyError):
        FunctionalDepth([frame], containment=name, to_compute=['nope'])
    with pytest.raises(ValueError, match='unique'):
        FunctionalDepth([frame.rename(columns={'c1': 'c0'})], containment=name)


def test_depths_are_the_normalised_records(frame):
    X = frame.to_numpy()
    T, n = X.shape
    U = _halfspace_directions(50, 3, T)
    Z = projections_np(X, U)
    R = records_np(Z)
    nk = np.int64(n * 50)
    want = {'rp_halfspace': (nk - R[:, 3]) / np.float64(nk), 'rp_fm': (2 * nk - R[:, 2]) / np.float64(2 * nk),
            'random_tukey': (n - R[:, 4]) / np.float64(n)}
    for name, w in want.items():
        assert np.array_equal(FunctionalDepth([frame], containment=name, directions=50, seed=3).to_numpy(), w), name
    tukey = np.array([[min((z <= v).sum(), (z >= v).sum()) / n for v in z] for z in Z])      # the definition, no records
    assert np.max(np.abs(want['rp_halfspace'] - tukey.mean(0))) <= 1e-14      # a mean of 50 proportions, summed in fp64
    assert np.array_equal(want['random_tukey'], tukey.min(0))


def test_curve_projections_frame(frame):
    U = _halfspace_directions(9, 1, frame.shape[0])
    for got in (CurveProjections(frame, directions=9, seed=1), CurveProjections([frame], directions=U)):
        assert isinstance(got, pd.DataFrame) and got.shape == (9, 40) and list(got.columns) == list(frame.columns)
        assert np.array_equal(bits(got.to_numpy()), bits(projections_np(frame.to_numpy(), U)))


# ---------------------------------------------------------------------------------------------------- 6. caller memory
ROWS = {
    'sd_curve_projections': [(7, lambda a: a[6] * a[2] * 8)],                    # X T n st sn U k out
    'sd_rp_depth_sums': [(10, lambda a: a[8] * 40)],                             # X T n st sn U k targets m algo out
    'sd_rp_outlyingness': [(9, lambda a: a[8] * 8)],                             # X T n st sn U k targets m out
}


@pytest.fixture
def contract(monkeypatch, eng):
    """with contract(poison): the engine runs behind the contract proxy, the three entry points in its tables for the
    duration of the test."""
    import contextlib
    for name, rows in ROWS.items():
        monkeypatch.setitem(workspace_contract.OUTPUTS, name, rows)
        monkeypatch.setitem(_native.SIGNATURES, name, _native.PROJECTION_SIGNATURES[name])
        assert workspace_contract.takes_stream(name) and workspace_contract.takes_workspace(name)

    @contextlib.contextmanager
    def use(poison, ws_word=None):
        real = eng._lib()
        proxy = ContractProxy(real, Memory(eng._device(None), real), poison=poison, ws_word=ws_word)
        with monkeypatch.context() as m:
            m.setattr(_native, '_LIB', proxy)
            yield proxy
    return use


@pytest.mark.parametrize('shape', [(17, 129, 65), (37, 300, 70)], ids=str)
def test_caller_memory_contract(eng, contract, shape):
    X, U, Z, R, O = depth_case(shape)
    T, n, k = shape
    tg = target_lists(n)[1]
    runs = {'sd_curve_projections': [(lambda X=X_: eng.curve_projections(X, U), Z) for X_ in (X, np.asfortranarray(X))]}
    runs['sd_rp_depth_sums'] = [(lambda algo=algo, ws=ws: eng.rp_depth_sums(X, U, tg, algo=algo, ws_bytes=ws), R[tg])
                                for algo in ('image', 'sort') for ws in three_sizes(eng.rp_depth_workspace_bytes(T, n, k, algo))]
    runs['sd_rp_outlyingness'] = [(lambda ws=ws: eng.rp_outlyingness(X, U, tg, ws_bytes=ws), O[tg])
                                  for ws in three_sizes(eng.rp_outlyingness_workspace_bytes(T, n, k))]
    for name, cases in runs.items():
        for run, want in cases:
            plain = run()
            assert np.array_equal(bits(plain) if plain.dtype == np.float64 else plain, bits(want) if want.dtype == np.float64 else want)
            for poison, word in [(p, None) for p in POISONS] + [(0xA5, 4)]:
                with contract(poison, ws_word=word) as proxy:
                    got = run()
                assert proxy.called[name] == 1 and proxy.guarded_outputs[name] == 1, name
                assert proxy.guarded_workspaces[name] == (0 if name == 'sd_curve_projections' else 1), name
                assert got.dtype == plain.dtype and np.array_equal(got, plain, equal_nan=False), (name, hex(poison), word)
