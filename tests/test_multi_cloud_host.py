"""Halfspace and projection depth of multivariate curves over time (containment='halfspace' / 'projection' of
FunctionalDepth, K18), the part that needs no GPU: the numpy restatement of the records against a hand-computed case, the
normalisation, every refusal of the host layer with the engine never reached, the handling of `aggregate`, `directions` and
`seed`, the one-frame form, the result types, and the C ABI's declarations, sizes and refusals.

The restatement (`multi_halfspace_records`, `multi_projection_records`, `depths_from_records`) is a loop over the
timepoints around the restatements of K10 and K12 (tests/test_halfspace_host.py, tests/test_projection_host.py); it is
imported by tests/test_multi_cloud_gpu.py as its oracle.  Every operation in it is one numpy operation on int64 or fp64.
"""
import os
import re

import numpy as np
import pandas as pd
import pytest

from statdepth_amd import FunctionalDepth, engine
from statdepth_amd.depth.calculations import _containment
from statdepth_amd.depth.calculations._functional import _cloud_depth_values
from statdepth_amd.depth.depth import _FunctionalDepthSeries, _FunctionalDepthUnivariate
from statdepth_amd.homogeneity import FunctionalHomogeneity

from test_halfspace_host import halfspace_counts, halfspace_counts_sorted, make_directions
from test_projection_host import projection_outlyingness
from test_rank_depths_host import records_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('halfspace', 'projection')


# ---------------------------------------------------------------- numpy restatement of the definition
def _targets(targets, n):
    return np.arange(n) if targets is None else np.asarray(targets, dtype=np.int64)


def multi_halfspace_records(P, U, targets=None):
    """int64 [m, 2] = (SH, MH): sum and minimum over t of K10's count of the curve's point inside the cloud at t."""
    P = np.asarray(P, dtype=np.float64)
    n, T, d = P.shape
    counts = halfspace_counts if n <= 128 else halfspace_counts_sorted     # the same integers (test_halfspace_host)
    H = np.stack([counts(P[:, t, :], U) for t in range(T)]).astype(np.int64)
    return np.stack([H.sum(axis=0), H.min(axis=0)], axis=1)[_targets(targets, n)]


def multi_projection_records(P, U, targets=None):
    """fp64 [m, 2] = (PS, OM): PS the sum over t of 1 / (1 + O_t) added in ascending t from 0.0, one rounded addition per
    timepoint; OM the maximum over t of K12's outlyingness O_t of the curve's point inside the cloud at t."""
    P = np.asarray(P, dtype=np.float64)
    n, T, d = P.shape
    O = np.stack([projection_outlyingness(P[:, t, :], U) for t in range(T)])
    ps = np.zeros(n, dtype=np.float64)
    for t in range(T):                                                     # sequential: the order of np.cumsum
        ps = ps + 1.0 / (1.0 + O[t])
    return np.stack([ps, O.max(axis=0)], axis=1)[_targets(targets, n)]


def depths_from_records(R, n, T, name, aggregate):
    """The host's normalisation, written out once more."""
    R = np.asarray(R)
    if name == 'halfspace':
        return (R[:, 0].astype(np.float64) / np.float64(n * T)) if aggregate == 'mean' else R[:, 1].astype(np.float64) / np.float64(n)
    return R[:, 0] / np.float64(T) if aggregate == 'mean' else 1.0 / (1.0 + R[:, 1])


RECORDS = {'halfspace': multi_halfspace_records, 'projection': multi_projection_records}
ENGINE_FN = {'halfspace': 'multi_halfspace_sums', 'projection': 'multi_projection_sums'}

# three curves A, B, C in the plane at two timepoints; the coordinate axes as directions
#   t0: A (0,0)  B (1,2)  C (2,1)      t1: A (1,1)  B (1,1)  C (5,0)
KNOWN_P = np.array([[[0.0, 0.0], [1.0, 1.0]], [[1.0, 2.0], [1.0, 1.0]], [[2.0, 1.0], [5.0, 0.0]]])
KNOWN_U = np.eye(2)
# t0: every point is extreme on one axis: h = 1.  t1: A = B share both projections (le = 2 or 3, ge = 3 or 2), C is alone
KNOWN_H = np.array([[3, 1], [3, 1], [2, 1]], dtype=np.int64)
# t0: med = 1, MAD = 1 on both axes: O = 1 for all.  t1: MAD = 0 on both axes: O = 0 on the median (A, B), inf off it (C)
KNOWN_O = np.array([[1.5, 1.0], [1.5, 1.0], [0.5, np.inf]])
KNOWN_DEPTHS = {('halfspace', 'mean'): [3 / 6, 3 / 6, 2 / 6], ('halfspace', 'inf'): [1 / 3, 1 / 3, 1 / 3],
                ('projection', 'mean'): [0.75, 0.75, 0.25], ('projection', 'inf'): [0.5, 0.5, 0.0]}


def _frames(P):
    return [pd.DataFrame(P[i]) for i in range(P.shape[0])]


def _curves(n=6, T=5, d=3, seed=1):
    return np.random.default_rng(seed).normal(size=(n, T, d))


@pytest.fixture
def restated(monkeypatch):
    """The engine's two functions replaced by the restatement; `calls` records (name, P, U, targets) of every call."""
    calls = []

    def fake(name):
        def f(P, U, targets=None, device=None, algo='auto', ws_bytes=None):
            calls.append((name, np.array(P), np.array(U), None if targets is None else np.array(targets)))
            return RECORDS[name](P, U, targets)
        return f
    for name in NAMES:
        monkeypatch.setattr(engine, ENGINE_FN[name], fake(name))
    return calls


@pytest.fixture
def no_engine(monkeypatch):
    def boom(*a, **k):
        raise AssertionError('the engine was reached')
    for name in NAMES:
        monkeypatch.setattr(engine, ENGINE_FN[name], boom)
    monkeypatch.setattr(engine, '_upload', boom)


# ---------------------------------------------------------------- names
def test_names_and_the_other_tuples_keep_their_contents():
    assert _containment.CLOUD_DEPTHS == NAMES
    assert _containment._is_cloud_depth('halfspace') and _containment._is_cloud_depth('projection')
    assert not _containment._is_cloud_depth('r2') and not _containment._is_cloud_depth(lambda data, curve, relax: 0.0)
    assert _containment.RANK_DEPTHS == ('fm', 'mei', 'mhi', 'half_region', 'integrated_halfspace', 'infimal_halfspace')
    assert _containment.ORDER_DEPTHS == ('extremal',) and _containment.SHAPE_DEPTHS == ('tvd', 'mss')


def test_unknown_containment_lists_the_new_names():
    with pytest.raises(ValueError) as e:
        FunctionalDepth(_frames(_curves()), containment='tukey')
    for name in NAMES + ('r2', 'fm', 'tvd', 'extremal'):
        assert f"'{name}'" in str(e.value)


# ---------------------------------------------------------------- the restatement and the normalisation, by hand
def test_known_answer_records_restated():
    assert np.array_equal(multi_halfspace_records(KNOWN_P, KNOWN_U), KNOWN_H)
    assert np.array_equal(multi_projection_records(KNOWN_P, KNOWN_U), KNOWN_O)
    assert np.array_equal(multi_halfspace_records(KNOWN_P, KNOWN_U, [2, 2, 0]), KNOWN_H[[2, 2, 0]])
    assert np.array_equal(multi_projection_records(KNOWN_P, KNOWN_U, [1]), KNOWN_O[[1]])


@pytest.mark.parametrize('name,aggregate', sorted(KNOWN_DEPTHS))
def test_known_answer_normalisation(name, aggregate):
    R = KNOWN_H if name == 'halfspace' else KNOWN_O
    got = _cloud_depth_values(R, 3, 2, name, aggregate)
    assert got.dtype == np.float64 and got.shape == (3,)
    assert np.array_equal(got, np.array(KNOWN_DEPTHS[(name, aggregate)]))
    assert np.array_equal(got, depths_from_records(R, 3, 2, name, aggregate))


@pytest.mark.parametrize('name,aggregate', sorted(KNOWN_DEPTHS))
def test_known_answer_through_the_public_call(name, aggregate, restated):
    d = FunctionalDepth(_frames(KNOWN_P), containment=name, directions=KNOWN_U, aggregate=aggregate)
    assert np.array_equal(d.to_numpy(), np.array(KNOWN_DEPTHS[(name, aggregate)]))
    assert len(restated) == 1 and restated[0][0] == name
    assert np.array_equal(restated[0][1], KNOWN_P) and np.array_equal(restated[0][2], KNOWN_U)


def test_projection_sum_is_added_in_ascending_t():
    """The order matters in the last bit, which is why it is part of the definition: a sum where it shows."""
    O = np.array([2.0 ** -60, 1.0, 1.0, 3.0])
    terms = 1.0 / (1.0 + O)
    fwd = np.cumsum(terms)[-1]
    ps = 0.0
    for v in terms:
        ps = ps + v
    assert ps == fwd
    P = np.zeros((3, 4, 1))
    P[0, :, 0], P[2, :, 0] = -1.0, 1.0                               # med = 0, MAD = 1 at every t: O = |x|
    P[1, :, 0] = 0.0
    R = multi_projection_records(P, [[1.0]])
    assert np.array_equal(R[:, 0], [2.0, 4.0, 2.0]) and np.array_equal(R[:, 1], [1.0, 0.0, 1.0])


# ---------------------------------------------------------------- refusals: ValueError that names the containment
@pytest.mark.parametrize('name', NAMES)
def test_refuses_K(name, no_engine):
    with pytest.raises(ValueError, match=name):
        FunctionalDepth(_frames(_curves()), K=2, containment=name)
    with pytest.raises(ValueError, match=name):
        FunctionalDepth([pd.DataFrame(_curves()[:, :, 0].T)], K=2, containment=name)


@pytest.mark.parametrize('name', NAMES)
def test_refuses_other_J(name, no_engine):
    for J in (3, np.int64(4), True, 2.0):
        with pytest.raises(ValueError, match=name):
            FunctionalDepth(_frames(_curves()), J=J, containment=name)


@pytest.mark.parametrize('name', NAMES)
def test_refuses_frames_of_unequal_shape(name, no_engine):
    fr = _frames(_curves())
    fr[3] = fr[3].iloc[:-1]
    with pytest.raises(ValueError, match=name):
        FunctionalDepth(fr, containment=name)
    fr = _frames(_curves())
    fr[0] = fr[0].iloc[:, :2]
    with pytest.raises(ValueError, match=name):
        FunctionalDepth(fr, containment=name)


@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('bad', [np.nan, np.inf, -np.inf])
def test_refuses_nan_and_inf(name, bad, no_engine):
    P = _curves()
    P[4, 2, 1] = bad
    with pytest.raises(ValueError, match=name):
        FunctionalDepth(_frames(P), containment=name)
    X = _curves()[:, :, 0].T.copy()
    X[1, 2] = bad
    with pytest.raises(ValueError, match=name):
        FunctionalDepth([pd.DataFrame(X)], containment=name)


def test_projection_refuses_magnitudes_above_2_500(no_engine):
    P = _curves()
    P[0, 0, 0] = 2.0 ** 501
    with pytest.raises(ValueError, match='projection'):
        FunctionalDepth(_frames(P), containment='projection')
    U = np.eye(3)
    U[0, 0] = 2.0 ** 501
    with pytest.raises(ValueError, match='projection'):
        FunctionalDepth(_frames(_curves()), containment='projection', directions=U)


@pytest.mark.parametrize('name', NAMES)
def test_refuses_fewer_than_two_curves(name, no_engine):
    with pytest.raises(ValueError, match=name):
        FunctionalDepth([pd.DataFrame(np.arange(5.0)[:, None])], containment=name)


@pytest.mark.parametrize('name', NAMES)
def test_refuses_no_timepoint(name, no_engine):
    with pytest.raises(ValueError, match=name):
        FunctionalDepth([pd.DataFrame(np.zeros((0, 3))) for _ in range(4)], containment=name)
    with pytest.raises(ValueError, match=name):
        FunctionalDepth([pd.DataFrame(np.zeros((0, 4)))], containment=name)


@pytest.mark.parametrize('name', NAMES)
def test_refuses_more_than_eight_features(name, no_engine):
    with pytest.raises(ValueError, match=name):
        FunctionalDepth(_frames(_curves(d=9)), containment=name)


@pytest.mark.parametrize('name', NAMES)
def test_refuses_homogeneity(name, no_engine):
    with pytest.raises(ValueError, match=name):
        FunctionalHomogeneity(_frames(_curves(seed=1)), _frames(_curves(seed=2)), containment=name, relax=True)


def test_refuses_duplicate_labels_in_the_one_frame_form(no_engine):
    df = pd.DataFrame(_curves()[:, :, 0].T)
    df.columns = ['a', 'b', 'a', 'c', 'd', 'e']
    with pytest.raises(ValueError, match='unique'):
        FunctionalDepth([df], containment='halfspace')


# ---------------------------------------------------------------- aggregate, directions, seed
@pytest.mark.parametrize('name', NAMES)
def test_aggregate_takes_mean_or_inf_only(name, no_engine):
    for bad in ('max', 'min', None, 1, 'Mean'):
        with pytest.raises(ValueError, match=name):
            FunctionalDepth(_frames(_curves()), containment=name, aggregate=bad)


@pytest.mark.parametrize('name', NAMES)
def test_aggregates_come_from_one_record(name, restated):
    P = _curves(7, 4, 2, seed=5)
    mean = FunctionalDepth(_frames(P), containment=name, directions=11, seed=3)
    inf = FunctionalDepth(_frames(P), containment=name, directions=11, seed=3, aggregate='inf')
    U = make_directions(11, 3, 2)
    R = RECORDS[name](P, U)
    assert np.array_equal(mean.to_numpy(), depths_from_records(R, 7, 4, name, 'mean'))
    assert np.array_equal(inf.to_numpy(), depths_from_records(R, 7, 4, name, 'inf'))
    assert (inf.to_numpy() <= mean.to_numpy()).all()
    assert all(np.array_equal(c[2], U) for c in restated) and len(restated) == 2


@pytest.mark.parametrize('name', NAMES)
def test_directions_and_seed_mean_what_they_mean_for_point_clouds(name, restated):
    P = _curves(5, 3, 3)
    FunctionalDepth(_frames(P), containment=name)                                       # the defaults: 1000, seed 0
    FunctionalDepth(_frames(P), containment=name, directions=7, seed=42)
    given = np.array([[1.0, 0.0, 0.0], [0.0, 2.0, -1.0]])
    FunctionalDepth(_frames(P), containment=name, directions=given, seed=9)
    assert np.array_equal(restated[0][2], make_directions(1000, 0, 3))
    assert np.array_equal(restated[1][2], make_directions(7, 42, 3))
    assert np.array_equal(restated[2][2], given)


@pytest.mark.parametrize('name', NAMES)
def test_bad_directions_are_refused(name, no_engine):
    fr = _frames(_curves())
    for bad in (0, -3, np.zeros((2, 3)), np.ones((2, 2)), [[np.nan, 1.0, 0.0]], 'all'):
        with pytest.raises(ValueError):
            FunctionalDepth(fr, containment=name, directions=bad)
    with pytest.raises(NotImplementedError, match='exact'):
        FunctionalDepth(fr, containment=name, directions='exact')
    with pytest.raises(NotImplementedError, match='exact'):
        FunctionalDepth(_frames(_curves(d=2)), containment=name, directions='exact')


@pytest.mark.parametrize('name', NAMES)
def test_exact_is_accepted_for_one_feature(name, restated):
    P = _curves(5, 4, 1)
    a = FunctionalDepth(_frames(P), containment=name, directions='exact')
    b = FunctionalDepth([pd.DataFrame(P[:, :, 0].T)], containment=name, directions='exact')
    assert np.array_equal(a.to_numpy(), b.to_numpy())
    assert all(np.array_equal(c[2], [[1.0]]) for c in restated)


def test_other_containments_ignore_the_three_arguments(monkeypatch):
    seen = []
    monkeypatch.setattr(engine, 'rank_depth_sums', lambda X, targets=None, **k: (seen.append(1), records_np(np.asarray(X))[targets])[1])
    df = pd.DataFrame(_curves()[:, :, 0].T)
    a = FunctionalDepth([df], containment='fm')
    b = FunctionalDepth([df], containment='fm', directions='nonsense', seed='x', aggregate='whatever')
    assert np.array_equal(a.to_numpy(), b.to_numpy()) and len(seen) == 2


@pytest.mark.parametrize('name', NAMES)
def test_relax_and_algo_are_ignored(name, restated):
    fr = _frames(_curves())
    a = FunctionalDepth(fr, containment=name, directions=5)
    b = FunctionalDepth(fr, containment=name, directions=5, relax=True, algo='rank')
    assert np.array_equal(a.to_numpy(), b.to_numpy())


# ---------------------------------------------------------------- the two forms: types, indices, targets
@pytest.mark.parametrize('name', NAMES)
def test_multivariate_form_is_indexed_by_list_position(name, restated):
    P = _curves(6, 5, 3)
    full = FunctionalDepth(_frames(P), containment=name, directions=9)
    assert type(full) is _FunctionalDepthSeries and list(full.index) == list(range(6))
    assert restated[-1][1].shape == (6, 5, 3) and list(restated[-1][3]) == list(range(6))
    part = FunctionalDepth(_frames(P), to_compute=[4, 1, 1], containment=name, directions=9)
    assert list(part.index) == [4, 1, 1] and list(restated[-1][3]) == [4, 1, 1]
    assert np.array_equal(part.to_numpy(), full.to_numpy()[[4, 1, 1]])
    assert list(full.deepest(1).index) == [int(np.argmax(full.to_numpy()))]


@pytest.mark.parametrize('name', NAMES)
def test_one_frame_form_takes_the_columns_as_curves(name, restated):
    X = np.round(np.random.default_rng(8).normal(size=(6, 5)), 1)            # T = 6 timepoints, n = 5 curves, ties
    df = pd.DataFrame(X, columns=list('abcde'))
    full = FunctionalDepth([df], containment=name)
    assert type(full) is _FunctionalDepthUnivariate and list(full.index) == list('abcde')
    nm, P, U, tg = restated[-1]
    assert P.shape == (5, 6, 1) and np.array_equal(P[:, :, 0], X.T) and np.array_equal(U, [[1.0]]) and list(tg) == [0, 1, 2, 3, 4]
    part = FunctionalDepth([df], to_compute=['d', 'a'], containment=name, aggregate='inf')
    assert list(part.index) == ['d', 'a'] and list(restated[-1][3]) == [3, 0]
    with pytest.raises(KeyError):
        FunctionalDepth([df], to_compute=['z'], containment=name)
    assert full.get_deepest_data(1).shape == (6, 1)


def test_one_frame_halfspace_is_the_integrated_and_the_infimal_halfspace_depth(restated):
    """min(#<=, #>=) = n - max(A, B): the same integers as K14's records, so the same doubles."""
    from statdepth_amd.depth.calculations._rank import _rank_depth_values
    X = np.round(np.random.default_rng(3).normal(size=(7, 9)), 1)
    df = pd.DataFrame(X)
    R = records_np(X)
    mean = FunctionalDepth([df], containment='halfspace')
    inf = FunctionalDepth([df], containment='halfspace', aggregate='inf')
    assert np.array_equal(mean.to_numpy(), _rank_depth_values(R, 9, 7, 'integrated_halfspace'))
    assert np.array_equal(inf.to_numpy(), _rank_depth_values(R, 9, 7, 'infimal_halfspace'))


# ---------------------------------------------------------------- engine arguments (no device)
def test_engine_refuses_an_unknown_algo():
    with pytest.raises(ValueError, match='algo'):
        engine.multi_halfspace_workspace_bytes(10, 3, 2, 5, algo='sort')
    with pytest.raises(ValueError, match='algo'):
        engine.multi_projection_workspace_bytes(10, 3, 2, 5, algo='pairwise')


# ---------------------------------------------------------------- the C ABI is declared and bound
NEW = [('sd_multi_cloud_lds_capacity', 'int64_t', 0),
       ('sd_multi_halfspace_workspace_bytes', 'size_t', 6), ('sd_multi_halfspace_min_workspace_bytes', 'size_t', 6),
       ('sd_multi_halfspace_sums', 'int', 13),
       ('sd_multi_projection_workspace_bytes', 'size_t', 6), ('sd_multi_projection_min_workspace_bytes', 'size_t', 6),
       ('sd_multi_projection_sums', 'int', 13)]


@pytest.mark.parametrize('fn,res,count', NEW)
def test_header_and_signatures_carry_the_entry_points(fn, res, count):
    from statdepth_amd import _native
    src = open(os.path.join(ROOT, 'include', 'statdepth_hip.h')).read()
    decl = re.search(r'\b%s\s+%s\s*\(([^;]*)\)\s*;' % (res, fn), src)
    assert decl, f'{fn} is not declared in statdepth_hip.h'
    params = [p for p in decl.group(1).split(',') if p.strip() != 'void']
    got_res, args = _native.SIGNATURES[fn]
    assert len(params) == count and len(args) == count
    assert got_res is {'size_t': _native._sz, 'int': _native._int, 'int64_t': _native._i64}[res]


def test_header_exports_equal_the_signatures():
    from statdepth_amd import _native
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'statdepth_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(sd_\w+)\s*\(', src))
    assert declared == set(_native.SIGNATURES)
    assert {fn for fn, _, _ in NEW} <= declared


def test_signatures_of_the_sums():
    """P, n, T, d, U, k, targets, m, algo, out, ws, ws_bytes, stream."""
    from statdepth_amd import _native as nv
    src = open(os.path.join(ROOT, 'include', 'statdepth_hip.h')).read()
    for fn in ('sd_multi_halfspace_sums', 'sd_multi_projection_sums'):
        res, args = nv.SIGNATURES[fn]
        assert res is nv._int
        assert args == [nv._vp, nv._i64, nv._i64, nv._int, nv._vp, nv._i64, nv._vp, nv._i64, nv._int, nv._vp, nv._vp, nv._sz, nv._vp]
        decl = re.search(r'int %s\(([^;]*)\);' % fn, src).group(1)
        names = [p.split()[-1].lstrip('*') for p in decl.split(',')]
        assert names == ['P', 'n', 'T', 'd', 'U', 'k', 'targets', 'm', 'algo', 'out', 'ws', 'ws_bytes', 'stream']
    assert nv.SIGNATURES['sd_multi_halfspace_workspace_bytes'][1] == [nv._i64, nv._i64, nv._int, nv._i64, nv._i64, nv._int]


@pytest.fixture(scope='module')
def native():
    from statdepth_amd import _native
    return _native, _native.load()


def test_the_capacity_holds_benchmark_config_4(native):
    nv, lib = native
    assert lib.sd_multi_cloud_lds_capacity() >= 5000
    assert engine.multi_cloud_lds_capacity() == lib.sd_multi_cloud_lds_capacity()


@pytest.mark.parametrize('fn', ['sd_multi_halfspace_sums', 'sd_multi_projection_sums'])
def test_abi_refusals_come_before_any_device_work(native, fn):
    nv, lib = native
    cap = lib.sd_multi_cloud_lds_capacity()
    order = ('P', 'n', 'T', 'd', 'U', 'k', 'targets', 'm', 'algo', 'out', 'ws', 'ws_bytes', 'stream')
    base = dict(P=1, n=10, T=4, d=3, U=1, k=5, targets=None, m=10, algo=0, out=1, ws=None, ws_bytes=0, stream=None)
    call = lambda **k: getattr(lib, fn)(*[{**base, **k}[a] for a in order])          # noqa: E731
    assert call(P=None) == nv.SD_ERR_INVALID and call(U=None) == nv.SD_ERR_INVALID and call(out=None) == nv.SD_ERR_INVALID
    for zero in ('n', 'T', 'd', 'k'):
        assert call(**{zero: 0}) == nv.SD_ERR_INVALID, zero
    assert call(algo=3) == nv.SD_ERR_INVALID and call(algo=-1) == nv.SD_ERR_INVALID
    assert call(m=4) == nv.SD_ERR_INVALID and b'targets=NULL' in lib.sd_last_error()
    assert call(d=9) == nv.SD_ERR_UNSUPPORTED and b'[1,8]' in lib.sd_last_error()
    assert call(n=1 << 31, m=1 << 31) == nv.SD_ERR_UNSUPPORTED and b'2^31' in lib.sd_last_error()
    assert call(n=10 ** 6, m=10 ** 6, T=10 ** 4, k=10 ** 3) == nv.SD_ERR_UNSUPPORTED and b'cap' in lib.sd_last_error()
    # the LDS route above its capacity is refused, nothing is launched
    assert call(n=cap + 1, m=cap + 1, algo=1) == nv.SD_ERR_UNSUPPORTED and str(cap).encode() in lib.sd_last_error()
    assert call() == nv.SD_ERR_WORKSPACE                            # a valid shape, no workspace
    floor = getattr(lib, fn.replace('_sums', '_min_workspace_bytes'))(10, 4, 3, 5, 10, 0)
    assert call(ws=256, ws_bytes=floor - 1) == nv.SD_ERR_WORKSPACE


@pytest.mark.parametrize('family,vbytes', [('halfspace', 4), ('projection', 8)])
def test_workspace_sizes(family, vbytes):
    size = getattr(engine, f'multi_{family}_workspace_bytes')
    point = getattr(engine, f'{family}_workspace_bytes')
    cap = engine.multi_cloud_lds_capacity()
    up = lambda x: -(-x // 256) * 256                              # noqa: E731
    for n, T, d, k in [(2, 1, 1, 1), (65, 3, 3, 5), (1000, 1000, 3, 64), (5000, 500, 8, 1000), (cap, 2, 2, 3)]:
        rec, floor = size(n, T, d, k, algo='lds')
        per = n * (8 * d + vbytes)                                  # the feature-major copy and every curve's value
        assert floor == 512 + per and rec == 512 + min(T, max(1, (1 << 25) // (n * d))) * per
        assert size(n, T, d, k, algo='auto') == (rec, floor)        # auto: the LDS route up to the capacity
        grec, gfloor = size(n, T, d, k, algo='global')
        prec, pfloor = point(n, d, k)
        fixed = up(8 * n * d) + up(8 * n) + 256                     # the cloud and the values in front of K10's / K12's
        assert (grec, gfloor) == (fixed + prec, fixed + pfloor)
    assert size(5000, 500, 8, 1000)[0] == 512 + 500 * 5000 * (64 + vbytes)            # config 4 is one batch
    assert size(cap + 1, 2, 2, 3, algo='lds') == (0, 0)
    assert size(cap + 1, 2, 2, 3, algo='auto') == size(cap + 1, 2, 2, 3, algo='global') != (0, 0)
    assert size(10, 0, 2, 3) == (0, 0) and size(10, 2, 9, 3) == (0, 0) and size(0, 2, 2, 3) == (0, 0)
