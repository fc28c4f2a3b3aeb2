"""Random projection depths of curves (K23), the part that needs no GPU: the companion header against the second signature
table and both libraries, the size functions and every refusal of the C entry points (called with fake pointers: a refusal
comes before any device work), the refusals of the host layer (before any upload), the four normalisations and the
direction set."""
import ctypes
import os
import re

import numpy as np
import pandas as pd
import pytest

from statdepth_amd import CurveProjections, FunctionalDepth, _native, engine
from statdepth_amd.depth.calculations import _functional
from statdepth_amd.depth.calculations._containment import PROJECTED_DEPTHS, _is_projected_depth, _is_valid_containment
from statdepth_amd.depth.calculations._pointcloud import _halfspace_directions
from statdepth_amd.depth.calculations._rank import _projected_depth_values

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('rp_halfspace', 'rp_fm', 'random_tukey', 'rp_projection')
COMPUTE = ('sd_curve_projections', 'sd_rp_depth_sums', 'sd_rp_outlyingness')
BIG = 1 << 31
FAKE = 4096                                              # a non-null "device pointer" that no refusal may touch


@pytest.fixture(scope='module')
def lib():
    return _native.load()


def _declared():
    src = open(os.path.join(ROOT, 'include', 'statdepth_hip_projections.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(sd_[a-z0-9_]+)\s*\(', src)))


# ---- the ABI ----
def test_companion_header_is_the_second_table():
    assert _declared() == sorted(_native.PROJECTION_SIGNATURES)
    assert not set(_native.PROJECTION_SIGNATURES) & set(_native.SIGNATURES)
    assert all(name in _native.PROJECTION_SIGNATURES for name in COMPUTE)


def test_both_libraries_export_and_bind_the_table(lib):
    for path in (_native.LIB_PATH, _native.XCHECK_LIB_PATH):
        raw = ctypes.CDLL(path)
        for name in _native.PROJECTION_SIGNATURES:
            assert hasattr(raw, name), (path, name)
    bound = _native.open_library(_native.XCHECK_LIB_PATH)
    for name, (res, args) in _native.PROJECTION_SIGNATURES.items():
        for l in (lib, bound):
            assert getattr(l, name).restype is res and getattr(l, name).argtypes == args, name


def test_abi_version_is_still_1(lib):
    assert lib.sd_abi_version() == 1
    assert '#define SD_ABI_VERSION 1' in open(os.path.join(ROOT, 'include', 'statdepth_hip.h')).read()


# ---- size functions ----
def _sizes(lib, family, T, n, k, algo=None, st=None, sn=1):
    tail = (n,) if algo is None else (n, algo)
    st = n if st is None else st
    return (getattr(lib, f'sd_{family}_workspace_bytes')(T, n, st, sn, k, *tail),
            getattr(lib, f'sd_{family}_min_workspace_bytes')(T, n, st, sn, k, *tail))


def test_projections_need_no_workspace(lib):
    for T, n, k in ((1, 2, 1), (1000, 257, 3), (16, 100000, 64)):
        assert lib.sd_curve_projections_workspace_bytes(T, n, n, 1, k) == 0
        assert lib.sd_curve_projections_workspace_bytes(T, n, 1, T, k) == 0
        assert engine.curve_projections_workspace_bytes(T, n, k) == (0, 0)


@pytest.mark.parametrize('family,algo', [('rp_depth', 0), ('rp_depth', 1), ('rp_depth', 2), ('rp_outlyingness', None)])
def test_sizes_floor_below_recommended_and_monotone(lib, family, algo):
    last = None
    for n in (2, 127, 300, 4096, 16384):
        row = []
        for k in (1, 2, 63, 64, 65, 1000):
            rec, floor = _sizes(lib, family, 37, n, k, algo)
            assert 0 < floor <= rec, (n, k, rec, floor)
            assert (rec, floor) == _sizes(lib, family, 37, n, k, algo, st=1, sn=37), 'neither layout takes a copy'
            row.append((rec, floor))
        assert all(a[0] <= b[0] and a[1] <= b[1] for a, b in zip(row, row[1:])), ('monotone in k', n, row)
        if last is not None:
            assert all(a[0] <= b[0] and a[1] <= b[1] for a, b in zip(last, row)), ('monotone in n', n)
        last = row


def test_sizes_hold_z_and_the_stage_it_feeds(lib):
    T, n, k = 50, 300, 70
    for algo in (0, 1, 2):
        rec, floor = _sizes(lib, 'rp_depth', T, n, k, algo)
        assert rec >= k * n * 8 + lib.sd_rank_depth_min_workspace_bytes(k, n, n, 1, n, algo)
        assert floor >= n * 8 + lib.sd_rank_depth_min_workspace_bytes(1, n, n, 1, n, algo)
        assert (rec, floor) == engine.rp_depth_workspace_bytes(T, n, k, algo)
    rec, floor = _sizes(lib, 'rp_outlyingness', T, n, k)
    assert floor >= 32 * n and rec >= k * 32 * n
    assert (rec, floor) == engine.rp_outlyingness_workspace_bytes(T, n, k)
    big = 16390                                          # above the image route: auto is the sort route
    assert _sizes(lib, 'rp_depth', 3, big, 2, 0) == _sizes(lib, 'rp_depth', 3, big, 2, 2)


def test_sizes_are_0_for_what_the_calls_refuse(lib):
    for T, n, k in ((0, 10, 3), (5, 1, 3), (5, 10, 0), (BIG, 10, 3), (5, BIG, 3), (5, 10, BIG)):
        assert _sizes(lib, 'rp_depth', T, n, k, 0) == (0, 0)
        assert _sizes(lib, 'rp_outlyingness', T, n, k) == (0, 0)
    assert _sizes(lib, 'rp_depth', 5, 10, 3, 3) == (0, 0)
    assert _sizes(lib, 'rp_depth', 5, 16385, 3, 1) == (0, 0)


# ---- refusals of the C entry points: the code, a message, no device work (the pointers are fake) ----
def _call(lib, name, X=FAKE, T=5, n=10, st=None, sn=1, U=FAKE, k=3, targets=None, m=None, algo=0, out=FAKE, ws=FAKE,
          ws_bytes=1 << 40):
    st = n if st is None else st
    m = n if m is None else m
    head = (X, T, n, st, sn, U, k)
    if name == 'sd_curve_projections':
        return lib.sd_curve_projections(*head, out, ws, ws_bytes, None)
    if name == 'sd_rp_depth_sums':
        return lib.sd_rp_depth_sums(*head, targets, m, algo, out, ws, ws_bytes, None)
    return lib.sd_rp_outlyingness(*head, targets, m, out, ws, ws_bytes, None)


def _refused(lib, code, name, **kw):
    lib.sd_mbd_counts(None, 10, 10, 10, 1, None, 10, 2, 0, None, None, 0, None)      # leaves another message behind
    before = lib.sd_last_error()
    assert _call(lib, name, **kw) == code, (name, kw, lib.sd_last_error())
    msg = lib.sd_last_error()
    assert msg and msg != before, (name, kw)
    return msg


@pytest.mark.parametrize('name', COMPUTE)
def test_invalid_arguments(lib, name):
    for null in ('X', 'U', 'out'):
        assert b'null' in _refused(lib, _native.SD_ERR_INVALID, name, **{null: None})
    _refused(lib, _native.SD_ERR_INVALID, name, T=0)
    _refused(lib, _native.SD_ERR_INVALID, name, k=0)
    _refused(lib, _native.SD_ERR_INVALID, name, n=0)
    assert b'time-major' in _refused(lib, _native.SD_ERR_INVALID, name, st=3, sn=7)
    if name != 'sd_curve_projections':
        _refused(lib, _native.SD_ERR_INVALID, name, n=1)
        _refused(lib, _native.SD_ERR_INVALID, name, targets=None, m=4)
        _refused(lib, _native.SD_ERR_INVALID, name, targets=FAKE, m=-1)


def test_unknown_algo(lib):
    for algo in (-1, 3):
        assert b'algo' in _refused(lib, _native.SD_ERR_INVALID, 'sd_rp_depth_sums', algo=algo)


@pytest.mark.parametrize('name', COMPUTE)
def test_unsupported_shapes(lib, name):
    assert b'2^31' in _refused(lib, _native.SD_ERR_UNSUPPORTED, name, n=BIG)
    assert b'2^31' in _refused(lib, _native.SD_ERR_UNSUPPORTED, name, T=BIG, n=2)
    assert b'2^31' in _refused(lib, _native.SD_ERR_UNSUPPORTED, name, k=BIG, n=2)
    # 10^14 multiply-adds and comparisons: just above the cap, every factor below 2^31
    assert b'cap' in _refused(lib, _native.SD_ERR_UNSUPPORTED, name, T=100000, n=1000000, k=1001)
    if name == 'sd_curve_projections':                   # 10^14 exactly is within the cap: the next refusal is not this one
        assert _call(lib, name, T=100000, n=1000000, k=1000, st=3, sn=7) == _native.SD_ERR_INVALID


def test_image_route_above_its_capacity(lib):
    assert b'16384' in _refused(lib, _native.SD_ERR_UNSUPPORTED, 'sd_rp_depth_sums', n=16385, algo=1)
    assert _call(lib, 'sd_rp_depth_sums', n=16384, algo=1, ws_bytes=8) == _native.SD_ERR_WORKSPACE


@pytest.mark.parametrize('name,family', [('sd_rp_depth_sums', 'rp_depth'), ('sd_rp_outlyingness', 'rp_outlyingness')])
def test_workspace_below_the_floor(lib, name, family):
    T, n, k = 5, 300, 7
    for algo in ((0, 1, 2) if family == 'rp_depth' else (None,)):
        floor = _sizes(lib, family, T, n, k, algo)[1]
        kw = {} if algo is None else {'algo': algo}
        assert b'min_workspace_bytes' in _refused(lib, _native.SD_ERR_WORKSPACE, name, T=T, n=n, k=k, ws_bytes=floor - 1, **kw)
        _refused(lib, _native.SD_ERR_WORKSPACE, name, T=T, n=n, k=k, ws_bytes=0, **kw)
        _refused(lib, _native.SD_ERR_WORKSPACE, name, T=T, n=n, k=k, ws=None, **kw)
    # no targets, nothing to do: not even a workspace is asked for
    assert _call(lib, name, T=T, n=n, k=k, targets=FAKE, m=0, ws=None, ws_bytes=0) == _native.SD_OK


# ---- the host layer ----
def test_names():
    assert tuple(PROJECTED_DEPTHS) == NAMES
    assert all(_is_projected_depth(name) for name in NAMES) and not _is_projected_depth('fm') and not _is_projected_depth(None)


def test_invalid_containment_names_the_tuple():
    with pytest.raises(ValueError) as e:
        _is_valid_containment('nonsense')
    for name in NAMES + ('fm', 'lens', 'halfspace'):
        assert repr(name) in str(e.value)


@pytest.fixture
def no_upload(monkeypatch):
    def boom(*a, **k):
        raise AssertionError('the engine was reached')
    for fn in ('rp_depth_sums', 'rp_outlyingness', 'curve_projections', 'to_device_matrix', '_upload', '_lib'):
        monkeypatch.setattr(engine, fn, boom)


def _frame(T=6, n=5, seed=3):
    return pd.DataFrame(np.random.default_rng(seed).normal(size=(T, n)), columns=[f'c{i}' for i in range(n)])


def _with(df, value):
    df = df.copy()
    df.iloc[2, 1] = value
    return df


@pytest.mark.parametrize('name', NAMES)
def test_host_refusals_of_the_data(name, no_upload):
    with pytest.raises(ValueError, match=name):
        FunctionalDepth([_frame(6, 2, s) for s in range(4)], containment=name)
    with pytest.raises(ValueError, match='NaN'):
        FunctionalDepth([_with(_frame(), np.nan)], containment=name)
    for bad in (np.inf, -np.inf):
        with pytest.raises(ValueError, match='infinite'):
            FunctionalDepth([_with(_frame(), bad)], containment=name)
    for bad in (2.0 ** 501, -2.0 ** 501):
        with pytest.raises(ValueError, match=r'2\^500'):
            FunctionalDepth([_with(_frame(), bad)], containment=name)
    with pytest.raises(ValueError, match='at least 2 curves'):
        FunctionalDepth([_frame(6, 1)], containment=name)
    with pytest.raises(ValueError, match='unique'):
        FunctionalDepth([pd.DataFrame(np.ones((3, 3)), columns=['a', 'b', 'a'])], containment=name)
    with pytest.raises(ValueError, match='K must be None'):
        FunctionalDepth([_frame()], containment=name, K=2)


@pytest.mark.parametrize('name', NAMES)
def test_host_refusals_of_the_directions(name, no_upload):
    df = _frame(6, 5)
    with pytest.raises(ValueError, match=r'k x 6'):
        FunctionalDepth([df], containment=name, directions=np.ones((3, 5)))
    for bad in (np.nan, np.inf):
        U = np.ones((3, 6))
        U[1, 2] = bad
        with pytest.raises(ValueError, match='finite'):
            FunctionalDepth([df], containment=name, directions=U)
    U = np.ones((3, 6))
    U[2] = 0.0
    with pytest.raises(ValueError, match='all-zero'):
        FunctionalDepth([df], containment=name, directions=U)
    U = np.ones((3, 6))
    U[0, 0] = 2.0 ** 501
    with pytest.raises(ValueError, match=r'2\^500'):
        FunctionalDepth([df], containment=name, directions=U)
    with pytest.raises(NotImplementedError, match='exact'):
        FunctionalDepth([df], containment=name, directions='exact')
    with pytest.raises(ValueError, match='directions'):
        FunctionalDepth([df], containment=name, directions='some')
    with pytest.raises(ValueError, match='positive'):
        FunctionalDepth([df], containment=name, directions=0)


@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('J', [3, 1, 2.0, True])
def test_host_refuses_a_band_size(name, J, no_upload):
    with pytest.raises(ValueError, match='J must be left at its default 2'):
        FunctionalDepth([_frame()], containment=name, J=J)


def test_curve_projections_refusals(no_upload):
    with pytest.raises(ValueError, match='CurveProjections'):
        CurveProjections([_frame(), _frame()])
    with pytest.raises(ValueError, match='infinite'):
        CurveProjections(_with(_frame(), np.inf))
    with pytest.raises(ValueError, match=r'k x 6'):
        CurveProjections(_frame(), directions=np.ones((2, 7)))


def test_an_int_is_the_seeded_direction_set(monkeypatch):
    """`directions=k` hands engine the rows of _halfspace_directions(k, seed, T), unit vectors of R^T."""
    seen = {}

    def fake(X, U, targets=None, device=None, **kw):
        seen['U'], seen['X'], seen['targets'] = np.array(U), np.array(X), np.array(targets)
        return np.zeros((len(targets), 5), dtype=np.int64)
    monkeypatch.setattr(engine, 'rp_depth_sums', fake)
    df = _frame(9, 5)
    for k, seed in ((4, 0), (17, 5)):
        FunctionalDepth([df], containment='random_tukey', directions=k, seed=seed, to_compute=['c3', 'c0'])
        want = _halfspace_directions(k, seed, 9)
        assert want.shape == (k, 9) and np.array_equal(seen['U'], want)
        assert np.allclose(np.linalg.norm(seen['U'], axis=1), 1.0)
        assert np.array_equal(seen['targets'], [3, 0]) and np.array_equal(seen['X'], df.to_numpy())
    FunctionalDepth([df], containment='random_tukey', directions=4, seed=1)
    assert not np.array_equal(seen['U'], _halfspace_directions(4, 0, 9))
    given = np.arange(18.0).reshape(2, 9) + 1.0
    FunctionalDepth([df], containment='rp_fm', directions=given, relax=True, algo='rank', aggregate='inf', quantile=0.5,
                    bandwidth=1.0, beta=3.0)             # ignored, as the rank depths ignore them
    assert np.array_equal(seen['U'], given)


# ---- the normalisations: integers up to one division, the division last ----
RECORDS = np.array([[0, 0, 0, 0, 0], [12, 9, 30, 14, 5], [3, 40, 77, 40, 6], [41, 1, 70, 41, 6], [7, 7, 1, 9, 3]], dtype=np.int64)


def test_normalisations_from_records():
    n, k = 7, 6
    SF, SM, MM = RECORDS[:, 2], RECORDS[:, 3], RECORDS[:, 4]
    nk = np.int64(n * k)
    got = {name: _projected_depth_values(RECORDS, n, k, name) for name in NAMES[:3]}
    assert all(v.dtype == np.float64 and v.shape == (5,) for v in got.values())
    assert np.array_equal(got['rp_halfspace'], (nk - SM).astype(np.float64) / np.float64(nk))
    assert np.array_equal(got['rp_fm'], (2 * nk - SF).astype(np.float64) / np.float64(2 * nk))      # = 1 - SF / (2 n k)
    assert np.max(np.abs(got['rp_fm'] - (1.0 - SF / (2.0 * n * k)))) <= 2.0 ** -52
    assert np.array_equal(got['random_tukey'], (np.int64(n) - MM).astype(np.float64) / np.float64(n))
    assert got['rp_halfspace'][0] == 1.0 and got['rp_fm'][0] == 1.0 and got['random_tukey'][0] == 1.0


def test_normalisation_of_the_outlyingness():
    O = np.array([0.0, 1.0, 0.5, 3.0, np.inf, 2.0 ** -1074])
    got = _projected_depth_values(O, 7, 6, 'rp_projection')
    assert np.array_equal(got, 1.0 / (1.0 + O))
    assert np.array_equal(got, [1.0, 0.5, 1.0 / 1.5, 0.25, 0.0, 1.0])
    with pytest.raises(ValueError, match='fm'):
        _projected_depth_values(RECORDS, 7, 6, 'fm')


def test_layer_constants():
    assert _functional.PROJECTED_MAX_T == 2 ** 23
