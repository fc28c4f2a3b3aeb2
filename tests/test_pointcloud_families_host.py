"""The family table of the point-cloud depths (_pointcloud._FAMILIES) without a GPU: for every family and every form (rows of
the sample, K-blocks, external points) the engine function the table names is the one reached -- and the only one --, and
the depths are its output put through the family's normaliser as written out here, with N = n, the block lengths and n + 1.
The engine functions are fakes that record their arguments and return fixed numbers; the Oja hull is the real one.  Beside
it the two helpers the drivers share: the -1 padded member matrix and the band-depth sum."""
import numpy as np
import pandas as pd
import pytest
from scipy.spatial import ConvexHull
from scipy.special import binom

from statdepth_amd import engine
from statdepth_amd.depth.calculations._helper import _band_depth_sum, _padded_members
from statdepth_amd.depth.calculations._pointcloud import _block_depths, _halfspace_directions, _pointwisedepth
from statdepth_amd.homogeneity.homogeneity import _external_point_depths

N, D = 9, 2
P = np.array([[i, i * i] for i in range(N)], dtype=np.float64)       # on a parabola: no three points on a line
Q = np.array([[1.0, 5.0], [20.0, 3.0]])
BLOCKS = [[4, 7, 2], [0, 8, 5, 3], [3, 1, 4, 2, 8, 6, 7, 5, 0]]      # ragged: 3, 4 and 9 members, the target last
INTS = np.array([3, 0, 7, 2, 5, 1, 4, 6, 2], dtype=np.int64)
FLOATS = np.array([0.5, 1.25, 3.0, 0.125, 2.0, 7.5, 0.75, 1.0, 4.0])

# containment (and kind) -> (rows, blocks, external) engine function, the directions argument, float output?, the normaliser
TABLE = {
    'simplex': ('pointcloud_simplex_counts', 'pointcloud_simplex_subset_counts', 'pointcloud_simplex_external_counts',
                None, False, lambda raw, n, vols: raw.astype(np.float64) / binom(n, D + 1)),
    'simplex_exact': ('simplicial_exact_counts', 'simplicial_exact_subset_counts', 'simplicial_exact_external_counts',
                      None, False, lambda raw, n, vols: raw.astype(np.float64) / binom(n, 3)),
    'l1': ('l1_depth', 'l1_subset_depth', 'l1_external_depth', None, True, lambda raw, n, vols: raw),
    'oja': ('oja_volume_sums', 'oja_subset_volume_sums', 'oja_external_volume_sums',
            None, True, lambda raw, n, vols: raw / vols),
    'halfspace': ('halfspace_counts', 'halfspace_subset_counts', 'halfspace_external_counts',
                  5, False, lambda raw, n, vols: raw.astype(np.float64) / n),
    'halfspace-exact': ('halfspace_exact_counts', 'halfspace_exact_subset_counts', None,
                        'exact', False, lambda raw, n, vols: raw.astype(np.float64) / n),
    'projection': ('projection_outlyingness', 'projection_subset_outlyingness', 'projection_external_outlyingness',
                   5, True, lambda raw, n, vols: 1.0 / (1.0 + raw)),
}
ENGINE_NAMES = [name for row in TABLE.values() for name in row[:3] if name is not None]
CASES = [(key, form) for key in TABLE for form in range(3) if TABLE[key][form] is not None]


@pytest.fixture
def calls(monkeypatch):
    """Every engine function the table names becomes a fake that records (name, args) and returns the first len-many
    fixed numbers; `calls.out` is set by the test."""
    class Calls(list):
        out = None
    rec = Calls()
    for name in ENGINE_NAMES:
        def fake(*args, _name=name, **kw):
            rec.append((_name, args))
            return rec.out.copy()
        monkeypatch.setattr(engine, name, fake)
    return rec


def _hulls(samples):
    return np.array([ConvexHull(S).volume for S in samples], dtype=np.float64)


@pytest.mark.parametrize('key,form', CASES, ids=[f'{k}-{("rows", "blocks", "external")[f]}' for k, f in CASES])
def test_each_form_reaches_its_engine_function_and_normaliser(calls, key, form):
    names, directions, floats, normalise = TABLE[key][:3], *TABLE[key][3:]
    containment = key.split('-')[0]
    frame = pd.DataFrame(P, index=[f'p{i}' for i in range(N)])
    if form == 0:
        calls.out = (FLOATS if floats else INTS)[:N]
        got = _pointwisedepth(frame, containment=containment, directions=directions, seed=1).to_numpy()
        want = normalise(calls.out, N, _hulls([P]))
        U = None if directions in (None, 'exact') else _halfspace_directions(5, 1, D)
        selector = np.arange(N)
    elif form == 1:
        calls.out = (FLOATS if floats else INTS)[:len(BLOCKS)]
        U = None if directions in (None, 'exact') else _halfspace_directions(5, 1, D)
        got = _block_depths(P, BLOCKS, containment, directions=U)
        want = normalise(calls.out, np.array([3.0, 4.0, 9.0]), _hulls([P[b] for b in BLOCKS]))
        selector = None
    else:
        calls.out = (FLOATS if floats else INTS)[:len(Q)]
        got = _external_point_depths(frame, pd.DataFrame(Q), None, containment)
        want = normalise(calls.out, N + 1, _hulls([np.vstack([P, q]) for q in Q]))
        U = None if directions is None else _halfspace_directions(1000, 0, D)      # PointcloudDepth's defaults
        selector = Q
    assert [name for name, _ in calls] == [names[form]]                           # that function, once, and no other
    assert np.array_equal(got, want)
    args = calls[0][1]
    assert np.array_equal(args[0], P)
    if U is not None:
        assert np.array_equal(args[1 if form == 0 else 2], U)
    else:
        assert len(args) == 2
    sel = args[2 if form == 0 and U is not None else 1]
    if form != 1:
        assert np.array_equal(sel, selector)
    else:                                                 # the members: the block in its order, target last, -1 only at the end
        assert sel.dtype == np.int32 and sel.shape == (len(BLOCKS), 9)
        for row, b in zip(sel, BLOCKS):
            assert list(row[:len(b)]) == b and row[len(b) - 1] == b[-1]
            assert (row[len(b):] == -1).all() and (row[:len(b)] >= 0).all()


def test_padded_members_ragged_and_equal():
    mem = _padded_members([[4, 7, 2], np.array([0, 8, 5, 3]), (1,)])
    assert mem.dtype == np.int32
    assert np.array_equal(mem, [[4, 7, 2, -1], [0, 8, 5, 3], [1, -1, -1, -1]])
    same = _padded_members([[1, 2], [3, 0]])
    assert same.dtype == np.int32 and np.array_equal(same, [[1, 2], [3, 0]])


@pytest.mark.parametrize('J', [2, 3, 4])
@pytest.mark.parametrize('n', [11, np.array([5.0, 7.0, 11.0, 6.0])], ids=['int', 'array'])
def test_band_depth_sum_is_the_written_out_loop(J, n):
    counts = np.random.default_rng(J).integers(0, 50, size=(4, J - 1)).astype(np.float64) / 7
    want = np.zeros(4)
    for j in range(2, J + 1):
        want += counts[:, j - 2] / binom(n, j)
    got = _band_depth_sum(counts, n, J)
    assert got.dtype == np.float64 and np.array_equal(got, want)
