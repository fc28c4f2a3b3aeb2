"""The three forms of a point-cloud depth tied to each other at the depth layer, normalisers included, for all seven
families: (a) PointcloudDepth of a row, (b) _block_depths on the one block `others + [t]`, (c) _external_point_depths of
the row against the cloud without it.  test_point_selection_gpu.py ties the engine functions below the normalisers.
Counting families and projection (bit-specified kernels, test_projection_gpu.py) must agree exactly; L1 and Oja to the
1e-12 test_point_selection_gpu.py gives these two kernels across forms."""
import numpy as np
import pandas as pd
import pytest

from conftest import assert_depths_close

pytestmark = pytest.mark.gpu
TOL = 1e-12
N = 10
TARGETS = (0, 4, 9)
FAMILIES = [   # id, containment, compared exactly, has a direction set, has an external form
    ('simplex', 'simplex', True, False, True),
    ('simplex_exact', 'simplex_exact', True, False, True),
    ('l1', 'l1', False, False, True),
    ('oja', 'oja', False, False, True),
    ('halfspace', 'halfspace', True, True, True),
    ('halfspace-exact', 'halfspace', True, False, False),
    ('projection', 'projection', True, True, True),
]


def _cloud():
    """n = 10 distinct integer points of the 7 x 7 grid around the origin."""
    cells = np.random.default_rng(7).choice(49, size=N, replace=False)
    return np.stack([cells // 7 - 3, cells % 7 - 3], axis=1).astype(np.float64)


def _agree(exact, got, want, what):
    if exact:
        assert np.array_equal(np.asarray(got), np.asarray(want)), (what, got, want)
    else:
        assert_depths_close(got, want, TOL)


@pytest.mark.parametrize('name,containment,exact,directed,external', FAMILIES, ids=[f[0] for f in FAMILIES])
def test_rows_blocks_and_external_give_one_depth(name, containment, exact, directed, external):
    from statdepth_amd import PointcloudDepth
    from statdepth_amd.depth.calculations._pointcloud import _block_depths, _halfspace_directions
    from statdepth_amd.homogeneity.homogeneity import _external_point_depths
    P = _cloud()
    assert len({tuple(p) for p in P}) == N
    frame = pd.DataFrame(P)

    def rows_and_block(t, directions, seed):
        a = PointcloudDepth(frame, to_compute=[t], containment=containment, directions=directions, seed=seed).to_numpy()
        U = _halfspace_directions(directions, seed, 2) if directed else None
        b = _block_depths(P, [[i for i in range(N) if i != t] + [t]], containment, directions=U)
        return a, b

    for t in TARGETS:
        a, b = rows_and_block(t, 'exact' if name == 'halfspace-exact' else 5, 1)
        assert a.shape == (1,) and np.isfinite(a).all()
        _agree(exact, b, a, (name, t, 'blocks'))
        if not external:
            continue
        if directed:                                     # the external form has PointcloudDepth's default directions
            a, b = rows_and_block(t, 1000, 0)
            _agree(exact, b, a, (name, t, 'blocks, default directions'))
        c = _external_point_depths(frame.drop(index=t), frame.iloc[[t]], None, containment)
        _agree(exact, c, a, (name, t, 'external'))
