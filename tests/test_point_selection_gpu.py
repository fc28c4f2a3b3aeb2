"""The three forms of a point-cloud depth (rows of P, external points, blocks of rows: DESIGN.md, "Point clouds: the
three forms") tied to each other on the GPU for the five families that share one selector: K4 simplex, K5 L1, K7 Oja,
K10 halfspace (pairwise entry points) and K11 exact halfspace (both routes).  Integer families must agree exactly; L1
and Oja to the 1e-12 that test_hip_parity.py and test_oja_gpu.py allow these kernels (no summation order is promised
across forms).  The repeated row constrains L1 least: a target with a coincident other has depth NaN (the reference's
0/0) in every form, so for targets 2 and 5 only the NaN's position is compared; the other targets, which see the
repeated pair among their others, are compared in value."""
import numpy as np
import pytest

from conftest import assert_depths_close

pytestmark = pytest.mark.gpu
TOL = 1e-12
N = 8
DUP = (2, 5)                                                         # row 5 repeats row 2


@pytest.fixture(scope="module")
def eng():
    from statdepth_amd import engine
    return engine


def _cloud(d):
    """n = 8 integer points, distinct but for the one repeated row."""
    rng = np.random.default_rng(40 + d)
    P = rng.integers(-3, 4, size=(N, d)).astype(np.float64)
    P[:, 0] = rng.permutation(N) - 3.0
    P[DUP[1]] = P[DUP[0]]
    return P


def _directions(d):
    U = np.random.default_rng(50 + d).integers(-2, 3, size=(5, d)).astype(np.float64)
    U[0] = 0.0
    U[0, 0] = 1.0
    U[np.all(U == 0.0, axis=1)] = 1.0
    return U


class Family:
    """(rows, external, blocks) of one family as functions of (P, targets | Q | members); `empty`: an empty block's value."""

    def __init__(self, name, rows, external, blocks, exact, empty):
        self.name, self.rows, self.external, self.blocks, self.exact, self.empty = name, rows, external, blocks, exact, empty

    def check(self, got, want):
        if self.exact:
            assert np.array_equal(np.asarray(got), np.asarray(want)), (self.name, got, want)
        else:
            assert_depths_close(got, want, TOL)


def _families(eng, d):
    U = _directions(d)
    fams = [
        Family("simplex", eng.pointcloud_simplex_counts, eng.pointcloud_simplex_external_counts,
               eng.pointcloud_simplex_subset_counts, True, 0),
        Family("l1", eng.l1_depth, eng.l1_external_depth, eng.l1_subset_depth, False, np.nan),
        Family("oja", eng.oja_volume_sums, eng.oja_external_volume_sums, eng.oja_subset_volume_sums, False, 0.0),
        Family("halfspace", lambda P, t: eng.halfspace_counts(P, U, t, algo="pairwise"),
               lambda P, Q: eng.halfspace_external_counts(P, Q, U), lambda P, M: eng.halfspace_subset_counts(P, M, U), True, 0),
    ]
    if d == 2:
        for algo in ("sweep", "pairwise"):
            fams.append(Family("exact-" + algo, lambda P, t, a=algo: eng.halfspace_exact_counts(P, t, algo=a),
                               lambda P, Q, a=algo: eng.halfspace_exact_external_counts(P, Q, algo=a),
                               lambda P, M, a=algo: eng.halfspace_exact_subset_counts(P, M, algo=a), True, 0))
    return fams


def _members(blocks, width):
    M = np.full((len(blocks), width), -1, dtype=np.int32)
    for r, b in enumerate(blocks):
        M[r, :len(b)] = b
    return M


@pytest.mark.parametrize("d", [1, 2, 3])
def test_rows_form_against_block_form(eng, d):
    P = _cloud(d)
    targets = [N - 1, 0, 3, 3]
    M = _members([[i for i in range(N) if i != t] + [t] for t in targets], N + 3)
    for f in _families(eng, d):
        f.check(f.blocks(P, M), f.rows(P, targets))


@pytest.mark.parametrize("d", [1, 2, 3])
def test_rows_form_against_external_form(eng, d):
    P = _cloud(d)
    for f in _families(eng, d):
        for t in (0, N - 1, DUP[1]):
            f.check(f.external(np.delete(P, t, axis=0), P[t:t + 1]), f.rows(P, [t]))


@pytest.mark.parametrize("d", [1, 2, 3])
def test_ragged_blocks(eng, d):
    """Blocks of 1, 2, d + 2 and n members and one without any, in one call: each is the rows form on its own rows."""
    P = _cloud(d)
    blocks = [[0], [5, N - 1], list(range(N - 1, N - 2 - d, -1)) + [0], [4, 1, 6, 0, 3, 5, 2, N - 1], []]
    assert [len(b) for b in blocks] == [1, 2, d + 2, N, 0]
    M = _members(blocks, N + 1)
    for f in _families(eng, d):
        got = f.blocks(P, M)
        for b, g in zip(blocks, got):
            f.check(np.array([g]), f.rows(P[b], [len(b) - 1]) if b else np.array([f.empty]))
