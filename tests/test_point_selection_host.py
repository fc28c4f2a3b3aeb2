"""The point-cloud block form's contract, checked on the host without a GPU: a block's members come first and its -1
padding last (the kernels of K4, K5, K7, K10 and K11 take the members up to the first -1 and the target from the last of
them), so a -1 in front of a member is refused before anything is uploaded.  The curve helpers, whose kernels skip a -1
wherever it stands, take the same array as before."""
from unittest import mock

import numpy as np
import pytest

INTERIOR = [[0, -1, 2]]
RAGGED = [[4, 1, 3], [2, 0, -1], [5, -1, -1], [-1, -1, -1]]


@pytest.fixture
def engine(monkeypatch):
    """The engine with the host as its device, a stand-in for the library, and an upload that fails the test."""
    from statdepth_amd import engine

    def no_upload(*a, **k):
        raise AssertionError("uploaded before the members were checked")
    monkeypatch.setattr(engine, "_device", lambda device=None: "cpu")
    monkeypatch.setattr(engine._native, "require_device", lambda: mock.MagicMock())
    monkeypatch.setattr(engine, "_upload", no_upload)
    return engine


P = np.arange(12, dtype=np.float64).reshape(6, 2)
U = np.eye(2)


@pytest.mark.parametrize("call, exc", [
    (lambda e, M: e.pointcloud_simplex_subset_counts(P, M), IndexError),
    (lambda e, M: e.l1_subset_depth(P, M), IndexError),
    (lambda e, M: e.oja_subset_volume_sums(P, M), IndexError),
    (lambda e, M: e.halfspace_subset_counts(P, M, U), IndexError),
    (lambda e, M: e.halfspace_exact_subset_counts(P, M), ValueError),
])
def test_block_form_refuses_interior_padding(engine, call, exc):
    with pytest.raises(exc, match="padding last"):
        call(engine, INTERIOR)
    with pytest.raises(exc, match="padding last"):
        call(engine, [[1, 2, 3], [-1, 0, -1]])
    with pytest.raises(exc, match="out of range"):                  # the check it stands next to, as before
        call(engine, [[0, 6, -1]])
    with pytest.raises(AssertionError, match="uploaded"):           # a well-formed ragged array gets as far as the upload
        call(engine, RAGGED)


def test_members_helper(engine):
    md, nb, bs = engine._members_dev(RAGGED, "cpu", 6, trailing_padding=True)
    assert (nb, bs) == (4, 3) and md.tolist() == RAGGED
    md, nb, bs = engine._members_dev(np.empty((0, 4), dtype=np.int32), "cpu", 6, trailing_padding=True)
    assert (nb, bs) == (0, 4)
    with pytest.raises(IndexError):
        engine._members_dev(INTERIOR, "cpu", 6, trailing_padding=True)
    # the curve helpers (mbd_subset_counts, bd_strict_subset_counts, prob_band_sums) do not pass the keyword
    md, nb, bs = engine._members_dev(INTERIOR, "cpu", 6, rows=1)
    assert (nb, bs) == (1, 3) and md.tolist() == INTERIOR
    with pytest.raises(AssertionError, match="uploaded"):           # prob_band_sums checks its indices first, then uploads
        engine.prob_band_sums(np.zeros((2, 6)), np.ones((2, 6)), True, targets=[1], members=INTERIOR)
