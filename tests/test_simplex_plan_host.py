"""sd_simplex_sampled_workspace_bytes returns what it did before the sampled workspace of K4 got its one plan behind
sizing, routing and launch: tests/golden/simplex_plan_sizes.json, recorded from a build of that commit by
tests/golden/make_golden_simplex_plan.py, whose table() asks the library under test the same questions here.  The
routing floor of a call is this function at min(samples, 256), so the grid's 255 / 256 / 257 pin it as well.  Host only."""
import os
import sys

import pytest

from conftest import GOLDEN, load_golden
from statdepth_amd import _native

sys.path.insert(0, GOLDEN)
import make_golden_simplex_plan as recipe  # noqa: E402


@pytest.fixture(scope='module')
def golden():
    g = load_golden('simplex_plan_sizes')
    assert g['kind'] == 'simplex_plan_sizes' and g['axes'] == recipe.AXES and g['bench_shapes'] == recipe.BENCH
    assert os.path.getsize(os.path.join(GOLDEN, 'simplex_plan_sizes.json')) < 100 * 1024
    return g


@pytest.fixture(scope='module')
def table():
    return recipe.table(_native.load())


def test_sizes_are_the_recorded_ones(golden, table):
    shapes = list(recipe.grid())
    assert len(table['grid']) == len(golden['grid']) == len(shapes) == 6 * 5 * 6 * 10
    differ = [(s, got, want) for s, got, want in zip(shapes, table['grid'], golden['grid']) if got != want]
    assert not differ, (len(differ), differ[:5])
    covered = [want for (n, T, d, s), want in zip(shapes, golden['grid']) if 1 <= d <= 8 and s > 0]
    assert len(covered) == 6 * 5 * 4 * 9 and all(covered)               # the table is not one of zeros
    assert not any(want for (n, T, d, s), want in zip(shapes, golden['grid']) if not (1 <= d <= 8 and s > 0))


def test_bench_sizes_are_the_recorded_ones(golden, table):
    assert len(golden['bench']) == 4 and all(golden['bench'])
    assert table['bench'] == golden['bench']
