"""The size and rows functions of the curve depths on the pair image (K14 rank depths, K15 extremal depth, K17 total
variation depth) and of K16, and what their entry points refuse, are those of the library before the pair-image plan went
behind sizing and launch: tests/golden/curve_plan_sizes.json, recorded from a build of that commit by
tests/golden/make_golden_curve_plan.py, whose table() and refused() ask the library under test the same questions here.

Host only.  The image route's rows per batch consult device_cus(), which is 256 without a device; its bound of 2048 rows
per compute unit lies at or above the cap of 65 536 rows per batch for any device of 32 compute units or more, so the table
recorded without a device holds on an MI355X as well.  Every refused call returns before anything touches a device, and
none is given a workspace."""
import itertools
import os
import sys

import pytest

from conftest import GOLDEN, load_golden
from statdepth_amd import _native

sys.path.insert(0, GOLDEN)
import make_golden_curve_plan as recipe  # noqa: E402


@pytest.fixture(scope='module')
def golden():
    g = load_golden('curve_plan_sizes')
    assert g['kind'] == 'curve_plan_sizes' and g['axes'] == recipe.AXES and g['levels'] == recipe.LEVELS
    assert os.path.getsize(os.path.join(GOLDEN, 'curve_plan_sizes.json')) < 200 * 1024
    return g


@pytest.fixture(scope='module')
def table():
    return recipe.table(_native.load())


@pytest.mark.parametrize('family', ['rank_depth', 'extremal', 'tvd'])
def test_sizes_and_rows_are_the_recorded_ones(golden, table, family):
    shapes = list(recipe.grid())
    assert len(table[family]) == len(golden[family]) == len(shapes) == 8 * 11 * 2 * 3 * 2
    differ = [(s, got, want) for s, got, want in zip(shapes, table[family], golden[family]) if got != want]
    assert not differ, (len(differ), differ[:5])
    assert all(len(row) == (2 if family == 'extremal' else 9) for row in table[family])
    assert sum(1 for row in golden[family] if row[0]) > len(shapes) // 2      # the table is not one of refusals


def test_central_regions_sizes_are_the_recorded_ones(golden, table):
    shapes = list(itertools.product(recipe.AXES['T'], recipe.AXES['n'], recipe.LEVELS, recipe.AXES['curve_major']))
    assert len(table['central_regions']) == len(golden['central_regions']) == len(shapes)
    differ = [x for x in zip(shapes, table['central_regions'], golden['central_regions']) if x[1] != x[2]]
    assert not differ, (len(differ), differ[:5])


def test_the_floor_of_two_curves_holds_32_rows(golden):
    """The case K17 sizes C for: at n = 2 the 256-byte padding of the floor's image leaves room for 32 rows, not one."""
    i = list(recipe.grid()).index((70, 2, 2, 1, 2, 0))
    rec, floor, *rows = golden['tvd'][i]
    assert rows[0] == 0 and rows[1] == 32 and rows[5] == 70


def test_refusals_are_the_recorded_ones(golden):
    got = recipe.refused(_native.load())
    assert len(got) == len(golden['refusals']) == len(recipe.CALLS)
    for g, w in zip(got, golden['refusals']):
        assert g == w and w['code'] != 0
    for fn in recipe.VALID:                                            # every entry point, and more than one kind of refusal
        assert len({(w['code'], w['message']) for w in golden['refusals'] if w['fn'] == fn}) >= 10
