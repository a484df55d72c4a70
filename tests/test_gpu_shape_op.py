"""Ops::cp_mode_update_shape_ragged of the HIP back end at the op level (tests/shape_shim: the op on host arrays,
with its route log): the three launches of kernels_shape.hip.h for the three shapes at rows {1, 2, 3, 63, 64, 65,
130} and ranks {1, 3, 17, 64}, around the row count at which the column loop's work arrays leave LDS, guards
around W and grad, leading dimensions wider than the rows, starts of different ranks in one call, the column
contents that matter (feasible, monotone, constant, all negative, peaks at the ends, a tie, a noisy double peak),
columns that must stay and starts that must not mix. Reference and bars: tests/shape_cases.py."""
import pytest

import shape_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def shim():
    lib = SC.load(hostsim=False)
    yield lib
    lib.shape_shim_close()


@pytest.mark.parametrize("shape", SC.SHAPES)
def test_rows_and_ranks_against_numpy(shim, shape):
    tags = SC.case_table(shim, shape)   # (the route of its call with four starts of ranks 2, 64, 5, 17 at 130 rows)
    assert tags == [f"update_shape kind={shape} R=64 starts=4 rows=130 lds"], tags


@pytest.mark.parametrize("shape", SC.SHAPES)
def test_rows_around_the_lds_boundary(shim, shape):
    n, tags = SC.case_lds_boundary(shim, shape)
    for rows, route in ((n - 1, "lds"), (n, "lds"), (n + 1, "global"), (n + 2, "global")):
        assert tags[rows] == [f"update_shape kind={shape} R=2 starts=1 rows={rows} {route}"], tags


@pytest.mark.parametrize("n", (65, 200))   # (200: more blocks than the 64 a wave keeps in registers)
@pytest.mark.parametrize("shape", SC.SHAPES)
def test_column_contents(shim, shape, n):
    exempt = SC.case_contents(shim, shape, n)
    assert exempt == (["two_peaks"] if shape == SC.UNIMODAL else []), exempt


@pytest.mark.parametrize("shape", SC.SHAPES)
def test_a_deep_stack_on_the_global_route(shim, shape):
    n, tags = SC.case_deep_global(shim, shape)
    assert tags == [f"update_shape kind={shape} R=1 starts=2 rows={n} global"], tags


@pytest.mark.parametrize("shape", SC.SHAPES)
def test_a_feasible_factor_comes_back(shim, shape):
    SC.case_feasible(shim, shape)


@pytest.mark.parametrize("shape", SC.SHAPES)
def test_columns_that_stay_and_starts_that_do_not_mix(shim, shape):
    SC.case_robust(shim, shape)
