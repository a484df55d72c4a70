"""Ops::cp_mode_update_shape_ragged at the op level on the host stand-in: the ops.h default (d2h, pool-adjacent-
violators in plain C++, h2d) through tests/shape_shim, with the cases of tests/shape_cases.py — no GPU here — and
the self-test of their checker. The HIP kernels: tests/test_gpu_shape_op.py."""
import pytest

import shape_cases as SC


@pytest.fixture(scope="module")
def shim():
    lib = SC.load(hostsim=True)
    yield lib
    lib.shape_shim_close()


@pytest.mark.parametrize("shape", SC.SHAPES)
def test_rows_and_ranks_against_numpy(shim, shape):
    SC.case_table(shim, shape)


@pytest.mark.parametrize("shape", SC.SHAPES)
def test_rows_around_the_lds_boundary(shim, shape):
    SC.case_lds_boundary(shim, shape)


@pytest.mark.parametrize("n", (65, 200))   # (200: more blocks than the 64 a wave keeps in registers)
@pytest.mark.parametrize("shape", SC.SHAPES)
def test_column_contents(shim, shape, n):
    exempt = SC.case_contents(shim, shape, n)
    assert exempt == (["two_peaks"] if shape == SC.UNIMODAL else []), exempt


@pytest.mark.parametrize("shape", SC.SHAPES)
def test_a_deep_stack_on_the_global_route(shim, shape):
    SC.case_deep_global(shim, shape)


@pytest.mark.parametrize("shape", SC.SHAPES)
def test_a_feasible_factor_comes_back(shim, shape):
    SC.case_feasible(shim, shape)


@pytest.mark.parametrize("shape", SC.SHAPES)
def test_columns_that_stay_and_starts_that_do_not_mix(shim, shape):
    SC.case_robust(shim, shape)


def test_the_checker_rejects_what_it_should(shim):
    SC.case_selftest(shim)
