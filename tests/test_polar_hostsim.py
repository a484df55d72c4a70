"""Ops::cp_mode_update_ortho_ragged at the op level on the host stand-in: the ops.h default (d2h, a cyclic Jacobi
in plain C++, h2d) through tests/polar_shim, with the cases of tests/polar_cases.py — no GPU here — and the
self-test of their checker. The HIP kernels: tests/test_gpu_polar_op.py."""
import pytest

import polar_cases as PC


@pytest.fixture(scope="module")
def shim():
    lib = PC.load(hostsim=True)
    yield lib
    lib.polar_shim_close()


def test_rows_and_ranks_against_numpy(shim):
    PC.case_table(shim)


def test_the_checker_rejects_what_it_should(shim):
    PC.case_selftest(shim)
