"""Non-negative multi-start sessions on the GPU (ppals_cp_multi_set_nonneg, include/ppals.h): the batched
HALS update of kernels_nn.hip.h — a grid of (row tiles x starts) and one finishing launch with a workgroup
per start — against a numpy fp64 restatement and against ordinary non-negative sessions, start by start;
that no start leaks into another; the launch count; take and the refusals. The cases and their bars live
in tests/multistart_nonneg_cases.py; they run in this process (no torch is needed), like
tests/test_gpu_multistart.py."""
import os
import subprocess
import sys

import pytest

import multistart_nonneg_cases as MC

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROWS = range(len(MC.ROWS))


def _id(k):
    lens, R, K = MC.ROWS[k]
    return "x".join(map(str, lens)) + f"-R{R}-K{K}"


@pytest.fixture(scope="module")
def pp():
    import ppals
    return ppals


@pytest.fixture(scope="module")
def ctx(pp):
    c = pp.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("k", ROWS, ids=_id)
def test_starts_match_numpy_within_ten_times_the_unconstrained_deviation(pp, ctx, k):
    MC.case_numpy(pp, ctx, rows=(k,))


@pytest.mark.parametrize("k", ROWS, ids=_id)
def test_starts_match_ordinary_non_negative_sessions(pp, ctx, k):
    MC.case_pairs(pp, ctx, rows=(k,))


def test_starts_do_not_couple(pp, ctx):
    MC.case_uncoupled(pp, ctx)


@pytest.mark.parametrize("k", ROWS, ids=_id)
def test_sweeps_are_reproducible_bit_for_bit(pp, ctx, k):
    MC.case_repeatable(pp, ctx, rows=(k,))


@pytest.mark.parametrize("k", ROWS, ids=_id)
def test_entries_stay_above_the_floor_and_no_residual_rises(pp, ctx, k):
    MC.case_properties(pp, ctx, rows=(k,))


def test_launch_count_does_not_grow_with_the_starts_and_the_scans_are_shared(pp, ctx):
    MC.case_launches(pp, ctx)


def test_take(pp, ctx):
    MC.case_take(pp, ctx)


def test_refusals_leave_the_session_sweeping_as_its_twin(pp, ctx):
    MC.case_refusals(pp, ctx)


def test_blocked_update_hook_is_refused(pp, ctx):
    MC.case_blocked_hook(pp, ctx)


def test_two_rank_context_creates_no_multi_session():
    """a two-rank context needs the callback communicator of tests/hipsim (the product's engine and HIP
    kernels without RCCL): a second library, so a child process of its own"""
    e = dict(os.environ, PYTHONNOUSERSITE="1")
    p = subprocess.run([sys.executable, os.path.join(HERE, "multistart_nonneg_cases.py"), "two_ranks"],
                       cwd=os.path.dirname(HERE), env=e, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, f"exit {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-6000:]}"
    assert "multistart nonneg case two_ranks: ok" in p.stdout


def test_flag_off_is_the_old_path(pp, ctx):
    MC.case_flag_off(pp, ctx)


def test_run_names_the_best_start(pp, ctx):
    MC.case_run(pp, ctx)
