"""Non-negative CP sessions on the GPU (ppals_cp_set_nonneg, include/ppals.h): the HALS mode update of
kernels_nn.hip.h against a numpy fp64 restatement, its properties, and what is refused.

Earlier test modules load libppals without torch, and the two must share one HIP runtime (torch first),
so every case runs in a fresh child process (tests/nonneg_cases.py), one at a time, under a time limit;
its exit status is the verdict."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def run_case(name, timeout=300, **env):
    e = dict(os.environ, **env)
    e["PYTHONNOUSERSITE"] = "1"
    e.pop("PPALS_NONNEG_BACKEND", None)
    p = subprocess.run([sys.executable, os.path.join(HERE, "nonneg_cases.py"), name], cwd=ROOT,
                       env=e, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, f"exit {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-6000:]}"
    assert f"nonneg case {name}: ok" in p.stdout


def test_sweeps_match_numpy_within_ten_times_the_unconstrained_deviation():
    run_case("sweeps")


def test_entries_stay_above_the_floor_and_the_residual_never_rises():
    run_case("properties")


def test_dt_and_msdt_agree():
    run_case("schedules")


def test_sweeps_are_reproducible_bit_for_bit():
    run_case("repeatable")


def test_em_on_a_non_negative_session():
    run_case("em")


def test_drivers_run_a_non_negative_session():
    run_case("drivers")


def test_refusals_leave_the_session_usable():
    run_case("refusals")


def test_flag_off_is_the_old_path():
    run_case("flag_off")
