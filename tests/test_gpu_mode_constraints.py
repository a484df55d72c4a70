"""Per-mode constraints of CP sessions on the GPU (ppals_cp_set_mode_constraints, include/ppals.h): the
orthonormal mode update of kernels_polar.hip.h and the per-mode dispatch of the engine against a numpy fp64
restatement, the exact statements, the launch counts and what is refused.

Earlier test modules load libppals without torch, and the two must share one HIP runtime (torch first),
so every case runs in a fresh child process (tests/mode_constraint_cases.py), one at a time, under a time
limit; its exit status is the verdict."""
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
    e.pop("PPALS_MC_BACKEND", None)
    p = subprocess.run([sys.executable, os.path.join(HERE, "mode_constraint_cases.py"), name], cwd=ROOT,
                       env=e, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, f"exit {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-6000:]}"
    assert f"mode constraint case {name}: ok" in p.stdout


def test_sweeps_match_numpy_within_the_bars_of_the_all_free_session():
    run_case("sweeps")


def test_orthonormality_and_optimality_after_every_update():
    run_case("orthonormal")


def test_exact_statements_bit_for_bit():
    run_case("exact")


def test_degenerate_mttkrp_leaves_the_factor_and_writes_the_gradient():
    run_case("degenerate")


def test_project_is_the_least_squares_scores():
    run_case("project")


def test_multi_start_and_rank_sweep_starts_match_ordinary_sessions():
    run_case("multi")


def test_normalize_is_skipped_with_a_fixed_or_orthonormal_mode():
    run_case("normalize")


def test_refusals_leave_the_kinds_and_the_session():
    run_case("refusals")


def test_kinds_changed_between_sweeps_keep_the_caches_right():
    run_case("rekind")


def test_launches_and_scans_are_what_the_kinds_say():
    run_case("counted")


def test_em_with_a_fixed_and_a_non_negative_mode():
    run_case("em")
