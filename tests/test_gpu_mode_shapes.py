"""Shapes on non-negative modes of CP sessions on the GPU (ppals_cp_set_mode_shapes, include/ppals.h): the shaped
mode update of kernels_shape.hip.h and the engine's dispatch against a numpy fp64 restatement, the properties
(shape, floor, a residual that does not rise), what the feature recovers, the exact statements, the launch counts
and what is refused.

Earlier test modules load libppals without torch, and the two must share one HIP runtime (torch first),
so every case runs in a fresh child process (tests/mode_shape_cases.py), one at a time, under a time
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
    p = subprocess.run([sys.executable, os.path.join(HERE, "mode_shape_cases.py"), name], cwd=ROOT,
                       env=e, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, f"exit {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-6000:]}"
    assert f"mode shape case {name}: ok" in p.stdout


def test_sweeps_match_numpy_within_the_bars_of_the_non_negative_session():
    run_case("sweeps")


def test_shape_floor_and_monotone_residual_after_every_sweep():
    run_case("properties")


def test_unimodal_loadings_where_the_non_negative_fit_has_none():
    run_case("recovers")


def test_shapes_all_none_take_the_launches_and_bits_of_an_untouched_session():
    run_case("none_is_free")


def test_multi_start_and_rank_sweep_starts_match_ordinary_sessions():
    run_case("multi")


def test_em_with_a_unimodal_mode():
    run_case("em")


def test_refusals_leave_shapes_kinds_and_the_session():
    run_case("refusals")


def test_blocked_update_hook_leaves_no_mode_to_shape():
    run_case("blocked_hook")


def test_a_shaped_update_is_three_launches_and_no_scan():
    run_case("counted")
