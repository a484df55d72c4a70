"""ppals_cp_export_model_device / ppals_tucker_export_model_device on the GPU: the fitted model and its
residual written into device tensors through strided views (include/ppals.h).

Earlier test modules load libppals without torch, and the two must share one HIP runtime (torch first),
so every case runs in a fresh child process (tests/model_export_cases.py), one at a time, under a time
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
    p = subprocess.run([sys.executable, os.path.join(HERE, "model_export_cases.py"), name], cwd=ROOT,
                       env=e, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, f"exit {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-6000:]}"
    assert f"model_export case {name}: ok" in p.stdout


def test_cp_model_and_residual_in_every_view():
    run_case("cp_values", timeout=600)


def test_tucker_model_and_residual_in_every_view():
    run_case("tucker_values", timeout=600)


def test_tucker_export_settles_deferred_checks_first():
    run_case("tucker_deferred", timeout=600, PPALS_EIG_DEFER_FAIL="2", PPALS_TUCKER_THIN="0",
             PPALS_EIG_DEBUG="1")


def test_residual_fused_and_two_pass():
    run_case("residual_forms")


def test_export_leaves_the_session_untouched():
    run_case("untouched")


def test_export_on_a_side_stream_without_synchronisation():
    run_case("stream_order")


def test_bad_views_are_refused_before_any_launch():
    run_case("refusals", PYTORCH_NO_CUDA_MEMORY_CACHING="1")


def test_shards_write_their_own_rows():
    subprocess.check_call(["make", "-s", "-j", "4", "-C", os.path.join(HERE, "hipsim")])
    run_case("shards", timeout=600)
