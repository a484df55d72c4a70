"""ppals_tucker_impute_device / ppals_tucker_em on the GPU: the missing entries of a Tucker session's tensor
overwritten with its model under a mask view, the observed residual, and the EM loop built on them
(include/ppals.h); r_0 on both sides of K = 16, where the imputation changes kernels.

Earlier test modules load libppals without torch, and the two must share one HIP runtime (torch first),
so every case runs in a fresh child process (tests/tucker_impute_cases.py), one at a time, under a time
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
    p = subprocess.run([sys.executable, os.path.join(HERE, "tucker_impute_cases.py"), name], cwd=ROOT,
                       env=e, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, f"exit {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-6000:]}"
    assert f"tucker impute case {name}: ok" in p.stdout


def test_imputed_values_and_observed_residual_under_every_mask():
    run_case("values")


def test_a_box_of_two_slabs():
    run_case("slabs")


def test_impute_is_reproducible_bit_for_bit():
    run_case("reproducible")


def test_sessions_sweep_on_the_imputed_tensor():
    run_case("session_consistent")


def test_em_recovers_the_missing_entries():
    run_case("em_recovers")


def test_impute_on_a_side_stream_without_synchronisation():
    run_case("stream_order")


def test_bad_masks_are_refused_before_any_launch():
    run_case("refusals", PYTORCH_NO_CUDA_MEMORY_CACHING="1")


def test_shards_rewrite_their_own_rows():
    subprocess.check_call(["make", "-s", "-j", "4", "-C", os.path.join(HERE, "hipsim")])
    run_case("shards")
