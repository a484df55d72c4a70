"""ppals_cp_wls_device / ppals_cp_wls on the GPU: the majorization step of weighted CP under every pair of data
and weights views, its loss, its bit-compatibility with the imputation, and the driver built on it
(include/ppals.h).

Earlier test modules load libppals without torch, and the two must share one HIP runtime (torch first),
so every case runs in a fresh child process (tests/wls_cases.py), one at a time, under a time limit;
its exit status is the verdict."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def run_case(*name, timeout=300, **env):
    e = dict(os.environ, **env)
    e["PYTHONNOUSERSITE"] = "1"
    p = subprocess.run([sys.executable, os.path.join(HERE, "wls_cases.py"), *name], cwd=ROOT,
                       env=e, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, f"exit {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-6000:]}"
    assert f"wls case {' '.join(name)}: ok" in p.stdout


@pytest.mark.parametrize("shape", range(4))   # (23, 17, 30), (9, 13, 7, 11), (5, 6, 4, 7, 3), (36, 40, 20, 24)
def test_stored_values_and_loss_under_every_pair_of_views(shape):
    run_case("values", str(shape))


def test_zero_one_weights_store_the_imputation_bit_for_bit():
    run_case("equals_impute")


def test_special_weights_and_non_finite_data_under_zero_weight():
    run_case("special_weights")


def test_step_is_reproducible_bit_for_bit():
    run_case("reproducible")


def test_sessions_sweep_on_the_rewritten_tensor():
    run_case("session_consistent")


def test_driver_fits_through_heteroscedastic_noise():
    run_case("driver", timeout=600)


def test_step_on_a_side_stream_without_synchronisation():
    run_case("stream_order")


def test_bad_views_are_refused_before_any_launch():
    run_case("refusals", PYTORCH_NO_CUDA_MEMORY_CACHING="1")


def test_shards_rewrite_their_own_rows():
    subprocess.check_call(["make", "-s", "-j", "4", "-C", os.path.join(HERE, "hipsim")])
    run_case("shards", timeout=600)
