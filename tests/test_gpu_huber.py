"""ppals_cp_huber_device / ppals_cp_robust / ppals_cp_abs_residual_quantile on the GPU: the Huber step under every
pair of data and weights views and without weights, its loss and clipped count, its bit-compatibility with the
weighted step at c = inf, the residual quantile, and the driver built on them (include/ppals.h).

Earlier test modules load libppals without torch, and the two must share one HIP runtime (torch first),
so every case runs in a fresh child process (tests/huber_cases.py), one at a time, under a time limit;
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
    p = subprocess.run([sys.executable, os.path.join(HERE, "huber_cases.py"), *name], cwd=ROOT,
                       env=e, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, f"exit {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-6000:]}"
    assert f"huber case {' '.join(name)}: ok" in p.stdout


@pytest.mark.parametrize("shape", range(4))   # (23, 17, 30), (9, 13, 7, 11), (5, 6, 4, 7, 3), (36, 40, 20, 24)
def test_stored_values_loss_and_clipped_count_under_every_pair_of_views(shape):
    run_case("values", str(shape))


def test_without_clipping_the_step_is_the_weighted_step_bit_for_bit():
    run_case("equals_wls")


def test_special_weights_non_finite_data_and_extreme_thresholds():
    run_case("special")


def test_step_is_reproducible_bit_for_bit():
    run_case("reproducible")


def test_sessions_sweep_on_the_rewritten_tensor():
    run_case("session_consistent")


def test_residual_quantile_ranks_counts_and_exact_ties():
    run_case("quantile")


def test_driver_fits_through_gross_outliers():
    run_case("driver", timeout=600)


def test_step_on_a_side_stream_without_synchronisation():
    run_case("stream_order")


def test_bad_views_thresholds_and_levels_are_refused_before_any_launch():
    run_case("refusals", PYTORCH_NO_CUDA_MEMORY_CACHING="1")


def test_shards_rewrite_their_own_rows_and_sum_loss_and_count():
    subprocess.check_call(["make", "-s", "-j", "4", "-C", os.path.join(HERE, "hipsim")])
    run_case("shards", timeout=600)
