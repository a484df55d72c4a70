"""ppals_parafac2_*_ragged on the GPU: PARAFAC2 on slices of unequal length. The projection step against the numpy
reference for f32 / f64 buffers, F32 / F64 storage and the packed, stacked and padded layouts; equal rows give the
bits of the equal-length path; agreement with the zero-padded equal-length step; exact projections at the truth;
slices without a polar factor; reproducibility; the driver with and without non-negativity; a step on a side
stream; the convenience function on a list; the refusals (include/ppals.h).

Every case runs in a fresh child process (tests/parafac2_ragged_cases.py), one at a time, under a time limit, as
tests/test_gpu_parafac2.py does it; its exit status is the verdict."""
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
    p = subprocess.run([sys.executable, os.path.join(HERE, "parafac2_ragged_cases.py"), *name], cwd=ROOT,
                       env=e, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, f"exit {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-6000:]}"
    assert f"parafac2 ragged case {' '.join(name)}: ok" in p.stdout


# rows (3, 64, 65, 17, 130) J 17 R 3; (5, 5) J 5 R 5; (40,) J 9 R 2; (33, 96, 64) J 70 R 33; (17, 129, 20) J 130 R 17;
# (64, 200, 65) J 64 R 64 — each for f32 / f64 buffers, F32 / F64 storage and the three layouts
@pytest.mark.parametrize("table", range(6))
def test_step_values_and_the_loss_identity(table):
    run_case("values", str(table))


def test_equal_rows_give_the_bits_of_the_equal_length_path():
    run_case("equal_bits")


def test_ragged_agrees_with_the_zero_padded_equal_length_step():
    run_case("vs_padded")


def test_exact_projections_at_the_truth():
    run_case("truth")


def test_a_zero_slice_and_a_rank_deficient_slice_keep_their_projections():
    run_case("failed_slices")


def test_step_is_reproducible_bit_for_bit():
    run_case("reproducible")


def test_driver_descends_to_the_reference_loss_and_keeps_the_floor():
    run_case("driver")


def test_step_on_a_side_stream_without_synchronisation():
    run_case("stream_order")


def test_the_torch_convenience_takes_a_list_of_matrices():
    run_case("convenience")


def test_refusals_come_before_any_launch_or_allocation():
    run_case("refusals", PYTORCH_NO_CUDA_MEMORY_CACHING="1")


def test_refused_steps_leave_the_state_unchanged():
    run_case("refusals_state", PYTORCH_NO_CUDA_MEMORY_CACHING="1")
