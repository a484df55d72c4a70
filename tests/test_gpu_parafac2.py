"""ppals_parafac2_* on the GPU: the projection step against the numpy reference for f32 / f64 views and F32 / F64
storage (padded slices among them), the loss identity, exact projections at the truth, a slice without a polar
factor, reproducibility, the driver with and without non-negativity, a step on a side stream, the refusals
(include/ppals.h).

Earlier test modules load libppals without torch, and the two must share one HIP runtime (torch first),
so every case runs in a fresh child process (tests/parafac2_cases.py), one at a time, under a time limit;
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
    p = subprocess.run([sys.executable, os.path.join(HERE, "parafac2_cases.py"), *name], cwd=ROOT,
                       env=e, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, f"exit {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-6000:]}"
    assert f"parafac2 case {' '.join(name)}: ok" in p.stdout


# (23, 17, 5, 3), (70, 9, 6, 2), (16, 130, 4, 5), (9, 7, 33, 4), (40, 33, 5, 17); then the wide generator's
# (65, 96, 2, 33), (130, 70, 3, 49), (64, 64, 2, 64): three and four rank tiles, and an inner CP session of rank 64
@pytest.mark.parametrize("shape", range(8))
def test_step_values_and_the_loss_identity(shape):
    run_case("values", str(shape))


def test_exact_projections_at_the_truth():
    run_case("truth")


def test_a_zero_slice_keeps_its_projection_and_counts_as_failed():
    run_case("zero_slice")


def test_step_is_reproducible_bit_for_bit():
    run_case("reproducible")


def test_driver_descends_monotonically_to_the_reference_loss():
    run_case("driver")


def test_non_negative_parafac2_descends_and_keeps_the_floor():
    run_case("nonneg")


def test_step_on_a_side_stream_without_synchronisation():
    run_case("stream_order")


def test_the_torch_convenience_fits_like_the_reference():
    run_case("convenience")


def test_refusals_come_before_any_launch_or_allocation():
    run_case("refusals", PYTORCH_NO_CUDA_MEMORY_CACHING="1")
