"""A Tucker session's influence plot on the GPU (ppals_tucker_residual, ppals_tucker_slice_residuals,
ppals_tucker_leverages; include/ppals.h): the pass that keeps the row and column sums of V - W_0 Z^T
(k_model_slices for r_0 <= 16 and above 112, k_model_slices_wide between), its fold, the slabs, and the leverages.
Reference and bars: tests/tucker_slices_ref.py.

Earlier test modules load libppals without torch, and the two must share one HIP runtime (torch first), so
every case runs in a fresh child process (tests/tucker_slices_cases.py), one at a time, under a time limit; its
exit status is the verdict."""
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
    p = subprocess.run([sys.executable, os.path.join(HERE, "tucker_slices_cases.py"), name], cwd=ROOT,
                       env=e, capture_output=True, text=True, timeout=timeout)
    print(p.stdout[-6000:])
    assert p.returncode == 0, f"exit {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-6000:]}"
    assert f"tucker slices case {name}: ok" in p.stdout


def test_slice_sums_against_numpy_on_every_route():
    run_case("values")


def test_fitted_sessions():
    run_case("fitted")


def test_exact_fit():
    run_case("exact_fit")


def test_a_box_of_two_slabs():
    run_case("slabs")


def test_two_calls_give_the_same_bytes():
    run_case("reproducible")


def test_work_cap_changes_nothing():
    run_case("slab_cap")


def test_sessions_are_undisturbed():
    run_case("undisturbed")


def test_leverages():
    run_case("leverages")


def test_explained():
    run_case("explained")


def test_null_arguments_are_refused():
    run_case("refusals")


def test_two_rank_context_is_unsupported():
    run_case("two_ranks_gpu")
