"""ppals_tensor_import_device / _export_device on the GPU through the torch helpers of the binding.

Earlier test modules load libppals without torch, and the two must share one HIP runtime (torch first),
so every case runs in a fresh child process (tests/device_io_cases.py), one at a time, under a time
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
    p = subprocess.run([sys.executable, os.path.join(HERE, "device_io_cases.py"), name], cwd=ROOT,
                       env=e, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, f"exit {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-6000:]}"
    assert f"device_io case {name}: ok" in p.stdout


def test_import_matches_upload_bitwise():
    run_case("parity")


def test_every_layout_and_narrow_sources():
    run_case("layouts")


def test_boxes_assemble_and_leave_the_rest():
    run_case("boxes")


def test_export_writes_only_the_box():
    run_case("export")


def test_live_sessions_see_an_import():
    run_case("sessions")


def test_stream_order_without_synchronisation():
    run_case("stream_order")


def test_shards_import_their_own_rows():
    subprocess.check_call(["make", "-s", "-j", "4", "-C", os.path.join(HERE, "hipsim")])
    run_case("shards", timeout=600)


def test_bad_views_are_refused_before_any_launch():
    run_case("refusals", PYTORCH_NO_CUDA_MEMORY_CACHING="1")
