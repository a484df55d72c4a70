"""Centring and scaling in place on the GPU (kernels_prep.hip.h), through `import ppals` and the C ABI: the cases,
long-double references and derived bars of tests/preprocess_cases.py on F32 / F64 / BF16 storage, every mode of
every shape, every route of the launchers' rule (preprocess_cases.ROUTES). Device offsets are the interior of a
larger NaN-filled torch tensor: the guards must stay and no result may be NaN."""
import os
import subprocess
import sys

import numpy as np
import pytest

import preprocess_cases as PC

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DTYPES = (PC.F32, PC.F64, PC.BF16)
CASES = [(lens, dt, mode) for lens, dt in PC.cases(DTYPES) for mode in range(len(lens))]
IDS = [f"{PC.DTNAME[dt]}-{'x'.join(map(str, lens))}-m{mode}" for lens, dt, mode in CASES]


@pytest.fixture(scope="module")
def pp():
    import ppals
    return ppals


@pytest.fixture(scope="module")
def ctx(pp):
    c = pp.Context(0)
    yield c
    c.close()


def run_torch_case(name, **env):
    """Earlier test modules load libppals without torch, and the two must share one HIP runtime (torch first): the
    cases that hand torch's device memory to the library run in a fresh child process (preprocess_cases.py)."""
    e = dict(os.environ, **env)
    e["PYTHONNOUSERSITE"] = "1"
    p = subprocess.run([sys.executable, os.path.join(HERE, "preprocess_cases.py"), name], cwd=os.path.dirname(HERE),
                       env=e, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, f"exit {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-6000:]}"
    assert f"preprocess case {name}: ok" in p.stdout


@pytest.mark.parametrize("lens,dt,mode", CASES, ids=IDS)
def test_center_and_shift(pp, ctx, lens, dt, mode):
    V0, centred, off = PC.check_center_host(pp, ctx, lens, dt, mode)
    PC.check_shift(pp, ctx, lens, dt, mode, V0, centred, off)


def test_device_offsets_between_nan_guards():
    run_torch_case("device_offsets")


def test_torch_offsets():
    run_torch_case("torch_offsets")


@pytest.mark.parametrize("lens,dt,mode", CASES, ids=IDS)
def test_sumsq_scale_rescale(pp, ctx, lens, dt, mode):
    PC.check_scale(pp, ctx, lens, dt, mode)


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: PC.DTNAME[d])
@pytest.mark.parametrize("lens,a,b", [([7, 6, 5], 0, 1), ([7, 6, 5], 2, 0), ([33, 20, 12], 1, 2), ([40, 30], 1, 0),
                                       ([256, 17, 3], 0, 2)])
def test_centring_survives_scaling(pp, ctx, lens, a, b, dt):
    PC.check_property(pp, ctx, lens, dt, a, b)


def test_planted_offsets(pp, ctx):
    PC.check_planted(pp, ctx)


@pytest.mark.parametrize("schedule", ["dt", "msdt"])
def test_cp_session_loses_the_packed_twin(pp, ctx, monkeypatch, schedule):
    """[16, 16, 16, 16], R = 10, F32, a positive tensor: the packed twin is in use before the centring and refused after
    it (mixed signs); the live session equals a new one on the preprocessed values bit for bit"""
    from test_gpu_packed_scan import shared_tensor
    monkeypatch.setenv("PPALS_PACK_LAYOUT", "1")
    lens = [16, 16, 16, 16]
    PC.check_cp_session(pp, ctx, lens, PC.F32, 10, schedule, shared_tensor(lens), packed=True)


@pytest.mark.parametrize("schedule", ["dt", "msdt"])
@pytest.mark.parametrize("dt", [PC.F64, PC.BF16], ids=lambda d: PC.DTNAME[d])
def test_cp_session_sees_the_new_contents(pp, ctx, dt, schedule):
    lens = [12, 10, 9]
    PC.check_cp_session(pp, ctx, lens, dt, 3, schedule, np.asfortranarray(0.5 + np.random.default_rng(3).random(lens)))


@pytest.mark.parametrize("lens,dt", [([12, 10, 9], PC.F64), ([12, 10, 9], PC.F32), ([16, 16, 16, 16], PC.F32)],
                         ids=["12x10x9-f64", "12x10x9-f32", "16x16x16x16-f32"])
def test_tucker_session_sees_the_new_contents(pp, ctx, lens, dt):
    """hosvd + 2 HOOI sweeps of a live session equal those of a new session, factors and core bit for bit"""
    PC.check_tucker_session(pp, ctx, lens, dt, [3] * len(lens), np.asfortranarray(0.5 + np.random.default_rng(4).random(lens)))


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: PC.DTNAME[d])
def test_refusals(pp, ctx, dt):
    PC.check_refusals(pp, ctx, dt)


def test_bad_device_offsets_are_refused():
    run_torch_case("refusals", PYTORCH_NO_CUDA_MEMORY_CACHING="1")


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: PC.DTNAME[d])
def test_preprocess_record(pp, ctx, dt):
    PC.check_preprocess(pp, ctx, dt)
