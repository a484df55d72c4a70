"""N-PLS regression on the GPU (kernels_npls.hip.h), through `import ppals` and the C ABI: the cases, long-double
references and derived bars of tests/npls_cases.py on F32 / F64 / BF16 storage, every mode of every shape, every route
of the launchers' rule (npls_cases.ROUTES); fit and predict against the deflating reference of tests/npls_ref.py
under the bar measured on the host stand-in."""
import os
import subprocess
import sys

import pytest

import npls_cases as NC

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DTYPES = (NC.F32, NC.F64, NC.BF16)
OPS = [(lens, dt, mode) for lens in NC.SHAPES for dt in DTYPES for mode in range(len(lens))]
OPS_IDS = [f"{NC.DTNAME[dt]}-{'x'.join(map(str, lens))}-m{mode}" for lens, dt, mode in OPS]


@pytest.fixture(scope="module")
def pp():
    import ppals
    return ppals


@pytest.fixture(scope="module")
def ctx(pp):
    c = pp.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("lens,dt,mode", OPS, ids=OPS_IDS)
def test_contract_and_slice_inner(pp, ctx, lens, dt, mode):
    NC.check_ops(pp, ctx, lens, dt, mode)


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: NC.DTNAME[d])
@pytest.mark.parametrize("case", NC.FIT_CASES, ids=[c[0] for c in NC.FIT_CASES])
def test_fit_and_predict(pp, ctx, case, dt):
    NC.check_fit(pp, ctx, case, dt)


def test_fit_ends_where_nothing_is_left(pp, ctx):
    NC.check_ends_early(pp, ctx, NC.F32)


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: NC.DTNAME[d])
def test_cp_session_stays_live(pp, ctx, dt):
    NC.check_cp_session_stays_live(pp, ctx, dt)


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: NC.DTNAME[d])
def test_refusals(pp, ctx, dt):
    NC.check_refusals(pp, ctx, dt)


def test_torch_inputs():
    """Earlier test modules load libppals without torch, and the two must share one HIP runtime (torch first): Y as a
    device tensor and X from a strided torch view run in a fresh child process (npls_cases.py)."""
    e = dict(os.environ, PYTHONNOUSERSITE="1")
    p = subprocess.run([sys.executable, os.path.join(HERE, "npls_cases.py"), "torch"], cwd=os.path.dirname(HERE), env=e,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, f"exit {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-6000:]}"
    assert "npls case torch: ok" in p.stdout
