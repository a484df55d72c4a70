"""N-PLS cross-validation and the wide-column passes on the GPU (kernels_npls_wide.hip.h), through `import ppals` and
the C ABI: the cases, references and bars of tests/npls_cv_cases.py on F32 / F64 / BF16 storage: the wide passes
against long double under the derived bars at every boundary shape and column count, cross-validation against the
per-segment reference under the bar measured on the host stand-in."""
import os
import subprocess
import sys

import pytest

import npls_cv_cases as CV

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DTYPES = (CV.F32, CV.F64, CV.BF16)
WIDE = [(lens, mode, dt) for lens, mode in CV.WIDE_SHAPES for dt in DTYPES]
WIDE_IDS = [f"{CV.DTNAME[dt]}-{i}" for i in CV.WIDE_IDS for dt in DTYPES]
CASES = CV.CV_CASES + [CV.GROUP_CASE]


@pytest.fixture(scope="module")
def pp():
    import ppals
    return ppals


@pytest.fixture(scope="module")
def ctx(pp):
    c = pp.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("lens,mode,dt", WIDE, ids=WIDE_IDS)
def test_wide_ops(pp, ctx, lens, mode, dt):
    CV.check_wide_ops(pp, ctx, lens, dt, mode)


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: CV.DTNAME[d])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_crossval(pp, ctx, case, dt):
    CV.check_cv(pp, ctx, case, dt)


def test_raw_and_centred_tensor_agree(pp, ctx):
    CV.check_centered_agrees(pp, ctx)


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: CV.DTNAME[d])
def test_segment_with_constant_training_y(pp, ctx, dt):
    CV.check_constant_segment(pp, ctx, dt)


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: CV.DTNAME[d])
def test_cp_session_stays_live(pp, ctx, dt):
    CV.check_cp_session_stays_live(pp, ctx, dt)


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: CV.DTNAME[d])
def test_refusals(pp, ctx, dt):
    CV.check_refusals(pp, ctx, dt)


def test_torch_inputs():
    """Earlier test modules load libppals without torch, and the two must share one HIP runtime (torch first): Y as a
    device tensor runs in a fresh child process (npls_cv_cases.py)."""
    e = dict(os.environ, PYTHONNOUSERSITE="1")
    p = subprocess.run([sys.executable, os.path.join(HERE, "npls_cv_cases.py"), "torch"], cwd=os.path.dirname(HERE), env=e,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, f"exit {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-6000:]}"
    assert "npls_cv case torch: ok" in p.stdout
