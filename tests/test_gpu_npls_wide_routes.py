"""Ops::npls_contract_wide and Ops::npls_slice_inner_wide of the HIP back end at the op level (tests/npls_wide_shim:
the ops on host arrays, with their route log): every shape and column count of tests/npls_cv_cases.py took the route
the restated rule names (a `wide` case did not silently go through the narrow op, a `narrow` case says so), the values
lie under the derived bars, and the guards around the output are untouched. F32, F64 and BF16 storage."""
import pytest

import npls_cv_cases as CV

pytestmark = pytest.mark.gpu

DTYPES = (CV.F32, CV.F64, CV.BF16)


@pytest.fixture(scope="module")
def shim():
    lib = CV.load_shim()
    yield lib
    lib.npls_wide_shim_close()


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: CV.DTNAME[d])
@pytest.mark.parametrize("lens,mode", CV.WIDE_SHAPES, ids=CV.WIDE_IDS)
def test_routes(shim, lens, mode, dt):
    CV.check_wide_routes(shim, lens, mode, dt)
