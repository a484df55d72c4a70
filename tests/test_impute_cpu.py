"""CP with missing entries, the part a box without a GPU can check: ppals_cp_impute_device and ppals_cp_em
are declared, exported and bound (with PPALS_U8 == ppals.U8 == 4), and on the host stand-in, which has
no device views, both are refused with that error before anything of the tensor or the session changes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "ppals.h")
LIB = os.path.join(ROOT, "pairwise-perturbation_amd", "lib", "libppals.so")
NAMES = ("ppals_cp_impute_device", "ppals_cp_em")


def test_header_declares_the_entry_points_and_the_mask_type():
    import ppals
    text = open(HDR).read()
    m = re.search(r"^#define\s+PPALS_U8\s+(\d+)", text, flags=re.M)
    assert m and int(m.group(1)) == ppals.U8 == 4
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*ppals_cp\s*\*", code), name
    assert re.search(r"ppals_cp_impute_device\s*\([^;]*double\s*\*\s*observed_sq", code)
    assert re.search(r"ppals_cp_em\s*\([^;]*int\s+inner_sweeps[^;]*double\s*\*\s*observed_res", code)


def test_library_and_binding_export_them():
    import ppals
    lib = C.CDLL(LIB)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in ppals.EXPORTS
    for meth in ("impute_device", "impute_torch", "run_em"):
        assert callable(getattr(ppals.CP, meth)), meth


def test_host_stand_in_refuses_and_changes_nothing():
    import hostsim_util
    pp = hostsim_util.load()
    assert pp.U8 == 4
    ctx = pp.Context(0)
    lens, R = [6, 5, 4], 2
    t = pp.Tensor(ctx, lens, pp.F64).fill_uniform(3)
    s = pp.CP(ctx, t, R)
    s.set_factors(pp.init_factors(lens, R, 1), pp.init_factors(lens, R, 2))
    s.sweeps_dt(1)
    V0, W0 = t.download(), s.get_factors()
    mask = np.zeros(lens, dtype=np.uint8, order="F")   # all missing: an imputation would rewrite everything
    with pytest.raises(pp.PpalsError, match="no device views"):
        s.impute_device(mask.ctypes.data, lens, [1, 6, 30], want_residual=True)
    with pytest.raises(pp.PpalsError, match="no device views"):
        s.impute_device(mask.ctypes.data, lens, [1, 6, 30])
    blo, blen, st = s._mask_view(lens, [1, 6, 30], None)
    o = pp._opts(maxiter=3)
    it, res = C.c_int(-1), C.c_double(-1.0)
    rc = pp.lib().ppals_cp_em(s._h, C.c_void_p(mask.ctypes.data), blo, blen, st, None, C.byref(o), 1,
                              C.byref(it), C.byref(res))
    assert rc == -5 and b"no device views" in pp.lib().ppals_last_error()   # PPALS_ERR_UNSUPPORTED
    assert it.value == -1 and res.value == -1.0
    # the arithmetic checks come first and need no device: a bad box is PPALS_ERR_ARG here too
    with pytest.raises(pp.PpalsError, match=r"ppals error -3: ppals_cp_impute_device: box mode 0"):
        s.impute_device(mask.ctypes.data, lens, [1, 6, 30], lo=[1, 0, 0])
    rc = pp.lib().ppals_cp_em(s._h, C.c_void_p(mask.ctypes.data), blo, blen, st, None, C.byref(o), 0,
                              C.byref(it), C.byref(res))
    assert rc == -3 and b"ppals_cp_em: inner_sweeps" in pp.lib().ppals_last_error()
    # PPALS_U8 is a mask's type only: as a source of tensor values it is refused as before
    assert t.check_view(0, mask.ctypes.data, pp.U8, lens, [1, 6, 30]) == -3
    assert b"bad source dtype" in pp.lib().ppals_last_error()
    assert np.array_equal(t.download(), V0)
    for a, b in zip(s.get_factors(), W0):
        assert np.array_equal(a, b)
    # ... and the session goes on exactly as one that never saw the calls
    s2 = pp.CP(ctx, t, R)
    s2.set_factors(pp.init_factors(lens, R, 1), pp.init_factors(lens, R, 2))
    s2.sweeps_dt(1)
    s2.sweeps_dt(1)
    s.sweeps_dt(1)
    for a, b in zip(s.get_factors(), s2.get_factors()):
        assert np.array_equal(a, b)
    for x in (s, s2, t, ctx):
        x.close()
