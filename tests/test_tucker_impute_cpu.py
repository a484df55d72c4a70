"""Tucker with missing entries, the part a box without a GPU can check: ppals_tucker_impute_device and
ppals_tucker_em are declared with their signatures, exported and bound, and on the host stand-in, which has
no device views, both are refused with that error (after the arithmetic checks of the box) before anything
of the tensor or the session changes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "ppals.h")
LIB = os.path.join(ROOT, "pairwise-perturbation_amd", "lib", "libppals.so")
NAMES = ("ppals_tucker_impute_device", "ppals_tucker_em")
VIEW = (r"\s*\(\s*ppals_tucker\s*\*\s*\w+\s*,\s*const\s+void\s*\*\s*mask\s*,\s*const\s+int64_t\s*\*\s*box_lo\s*,"
        r"\s*const\s+int64_t\s*\*\s*box_len\s*,\s*const\s+int64_t\s*\*\s*strides\s*,\s*void\s*\*\s*stream\s*,")


def test_header_declares_the_entry_points_with_their_signatures():
    code = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    assert re.search(r"\bint\s+ppals_tucker_impute_device" + VIEW + r"\s*double\s*\*\s*observed_sq\s*\)\s*;", code)
    assert re.search(r"\bint\s+ppals_tucker_em" + VIEW + r"\s*const\s+ppals_cp_opts\s*\*\s*\w+\s*,"
                     r"\s*int\s+inner_sweeps\s*,\s*int\s*\*\s*iters\s*,\s*double\s*\*\s*observed_res\s*\)\s*;",
                     code)


def test_library_and_binding_export_them():
    import ppals
    lib = C.CDLL(LIB)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in ppals.EXPORTS
    for meth in ("impute_device", "impute_torch", "run_em"):
        assert callable(getattr(ppals.Tucker, meth)), meth
    # one implementation of the mask helpers for both kinds of session
    assert ppals.Tucker._mask_view is ppals.CP._mask_view
    assert ppals.Tucker._torch_mask is ppals.CP._torch_mask


def _session(pp, ctx, t, lens, ranks):
    k = pp.Tucker(ctx, t, ranks)
    k.set_factors([np.linalg.qr(pp.fill_uniform_host(s * r, 1 + i).reshape((s, r), order="F"))[0]
                   for i, (s, r) in enumerate(zip(lens, ranks))])
    k.set_core(None)
    k.sweeps_dt(1)
    return k


def test_host_stand_in_refuses_and_changes_nothing():
    import hostsim_util
    pp = hostsim_util.load()
    ctx = pp.Context(0)
    lens, ranks = [6, 5, 4], [2, 3, 2]
    t = pp.Tensor(ctx, lens, pp.F64).fill_uniform(3)
    k, k2 = _session(pp, ctx, t, lens, ranks), _session(pp, ctx, t, lens, ranks)   # k2 never sees the calls
    V0 = t.download()
    mask = np.zeros(lens, dtype=np.uint8, order="F")   # all missing: an imputation would rewrite everything
    with pytest.raises(pp.PpalsError, match="ppals error -5: .*no device views"):
        k.impute_device(mask.ctypes.data, lens, [1, 6, 30], want_residual=True)
    with pytest.raises(pp.PpalsError, match="ppals error -5: .*no device views"):
        k.impute_device(mask.ctypes.data, lens, [1, 6, 30])
    blo, blen, st = k._mask_view(lens, [1, 6, 30], None)
    o = pp._opts(maxiter=3)
    it, res = C.c_int(-1), C.c_double(-1.0)
    rc = pp.lib().ppals_tucker_em(k._h, C.c_void_p(mask.ctypes.data), blo, blen, st, None, C.byref(o), 1,
                                  C.byref(it), C.byref(res))
    assert rc == -5 and b"no device views" in pp.lib().ppals_last_error()   # PPALS_ERR_UNSUPPORTED
    assert it.value == -1 and res.value == -1.0
    # the arithmetic checks come first and need no device: a bad box is PPALS_ERR_ARG here too
    with pytest.raises(pp.PpalsError, match=r"ppals error -3: ppals_tucker_impute_device: box mode 0"):
        k.impute_device(mask.ctypes.data, lens, [1, 6, 30], lo=[1, 0, 0])
    rc = pp.lib().ppals_tucker_em(k._h, C.c_void_p(mask.ctypes.data), blo, blen, st, None, C.byref(o), 0,
                                  C.byref(it), C.byref(res))
    assert rc == -3 and b"ppals_tucker_em: inner_sweeps" in pp.lib().ppals_last_error()
    assert it.value == -1 and res.value == -1.0
    assert np.array_equal(t.download(), V0)
    # factors and core are those of the session that never saw the calls (a refused call does not even
    # settle or rotate: the pointer check refuses it before the engine is reached) ...
    (Wa, ca), (Wb, cb) = k.get_factors(), k2.get_factors()
    for a, b in zip(Wa + [ca], Wb + [cb]):
        assert np.array_equal(a, b)
    # ... and the session goes on exactly as that one
    k2.sweeps_dt(1)
    k.sweeps_dt(1)
    (Wa, ca), (Wb, cb) = k.get_factors(), k2.get_factors()
    for a, b in zip(Wa + [ca], Wb + [cb]):
        assert np.array_equal(a, b)
    for x in (k, k2, t, ctx):
        x.close()
