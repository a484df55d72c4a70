"""Robust CP, the part a box without a GPU can check: ppals_cp_huber_device, ppals_cp_robust and
ppals_cp_abs_residual_quantile are declared with their argument names, exported and bound, and on the host
stand-in, which has no device views, each is refused with that error, after the arithmetic checks, before
anything of the tensor or the session changes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "ppals.h")
LIB = os.path.join(ROOT, "pairwise-perturbation_amd", "lib", "libppals.so")
NAMES = ("ppals_cp_huber_device", "ppals_cp_robust", "ppals_cp_abs_residual_quantile")
ERR_ARG, ERR_UNSUPPORTED = -3, -5      # PPALS_ERR_ARG, PPALS_ERR_UNSUPPORTED (include/ppals.h)


def test_header_declares_the_entry_points_with_their_arguments():
    text = open(HDR).read()
    assert re.search(r"#define\s+PPALS_ERR_ARG\s+\(-3\)", text) and re.search(r"#define\s+PPALS_ERR_UNSUPPORTED\s+\(-5\)", text)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*ppals_cp\s*\*\s*s\s*,", code), name
    views = (r"const\s+void\s*\*\s*data\s*,\s*const\s+void\s*\*\s*weights\s*,\s*int\s+dtype\s*,\s*const\s+int64_t\s*\*\s*"
             r"box_lo\s*,\s*const\s+int64_t\s*\*\s*box_len\s*,\s*const\s+int64_t\s*\*\s*data_strides\s*,\s*const\s+"
             r"int64_t\s*\*\s*weight_strides\s*,\s*")
    assert re.search(r"ppals_cp_huber_device\s*\([^;]*" + views + r"double\s+c\s*,\s*void\s*\*\s*stream\s*,\s*double\s*\*\s*"
                     r"huber_loss\s*,\s*int64_t\s*\*\s*clipped\s*\)", code)
    assert re.search(r"ppals_cp_robust\s*\([^;]*" + views + r"void\s*\*\s*stream\s*,\s*double\s+c\s*,\s*const\s+ppals_cp_opts"
                     r"\s*\*\s*o\s*,\s*int\s+inner_sweeps\s*,\s*double\s+rel_change\s*,\s*int\s*\*\s*iters\s*,\s*double"
                     r"\s*\*\s*robust_res\s*\)", code)
    assert re.search(r"ppals_cp_abs_residual_quantile\s*\([^;]*" + views + r"void\s*\*\s*stream\s*,\s*double\s+p\s*,\s*"
                     r"double\s*\*\s*value\s*,\s*int64_t\s*\*\s*count\s*\)", code)


def test_library_and_binding_export_them():
    import ppals
    lib = C.CDLL(LIB)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in ppals.EXPORTS
    for meth in ("huber_device", "huber_torch", "abs_residual_quantile_torch", "robust_scale", "run_robust"):
        assert callable(getattr(ppals.CP, meth)), meth


def test_host_stand_in_refuses_and_changes_nothing():
    import hostsim_util
    pp = hostsim_util.load()
    ctx = pp.Context(0)
    lens, R = [6, 5, 4], 2
    fstr = [1, 6, 30]
    t = pp.Tensor(ctx, lens, pp.F64).fill_uniform(3)
    s = pp.CP(ctx, t, R)
    s.set_factors(pp.init_factors(lens, R, 1), pp.init_factors(lens, R, 2))
    s.sweeps_dt(1)
    V0, W0 = t.download(), s.get_factors()
    data = np.zeros(lens, dtype=np.float64, order="F")          # a step would rewrite everything
    wts = np.full(lens, 0.5, dtype=np.float64, order="F")
    dp, wp = data.ctypes.data, wts.ctypes.data
    for want_loss in (True, False):
        for w in (wp, None):
            with pytest.raises(pp.PpalsError, match="ppals error -5: .*no device views"):
                s.huber_device(dp, w, pp.F64, lens, fstr, fstr, 0.25, want_loss=want_loss)
    blo, blen, ds, ws = s._wls_views(lens, fstr, fstr, None)
    o = pp._opts(maxiter=3)
    it, res = C.c_int(-1), C.c_double(-1.0)
    L = pp.lib()

    def ptr(v):
        return C.c_void_p(v) if v else None

    def step(d=dp, w=wp, dt=pp.F64, lo=blo, dstr=ds, wstr=ws, c=0.25):
        loss, n = C.c_double(-1.0), C.c_int64(-1)
        rc = L.ppals_cp_huber_device(s._h, ptr(d), ptr(w), dt, lo, blen, dstr, wstr, C.c_double(c), None,
                                     C.byref(loss), C.byref(n))
        assert loss.value == -1.0 and n.value == -1
        return rc

    def driver(d=dp, w=wp, dt=pp.F64, lo=blo, dstr=ds, wstr=ws, c=0.25, inner=1, rel=0.0):
        return L.ppals_cp_robust(s._h, ptr(d), ptr(w), dt, lo, blen, dstr, wstr, None, C.c_double(c), C.byref(o),
                                 inner, C.c_double(rel), C.byref(it), C.byref(res))

    def quant(d=dp, w=wp, dt=pp.F64, lo=blo, dstr=ds, wstr=ws, p=0.5, null_value=False):
        v, n = C.c_double(-1.0), C.c_int64(-1)
        rc = L.ppals_cp_abs_residual_quantile(s._h, ptr(d), ptr(w), dt, lo, blen, dstr, wstr, None, C.c_double(p),
                                              None if null_value else C.byref(v), C.byref(n))
        assert v.value == -1.0 and n.value == -1
        return rc

    fns = ((step, b"ppals_cp_huber_device: "), (driver, b"ppals_cp_robust: "),
           (quant, b"ppals_cp_abs_residual_quantile: "))
    for fn, name in fns:
        for kw in ({}, dict(w=None), dict(w=None, wstr=None)):
            assert fn(**kw) == ERR_UNSUPPORTED and b"no device views" in L.ppals_last_error(), (name, kw)
    assert step(c=float("inf")) == ERR_UNSUPPORTED          # +inf is allowed: it gets as far as the views
    assert it.value == -1 and res.value == -1.0
    # the arithmetic checks come first and need no device: each is PPALS_ERR_ARG here too
    bad_lo = (C.c_int64 * 3)(1, 0, 0)
    neg = (C.c_int64 * 3)(1, -6, 30)
    for fn, name in fns:
        for kw, text in ((dict(lo=bad_lo), b"the data view: box mode 0"),
                         (dict(dt=pp.BF16), b"bad dtype"), (dict(dt=pp.U8), b"bad dtype"),
                         (dict(d=None), b"the data pointer is NULL"),
                         (dict(dstr=neg), b"the data view: negative stride in mode 1"),
                         (dict(wstr=neg), b"the weights view: negative stride in mode 1")):
            assert fn(**kw) == ERR_ARG, (name, kw)
            err = L.ppals_last_error()
            assert err.startswith(name) and text in err, (name, kw, err)
        # without weights their strides are not looked at
        assert fn(w=None, wstr=neg) == ERR_UNSUPPORTED, name
    for fn, name in fns[:2]:
        for c in (0.0, -1.0, float("nan"), float("-inf")):
            assert fn(c=c) == ERR_ARG, (name, c)
            err = L.ppals_last_error()
            assert err.startswith(name) and b"c must be positive" in err, (name, c, err)
    for p in (-0.1, 1.1, float("nan")):
        assert quant(p=p) == ERR_ARG, p
        assert b"ppals_cp_abs_residual_quantile: p must lie in [0, 1]" in L.ppals_last_error(), p
    assert quant(null_value=True) == ERR_ARG and b"NULL value" in L.ppals_last_error()
    for kw, text in ((dict(inner=0), b"ppals_cp_robust: inner_sweeps"),
                     (dict(rel=-1e-3), b"ppals_cp_robust: rel_change"),
                     (dict(rel=float("nan")), b"ppals_cp_robust: rel_change")):
        assert driver(**kw) == ERR_ARG, kw
        assert text in L.ppals_last_error(), kw
    assert it.value == -1 and res.value == -1.0
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


def test_host_stand_in_refuses_a_rank_above_128_as_unsupported_before_the_pointer_queries():
    import hostsim_util
    pp = hostsim_util.load()
    ctx = pp.Context(0)
    lens, fstr = [6, 5, 4], [1, 6, 30]
    buf = np.zeros(lens, dtype=np.float64, order="F")
    t = pp.Tensor(ctx, lens, pp.F64).fill_uniform(3)
    s = pp.CP(ctx, t, 129)
    with pytest.raises(pp.PpalsError, match="ppals error -5: ppals_cp_huber_device: R > 128"):
        s.huber_device(buf.ctypes.data, None, pp.F64, lens, fstr, fstr, 1.0)
    v, n = C.c_double(-1.0), C.c_int64(-1)
    blo, blen, ds, ws = s._wls_views(lens, fstr, fstr, None)
    rc = pp.lib().ppals_cp_abs_residual_quantile(s._h, C.c_void_p(buf.ctypes.data), None, pp.F64, blo, blen, ds, ws,
                                                 None, C.c_double(0.5), C.byref(v), C.byref(n))
    assert rc == ERR_UNSUPPORTED and b"ppals_cp_abs_residual_quantile: R > 128" in pp.lib().ppals_last_error()
    for x in (s, t, ctx):
        x.close()
