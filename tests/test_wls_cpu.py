"""CP with element weights, the part a box without a GPU can check: ppals_cp_wls_device and ppals_cp_wls are
declared with their argument names, exported and bound, and on the host stand-in, which has no device views,
both are refused with that error, after the arithmetic checks, before anything of the tensor or the session
changes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "ppals.h")
LIB = os.path.join(ROOT, "pairwise-perturbation_amd", "lib", "libppals.so")
NAMES = ("ppals_cp_wls_device", "ppals_cp_wls")


def test_header_declares_the_entry_points_with_their_arguments():
    code = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*ppals_cp\s*\*", code), name
    views = (r"const\s+void\s*\*\s*data\s*,\s*const\s+void\s*\*\s*weights\s*,\s*int\s+dtype\s*,[^;]*box_lo[^;]*"
             r"box_len[^;]*data_strides[^;]*weight_strides[^;]*void\s*\*\s*stream")
    assert re.search(r"ppals_cp_wls_device\s*\([^;]*" + views + r"[^;]*double\s*\*\s*weighted_sq", code)
    assert re.search(r"ppals_cp_wls\s*\([^;]*" + views + r"[^;]*const\s+ppals_cp_opts\s*\*\s*o\s*,\s*int\s+"
                     r"inner_sweeps\s*,\s*double\s+rel_change\s*,\s*int\s*\*\s*iters\s*,\s*double\s*\*\s*"
                     r"weighted_res", code)


def test_library_and_binding_export_them():
    import ppals
    lib = C.CDLL(LIB)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in ppals.EXPORTS
    for meth in ("wls_device", "wls_torch", "run_wls"):
        assert callable(getattr(ppals.CP, meth)), meth


def test_weights_from_std():
    import ppals
    std = np.array([[0.5, 1.0, np.inf], [2.0, np.nan, 0.5]])
    h = ppals.weights_from_std(std)
    assert np.array_equal(h, [[1.0, 0.25, 0.0], [0.0625, 0.0, 1.0]])


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
    data = np.zeros(lens, dtype=np.float64, order="F")
    wts = np.full(lens, 0.5, dtype=np.float64, order="F")   # a step would rewrite everything
    dp, wp = data.ctypes.data, wts.ctypes.data
    for want_loss in (True, False):
        with pytest.raises(pp.PpalsError, match="ppals error -5: .*no device views"):
            s.wls_device(dp, wp, pp.F64, lens, fstr, fstr, want_loss=want_loss)
    blo, blen, ds, ws = s._wls_views(lens, fstr, fstr, None)
    o = pp._opts(maxiter=3)
    it, res = C.c_int(-1), C.c_double(-1.0)

    def driver(d=dp, w=wp, dt=pp.F64, lo=blo, dstr=ds, wstr=ws, inner=1, rel=0.0):
        return pp.lib().ppals_cp_wls(s._h, C.c_void_p(d), C.c_void_p(w), dt, lo, blen, dstr, wstr, None,
                                     C.byref(o), inner, C.c_double(rel), C.byref(it), C.byref(res))

    def step(d=dp, w=wp, dt=pp.F64, lo=blo, dstr=ds, wstr=ws):
        sq = C.c_double(-1.0)
        rc = pp.lib().ppals_cp_wls_device(s._h, C.c_void_p(d), C.c_void_p(w), dt, lo, blen, dstr, wstr, None,
                                          C.byref(sq))
        assert sq.value == -1.0
        return rc

    assert driver() == -5 and b"no device views" in pp.lib().ppals_last_error()   # PPALS_ERR_UNSUPPORTED
    assert it.value == -1 and res.value == -1.0
    # the arithmetic checks come first and need no device: each is PPALS_ERR_ARG here too
    bad_lo = (C.c_int64 * 3)(1, 0, 0)
    neg = (C.c_int64 * 3)(1, -6, 30)
    for fn, name in ((step, b"ppals_cp_wls_device: "), (driver, b"ppals_cp_wls: ")):
        for kw, text in ((dict(lo=bad_lo), b"the data view: box mode 0"),
                         (dict(dt=pp.BF16), b"bad dtype"), (dict(dt=pp.U8), b"bad dtype"),
                         (dict(w=None), b"the weights pointer is NULL"),
                         (dict(d=None), b"the data pointer is NULL"),
                         (dict(dstr=neg), b"the data view: negative stride in mode 1"),
                         (dict(wstr=neg), b"the weights view: negative stride in mode 1")):
            assert fn(**kw) == -3, (name, kw)
            err = pp.lib().ppals_last_error()
            assert err.startswith(name) and text in err, (name, kw, err)
    for kw, text in ((dict(inner=0), b"ppals_cp_wls: inner_sweeps"),
                     (dict(rel=-1e-3), b"ppals_cp_wls: rel_change"),
                     (dict(rel=float("nan")), b"ppals_cp_wls: rel_change")):
        assert driver(**kw) == -3, kw
        assert text in pp.lib().ppals_last_error(), kw
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
    with pytest.raises(pp.PpalsError, match="ppals error -5: ppals_cp_wls_device: R > 128"):
        s.wls_device(buf.ctypes.data, buf.ctypes.data, pp.F64, lens, fstr, fstr)
    for x in (s, t, ctx):
        x.close()
