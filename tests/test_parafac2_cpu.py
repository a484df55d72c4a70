"""PARAFAC2, the part a box without a GPU can check: the ppals_parafac2_* entry points are declared with their
argument names, exported and bound, and on the host stand-in, which has no device views, ppals_parafac2_create is
refused with that error after the argument checks."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "ppals.h")
LIB = os.path.join(ROOT, "pairwise-perturbation_amd", "lib", "libppals.so")
NAMES = ("ppals_parafac2_create", "ppals_parafac2_destroy", "ppals_parafac2_cp", "ppals_parafac2_tensor",
         "ppals_parafac2_step_device", "ppals_parafac2_run", "ppals_parafac2_projections",
         "ppals_parafac2_projections_device")
ERR_ARG, ERR_UNSUPPORTED = -3, -5      # PPALS_ERR_ARG, PPALS_ERR_UNSUPPORTED (include/ppals.h)


def test_header_declares_the_entry_points_with_their_arguments():
    code = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    code = re.sub(r"\s+", " ", code)
    code = re.sub(r" ([,)])", r"\1", code)      # (where a comment stood between a name and its comma)
    view = r"const void \*data, int dtype, const int64_t \*strides, void \*stream, "
    for decl in (r"int ppals_parafac2_create\(ppals_ctx \*ctx, int64_t I, int64_t J, int64_t K, int R, int storage_dtype, "
                 r"ppals_parafac2 \*\*out\);",
                 r"void ppals_parafac2_destroy\(ppals_parafac2 \*p\);",
                 r"ppals_cp \*ppals_parafac2_cp\(ppals_parafac2 \*p\);",
                 r"ppals_tensor \*ppals_parafac2_tensor\(ppals_parafac2 \*p\);",
                 r"int ppals_parafac2_step_device\(ppals_parafac2 \*p, " + view + r"double \*lost_sq, int \*failed\);",
                 r"int ppals_parafac2_run\(ppals_parafac2 \*p, " + view + r"const ppals_cp_opts \*o, int inner_sweeps, "
                 r"double rel_change, int \*iters, double \*res\);",
                 r"int ppals_parafac2_projections\(ppals_parafac2 \*p, double \*P_host\);",
                 r"int ppals_parafac2_projections_device\(ppals_parafac2 \*p, const double \*\*P\);"):
        assert re.search(decl, code), decl


def test_library_and_binding_export_them():
    import ppals
    lib = C.CDLL(LIB)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in ppals.EXPORTS
    for meth in ("step_device", "step_torch", "run", "projections", "projections_device", "profiles", "loss", "close"):
        assert callable(getattr(ppals.Parafac2, meth)), meth
    assert callable(ppals.parafac2)


def test_host_stand_in_refuses_create_after_the_argument_checks():
    import hostsim_util
    pp = hostsim_util.load()
    ctx = pp.Context(0)
    L = pp.lib()
    h = C.c_void_p()

    def create(I, J, K, R, dt):
        rc = L.ppals_parafac2_create(ctx._h, C.c_int64(I), C.c_int64(J), C.c_int64(K), R, dt, C.byref(h))
        assert not h.value
        return rc, L.ppals_last_error()

    for args, text in (((9, 7, 4, 1, pp.F64), b"[2, 64]"), ((90, 70, 4, 65, pp.F64), b"[2, 64]"),
                       ((9, 7, 4, 8, pp.F64), b"min(I, J)"), ((9, 7, 0, 3, pp.F64), b"positive"), ((9, 7, 4, 3, 7), b"dtype")):
        rc, err = create(*args)
        assert rc == ERR_ARG and err.startswith(b"ppals_parafac2_create: ") and text in err, (args, rc, err)
    rc, err = create(9, 7, 4, 3, pp.BF16)
    assert rc == ERR_UNSUPPORTED and b"BF16" in err
    for dt in (pp.F32, pp.F64):
        rc, err = create(9, 7, 4, 3, dt)
        assert rc == ERR_UNSUPPORTED and b"no device views" in err, (rc, err)
    assert L.ppals_parafac2_create(None, C.c_int64(9), C.c_int64(7), C.c_int64(4), 3, pp.F64, C.byref(h)) == ERR_ARG
    # the entry points take a NULL handle as an argument error, and destroy takes it silently
    L.ppals_parafac2_cp.restype = C.c_void_p
    L.ppals_parafac2_tensor.restype = C.c_void_p
    assert L.ppals_parafac2_cp(None) is None and L.ppals_parafac2_tensor(None) is None
    assert L.ppals_parafac2_step_device(None, None, pp.F64, None, None, None, None) == ERR_ARG
    assert L.ppals_parafac2_projections(None, None) == ERR_ARG
    L.ppals_parafac2_destroy(None)
    # ... and a session of the stand-in goes on as before
    t = pp.Tensor(ctx, [6, 5, 4], pp.F64).fill_uniform(3)
    s = pp.CP(ctx, t, 2)
    s.set_factors(pp.init_factors([6, 5, 4], 2, 1), pp.init_factors([6, 5, 4], 2, 2))
    s.sweeps_dt(1)
    for x in (s, t, ctx):
        x.close()
