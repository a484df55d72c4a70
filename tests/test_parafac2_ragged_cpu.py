"""PARAFAC2 on slices of unequal length, the part a box without a GPU can check: the ragged entry points are
declared with their argument names, exported and bound; on the host stand-in, which has no device views,
ppals_parafac2_create_ragged is refused with that error after the argument checks; the ragged numpy reference agrees
with tests/parafac2_ref.py on the zero-padded tensor; the packer's three layouts read back to the same slices; the
inputs of the GPU cases stay under the caps their tolerances rely on."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import parafac2_ref as ref  # noqa: E402
import parafac2_ragged_ref as rref  # noqa: E402

HDR = os.path.join(ROOT, "include", "ppals.h")
LIB = os.path.join(ROOT, "pairwise-perturbation_amd", "lib", "libppals.so")
NAMES = ("ppals_parafac2_create_ragged", "ppals_parafac2_rows", "ppals_parafac2_step_ragged_device",
         "ppals_parafac2_run_ragged")
ERR_ARG, ERR_UNSUPPORTED = -3, -5      # PPALS_ERR_ARG, PPALS_ERR_UNSUPPORTED (include/ppals.h)


def test_header_declares_the_entry_points_with_their_arguments():
    code = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    code = re.sub(r"\s+", " ", code)
    code = re.sub(r" ([,)])", r"\1", code)      # (where a comment stood between a name and its comma)
    view = (r"const void \*data, int dtype, const int64_t \*offsets, const int64_t \*col_strides, "
            r"void \*stream, ")
    for decl in (r"int ppals_parafac2_create_ragged\(ppals_ctx \*ctx, int64_t K, const int64_t \*rows, int64_t J, "
                 r"int R, int storage_dtype, ppals_parafac2 \*\*out\);",
                 r"int ppals_parafac2_rows\(ppals_parafac2 \*p, int64_t \*rows, int64_t \*total\);",
                 r"int ppals_parafac2_step_ragged_device\(ppals_parafac2 \*p, " + view +
                 r"double \*lost_sq, int \*failed\);",
                 r"int ppals_parafac2_run_ragged\(ppals_parafac2 \*p, " + view + r"const ppals_cp_opts \*o, "
                 r"int inner_sweeps, double rel_change, int \*iters, double \*res\);"):
        assert re.search(decl, code), decl


def test_library_and_binding_export_them():
    import ppals
    lib = C.CDLL(LIB)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in ppals.EXPORTS
    for meth in ("ragged", "step_slices_device", "step_torch", "run", "loss", "projections", "profiles"):
        assert callable(getattr(ppals.Parafac2, meth)), meth
    assert isinstance(ppals.Parafac2.rows, property)


def test_host_stand_in_refuses_create_after_the_argument_checks():
    import hostsim_util
    pp = hostsim_util.load()
    ctx = pp.Context(0)
    L = pp.lib()
    h = C.c_void_p()

    def create(rows, J, R, dt, K=None):
        arr = (C.c_int64 * max(len(rows), 1))(*rows) if rows is not None else None
        rc = L.ppals_parafac2_create_ragged(ctx._h, C.c_int64(len(rows) if K is None else K), arr, C.c_int64(J), R, dt,
                                            C.byref(h))
        assert not h.value
        return rc, L.ppals_last_error()

    for args, text in (((None, 7, 3, pp.F64, 2), b"rows is NULL"), (((), 7, 3, pp.F64), b"positive"),
                       (((9, 8, 2, 9, 1), 7, 3, pp.F64), b"slice 2 "), (((9, 8), 7, 1, pp.F64), b"[2, 64]"),
                       (((90, 80), 70, 65, pp.F64), b"[2, 64]"), (((9, 9), 7, 8, pp.F64), b"exceed J"),
                       (((9, 8), 7, 3, 7), b"dtype")):
        rc, err = create(*args)
        assert rc == ERR_ARG and err.startswith(b"ppals_parafac2_create_ragged: ") and text in err, (args, rc, err)
    rc, err = create((9, 8), 7, 3, pp.BF16)
    assert rc == ERR_UNSUPPORTED and b"BF16" in err
    for dt in (pp.F32, pp.F64):
        rc, err = create((9, 8, 3), 7, 3, dt)
        assert rc == ERR_UNSUPPORTED and b"no device views" in err, (rc, err)
    with pytest.raises(pp.PpalsError, match="no device views"):
        pp.Parafac2.ragged(ctx, (9, 8, 3), 7, 3)
    rows = (C.c_int64 * 2)(9, 8)
    assert L.ppals_parafac2_create_ragged(None, C.c_int64(2), rows, C.c_int64(7), 3, pp.F64, C.byref(h)) == ERR_ARG
    # NULL handles are argument errors
    assert L.ppals_parafac2_rows(None, rows, None) == ERR_ARG
    assert L.ppals_parafac2_step_ragged_device(None, None, pp.F64, None, None, None, None, None) == ERR_ARG
    o = pp._opts(maxiter=1)
    assert L.ppals_parafac2_run_ragged(None, None, pp.F64, None, None, None, C.byref(o), 1, C.c_double(0.0), None,
                                       None) == ERR_ARG
    ctx.close()


@pytest.mark.parametrize("t", range(len(rref.TABLES)))
def test_ragged_reference_agrees_with_the_reference_on_the_zero_padded_tensor(t):
    """both sides are numpy SVDs of matrices that differ by zero rows: 1e-12 relative in fp64"""
    rows, J, R = rref.TABLES[t]
    slices, B, A, Cm = rref.values_inputs(t)
    P, Y, lost, failed = rref.step_ragged(slices, B, A, Cm)
    Pp, Yp, lost_p, failed_p = ref.step(rref.zero_pad(slices), B, A, Cm)
    assert failed == failed_p == 0
    for k, n in enumerate(rows):
        assert np.abs(Pp[k][:n] - P[k]).max() <= 1e-12 * np.abs(P[k]).max(), k
        assert not Pp[k][n:].any(), k
    assert np.abs(Y - Yp).max() <= 1e-12 * np.abs(Y).max()
    xx = sum(np.sum(X * X) for X in slices)
    assert abs(lost - lost_p) <= 1e-12 * xx
    assert np.allclose(rref.kappas(slices, B, A, Cm), ref.kappas(rref.zero_pad(slices), B, A, Cm), rtol=1e-9)
    # and the loss of the step's projections is the loss of the padded model
    assert abs(rref.loss(slices, P, B, A, Cm) - ref.loss(rref.zero_pad(slices), Pp, B, A, Cm)) <= 1e-12 * xx


def test_failed_slices_keep_their_projection_in_the_reference():
    rows, J, R = rref.FAILED
    slices, B, A, Cm = rref.failed_inputs()
    P, Y, _, failed = rref.step_ragged(slices, B, A, Cm)
    ident = rref.identity_projections(rows, R)
    assert failed == 2 and np.array_equal(P[0], ident[0]) and np.array_equal(P[2], ident[2])
    assert np.linalg.matrix_rank(slices[2]) == R - 1 and not slices[0].any()
    assert np.array_equal(slices[2], slices[2].astype(np.float32))          # exact in fp32
    P2 = rref.step_ragged(slices, B, A, Cm, [2 * p for p in P])[0]
    assert np.array_equal(P2[0], 2 * P[0]) and np.array_equal(P2[1], P[1])


@pytest.mark.parametrize("dtype", (np.float32, np.float64))
def test_the_three_layouts_read_back_to_the_same_slices(dtype):
    rows, J, R = rref.TABLES[0]
    slices = [np.asarray(X, dtype=dtype) for X in rref.values_inputs(0)[0]]
    N = sum(rows)
    for layout in rref.LAYOUTS:
        buf, off, cs = rref.pack(slices, layout, dtype)
        back = rref.unpack(buf, off, cs, rows, J)
        assert all(np.array_equal(a, b) for a, b in zip(back, slices)), layout
        assert all(c >= n for c, n in zip(cs, rows)) and min(off) >= 0
        owned = np.zeros(buf.size, dtype=bool)
        for o, c, n in zip(off, cs, rows):
            owned[o + np.arange(n)[:, None] + c * np.arange(J)[None, :]] = True
        assert np.count_nonzero(owned) == N * J
        assert np.isnan(buf[~owned]).all() and not np.isnan(buf[owned]).any()
        if layout == "padded":
            assert (~owned).any() and not owned[0] and not owned[-1]
        else:
            assert owned.all()
    buf, off, cs = rref.pack(slices, "packed", dtype)
    assert off == [J * o for o in np.cumsum((0,) + rows[:-1])] and cs == list(rows)      # what NULL means in the ABI
    buf, off, cs = rref.pack(slices, "stacked", dtype)
    assert np.array_equal(buf.reshape((N, J), order="F"), np.vstack(slices))


def test_the_inputs_of_the_gpu_cases_stay_under_their_caps():
    for t, (rows, J, R) in enumerate(rref.TABLES):
        for name, (slices, B, A, Cm) in (("values", rref.values_inputs(t)),
                                         ("truth", rref.truth_inputs(t)[:1] + rref.truth_inputs(t)[2:])):
            for dt in (np.float32, np.float64):
                Xh = [X.astype(dt).astype(np.float64) for X in slices]
                assert rref.kappas(Xh, B, A, Cm).max() <= rref.cap(R), (name, t, dt)
    for t in range(len(rref.EQUAL)):
        slices, B, A, Cm = rref.equal_inputs(t)
        assert rref.kappas(slices, B, A, Cm).max() <= rref.cap(rref.EQUAL[t][2])
    slices, B, A, Cm = rref.driver_inputs()
    assert rref.kappas(slices, B, A, Cm).max() <= ref.KAPPA_CAP
    kap = rref.kappas(*rref.failed_inputs())
    assert np.isinf(kap[0]) and np.isinf(kap[2]) and kap[1] <= ref.KAPPA_CAP
