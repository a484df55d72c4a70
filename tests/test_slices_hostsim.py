"""The influence plot (ppals_cp_slice_residuals, ppals_cp_leverages) on the host stand-in: the engine's
control flow — the operands of residual(), the two marginals of the M x K split, their fold onto the modes,
the pseudo-inverse factors shared with the core consistency, the NaN rule — the binding and every refusal
of the C ABI, over the fp64 host twins of the three new ops (the defaults of ops.h). The HIP kernels are
tests/test_gpu_slices.py's. Reference and bars: tests/slices_ref.py (numpy, fp64, V as stored)."""
import ctypes as C

import numpy as np
import pytest

import bf16_util
import hostsim_util
import slices_cases as K

F32, F64 = 0, 1


@pytest.fixture(scope="module")
def pp():
    return hostsim_util.load()


@pytest.fixture(scope="module")
def ctx(pp):
    c = pp.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("dtype", [F64, F32], ids=K.ident)
@pytest.mark.parametrize("lens,rank", K.SHAPES, ids=K.ident)
def test_sums_against_numpy(pp, ctx, lens, rank, dtype):
    K.reference(pp, ctx, lens, rank, dtype)


def test_planted_slices(pp, ctx):
    K.planted(pp, ctx)


@pytest.mark.parametrize("lens,rank", [([12, 10, 9, 7], 9), ([8, 6, 40, 30], 16), ([7, 6, 5], 3)], ids=K.ident)
def test_exact_fit(pp, ctx, lens, rank):
    K.exact_fit(pp, ctx, lens, rank)


@pytest.mark.parametrize("lens,rank", K.LEV_SHAPES, ids=K.ident)
def test_leverages_against_pinv(pp, ctx, lens, rank):
    K.leverages(pp, ctx, lens, rank, F64)


def test_leverages_after_sweeps(pp, ctx):
    K.leverages_after_sweeps(pp, ctx, F64)


def test_leverages_nan_rule(pp, ctx):
    K.leverages_nan_rule(pp, ctx, F64)


def test_rank_70(pp, ctx):
    K.rank_70(pp, ctx, F64)


@pytest.mark.parametrize("schedule", ["msdt", "dt"])
def test_read_only(pp, ctx, schedule):
    K.read_only(pp, ctx, F64, schedule)


def test_read_only_nonneg(pp, ctx):
    K.read_only(pp, ctx, F32, "msdt", nonneg=True)


@pytest.mark.parametrize("lens,rank", K.SLAB_SHAPES, ids=K.ident)
def test_work_cap_changes_nothing(pp, ctx, lens, rank):
    """the host twin needs no partial sums: under the cap it gives the bits it gives without"""
    free = K.reference(pp, ctx, lens, rank, F32)
    capped = K.reference(pp, ctx, lens, rank, F32, cap=1)
    assert all(bf16_util.same_values(a, b) for a, b in zip(free[0], capped[0])) and free[1] == capped[1]


def test_a_bad_cap_is_refused_at_session_creation(pp, ctx):
    t = pp.Tensor(ctx, [8, 6, 5], F64)
    with K.work_cap("many"):
        with pytest.raises(pp.PpalsError, match="PPALS_TEST_SLICE_WORK_BYTES"):
            pp.CP(ctx, t, 3)
    t.close()


def test_refusals(pp, ctx):
    K.refusals(pp, ctx)


def test_binding(pp, ctx):
    K.binding(pp, ctx)


def test_two_rank_context_is_unsupported(pp):
    """before any launch: the stand-in communicator's collectives raise when called"""
    AR = C.CFUNCTYPE(None, C.POINTER(C.c_double), C.c_int64)
    RS = C.CFUNCTYPE(None, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int64)

    def never(*a):
        raise AssertionError("a collective was called")
    cbs = (AR(never), RS(never), RS(never))
    uid = C.create_string_buffer(128)
    for i, cb in enumerate(cbs):
        C.memmove(C.byref(uid, 8 * i), C.byref(C.cast(cb, C.c_void_p)), 8)
    c = pp.Context(0)
    c.init_comm(0, 2, uid)
    assert c.nranks == 2
    t = pp.Tensor(c, [6, 5, 4], F64)
    s = pp.CP(c, t, 2)
    out = np.zeros(15)
    L = pp.lib()
    assert L.ppals_cp_slice_residuals(s._h, pp._dp(out), None) == -5
    err = L.ppals_last_error().decode()
    assert err.startswith("ppals_cp_slice_residuals: ") and "one rank" in err
    assert L.ppals_cp_leverages(s._h, pp._dp(out)) == -5
    err = L.ppals_last_error().decode()
    assert err.startswith("ppals_cp_leverages: ") and "one rank" in err
    assert not out.any()
    s.close()
    t.close()
    c.close()
