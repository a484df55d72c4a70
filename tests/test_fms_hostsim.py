"""The factor congruence and the factor match score (ppals_cp_congruence, ppals_cp_fms,
ppals_cp_multi_congruence, ppals_cp_multi_fms, ppals_cp_multi_fms_between) on the host stand-in: the
engine's control flow — the column table, the one download, the matching of every pair of starts, the kept
buffers — and every refusal of the C ABI, over the fp64 host twin of Ops::factor_congruence (the default of
ops.h). The HIP kernels are tests/test_gpu_fms.py's. Reference and bars: tests/fms_ref.py."""
import ctypes as C

import numpy as np
import pytest

import fms_cases as K
import fms_ref as R
import hostsim_util

F32, F64 = 0, 1


@pytest.fixture(scope="module")
def pp():
    return hostsim_util.load()


@pytest.fixture(scope="module")
def ctx(pp):
    c = pp.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("lens,ranks", K.MULTI, ids=K.ident)
def test_multi_phi_against_numpy(pp, ctx, lens, ranks):
    K.multi_phi(pp, ctx, lens, ranks)


def test_ordinary_phi_with_an_extent_1_mode(pp, ctx):
    K.ordinary_phi(pp, ctx, [1, 3, 5], 5, 3)


def test_ordinary_phi_order_8(pp, ctx):
    K.ordinary_phi(pp, ctx, [3, 2, 2, 2, 2, 2, 2, 2], 2, 2)


def test_skipped_mode_with_different_extents(pp, ctx):
    K.skipped_mode_phi(pp, ctx)


def test_invariance(pp, ctx):
    K.invariance(pp, ctx)


def test_ordinary_fms_against_brute_force(pp, ctx):
    K.ordinary_fms(pp, ctx, [1, 3, 5], 5, 3)
    K.ordinary_fms(pp, ctx, [13, 6, 5], 4, 5)


def test_multi_fms_between_and_take(pp, ctx):
    K.multi_fms(pp, ctx)


def test_queued_work_is_seen(pp, ctx):
    K.queued_work(pp, ctx, F64)


@pytest.mark.parametrize("schedule", ["msdt", "dt"])
@pytest.mark.parametrize("kind", ["ordinary", "multi", "nonneg"])
def test_read_only(pp, ctx, kind, schedule):
    K.read_only(pp, ctx, F64, kind, schedule)


def test_same_bits_twice(pp, ctx):
    K.same_bits_twice(pp, ctx)


def test_zero_rule(pp, ctx):
    K.zero_rule(pp, ctx)


def _err(pp):
    return pp.lib().ppals_last_error().decode()


def _launches(ctx):
    return ctx.profile_read(0)[0] + ctx.profile_read(1)[0]


def test_refusals_and_size_queries(pp, ctx):
    L = pp.lib()
    ARG = -3
    lens = [6, 5, 4]
    t = K.tensor(pp, ctx, lens)
    t2 = K.tensor(pp, ctx, [6, 7, 4])
    t4 = K.tensor(pp, ctx, [6, 5, 4, 3])
    a = K.cp(pp, ctx, t, R.factors(lens, 3, 1))
    b = K.cp(pp, ctx, t, R.factors(lens, 2, 2))
    b2 = K.cp(pp, ctx, t2, R.factors([6, 7, 4], 2, 3))
    b4 = K.cp(pp, ctx, t4, R.factors([6, 5, 4, 3], 2, 4))
    m = K.multi(pp, ctx, t, K.starts_of(lens, [2, 3], 5))
    m3 = K.multi(pp, ctx, t, K.starts_of(lens, [2, 3, 1], 6))
    m2 = K.multi(pp, ctx, t2, K.starts_of([6, 7, 4], [1, 2], 7))
    other_ctx = pp.Context(0)
    to = K.tensor(pp, other_ctx, lens)
    ao = K.cp(pp, other_ctx, to, R.factors(lens, 3, 8))
    mo = K.multi(pp, other_ctx, to, K.starts_of(lens, [2, 3], 9))
    phi, n, f = np.zeros(64), C.c_int64(-1), C.c_double(0)
    out = np.zeros(16)
    P, fp = pp._dp(phi), C.byref(f)

    def refused(rc, name, *words):
        assert rc == ARG, (rc, _err(pp))
        assert _err(pp).startswith(name + ": "), _err(pp)
        assert all(w in _err(pp) for w in words), _err(pp)

    # NULL sessions and outputs
    refused(L.ppals_cp_congruence(None, b._h, -1, P, C.byref(n)), "ppals_cp_congruence")
    refused(L.ppals_cp_congruence(a._h, None, -1, P, C.byref(n)), "ppals_cp_congruence")
    refused(L.ppals_cp_congruence(a._h, b._h, -1, None, None), "ppals_cp_congruence")
    refused(L.ppals_cp_fms(None, b._h, -1, 0, fp, None), "ppals_cp_fms")
    refused(L.ppals_cp_fms(a._h, b._h, -1, 0, None, None), "ppals_cp_fms")
    refused(L.ppals_cp_multi_congruence(None, None, -1, P, C.byref(n)), "ppals_cp_multi_congruence")
    refused(L.ppals_cp_multi_congruence(m._h, None, -1, None, None), "ppals_cp_multi_congruence")
    refused(L.ppals_cp_multi_fms(None, -1, 0, pp._dp(out)), "ppals_cp_multi_fms")
    refused(L.ppals_cp_multi_fms(m._h, -1, 0, None), "ppals_cp_multi_fms")
    refused(L.ppals_cp_multi_fms_between(None, m._h, -1, 0, pp._dp(out)), "ppals_cp_multi_fms_between")
    refused(L.ppals_cp_multi_fms_between(m._h, None, -1, 0, pp._dp(out)), "ppals_cp_multi_fms_between")
    refused(L.ppals_cp_multi_fms_between(m._h, m._h, -1, 0, None), "ppals_cp_multi_fms_between")
    # different contexts
    refused(L.ppals_cp_congruence(a._h, ao._h, -1, P, C.byref(n)), "ppals_cp_congruence", "context")
    refused(L.ppals_cp_fms(a._h, ao._h, -1, 0, fp, None), "ppals_cp_fms", "context")
    refused(L.ppals_cp_multi_congruence(m._h, mo._h, -1, P, C.byref(n)), "ppals_cp_multi_congruence", "context")
    refused(L.ppals_cp_multi_fms_between(m._h, mo._h, -1, 0, pp._dp(out)), "ppals_cp_multi_fms_between", "context")
    # different order
    refused(L.ppals_cp_congruence(a._h, b4._h, -1, P, C.byref(n)), "ppals_cp_congruence", "order")
    refused(L.ppals_cp_fms(a._h, b4._h, -1, 0, fp, None), "ppals_cp_fms", "order")
    # different extents in a compared mode: the mode and both extents are named
    refused(L.ppals_cp_congruence(a._h, b2._h, -1, P, C.byref(n)), "ppals_cp_congruence", "mode 1", "5", "7")
    refused(L.ppals_cp_fms(a._h, b2._h, 0, 0, fp, None), "ppals_cp_fms", "mode 1", "5", "7")
    refused(L.ppals_cp_multi_congruence(m._h, m2._h, 2, P, C.byref(n)), "ppals_cp_multi_congruence", "mode 1", "5", "7")
    refused(L.ppals_cp_multi_fms_between(m._h, m2._h, -1, 0, pp._dp(out)), "ppals_cp_multi_fms_between", "mode 1")
    assert L.ppals_cp_congruence(a._h, b2._h, 1, P, C.byref(n)) == 0 and n.value == 6   # ... but not in the skipped one
    assert L.ppals_cp_multi_fms_between(m._h, m2._h, 1, 0, pp._dp(out)) == 0
    # skip_mode outside [-1, N)
    for bad in (-2, 3, 99):
        refused(L.ppals_cp_congruence(a._h, b._h, bad, P, C.byref(n)), "ppals_cp_congruence", "skip_mode")
        refused(L.ppals_cp_fms(a._h, b._h, bad, 0, fp, None), "ppals_cp_fms", "skip_mode")
        refused(L.ppals_cp_multi_congruence(m._h, None, bad, P, C.byref(n)), "ppals_cp_multi_congruence", "skip_mode")
        refused(L.ppals_cp_multi_fms(m._h, bad, 0, pp._dp(out)), "ppals_cp_multi_fms", "skip_mode")
        refused(L.ppals_cp_multi_fms_between(m._h, m._h, bad, 0, pp._dp(out)), "ppals_cp_multi_fms_between", "skip_mode")
    # unknown flag bits
    for bad in (2, 3, -1, 1 << 20):
        refused(L.ppals_cp_fms(a._h, b._h, -1, bad, fp, None), "ppals_cp_fms", "flag")
        refused(L.ppals_cp_multi_fms(m._h, -1, bad, pp._dp(out)), "ppals_cp_multi_fms", "flag")
        refused(L.ppals_cp_multi_fms_between(m._h, m._h, -1, bad, pp._dp(out)), "ppals_cp_multi_fms_between", "flag")
    # fms_between with different numbers of starts
    refused(L.ppals_cp_multi_fms_between(m._h, m3._h, -1, 0, pp._dp(out)), "ppals_cp_multi_fms_between", "starts")
    # the size queries launch nothing
    ctx.sync()
    ctx.profile_enable(2)
    ctx.profile_reset()
    n.value = -1
    assert L.ppals_cp_congruence(a._h, b._h, -1, None, C.byref(n)) == 0 and n.value == 6
    assert L.ppals_cp_multi_congruence(m._h, None, -1, None, C.byref(n)) == 0 and n.value == 25
    assert L.ppals_cp_multi_congruence(m._h, m3._h, -1, None, C.byref(n)) == 0 and n.value == 30
    assert _launches(ctx) == 0
    ctx.profile_enable(0)
    assert L.ppals_cp_congruence(a._h, b._h, -1, P, None) == 0    # n may be NULL when Phi is not
    assert np.array_equal(phi[:6].reshape((3, 2), order="F"), a.congruence(b))
    K.close(ao, mo, to)
    other_ctx.close()
    K.close(a, b, b2, b4, m, m3, m2, t, t2, t4)


def test_two_rank_context_is_unsupported(pp):
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
    phi, n, f = np.zeros(4), C.c_int64(0), C.c_double(0)
    L = pp.lib()
    assert L.ppals_cp_congruence(s._h, s._h, -1, pp._dp(phi), C.byref(n)) == -5
    assert _err(pp).startswith("ppals_cp_congruence: ") and "one rank" in _err(pp)
    assert L.ppals_cp_fms(s._h, s._h, -1, 0, C.byref(f), None) == -5
    assert _err(pp).startswith("ppals_cp_fms: ") and "one rank" in _err(pp)
    s.close()
    t.close()
    c.close()
