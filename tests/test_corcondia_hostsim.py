"""The core consistency diagnostic (ppals_cp_core_consistency, ppals_cp_multi_core_consistency,
ppals_cp_multi_core) on the host stand-in: the engine's control flow — the column table, the one shared
scan, the chain per start, the index order of the returned core, the kept buffers — and every refusal of
the C ABI, over the fp64 host twins of the new ops (the defaults of ops.h). The HIP kernels are
tests/test_gpu_corcondia.py's. Reference and bars: tests/corcondia_ref.py (numpy, fp64, V as stored)."""
import ctypes as C

import numpy as np
import pytest

import corcondia_cases as K
import corcondia_ref as R
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


@pytest.mark.parametrize("dtype", [F64, F32], ids=K.ident)
@pytest.mark.parametrize("lens,rank", K.SINGLE, ids=K.ident)
def test_closed_form(pp, ctx, lens, rank, dtype):
    K.closed_form(pp, ctx, lens, rank, dtype)


@pytest.mark.parametrize("lens,rank", K.SINGLE, ids=K.ident)
def test_exact_cp_tensor_scores_100(pp, ctx, lens, rank):
    K.exact_cp(pp, ctx, lens, rank, F64)


def test_exact_cp_identity_in_numpy():
    """the identity itself, on the shapes of the suite (wide case included): V = [[W]] gives G = T"""
    for lens, rank in K.SINGLE + [(K.WIDE_LENS, K.WIDE_RANK)]:
        Ws = R.factors(lens, rank, 5)
        G, cc = R.reference(R.cp_tensor(Ws), Ws)
        assert np.linalg.norm(G - R.superdiagonal(rank, len(lens))) < 1e-9 and abs(cc - 100.0) < 1e-8


@pytest.mark.parametrize("equal", [False, True], ids=["ragged", "equal"])
def test_multi_equals_ordinary(pp, ctx, equal):
    ranks = [3, 3, 3] if equal else K.SWEEP_RANKS
    K.multi_equals_ordinary(pp, ctx, F64, K.SWEEP_LENS, ranks, equal)


def test_multi_order_3(pp, ctx):
    K.multi_equals_ordinary(pp, ctx, F32, [9, 8, 7], [1, 3, 2], False)


@pytest.mark.parametrize("schedule", ["msdt", "dt"])
@pytest.mark.parametrize("multi", [False, True], ids=["ordinary", "multi"])
def test_read_only(pp, ctx, multi, schedule):
    K.read_only(pp, ctx, F64, multi, schedule)


def test_nan_rule(pp, ctx):
    K.nan_rule(pp, ctx, F64)


def test_nonneg_sessions(pp, ctx):
    K.multi_equals_ordinary(pp, ctx, F64, K.SWEEP_LENS, K.SWEEP_RANKS, False, nonneg=True)


def _err(pp):
    return pp.lib().ppals_last_error().decode()


def test_refusals_and_size_queries(pp, ctx):
    L = pp.lib()
    cc, n = C.c_double(0), C.c_int64(-1)
    # R = 65, N = 4: 65^4 > 2^24
    t4 = pp.Tensor(ctx, [3, 3, 3, 3], F64).fill_uniform(1)
    big = pp.CP(ctx, t4, 65)
    assert L.ppals_cp_core_consistency(big._h, C.byref(cc), None, C.byref(n)) == -5
    assert _err(pp).startswith("ppals_cp_core_consistency: ") and "2^24" in _err(pp)
    mb = pp.CPMulti.with_ranks(ctx, t4, [2, 65])
    out = np.zeros(2)
    assert L.ppals_cp_multi_core_consistency(mb._h, pp._dp(out)) == -5
    assert _err(pp).startswith("ppals_cp_multi_core_consistency: ")
    assert L.ppals_cp_multi_core(mb._h, 1, None, C.byref(n)) == -5
    assert _err(pp).startswith("ppals_cp_multi_core: ")
    assert L.ppals_cp_multi_core(mb._h, 0, None, C.byref(n)) == 0 and n.value == 16   # the start under the cap
    # a rank above 64 under the cap (order 3): refused too, by name
    t3 = pp.Tensor(ctx, [4, 3, 5], F64).fill_uniform(1)
    r70 = pp.CP(ctx, t3, 70)
    assert L.ppals_cp_core_consistency(r70._h, C.byref(cc), None, None) == -5
    assert _err(pp).startswith("ppals_cp_core_consistency: ") and "64" in _err(pp)
    # NULL arguments, start out of range
    s = pp.CP(ctx, t3, 3)
    s.set_factors(R.factors([4, 3, 5], 3, 1))
    m = pp.CPMulti.with_ranks(ctx, t3, [2, 3])
    m.set_factors(-1, [R.factors([4, 3, 5], r, 2 + r) for r in (2, 3)])
    assert L.ppals_cp_core_consistency(s._h, None, None, C.byref(n)) == -3
    assert L.ppals_cp_core_consistency(None, C.byref(cc), None, None) == -3
    assert L.ppals_cp_multi_core_consistency(m._h, None) == -3
    assert L.ppals_cp_multi_core_consistency(None, pp._dp(out)) == -3
    core = np.zeros(27)
    for bad in (-1, 2, 99):
        assert L.ppals_cp_multi_core(m._h, bad, pp._dp(core), C.byref(n)) == -3
    assert L.ppals_cp_multi_core(None, 0, pp._dp(core), C.byref(n)) == -3
    assert L.ppals_cp_multi_core(m._h, 0, None, None) == -3
    # the size queries
    n.value = -1
    assert L.ppals_cp_core_consistency(s._h, C.byref(cc), None, C.byref(n)) == 0 and n.value == 27
    assert L.ppals_cp_core_consistency(s._h, C.byref(cc), None, None) == 0   # n may be NULL
    assert L.ppals_cp_multi_core(m._h, 0, None, C.byref(n)) == 0 and n.value == 8
    assert L.ppals_cp_multi_core(m._h, 1, None, C.byref(n)) == 0 and n.value == 27
    assert L.ppals_cp_multi_core(m._h, 1, pp._dp(core), None) == 0           # and here
    assert m.core(1).shape == (3, 3, 3) and np.array_equal(m.core(1).ravel(order="F"), core)
    for h in (m, s, r70, mb, big, t3, t4):
        h.close()


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
    cc = C.c_double(0)
    assert pp.lib().ppals_cp_core_consistency(s._h, C.byref(cc), None, None) == -5
    assert _err(pp).startswith("ppals_cp_core_consistency: ") and "one rank" in _err(pp)
    s.close()
    t.close()
    c.close()
