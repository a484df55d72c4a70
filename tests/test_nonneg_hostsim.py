"""Non-negative CP sessions on the host stand-in (tests/hostsim): the engine's wiring of the flag, the
portable default of Ops::cp_mode_update_nn (ops.h: d2h / h2d and a host loop) and the refusals, with the
cases of tests/nonneg_cases.py — no GPU here. The HIP kernel itself: tests/test_gpu_nonneg.py."""
import ctypes as C

import numpy as np
import pytest

import hostsim_util
import nonneg_cases as NC


@pytest.fixture(scope="module")
def pp():
    return hostsim_util.load()


@pytest.fixture()
def ctx(pp):
    c = pp.Context(0)
    yield c
    c.close()


def test_binding_and_abi(pp):
    import ppals
    assert "ppals_cp_set_nonneg" in ppals.EXPORTS and "ppals_cp_get_nonneg" in ppals.EXPORTS
    assert callable(ppals.CP.set_nonneg) and isinstance(ppals.CP.nonneg, property)
    assert pp.lib().ppals_cp_set_nonneg(None, 1) == -3 and pp.lib().ppals_cp_get_nonneg(None) == -3


def test_numpy_restatement_of_one_update():
    """the vectorised restatement against the formula written out entry by entry"""
    rng = np.random.default_rng(0)
    s, R = 7, 4
    W, M = np.abs(rng.standard_normal((s, R))), rng.standard_normal((s, R))
    A = rng.standard_normal((9, R))
    S = A.T @ A
    S[2, 2] = 0.0   # a column that stays
    got, _ = NC.hals_update(M, W, S)
    want = W.copy()
    for x in range(s):
        for r in range(R):
            if not S[r, r] > 0:
                continue
            acc = sum(want[x, q] * S[q, r] for q in range(R))
            want[x, r] = max(NC.FLOOR, want[x, r] + (M[x, r] - acc) / S[r, r])
    assert np.allclose(got, want, rtol=1e-13, atol=0) and np.array_equal(got[:, 2], W[:, 2])
    assert got.min() >= NC.FLOOR and (got == NC.FLOOR).any()


def test_sweeps_match_numpy(pp, ctx):
    NC.case_sweeps(pp, ctx, NC.SHAPES[:2])


def test_properties(pp, ctx):
    NC.case_properties(pp, ctx)


def test_dt_and_msdt_agree(pp, ctx):
    NC.case_schedules(pp, ctx)


def test_em(pp, ctx):
    lens, R = [6, 5, 4], 2
    t = pp.Tensor(ctx, lens, pp.F64).fill_uniform(3)
    s = pp.CP(ctx, t, R)
    mask = np.ones(lens, dtype=np.uint8, order="F")
    try:
        s.impute_device(mask.ctypes.data, lens, [1, 6, 30])
    except pp.PpalsError as e:
        assert "no device views" in str(e)
        pytest.skip("the host stand-in has no impute op (no device views): EM runs in tests/test_gpu_nonneg.py")
    raise AssertionError("the stand-in imputes now: run nonneg_cases.case_em here")


def test_refusals(pp, ctx):
    NC.case_refusals(pp, ctx)


def test_flag_on_two_ranks_is_refused(pp):
    """a context of two ranks (the callbacks are never reached: nothing is launched before the refusal)"""
    AR = C.CFUNCTYPE(None, C.POINTER(C.c_double), C.c_int64)
    RS = C.CFUNCTYPE(None, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int64)
    calls = []
    cbs = (AR(lambda b, n: calls.append("ar")), RS(lambda a, b, n: calls.append("rs")),
           RS(lambda a, b, n: calls.append("ag")))
    uid = C.create_string_buffer(128)
    for i, cb in enumerate(cbs):
        C.memmove(C.byref(uid, 8 * i), C.byref(C.cast(cb, C.c_void_p)), 8)
    ctx = pp.Context(0)
    ctx.init_comm(0, 2, uid)
    assert ctx.nranks == 2
    lens, R = [8, 5, 4], 2
    t = pp.Tensor(ctx, lens, pp.F64)
    s = pp.CP(ctx, t, R)
    with pytest.raises(pp.PpalsError, match=r"ppals error -5: .*one rank"):
        s.set_nonneg(True)
    assert not s.nonneg and not calls
    for x in (s, t, ctx):
        x.close()


def test_blocked_update_hook_is_refused(pp, ctx, monkeypatch):
    monkeypatch.setenv("PPALS_TEST_BLOCKED_UPDATE", "2")
    lens, R = NC.SHAPES[0]
    V, W0 = NC.problem(lens, R, 100)
    t, s = NC.session(pp, ctx, lens, R, pp.F64, V, W0, "msdt", False)
    with pytest.raises(pp.PpalsError, match=r"ppals error -5: .*PPALS_TEST_BLOCKED_UPDATE"):
        s.set_nonneg(True)
    assert not s.nonneg
    s.sweeps_dt(1)
    assert np.isfinite(s.residual())
    s.close()
    t.close()


def test_flag_off_is_the_old_path(pp, ctx):
    NC.case_flag_off(pp, ctx)


def test_drivers(pp, ctx):
    NC.case_drivers(pp, ctx)
