"""Per-mode constraints of CP sessions on the host stand-in (tests/hostsim): the engine's per-mode dispatch,
the FIXED skip in both schedules, the skipped Normalize, the refusals and the portable default of
Ops::cp_mode_update_ortho_ragged (ops.h: d2h / h2d and a cyclic Jacobi in plain C++), with the cases of
tests/mode_constraint_cases.py — no GPU here. The HIP kernels: tests/test_gpu_mode_constraints.py."""
import ctypes as C

import numpy as np
import pytest

import hostsim_util
import mode_constraint_cases as MC


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
    for name in ("ppals_cp_set_mode_constraints", "ppals_cp_get_mode_constraints",
                 "ppals_cp_multi_set_mode_constraints", "ppals_cp_multi_get_mode_constraints"):
        assert name in ppals.EXPORTS and hasattr(pp.lib(), name)
    assert callable(ppals.CP.set_mode_constraints) and isinstance(ppals.CP.mode_constraints, property)
    assert callable(ppals.CPMulti.set_mode_constraints) and isinstance(ppals.CPMulti.mode_constraints, property)
    assert callable(ppals.project)
    assert ppals.MODE_KINDS == ("free", "nonneg", "fixed", "ortho")


def test_numpy_polar_update_is_the_constrained_minimiser():
    """U V^T of the SVD: orthonormal, W^T M symmetric positive definite, and no orthonormal neighbour fits
    M better; a rank-deficient M leaves W alone"""
    rng = np.random.default_rng(0)
    M, W = rng.standard_normal((9, 4)), rng.standard_normal((9, 4))
    P, kappa, ratio, stayed = MC.polar_update(M, W)
    assert not stayed and abs(kappa - np.linalg.cond(M)) < 1e-9 * kappa and abs(ratio - kappa ** -2) < 1e-12
    assert np.abs(P.T @ P - np.eye(4)).max() < 1e-14
    A = P.T @ M
    assert np.abs(A - A.T).max() < 1e-13 and np.linalg.eigvalsh(0.5 * (A + A.T)).min() > 0
    for _ in range(20):
        Q = np.linalg.qr(P + 1e-3 * rng.standard_normal(P.shape))[0]
        Q = Q * np.sign(np.sum(Q * P, axis=0))
        assert np.trace(Q.T @ M) <= np.trace(A) + 1e-12
    M[:, 3] = M[:, 0] + M[:, 1]
    P, _, ratio, stayed = MC.polar_update(M, W)
    assert stayed and ratio < 2.0 ** -45 and np.array_equal(P, W)


def test_the_table_reaches_what_it_claims():
    """the preconditions of the cases, from numpy alone (the figures of the issue)"""
    kappas = []
    for k in MC.WELL_POSED:
        lens, R, kinds, V, W0 = MC.case_problem(k)
        W, G, _, info = MC.numpy_run(V, W0, 0.0, kinds, "cpd")
        assert 0.049 <= NR_residual(V, W) <= 0.053, (k, NR_residual(V, W))
        if "nonneg" in kinds:
            assert info["clamped"] >= 1, (k, info["clamped"])
        if "ortho" in kinds:
            kappas.append(info["kappaM"])
            assert info["kappaM"] <= 1e4 and info["stayed"] == 0
    # kappa_2(M) of the five ORTHO cases, as the issue lists them (4, 9, 181, 105, 2950), to 2 %
    assert np.allclose(kappas, [4.01, 9.40, 180.6, 105.2, 2951], rtol=0.02), kappas
    lens, R, kinds, V, W0 = MC.case_problem(MC.DEGENERATE)
    _, _, _, info = MC.numpy_run(V, W0, 0.0, kinds, "cpd", 1)
    assert info["stayed"] == 1 and info["ratio"] < 2.0 ** -45


def NR_residual(V, W):
    return MC.NR._residual(V, W) / np.linalg.norm(V)


def test_sweeps_match_numpy(pp, ctx):
    MC.case_sweeps(pp, ctx, MC.WELL_POSED[:6])


def test_rank_64(pp, ctx):
    MC.case_sweeps(pp, ctx, MC.WELL_POSED[6:])


def test_orthonormality_and_optimality(pp, ctx):
    MC.case_orthonormal(pp, ctx)


def test_exact_statements(pp, ctx):
    MC.case_exact(pp, ctx)


def test_degenerate_mttkrp_leaves_the_factor(pp, ctx):
    MC.case_degenerate(pp, ctx)


def test_project(pp, ctx):
    MC.case_project(pp, ctx)


def test_multi_start_and_rank_sweep(pp, ctx):
    MC.case_multi(pp, ctx)


def test_normalize(pp, ctx):
    MC.case_normalize(pp, ctx)


def test_kinds_changed_between_sweeps_keep_the_caches_right(pp, ctx):
    MC.case_rekind(pp, ctx)


def test_refusals(pp, ctx):
    MC.case_refusals(pp, ctx)


def test_two_ranks_are_refused(pp):
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
    t = pp.Tensor(ctx, [8, 5, 4], pp.F64)
    s = pp.CP(ctx, t, 2)
    for kinds in (["fixed", "free", "free"], ["free", "nonneg", "free"], ["free", "free", "ortho"]):
        with pytest.raises(pp.PpalsError, match=r"ppals error -5: ppals_cp_set_mode_constraints: .*one rank"):
            s.set_mode_constraints(kinds)
    s.set_mode_constraints(["free"] * 3)
    assert s.mode_constraints == ["free"] * 3 and not calls
    for x in (s, t, ctx):
        x.close()


def test_forced_collective_paths_are_refused(pp, monkeypatch):
    monkeypatch.setenv("PPALS_FORCE_COMM", "1")
    ctx = pp.Context(0)
    AR = C.CFUNCTYPE(None, C.POINTER(C.c_double), C.c_int64)
    RS = C.CFUNCTYPE(None, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int64)
    calls = []   # (a one-rank communicator as tests/test_forced_comm_hostsim.py builds it; never reached)
    cbs = (AR(lambda b, n: calls.append("ar")), RS(lambda a, b, n: calls.append("rs")),
           RS(lambda a, b, n: calls.append("ag")))
    uid = C.create_string_buffer(128)
    for i, cb in enumerate(cbs):
        C.memmove(C.byref(uid, 8 * i), C.byref(C.cast(cb, C.c_void_p)), 8)
    ctx.init_comm(0, 1, uid)
    t = pp.Tensor(ctx, [8, 5, 4], pp.F64)
    s = pp.CP(ctx, t, 2)
    with pytest.raises(pp.PpalsError, match=r"ppals error -5: ppals_cp_set_mode_constraints: "):
        s.set_mode_constraints(["fixed", "free", "free"])
    assert s.mode_constraints == ["free"] * 3 and not calls
    for x in (s, t, ctx):
        x.close()


def test_blocked_update_hook_is_refused(pp, ctx, monkeypatch):
    monkeypatch.setenv("PPALS_TEST_BLOCKED_UPDATE", "2")
    lens, R, kinds, V, W0 = MC.case_problem(0)
    t, s = MC.session(pp, ctx, lens, R, pp.F64, V, W0, "msdt", None)
    with pytest.raises(pp.PpalsError,
                       match=r"ppals error -5: ppals_cp_set_mode_constraints: .*PPALS_TEST_BLOCKED_UPDATE"):
        s.set_mode_constraints(kinds)
    assert s.mode_constraints == ["free"] * 3
    s.sweeps_dt(1)
    assert np.isfinite(s.residual())
    s.close()
    t.close()
