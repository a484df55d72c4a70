"""Shapes on non-negative modes of CP sessions on the host stand-in (tests/hostsim): the engine's dispatch of a
shaped mode through the start table, the shapes' bookkeeping and refusals, and the portable default of
Ops::cp_mode_update_shape_ragged (ops.h: d2h / h2d and pool-adjacent-violators in plain C++), with the cases of
tests/mode_shape_cases.py — no GPU here. The HIP kernels: tests/test_gpu_mode_shapes.py.

This file does not mirror the GPU one case for case. Two cases run on the device only: `em` hands run_em a
mask that is a torch tensor in device memory, which the stand-in has none of, and `counted` counts the three
HIP launches of the shaped update in the launch profile, which the stand-in's host loop does not book. One
refusal runs here only: a context of more than one rank, which the stand-in gets from callbacks and the device
would need a second GPU for."""
import ctypes as C

import numpy as np
import pytest

import hostsim_util
import mode_shape_cases as MS
import shape_cases as SC


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
    for name in ("ppals_cp_set_mode_shapes", "ppals_cp_get_mode_shapes",
                 "ppals_cp_multi_set_mode_shapes", "ppals_cp_multi_get_mode_shapes"):
        assert name in ppals.EXPORTS and hasattr(pp.lib(), name)
    assert callable(ppals.CP.set_mode_shapes) and isinstance(ppals.CP.mode_shapes, property)
    assert callable(ppals.CPMulti.set_mode_shapes) and isinstance(ppals.CPMulti.mode_shapes, property)
    assert ppals.SHAPE_KINDS == ("none", "unimodal", "increasing", "decreasing")
    assert (ppals.SHAPE_NONE, ppals.SHAPE_UNIMODAL, ppals.SHAPE_INCREASING, ppals.SHAPE_DECREASING) == (0, 1, 2, 3)


def test_numpy_projection_is_the_constrained_minimiser():
    """the reference of tests/shape_cases.py: feasible, and no feasible neighbour fits v better; clipping the
    unbounded isotonic fit is the bounded fit, and the best split's error is the least of prefix + suffix"""
    rng = np.random.default_rng(0)
    for n in (3, 17, 64):
        for _ in range(10):
            v = rng.standard_normal(n) + np.exp(-0.5 * ((np.arange(n) - n / 2) / (n / 6)) ** 2)
            for shape in SC.SHAPES:
                u, _ = SC.project(v, shape, 0.0)
                assert SC.has_shape(u, shape) and u.min() >= SC.FLOOR
                best = np.sum((u - v) ** 2)
                for _ in range(20):
                    z, _ = SC.project(u + 0.05 * rng.standard_normal(n), shape, 0.0)   # a feasible neighbour
                    assert np.sum((z - v) ** 2) >= best - 1e-12
            assert np.array_equal(SC.project(v, SC.DECREASING, 0.0)[0], SC.project(v[::-1], SC.INCREASING, 0.0)[0][::-1])


def test_the_recovers_problem_shows_the_feature_in_numpy():
    R = MS.RECOVERS
    V, W0 = MS.problem(R["lens"], R["R"], ("unimodal", "none", "none"), R["seed"], R["noise"])
    W, _, _, _ = MS.numpy_run(V, W0, 0.0, ("nonneg",) * 3, ("none",) * 3, R["sweeps"])
    assert MS.unimodal_columns(W[0]) == 0
    W, _, _, _ = MS.numpy_run(V, W0, 0.0, ("nonneg",) * 3, ("unimodal", "none", "none"), R["sweeps"])
    assert MS.unimodal_columns(W[0]) == R["R"]


def test_sweeps_match_numpy(pp, ctx):
    MS.case_sweeps(pp, ctx)


def test_shape_floor_and_monotone_residual(pp, ctx):
    MS.case_properties(pp, ctx)


def test_unimodal_loadings_where_the_non_negative_fit_has_none(pp, ctx):
    MS.case_recovers(pp, ctx)


def test_shapes_all_none_change_nothing(pp, ctx):
    MS.case_none_is_free(pp, ctx)


def test_multi_start_and_rank_sweep(pp, ctx):
    MS.case_multi(pp, ctx)


def test_refusals(pp, ctx):
    MS.case_refusals(pp, ctx)


def test_blocked_update_hook_is_refused(pp, ctx):
    MS.case_blocked_hook(pp, ctx)


def test_two_ranks_are_refused(pp):
    """a context of two ranks (the callbacks are never reached: nothing is launched before the refusal): no mode
    becomes NONNEG there (-5), so no mode takes a shape (-3), and the shapes stay all none"""
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
    with pytest.raises(pp.PpalsError, match=r"ppals error -5: ppals_cp_set_mode_constraints: .*one rank"):
        s.set_mode_constraints(["nonneg", "free", "free"])
    with pytest.raises(pp.PpalsError, match=r"ppals error -3: ppals_cp_set_mode_shapes: "):
        s.set_mode_shapes(["unimodal", "none", "none"])
    s.set_mode_shapes(["none"] * 3)
    assert s.mode_shapes == ["none"] * 3 and s.mode_constraints == ["free"] * 3 and not calls
    for x in (s, t, ctx):
        x.close()
