"""Non-negative multi-start sessions on the host stand-in (tests/hostsim): the engine's wiring of the flag
into a multi-start session, the portable default of Ops::cp_mode_update_nn_batched (ops.h: a loop of the
one-start update), take and the refusals, with the cases of tests/multistart_nonneg_cases.py — no GPU
here. The batched HIP launch itself: tests/test_gpu_multistart_nonneg.py."""
import pytest

import hostsim_util
import multistart_nonneg_cases as MC


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
    assert "ppals_cp_multi_set_nonneg" in ppals.EXPORTS and "ppals_cp_multi_get_nonneg" in ppals.EXPORTS
    assert callable(ppals.CPMulti.set_nonneg) and isinstance(ppals.CPMulti.nonneg, property)
    L = pp.lib()
    assert L.ppals_cp_multi_set_nonneg(None, 1) == -3 and L.ppals_cp_multi_get_nonneg(None) == -3


def test_starts_match_numpy(pp, ctx):
    MC.case_numpy(pp, ctx, rows=(0, 1))


def test_starts_do_not_couple(pp, ctx):
    MC.case_uncoupled(pp, ctx)


def test_properties(pp, ctx):
    MC.case_properties(pp, ctx)


def test_take(pp, ctx):
    MC.case_take(pp, ctx)


def test_refusals(pp, ctx):
    MC.case_refusals(pp, ctx)


def test_blocked_update_hook_is_refused(pp, ctx):
    MC.case_blocked_hook(pp, ctx)


def test_two_rank_context_creates_no_multi_session(pp):
    MC.case_two_ranks(pp)


def test_flag_off_is_the_old_path(pp, ctx):
    MC.case_flag_off(pp, ctx)


def test_run(pp, ctx):
    MC.case_run(pp, ctx)
