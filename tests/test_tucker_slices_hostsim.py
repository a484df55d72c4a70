"""A Tucker session's influence plot (ppals_tucker_residual, ppals_tucker_slice_residuals,
ppals_tucker_leverages, Tucker.explained) on the host stand-in: the engine's control flow — the settle, the
slabs of the model, the sums over b onto mode 0, the fold of the sums over a onto the other modes, the
leverages from a QR of a scratch copy, the NaN rule — the binding and every refusal of the C ABI, over the
fp64 host twin of Ops::model_slice_sums (the default of ops.h). The HIP kernels are
tests/test_gpu_tucker_slices.py's. Reference and bars: tests/tucker_slices_ref.py (numpy, fp64, V as stored)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import hostsim_util
import tucker_slices_cases as K
import tucker_slices_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "ppals.h")
LIB = os.path.join(ROOT, "pairwise-perturbation_amd", "lib", "libppals.so")
NAMES = ("ppals_tucker_residual", "ppals_tucker_slice_residuals", "ppals_tucker_leverages")


@pytest.fixture(scope="module")
def pp():
    return hostsim_util.load()


@pytest.fixture(scope="module")
def ctx(pp):
    c = pp.Context(0)
    yield c
    c.close()


def test_header_declares_the_entries_with_their_signatures():
    code = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    s = r"\s*\(\s*ppals_tucker\s*\*\s*s\s*,\s*double\s*\*\s*"
    assert re.search(r"\bint\s+ppals_tucker_residual" + s + r"out\s*\)\s*;", code)
    assert re.search(r"\bint\s+ppals_tucker_slice_residuals" + s + r"ss\s*,\s*double\s*\*\s*total\s*\)\s*;", code)
    assert re.search(r"\bint\s+ppals_tucker_leverages" + s + r"lev\s*\)\s*;", code)


def test_library_and_binding_export_them(pp):
    import ppals
    lib = C.CDLL(LIB)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert hasattr(pp.lib(), name), name
        assert name in ppals.EXPORTS
    for meth in ("residual", "slice_residuals", "leverages", "explained"):
        assert callable(getattr(ppals.Tucker, meth)), meth
    assert ppals.Tucker._per_mode is ppals.CP._per_mode   # one splitter for both kinds of session


def test_sums_against_numpy(pp, ctx):
    K.values(pp, ctx)


def test_fitted_sessions(pp, ctx):
    K.fitted(pp, ctx)


def test_exact_fit(pp, ctx):
    K.exact_fit(pp, ctx)


def test_two_calls_give_the_same_bytes(pp, ctx):
    K.reproducible(pp, ctx)


def test_work_cap_changes_nothing(pp, ctx):
    K.slab_cap(pp, ctx)


def test_sessions_are_undisturbed(pp, ctx):
    K.undisturbed(pp, ctx)


def test_leverages(pp, ctx):
    K.leverages(pp, ctx)


def test_explained(pp, ctx):
    K.explained(pp, ctx)


def test_refusals(pp, ctx):
    K.refusals(pp, ctx)


def test_two_rank_context_is_unsupported(pp):
    K.two_ranks(pp)


def test_binding_shapes(pp, ctx):
    lens, ranks = [8, 66, 7, 5], (3, 4, 2, 3)
    t = pp.Tensor(ctx, lens, K.F32).fill_uniform(2)
    k = K.given_session(ctx, t, ranks, 9, mod=pp)
    ss, lev, both = k.slice_residuals(), k.leverages(), k.slice_residuals(return_total=True)
    assert isinstance(ss, list) and isinstance(lev, list) and isinstance(both, tuple) and isinstance(both[1], float)
    assert [a.shape for a in ss] == [(n,) for n in lens] == [a.shape for a in lev]
    assert all(a.dtype == np.float64 for a in ss + lev) and isinstance(k.residual(), float)
    k.close()
    t.close()


# ---- 10. the checkers themselves: each planted fault must fail its bar
@pytest.fixture(scope="module")
def planted():
    shape, ranks = (70, 12, 9), (4, 3, 5)
    W, core = K.random_model(shape, ranks, 5)
    V = np.random.default_rng(6).uniform(0.5, 1.5, shape)
    return V, W, core, R.slice_sums(V, W, core)


def test_checker_passes_the_reference_itself(planted):
    V, W, core, (ss, total) = planted
    R.check_sums("self", [a.copy() for a in ss], total, V, W, core)


def test_checker_sees_a_dropped_element(planted):
    V, W, core, (ss, total) = planted
    E2 = (V - K.tucker_model(W, core)) ** 2
    bad = [a.copy() for a in ss]
    bad[1][7] -= E2[33, 7, 4]   # one element dropped from slice 7 of mode 1
    with pytest.raises(AssertionError):
        R.check_sums("dropped", bad, total, V, W, core)


def test_checker_sees_two_swapped_entries(planted):
    V, W, core, (ss, total) = planted
    bad = [a.copy() for a in ss]
    bad[0][[3, 64]] = bad[0][[64, 3]]   # across the two row tiles
    with pytest.raises(AssertionError):
        R.check_sums("swapped", bad, total, V, W, core)


def test_checker_sees_a_leverage_without_the_inverse_gram(planted):
    _, W, _, _ = planted
    with pytest.raises(AssertionError):
        R.check_leverages("no inverse Gram", [np.sum(w * w, axis=1) for w in W], W)
