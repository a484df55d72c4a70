"""Multi-start CP sessions (ppals_cp_multi) on the host stand-in: K starts of rank R swept together on
K * R columns must evolve, start by start, exactly as ordinary sessions do under cpd_als with
PPALS_OPT_SIMPLE (cyclic mode updates, no Normalize) from the same factors. Host logic only — the
layout of the starts, the block-diagonal update, the per-start Grams / gradient sums, take() and every
refusal; the batched HIP launch is tests/test_gpu_multistart.py's."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import hostsim_util

HERE = os.path.dirname(os.path.abspath(__file__))
F64 = 1
FTOL = 1e-8   # the fp64 bar of the hostsim suites (tests/test_gpu_cp.py FTOL[1])
NSWEEPS = 3


@pytest.fixture(scope="module")
def pp():
    return hostsim_util.load()


@pytest.fixture(scope="module")
def ctx(pp):
    c = pp.Context(0)
    yield c
    c.close()


def relerr(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def starts(pp, lens, R, K, seed=0):
    W = [pp.init_factors(lens, R, 100 + 17 * b + seed) for b in range(K)]
    G = [pp.init_factors(lens, R, 5000 + 13 * b + seed) for b in range(K)]
    return W, G


def solo(pp, ctx, t, R, W, G, n, lam, schedule):
    """an ordinary session advanced by n sweeps of the class API's Simple optimizer"""
    s = pp.CP(ctx, t, R)
    s.set_schedule(schedule)
    s.set_factors(W, G)
    if n > 0:
        s.cpd_als(0, tol=0.0, maxiter=n - 1, lam=lam, resprint=10 ** 9)   # maxsweep + 1 sweeps
    return s


def assert_same(got, want, tol=FTOL):
    for a, b in zip(got, want):
        assert relerr(a, b) < tol, relerr(a, b)


@pytest.mark.parametrize("schedule", ["msdt", "dt"])
@pytest.mark.parametrize("lam", [0.0, 1e-3])
@pytest.mark.parametrize("K", [1, 2, 5])
@pytest.mark.parametrize("lens,R", [([7, 6, 5], 3), ([6, 5, 4, 5], 2), ([4, 3, 4, 3, 3], 2)])
def test_starts_match_ordinary_sessions(pp, ctx, lens, R, K, lam, schedule):
    t = pp.Tensor(ctx, lens, F64).fill_uniform(11)
    W0, G0 = starts(pp, lens, R, K)
    m = pp.CPMulti(ctx, t, R, K)
    m.set_schedule(schedule)
    for b in range(K):
        m.set_factors(b, W0[b], G0[b])
    gn0 = m.gradnorms()
    for b in range(K):   # before any sweep: the norm of the caller's gradients
        assert abs(gn0[b] - np.sqrt(sum(np.sum(g * g) for g in G0[b]))) < 1e-12 * gn0[b]
    m.sweeps(NSWEEPS, lam)
    res, gn = m.residuals(), m.gradnorms()
    for b in range(K):
        s = solo(pp, ctx, t, R, W0[b], G0[b], NSWEEPS, lam, schedule)
        W_ref, G_ref = s.get_factors(with_grad=True)
        W, G = m.get_factors(b, with_grad=True)
        assert_same(W, W_ref)
        for a, r in zip(G, G_ref):
            assert np.linalg.norm(a - r) < FTOL * (1 + np.linalg.norm(r))
        assert abs(res[b] - s.residual()) < FTOL * s.residual()
        assert abs(gn[b] - s.gradnorm()) < FTOL * s.gradnorm() + 1e-14
        s.close()
    m.close()
    t.close()


def test_sweeps_continue_across_calls(pp, ctx):
    """2 + 1 sweeps in two calls (the multi-sweep cache carries over) are 3 sweeps"""
    lens, R, K = [6, 5, 4, 5], 3, 3
    t = pp.Tensor(ctx, lens, F64).fill_uniform(4)
    W0, G0 = starts(pp, lens, R, K)
    m = pp.CPMulti(ctx, t, R, K)
    m.set_factors(-1, W0, G0)
    m.sweeps(2)
    m.sweeps(1)
    for b in range(K):
        s = solo(pp, ctx, t, R, W0[b], G0[b], 3, 0.0, "msdt")
        assert_same(m.get_factors(b), s.get_factors())
        s.close()
    m.close()
    t.close()


def test_factor_round_trips(pp, ctx):
    lens, R, K = [5, 4, 6], 2, 3
    t = pp.Tensor(ctx, lens, F64).fill_uniform(2)
    W0, G0 = starts(pp, lens, R, K)
    m = pp.CPMulti(ctx, t, R, K)
    m.set_factors(-1, W0, G0)                       # all at once, start-major
    Wall, Gall = m.get_factors(-1, with_grad=True)
    for b in range(K):
        W, G = m.get_factors(b, with_grad=True)     # ... read back start by start
        for got in (W, Wall[b]):
            assert all(np.array_equal(a, r) for a, r in zip(got, W0[b]))
        for got in (G, Gall[b]):
            assert all(np.array_equal(a, r) for a, r in zip(got, G0[b]))
    W1, G1 = starts(pp, lens, R, K, seed=1)
    m.set_factors(1, W1[1], G1[1])                  # one start replaced: the others stay
    Wall = m.get_factors(-1)
    for b in range(K):
        want = W1[1] if b == 1 else W0[b]
        assert all(np.array_equal(a, r) for a, r in zip(Wall[b], want))
    gn = m.gradnorms()
    for b in range(K):
        want = np.sqrt(sum(np.sum(g * g) for g in (G1[1] if b == 1 else G0[b])))
        assert abs(gn[b] - want) < 1e-12 * want
    m.set_factors(2, W1[2])                         # without gradients: as ppals_cp_set_factors, norm 0
    assert m.gradnorms()[2] == 0.0
    # the raw layout: start = -1 is the per-start Wflat blocks one after the other
    n = sum(s * R for s in lens)
    wf = np.empty(n * K)
    pp._check(pp.lib().ppals_cp_multi_get_factors(m._h, -1, pp._dp(wf), None))
    for b in range(K):
        one = np.empty(n)
        pp._check(pp.lib().ppals_cp_multi_get_factors(m._h, b, pp._dp(one), None))
        assert np.array_equal(wf[b * n:(b + 1) * n], one)
    m.close()
    t.close()


@pytest.mark.parametrize("lam", [0.0, 1e-3])
def test_take_then_ordinary_sweeps(pp, ctx, lam):
    """take() is set_factors on the destination: Normalize sweeps, the gradient norm and the PP driver
    go on from the taken start as from the same values handed over by the host"""
    lens, R, K = [7, 6, 5, 4], 3, 4
    t = pp.Tensor(ctx, lens, F64).fill_uniform(8)
    W0, G0 = starts(pp, lens, R, K)
    m = pp.CPMulti(ctx, t, R, K)
    m.set_factors(-1, W0, G0)
    m.sweeps(2, lam)
    for b in (0, 3):
        W, G = m.get_factors(b, with_grad=True)
        d = pp.CP(ctx, t, R)
        d.set_factors(pp.init_factors(lens, R, 1))
        d.sweeps_dt(1, lam)                          # caches alive in the destination
        m.take(b, d)
        r = pp.CP(ctx, t, R)
        r.set_factors(W, G)
        Wd, Gd = d.get_factors(with_grad=True)
        assert all(np.array_equal(a, x) for a, x in zip(Wd, W))
        assert all(np.array_equal(a, x) for a, x in zip(Gd, G))
        assert abs(d.gradnorm() - r.gradnorm()) < 1e-12 * r.gradnorm()
        assert abs(d.residual() - r.residual()) < 1e-12 * r.residual()
        d.sweeps_dt(2, lam)
        r.sweeps_dt(2, lam)
        assert_same(d.get_factors(), r.get_factors())
        assert d.run_pp(tol=0.0, tol_init=0.5, maxiter=4, lam=lam) == r.run_pp(tol=0.0, tol_init=0.5,
                                                                              maxiter=4, lam=lam)
        assert_same(d.get_factors(), r.get_factors())
        d.close()
        r.close()
    # the multi session is untouched by take and by what the destination did afterwards
    s = solo(pp, ctx, t, R, W0[1], G0[1], 2, lam, "msdt")
    assert_same(m.get_factors(1), s.get_factors())
    s.close()
    m.close()
    t.close()


def test_run_stops_and_names_the_best_start(pp, ctx):
    lens, R, K = [6, 5, 4, 5], 2, 3
    t = pp.Tensor(ctx, lens, F64).fill_cp(pp.init_factors(lens, R, 77))
    W0, G0 = starts(pp, lens, R, K)
    m = pp.CPMulti(ctx, t, R, K)
    m.set_factors(-1, W0, G0)
    rc, sweeps, best = m.run(tol=0.0, maxiter=5, resprint=2)
    assert (rc, sweeps) == (0, 5)
    assert best == int(np.argmin(m.residuals()))
    ref = pp.CPMulti(ctx, t, R, K)
    ref.set_factors(-1, W0, G0)
    ref.sweeps(5)
    for b in range(K):
        assert all(np.array_equal(a, x) for a, x in zip(m.get_factors(b), ref.get_factors(b)))
    # a tolerance the best start meets at a look: stops there, before maxiter
    gn = m.gradnorms()
    rc, sweeps, best2 = m.run(tol=2.0 * gn[best], maxiter=50, resprint=1)
    assert rc == 1 and sweeps == 0 and best2 == best
    # the time limit
    rc, sweeps, _ = m.run(tol=0.0, timelimit=0.0, maxiter=50, resprint=1)
    assert rc == 1 and sweeps <= 1
    ref.close()
    m.close()
    t.close()


def _dummy_comm_uid():
    """callbacks of the stand-in communicator that must never be called"""
    AR = C.CFUNCTYPE(None, C.POINTER(C.c_double), C.c_int64)
    RS = C.CFUNCTYPE(None, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int64)

    def never(*a):
        raise AssertionError("a collective was called")
    cbs = (AR(never), RS(never), RS(never))
    uid = C.create_string_buffer(128)
    for i, cb in enumerate(cbs):
        C.memmove(C.byref(uid, 8 * i), C.byref(C.cast(cb, C.c_void_p)), 8)
    return uid, cbs


def test_refusals(pp, ctx):
    lens, R = [6, 5, 4], 3
    t = pp.Tensor(ctx, lens, F64).fill_uniform(1)
    for r, k in ((R, 0), (R, -1), (R, 33), (0, 2), (-1, 2), (5, 26), (65, 2), (129, 1)):
        with pytest.raises(pp.PpalsError, match="error -3"):
            pp.CPMulti(ctx, t, r, k)
    other = pp.Context(0)
    t2 = pp.Tensor(other, lens, F64).fill_uniform(1)
    with pytest.raises(pp.PpalsError, match="error -3.*another context"):
        pp.CPMulti(ctx, t2, R, 2)
    m = pp.CPMulti(ctx, t, R, 2)
    W = pp.init_factors(lens, R, 3)
    for start in (-2, 2, 7):
        with pytest.raises(pp.PpalsError, match="error -3.*start"):
            m.set_factors(start, W)
        with pytest.raises(pp.PpalsError, match="error -3.*start"):
            m.get_factors(start)
    with pytest.raises(pp.PpalsError, match="error -3"):
        m.set_schedule(2)
    with pytest.raises(pp.PpalsError, match="error -3"):
        m.sweeps(-1)
    assert pp.lib().ppals_cp_multi_set_factors(m._h, 0, None, None) == -3
    assert pp.lib().ppals_cp_multi_residuals(m._h, None) == -3
    assert pp.lib().ppals_cp_multi_gradnorms(None, None) == -3
    m.set_factors(-1, [W, W])
    # take: a start (not -1), a session of the same context, tensor and R
    d = pp.CP(ctx, t, R)
    for start in (-1, 2):
        with pytest.raises(pp.PpalsError, match="error -3.*start"):
            m.take(start, d)
    d4 = pp.CP(ctx, t, R + 1)
    with pytest.raises(pp.PpalsError, match="error -3.*rank"):
        m.take(0, d4)
    tb = pp.Tensor(ctx, lens, F64).fill_uniform(1)
    db = pp.CP(ctx, tb, R)
    with pytest.raises(pp.PpalsError, match="error -3.*tensor"):
        m.take(0, db)
    do = pp.CP(other, t2, R)
    with pytest.raises(pp.PpalsError, match="error -3.*context"):
        m.take(0, do)
    assert pp.lib().ppals_cp_multi_take(m._h, 0, None) == -3
    m.take(1, d)   # and the good call goes through
    other.close()
    for h in (d, d4, db, m, tb, t):
        h.close()


def test_two_rank_context_is_unsupported(pp):
    uid, keep = _dummy_comm_uid()
    c = pp.Context(0)
    c.init_comm(0, 2, uid)
    assert c.nranks == 2
    t = pp.Tensor(c, [6, 5, 4], F64)
    with pytest.raises(pp.PpalsError, match="error -5.*one rank"):
        pp.CPMulti(c, t, 2, 2)
    t.close()
    c.close()
    del keep


def test_context_destroyed_before_a_multi_session(pp):
    c = pp.Context(0)
    t = pp.Tensor(c, [6, 5, 4], F64).fill_uniform(3)
    m = pp.CPMulti(c, t, 2, 2)
    pp.lib().ppals_ctx_destroy(c._h)   # behind the binding's back: the session is left dead
    c._h = C.c_void_p()
    with pytest.raises(pp.PpalsError):
        m.sweeps(1)
    m.close()
    t.close()


def test_multistart_under_asan_ubsan():
    """this file's cases against the AddressSanitizer + UBSan build of the stand-in
    (tests/test_sanitizers.py does the same for the suites on its list)"""
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "hostsim"), "asan"])
    lib = os.path.join(HERE, "hostsim", "build_asan", "libppals_hostsim.so")
    asan = subprocess.check_output(["gcc", "-print-file-name=libasan.so"], text=True).strip()
    ubsan = subprocess.check_output(["gcc", "-print-file-name=libubsan.so"], text=True).strip()
    if not os.path.isabs(asan) or not os.path.exists(asan):
        pytest.skip("no libasan in this toolchain")
    env = dict(os.environ, PPALS_HOSTSIM_LIB=lib,
               LD_PRELOAD=":".join(p for p in (asan, ubsan) if os.path.isabs(p)),
               ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1:exitcode=97",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1:exitcode=98")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider",
                        os.path.abspath(__file__), "-k", "not under_asan"],
                       env=env, capture_output=True, text=True, timeout=1500)
    tail = (r.stdout + r.stderr)[-4000:]
    assert r.returncode == 0, tail
    assert "ERROR: AddressSanitizer" not in tail and "runtime error:" not in tail, tail
    assert " passed" in r.stdout
