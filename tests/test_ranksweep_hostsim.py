"""Rank-sweep sessions (ppals_cp_multi_create_ranks: a multi-start session whose starts have their own
ranks) on the host stand-in: the engine's per-start table — column, Gram and system offsets —, the factor
layout, take, run's stopping rule and every refusal, on the ops.h defaults of the ragged ops (a loop of
the one-start update). Host logic only; the HIP launches are tests/test_gpu_ranksweep.py's.
Bars: 1e-8, what tests/test_multistart_hostsim.py holds the pairing with ordinary sessions to; the
non-negative pairing at multistart_nonneg_cases.PAIR_BARS of the stand-in."""
import ctypes as C

import numpy as np
import pytest

import hostsim_util
import multistart_nonneg_cases as MC
import oracle_lib as O
import ranksweep_util as U

F32, F64 = 0, 1
FTOL = 1e-8
NSWEEPS = 3
CASES = [([8, 7, 6, 5], [2, 5, 3]), ([10, 8, 9], [1, 4, 2, 7])]


@pytest.fixture(scope="module")
def pp():
    return hostsim_util.load()


@pytest.fixture(scope="module")
def ctx(pp):
    c = pp.Context(0)
    yield c
    c.close()


def create_rc(pp, ctx, t, nstarts, ranks):
    """the raw entry point: (return code, handle)"""
    h = C.c_void_p()
    arr = None if ranks is None else (C.c_int * max(len(ranks), 1))(*ranks)
    rc = pp.lib().ppals_cp_multi_create_ranks(ctx._h, t._h, nstarts, arr, C.byref(h))
    return rc, h


@pytest.mark.parametrize("schedule", ["msdt", "dt"])
@pytest.mark.parametrize("lam", [0.0, 1e-3])
@pytest.mark.parametrize("lens,ranks", CASES)
def test_starts_match_ordinary_sessions_and_the_oracle(pp, ctx, lens, ranks, lam, schedule):
    V = O.build_V(O.init_factors(lens, max(ranks), 1003))
    t = pp.Tensor(ctx, lens, F64).upload(V)
    W0, G0 = U.starts(pp.init_factors, lens, ranks)
    m = pp.CPMulti.with_ranks(ctx, t, ranks)
    assert m.ranks == list(ranks) and m.nstarts == len(ranks)
    m.set_schedule(schedule)
    for b in range(len(ranks)):
        m.set_factors(b, W0[b], G0[b])
    gn0 = m.gradnorms()
    for b in range(len(ranks)):   # before any sweep: the norm of the caller's gradients
        assert abs(gn0[b] - np.sqrt(sum(np.sum(g * g) for g in G0[b]))) < 1e-12 * gn0[b]
    m.sweeps(NSWEEPS, lam)
    res, gn = m.residuals(), m.gradnorms()
    for b, r in enumerate(ranks):
        s = U.solo(pp, ctx, t, r, W0[b], G0[b], NSWEEPS, lam, schedule)
        U.check_start(m, b, s, FTOL, res, gn)
        s.close()
        _, _, _, W_ref, G_ref = O.cpd_als(V, W0[b], G0[b], 0, tol=0.0, maxsweep=NSWEEPS - 1, lam=lam,
                                          resprint=10 ** 9)
        W, G = m.get_factors(b, with_grad=True)
        for a, x in zip(W, W_ref):
            assert U.relerr(a, x) < FTOL, (b, U.relerr(a, x))
        for a, x in zip(G, G_ref):
            assert np.linalg.norm(a - x) < 100 * FTOL * (1 + np.linalg.norm(x))
    m.close()
    t.close()


def test_factor_round_trips_and_reported_ranks(pp, ctx):
    lens, ranks = [5, 4, 6], [3, 1, 4]
    t = pp.Tensor(ctx, lens, F64).fill_uniform(2)
    W0, G0 = U.starts(pp.init_factors, lens, ranks)
    m = pp.CPMulti.with_ranks(ctx, t, ranks)
    m.set_factors(-1, W0, G0)                       # all at once: the blocks one after another
    Wall, Gall = m.get_factors(-1, with_grad=True)
    for b in range(len(ranks)):
        W, G = m.get_factors(b, with_grad=True)     # ... read back start by start
        for got in (W, Wall[b]):
            assert U.same(got, W0[b])
        for got in (G, Gall[b]):
            assert U.same(got, G0[b])
    W1, G1 = U.starts(pp.init_factors, lens, ranks, seed=1)
    m.set_factors(1, W1[1], G1[1])                  # one start replaced: the others stay
    Wall = m.get_factors(-1)
    for b in range(len(ranks)):
        assert U.same(Wall[b], W1[1] if b == 1 else W0[b])
    gn = m.gradnorms()
    for b in range(len(ranks)):
        want = np.sqrt(sum(np.sum(g * g) for g in (G1[1] if b == 1 else G0[b])))
        assert abs(gn[b] - want) < 1e-12 * want
    # the raw layout: start = -1 is the per-start Wflat blocks, each of its own length
    n = [sum(s * r for s in lens) for r in ranks]
    wf = np.empty(sum(n))
    pp._check(pp.lib().ppals_cp_multi_get_factors(m._h, -1, pp._dp(wf), None))
    at = 0
    for b in range(len(ranks)):
        one = np.empty(n[b])
        pp._check(pp.lib().ppals_cp_multi_get_factors(m._h, b, pp._dp(one), None))
        assert np.array_equal(wf[at:at + n[b]], one)
        assert np.array_equal(one, pp.flat(W1[1] if b == 1 else W0[b]))
        at += n[b]
    # ppals_cp_multi_ranks: with and without the array, on a session of the old constructor too
    L = pp.lib()
    k, arr = C.c_int(-1), (C.c_int * 8)(*([-7] * 8))
    assert L.ppals_cp_multi_ranks(m._h, C.byref(k), None) == 0 and k.value == 3
    assert L.ppals_cp_multi_ranks(m._h, C.byref(k), arr) == 0 and list(arr) == ranks + [-7] * 5
    old = pp.CPMulti(ctx, t, 2, 4)
    assert old.ranks == [2, 2, 2, 2] and old.R == 2
    assert L.ppals_cp_multi_ranks(old._h, C.byref(k), arr) == 0 and k.value == 4 and list(arr)[:5] == [2] * 4 + [-7]
    assert L.ppals_cp_multi_ranks(None, C.byref(k), arr) == -3
    assert L.ppals_cp_multi_ranks(m._h, None, arr) == -3
    for h in (old, m, t):
        h.close()


@pytest.mark.parametrize("schedule", ["msdt", "dt"])
def test_equal_ranks_are_the_old_constructor_bit_for_bit(pp, ctx, schedule):
    lens, R, K = [7, 6, 5, 4], 3, 4
    t = pp.Tensor(ctx, lens, F64).fill_uniform(8)
    W0, G0 = U.starts(pp.init_factors, lens, [R] * K)
    old = pp.CPMulti(ctx, t, R, K)
    new = pp.CPMulti.with_ranks(ctx, t, [R] * K)
    assert new.ranks == old.ranks == [R] * K and new.R == R
    for m in (old, new):
        m.set_schedule(schedule)
        m.set_factors(-1, W0, G0)
        m.sweeps(3, 1e-3)
    for a, b in zip(U.state(old), U.state(new)):
        assert U.same(a, b)
    for h in (old, new, t):
        h.close()


def test_take_then_ordinary_sweeps(pp, ctx):
    lens, ranks = [7, 6, 5, 4], [2, 5, 3, 4]
    t = pp.Tensor(ctx, lens, F64).fill_uniform(8)
    W0, G0 = U.starts(pp.init_factors, lens, ranks)
    m = U.sweep(pp, ctx, t, ranks, W0, G0, 2)
    for b in (0, 2, 3):
        W, G = m.get_factors(b, with_grad=True)
        d = pp.CP(ctx, t, ranks[b])
        d.set_factors(pp.init_factors(lens, ranks[b], 1))
        d.sweeps_dt(1)                               # caches alive in the destination
        m.take(b, d)
        r = pp.CP(ctx, t, ranks[b])
        r.set_factors(W, G)
        Wd, Gd = d.get_factors(with_grad=True)
        assert U.same(Wd, W) and U.same(Gd, G)
        assert abs(d.gradnorm() - r.gradnorm()) < 1e-12 * r.gradnorm()
        d.sweeps_dt(2)
        r.sweeps_dt(2)
        assert U.same(d.get_factors(), r.get_factors())
        d.close()
        r.close()
    d = pp.CP(ctx, t, 4)                             # start 2 has rank 3
    with pytest.raises(pp.PpalsError, match=r"error -3.*rank 4.*rank 3"):
        m.take(2, d)
    assert pp.lib().ppals_cp_multi_take(m._h, 2, d._h) == -3
    # the multi session is untouched by take
    s = U.solo(pp, ctx, t, ranks[1], W0[1], G0[1], 2)
    U.check_start(m, 1, s, FTOL)
    for h in (s, d, m, t):
        h.close()


def test_run_waits_for_every_start_of_a_mixed_session(pp, ctx):
    """an exact rank-2 tensor; start 0 is the true rank-2 model with zero gradients (converged at sweep
    0: the smallest residual, gradient norm 0), start 1 a rank-3 model from random factors (not
    converged). A uniform session would stop at once on the best start's gradient; the mixed one stops
    only when the largest gradient norm is under tol"""
    lens, ranks = [6, 5, 4, 5], [2, 3]
    Wtrue = pp.init_factors(lens, 2, 77)
    t = pp.Tensor(ctx, lens, F64).fill_cp(Wtrue)
    W1 = pp.init_factors(lens, 3, 5)
    G1 = pp.init_factors(lens, 3, 6)
    m = pp.CPMulti.with_ranks(ctx, t, ranks)
    m.set_factors(0, Wtrue, [np.zeros_like(w) for w in Wtrue])
    m.set_factors(1, W1, G1)
    gn, res = m.gradnorms(), m.residuals()
    assert gn[0] == 0.0 and gn[1] > 1.0 and res[0] < 1e-12 < res[1]
    tol = 0.5 * gn[1]
    rc, sweeps, best = m.run(tol=tol, maxiter=3, resprint=1)   # start 0 is under tol from the first look on
    gn = m.gradnorms()
    print("sweeps", sweeps, "gradnorms", gn, "tol", tol)
    assert sweeps >= 1 and best == int(np.argmin(m.residuals())) == 0
    assert (rc == 1 and gn.max() < tol) or (rc == 0 and sweeps == 3)
    # the same pair of looks, replayed by hand: the run stopped at the first look with every start under tol
    ref = pp.CPMulti.with_ranks(ctx, t, ranks)
    ref.set_factors(0, Wtrue, [np.zeros_like(w) for w in Wtrue])
    ref.set_factors(1, W1, G1)
    n = 0
    while n < 3 and not ref.gradnorms().max() < tol:
        ref.sweeps(1)
        n += 1
    assert n == sweeps
    for a, b in zip(U.state(m), U.state(ref)):
        assert U.same(a, b)
    # a tolerance every start meets at the first look: no sweep; the time limit
    rc, sweeps, _ = m.run(tol=2.0 * gn.max() + 1.0, maxiter=50, resprint=1)
    assert (rc, sweeps) == (1, 0)
    rc, sweeps, _ = m.run(tol=0.0, timelimit=0.0, maxiter=50, resprint=1)
    assert rc == 1 and sweeps <= 1
    for h in (ref, m, t):
        h.close()


def test_refusals_leave_the_session_sweeping(pp, ctx):
    lens = [6, 5, 4]
    t = pp.Tensor(ctx, lens, F64).fill_uniform(1)
    ranks = [2, 3, 1]
    W0, G0 = U.starts(pp.init_factors, lens, ranks)
    m = pp.CPMulti.with_ranks(ctx, t, ranks)
    twin = pp.CPMulti.with_ranks(ctx, t, ranks)
    for h in (m, twin):
        h.set_factors(-1, W0, G0)
    for nstarts, rk in ((3, None), (3, [2, 0, 1]), (2, [3, -1]), (0, [1]), (33, [1] * 33), (-1, [1]),
                        (3, [64, 64, 1]), (32, [4] * 31 + [5])):   # NULL, rank 0, nstarts, 129 columns twice
        rc, h = create_rc(pp, ctx, t, nstarts, rk)
        assert rc == -3 and not h.value, (nstarts, rk, rc)
        assert pp.lib().ppals_last_error()
    for rk in ([], [0], [1] * 33, [127, 2]):
        with pytest.raises(pp.PpalsError, match="error -3"):
            pp.CPMulti.with_ranks(ctx, t, rk)
    assert pp.lib().ppals_cp_multi_create_ranks(ctx._h, t._h, 1, (C.c_int * 1)(2), None) == -3
    rc, h = create_rc(pp, ctx, t, 2, [64, 64])      # the limits themselves are admitted
    assert rc == 0
    pp.lib().ppals_cp_multi_destroy(h)
    for start in (-2, 3):
        with pytest.raises(pp.PpalsError, match="error -3.*start"):
            m.set_factors(start, W0[0])
        with pytest.raises(pp.PpalsError, match="error -3.*start"):
            m.get_factors(start)
    # set_nonneg with a rank above 64: unsupported, the flag stays off
    big = pp.CPMulti.with_ranks(ctx, t, [2, 65])
    with pytest.raises(pp.PpalsError, match="error -5"):
        big.set_nonneg(True)
    assert not big.nonneg
    big.sweeps(1)
    big.close()
    # after all of that the session sweeps as its untouched twin
    m.sweeps(2)
    twin.sweeps(2)
    for a, b in zip(U.state(m), U.state(twin)):
        assert U.same(a, b)
    # non-negative factors with a negative entry in the SECOND start's block only
    pos = [[np.abs(w) + 0.1 for w in W] for W in W0]
    for h in (m, twin):
        h.set_factors(-1, pos)
        h.set_nonneg(True)
    bad = [[w.copy() for w in W] for W in pos]
    bad[1][2][3, 2] = -1e-300                       # last mode, last row and column of start 1's block
    with pytest.raises(pp.PpalsError, match="error -3"):
        m.set_factors(-1, bad)
    with pytest.raises(pp.PpalsError, match="error -3"):
        m.set_factors(1, bad[1])
    m.set_factors(0, bad[0])                        # (start 0's own block is clean)
    m.set_factors(2, bad[2])
    # turning the flag on over a start with a negative entry: refused, the flag stays off
    for h in (m, twin):
        h.set_nonneg(False)
        h.set_factors(-1, bad)
    with pytest.raises(pp.PpalsError, match="error -3"):
        m.set_nonneg(True)
    assert not m.nonneg
    for h in (m, twin):
        h.set_factors(-1, pos)
        h.set_nonneg(True)
        h.sweeps(2)
    for a, b in zip(U.state(m), U.state(twin)):
        assert U.same(a, b)
    for h in (m, twin, t):
        h.close()


@pytest.mark.parametrize("schedule", MC.SCHEDULES)
@pytest.mark.parametrize("lam", MC.LAMBDAS)
@pytest.mark.parametrize("dtype", [F32, F64])
def test_non_negative_mixed_session(pp, ctx, dtype, lam, schedule):
    lens, ranks = (9, 8, 7), [2, 4, 3]
    V, W0 = U.nonneg_problem(lens, ranks, 300)
    bar = MC.PAIR_BARS["hostsim"][dtype]
    t = pp.Tensor(ctx, list(lens), dtype).upload(V)
    m = U.sweep(pp, ctx, t, ranks, W0, None, MC.SWEEPS, lam, schedule, nonneg=True)
    assert m.nonneg
    d = U.nonneg_pair_deviation(pp, ctx, t, m, W0, lam, schedule, MC.SWEEPS)
    print(d, bar)
    for q in U.FIGURES:
        assert d[q] <= bar[q], (q, d[q], bar[q])
    assert min(w.min() for W in m.get_factors(-1) for w in W) >= MC.FLOOR
    m.close()
    t.close()
