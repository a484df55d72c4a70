"""Rank-sweep sessions (ppals_cp_multi_create_ranks) on the GPU: starts of DIFFERENT ranks ride the same
tensor scans, and one launch with a workgroup per start — each with its own rank, column block, Grams and
system, all from a table in the kernel arguments (k_cp_mode_update_ragged, k_cp_update_nn_ragged,
k_gram_ragged) — updates a mode. Every start must evolve as an ordinary session of its own rank does under
cpd_als with PPALS_OPT_SIMPLE from the same factors, to the bars of tests/test_gpu_multistart.py
(FTOL = 1e-5 / 1e-8 / 1e-5 for F32 / F64 / BF16 storage); the non-negative pairing to
multistart_nonneg_cases.PAIR_BARS. Counted checks read the launch profile; nothing uses a stopwatch."""
import os
import subprocess
import sys

import numpy as np
import pytest

import multistart_nonneg_cases as MC
import oracle_lib as O
import ranksweep_util as U

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

F32, F64, BF16 = 0, 1, 3
FTOL = {F32: 1e-5, F64: 1e-8, BF16: 1e-5}
NSWEEPS = 3


def update_lds(R):
    """bytes of LDS the fused mode update needs beside its staged M and W (hip_ops.hip)"""
    return 8 * (32 + 2 * R * R + 2 * R * (R + 1) + 64) + 4 * 64


def staged(rows, R):
    return update_lds(R) + 2 * 8 * rows * R <= 150 * 1024


# A mode so long that the launch is UNSTAGED at the largest rank and staged at the smallest, and short
# enough (rows * R_max <= 6144) not to take the start-by-start loop. R_max = 48: update_lds = 75520 B, so
# 75520 + 768 rows > 153600 from rows = 102 on, and 48 rows <= 6144 up to rows = 128. The other modes (64,
# 60 rows) are staged for every start.
UNSTAGED = ([104, 64, 60], [2, 48, 5])
assert not staged(104, 48) and staged(101, 48) and 104 * 48 <= 6144
assert staged(104, 2) and staged(104, 5) and staged(64, 48) and staged(60, 48)

# (lens, ranks, storage types)
ALL = (F32, F64, BF16)
CASES = [
    ([12, 11, 10, 9], [2, 5, 3, 4], ALL),          # the ordinary case
    ([10, 8, 9], [1, 4, 2, 7], ALL),               # a rank-1 start, order 3
    ([16, 12, 10, 9], [16, 10, 16, 12, 16], ALL),  # 70 columns: the scan route above 64
    ([16, 12, 10, 9], [1, 33, 64], ALL),           # 98 columns: the largest staged system beside a 1 x 1 one
    ([12, 10, 8, 6], [70, 10], (F64,)),            # a rank above 64: the loop route
    UNSTAGED + ((F32, F64),),                      # unstaged at R_max, staged at the smallest rank
]
CASES = [(lens, ranks, dt) for lens, ranks, dts in CASES for dt in dts]


def _id(v):
    if isinstance(v, (list, tuple)):
        return "x".join(map(str, v))
    return {F32: "F32", F64: "F64", BF16: "BF16"}[v] if isinstance(v, int) else str(v)


@pytest.fixture(scope="module")
def pp():
    import ppals
    return ppals


@pytest.fixture(scope="module")
def ctx(pp):
    c = pp.Context(0)
    yield c
    c.close()


_V = {}


def tensor_of(lens):
    """one dense tensor per shape, shared and never changed: uniform in [-1, 1). Zero mean on purpose: a
    positive tensor is nearly rank 1, its rank-1 start converges within the three sweeps, and a converged
    start's gradient W S - M is a rounding residue of M (1e-7 of it with F32 storage) that no relative bar
    on the gradient norm can hold; noise keeps every rank's gradient at the size of M. It also gives every
    rank of a sweep a well-conditioned system, unlike an exact low-rank tensor at the larger ranks"""
    key = tuple(lens)
    if key not in _V:
        _V[key] = O.fill_uniform(int(np.prod(lens)), 86 + len(lens), lo=-1.0, hi=1.0).reshape(lens, order="F")
    return _V[key]


@pytest.mark.parametrize("lens,ranks,dtype", CASES, ids=_id)
def test_starts_match_ordinary_sessions(pp, ctx, lens, ranks, dtype):
    t = pp.Tensor(ctx, lens, dtype).upload(tensor_of(lens))
    W0, G0 = U.starts(O.init_factors, lens, ranks)
    m = U.sweep(pp, ctx, t, ranks, W0, G0, NSWEEPS)
    res, gn = m.residuals(), m.gradnorms()
    for b, r in enumerate(ranks):
        s = U.solo(pp, ctx, t, r, W0[b], G0[b], NSWEEPS)
        U.check_start(m, b, s, FTOL[dtype], res, gn)
        s.close()
    m.close()
    t.close()


@pytest.mark.parametrize("schedule", ["msdt", "dt"])
@pytest.mark.parametrize("lens,ranks,lam", [([12, 11, 10, 9], [2, 5, 3, 4], 0.0), ([10, 8, 9], [1, 4, 2, 7], 1e-3),
                                            ([12, 11, 10, 9], [2, 5, 3, 4], 1e-3), ([10, 8, 9], [1, 4, 2, 7], 0.0)],
                         ids=_id)
def test_starts_match_the_oracle(pp, ctx, lens, ranks, lam, schedule):
    V = tensor_of(lens)
    t = pp.Tensor(ctx, lens, F64).upload(V)
    W0, G0 = U.starts(O.init_factors, lens, ranks, seed=5)
    m = U.sweep(pp, ctx, t, ranks, W0, G0, NSWEEPS, lam, schedule)
    for b in range(len(ranks)):
        _, _, _, W_ref, G_ref = O.cpd_als(V, W0[b], G0[b], 0, tol=0.0, maxsweep=NSWEEPS - 1, lam=lam,
                                          resprint=10 ** 9)
        W, G = m.get_factors(b, with_grad=True)
        for a, r in zip(W, W_ref):
            print("start", b, "factor error", U.relerr(a, r))
            assert U.relerr(a, r) < 1e-8, (b, U.relerr(a, r))
        for a, r in zip(G, G_ref):
            assert np.linalg.norm(a - r) < 100 * 1e-8 * (1 + np.linalg.norm(r))
    m.close()
    t.close()


@pytest.mark.parametrize("dtype", [F32, F64])
def test_a_singular_start_leaves_the_others_alone(pp, ctx, dtype):
    """start 1 (rank 4) has two identical columns in every factor: with a small lambda > 0 its S is
    nearly singular and that workgroup alone takes the inverse's fallback; starts 0 and 2, of ranks 3 and
    5 in the same launch, match their solo runs"""
    lens, ranks, lam = [12, 10, 9, 11], [3, 4, 5], 1e-10
    t = pp.Tensor(ctx, lens, dtype).upload(tensor_of(lens))
    W0, G0 = U.starts(O.init_factors, lens, ranks, seed=9)
    for w in W0[1]:
        w[:, 1] = w[:, 0]
    m = U.sweep(pp, ctx, t, ranks, W0, G0, NSWEEPS, lam)
    for b in (0, 2):
        s = U.solo(pp, ctx, t, ranks[b], W0[b], G0[b], NSWEEPS, lam)
        U.check_start(m, b, s, FTOL[dtype])
        s.close()
    m.close()
    t.close()


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("lens,ranks", [([12, 11, 10, 9], [2, 5, 3, 4]), UNSTAGED], ids=_id)
def test_reproducible_and_uncoupled(pp, ctx, lens, ranks, dtype):
    """two sessions from the same starts are bit-identical after 3 sweeps; changing start 1's initial
    factors leaves every other start bit-identical (a wrong column, Gram or system offset would leak)"""
    t = pp.Tensor(ctx, lens, dtype).upload(tensor_of(lens))
    W0, G0 = U.starts(O.init_factors, lens, ranks)
    other = [w * (1 + 0.05 * np.random.default_rng(77).random(w.shape)) for w in W0[1]]
    runs = []
    for w1 in (W0[1], W0[1], other):
        m = U.sweep(pp, ctx, t, ranks, [W0[0], w1] + W0[2:], G0, NSWEEPS, 1e-3)
        runs.append(U.state(m))
        m.close()
    for b in range(len(ranks)):
        assert U.same(runs[0][b], runs[1][b]), b
        assert U.same(runs[0][b], runs[2][b]) == (b != 1), b
    t.close()


@pytest.mark.parametrize("dtype", [F32, F64])
def test_equal_ranks_are_the_old_constructor_bit_for_bit(pp, ctx, dtype):
    lens, R, K = [12, 11, 10, 9], 5, 4
    t = pp.Tensor(ctx, lens, dtype).upload(tensor_of(lens))
    W0, G0 = U.starts(O.init_factors, lens, [R] * K)
    old = pp.CPMulti(ctx, t, R, K)
    old.set_factors(-1, W0, G0)
    old.sweeps(NSWEEPS, 1e-3)
    new = U.sweep(pp, ctx, t, [R] * K, W0, G0, NSWEEPS, 1e-3)
    assert new.ranks == old.ranks == [R] * K
    for a, b in zip(U.state(old), U.state(new)):
        assert U.same(a, b)
    for h in (old, new, t):
        h.close()


def _profile(ctx, level, slot, fn):
    ctx.sync()
    ctx.profile_enable(level)
    ctx.profile_reset()
    fn()
    ctx.sync()
    n, _, by = ctx.profile_read(slot)
    ctx.profile_enable(0)
    return n, by


def test_the_tensor_is_read_once_for_all_ranks(pp, ctx):
    lens, ranks, n = [40, 40, 40, 40], [4, 10, 6, 20], 3
    t = pp.Tensor(ctx, lens, F32).fill_uniform(5)
    W0, G0 = U.starts(O.init_factors, lens, ranks)
    m = pp.CPMulti.with_ranks(ctx, t, ranks)
    m.set_factors(-1, W0, G0)
    wide = pp.CP(ctx, t, sum(ranks))
    wide.set_factors([np.hstack([W0[b][i] for b in range(len(ranks))]) for i in range(len(lens))])
    got = _profile(ctx, 1, 0, lambda: m.sweeps(n))
    want = _profile(ctx, 1, 0, lambda: wide.cpd_als(0, tol=0.0, maxiter=n - 1, resprint=10 ** 9))
    print("scan launches / bytes: rank sweep", got, "R = 40 session", want)
    assert got[0] > 0 and got == want
    for h in (m, wide, t):
        h.close()


def test_one_launch_per_update_whatever_the_ranks(pp, ctx):
    """the bracketed non-scan kernels of a sweep do not grow with the number of starts or their ranks"""
    lens, n = [20, 12, 16, 10], 3
    t = pp.Tensor(ctx, lens, F32).fill_uniform(6)
    counts = {}
    for ranks in ([3, 5], [2, 3, 4, 5, 6, 7, 8]):
        W0, G0 = U.starts(O.init_factors, lens, ranks)
        m = pp.CPMulti.with_ranks(ctx, t, ranks)
        m.set_factors(-1, W0, G0)
        counts[len(ranks)] = _profile(ctx, 2, 1, lambda: m.sweeps(n))[0]
        m.close()
    print("other bracketed kernels in", n, "sweeps:", counts)
    assert counts[2] >= n * len(lens)          # at least the mode updates themselves
    assert counts[7] <= counts[2]
    t.close()


NN_CASES = [((9, 8, 7), [2, 4, 3]), ((16, 12, 10, 9), [1, 33, 64])]


@pytest.mark.parametrize("dtype", [F32, F64, BF16], ids=_id)
@pytest.mark.parametrize("lens,ranks", NN_CASES, ids=_id)
def test_non_negative_mixed_session(pp, ctx, lens, ranks, dtype):
    V, W0 = U.nonneg_problem(lens, ranks, 300)
    bar = MC.PAIR_BARS["hip"][dtype]
    t = pp.Tensor(ctx, list(lens), dtype).upload(V)
    for lam in MC.LAMBDAS:
        for schedule in MC.SCHEDULES:
            m = U.sweep(pp, ctx, t, ranks, W0, None, MC.SWEEPS, lam, schedule, nonneg=True)
            d = U.nonneg_pair_deviation(pp, ctx, t, m, W0, lam, schedule, MC.SWEEPS)
            print(lens, ranks, dtype, lam, schedule, d, bar)
            for q in U.FIGURES:
                assert d[q] <= bar[q], (lam, schedule, q, d[q], bar[q])
            assert min(w.min() for W in m.get_factors(-1) for w in W) >= MC.FLOOR
            m.close()
    t.close()


def test_non_negative_update_is_two_launches_whatever_the_ranks(pp, ctx):
    """one bracket per mode update — the row kernel and the finishing launch inside it — for both rank
    lists and for a uniform session of as many starts: the bracketed non-scan counts of three sweeps agree"""
    n = 3
    counts = {}
    for lens, ranks in NN_CASES:
        V, W0 = U.nonneg_problem(lens, ranks, 300)
        t = pp.Tensor(ctx, list(lens), F32).upload(V)
        m = pp.CPMulti.with_ranks(ctx, t, ranks)
        m.set_nonneg(True)
        m.set_factors(-1, W0)
        mixed = _profile(ctx, 2, 1, lambda: m.sweeps(n))[0]
        m.close()
        R = min(ranks)
        u = pp.CPMulti(ctx, t, R, len(ranks))
        u.set_nonneg(True)
        u.set_factors(-1, [[w[:, :R] for w in W] for W in W0])
        uniform = _profile(ctx, 2, 1, lambda: u.sweeps(n))[0]
        u.close()
        t.close()
        print(lens, ranks, "bracketed non-scan launches: mixed", mixed, "uniform", uniform)
        counts[tuple(ranks)] = (mixed, uniform, len(lens))
    for mixed, uniform, N in counts.values():
        assert mixed >= n * N and mixed <= uniform


@pytest.mark.parametrize("dtype", [F32, F64])
def test_tensor_refill_while_a_mixed_session_is_alive(pp, ctx, dtype):
    lens, ranks = [12, 10, 8, 6], [2, 4, 3]
    V1 = O.build_V(O.init_factors(lens, 3, 1004))
    V2 = tensor_of(lens)
    W0, G0 = U.starts(O.init_factors, lens, ranks)
    t = pp.Tensor(ctx, lens, dtype).upload(V1)
    m = U.sweep(pp, ctx, t, ranks, W0, G0, 2)   # the second layout and the cached contractions hold V1 now
    t.upload(V2)
    m.set_factors(-1, W0, G0)
    m.sweeps(NSWEEPS)
    t2 = pp.Tensor(ctx, lens, dtype).upload(V2)
    fresh = U.sweep(pp, ctx, t2, ranks, W0, G0, NSWEEPS)
    for b in range(len(ranks)):
        for a, r in zip(m.get_factors(b), fresh.get_factors(b)):
            assert U.relerr(a, r) < FTOL[dtype], (b, U.relerr(a, r))
    s = U.solo(pp, ctx, t2, ranks[1], W0[1], G0[1], NSWEEPS)
    U.check_start(m, 1, s, FTOL[dtype])
    for h in (s, fresh, m, t2, t):
        h.close()


def test_take_then_pp_and_model_export():
    """start 2 of ranks [2, 5, 3, 4] into a rank-3 session, then the model export and a PP run as after
    set_factors with the same values; a rank-4 destination is refused. The export goes through torch,
    which must be imported before the library is loaded: a child process (tests/ranksweep_cases.py)"""
    e = dict(os.environ, PYTHONNOUSERSITE="1")
    p = subprocess.run([sys.executable, os.path.join(HERE, "ranksweep_cases.py"), "take"],
                       cwd=os.path.dirname(HERE), env=e, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, f"exit {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-6000:]}"
    assert "ranksweep case take: ok" in p.stdout
