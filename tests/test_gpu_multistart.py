"""Multi-start CP sessions (ppals_cp_multi) on the GPU: K starts of rank R ride the same tensor scans on
K * R columns, and one batched launch (a workgroup per start) solves the K normal equations of a mode
update. Every start must evolve as an ordinary session of the same tensor does under cpd_als with
PPALS_OPT_SIMPLE from the same factors — to the bars the project holds that pairing to: FTOL = 1e-5
for F32 and BF16 storage (tests/test_gpu_bf16.py), 1e-8 for F64 (tests/test_gpu_cp.py FTOL[1]).
The counted checks read the launch profile (ppals_profile_read); nothing here uses a stopwatch."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
from test_gpu_bf16 import SHAPES

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

F32, F64, BF16 = 0, 1, 3
FTOL = {F32: 1e-5, F64: 1e-8, BF16: 1e-5}
NSWEEPS = 3
MAXCOLS = 128
# every K of the issue that the column limit R * K <= 128 admits, on the shape list of the bf16 suite
# (R = 10: 40 and 70 columns, the route above 64), plus a 64-column case (R = 16, K = 4)
CASES = [(lens, R, K) for lens, R in SHAPES + [([16, 12, 10, 9], 16)] for K in (1, 2, 4, 7)
         if R * K <= MAXCOLS]
assert {40, 64, 70} <= {R * K for _, R, K in CASES}


@pytest.fixture(scope="module")
def pp():
    import ppals
    return ppals


@pytest.fixture(scope="module")
def ctx(pp):
    c = pp.Context(0)
    yield c
    c.close()


def relerr(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def starts(lens, R, K, seed=0):
    W = [O.init_factors(lens, R, 2000 + 31 * b + seed) for b in range(K)]
    G = [O.init_factors(lens, R, 7000 + 29 * b + seed) for b in range(K)]
    return W, G


def solo(pp, ctx, t, R, W, G, n, lam=0.0, schedule="msdt"):
    s = pp.CP(ctx, t, R)
    s.set_schedule(schedule)
    s.set_factors(W, G)
    s.cpd_als(0, tol=0.0, maxiter=n - 1, lam=lam, resprint=10 ** 9)   # maxsweep + 1 sweeps
    return s


def check_start(m, b, s, tol):
    W_ref, G_ref = s.get_factors(with_grad=True)
    W, G = m.get_factors(b, with_grad=True)
    errs = [relerr(a, r) for a, r in zip(W, W_ref)]
    print("start", b, "factor errors", errs)
    assert max(errs) < tol, (b, errs)
    for a, r in zip(G, G_ref):
        assert np.linalg.norm(a - r) < 100 * tol * (1 + np.linalg.norm(r)), b


@pytest.mark.parametrize("dtype", [F32, F64, BF16])
@pytest.mark.parametrize("lens,R,K", CASES)
def test_starts_match_ordinary_sessions(pp, ctx, lens, R, K, dtype):
    V = O.build_V(O.init_factors(lens, R, 1003))
    t = pp.Tensor(ctx, lens, dtype).upload(V)
    W0, G0 = starts(lens, R, K)
    m = pp.CPMulti(ctx, t, R, K)
    m.set_factors(-1, W0, G0)
    m.sweeps(NSWEEPS)
    res, gn = m.residuals(), m.gradnorms()
    tol = FTOL[dtype]
    for b in range(K):
        s = solo(pp, ctx, t, R, W0[b], G0[b], NSWEEPS)
        check_start(m, b, s, tol)
        r_ref, g_ref = s.residual(), s.gradnorm()
        print("start", b, "residual", res[b], r_ref, "gradnorm", gn[b], g_ref)
        assert abs(res[b] - r_ref) < tol * r_ref
        assert abs(gn[b] - g_ref) < tol * g_ref
        s.close()
    m.close()
    t.close()


@pytest.mark.parametrize("schedule", ["msdt", "dt"])
@pytest.mark.parametrize("lens,R,K,lam", [([8, 7, 6, 5], 3, 2, 0.0), ([10, 8, 9], 4, 4, 1e-3),
                                          ([12, 10, 8, 6], 10, 7, 0.0)])
def test_starts_match_the_oracle(pp, ctx, lens, R, K, lam, schedule):
    """directly against the oracle's restatement of CPD::als with the Simple optimizer (fp64 storage),
    as tests/test_gpu_cp.py checks the class-API runs"""
    V = O.build_V(O.init_factors(lens, R, 1005))
    t = pp.Tensor(ctx, lens, F64).upload(V)
    W0, G0 = starts(lens, R, K, seed=5)
    m = pp.CPMulti(ctx, t, R, K)
    m.set_schedule(schedule)
    for b in range(K):
        m.set_factors(b, W0[b], G0[b])
    m.sweeps(NSWEEPS, lam)
    for b in range(K):
        _, _, _, W_ref, G_ref = O.cpd_als(V, W0[b], G0[b], 0, tol=0.0, maxsweep=NSWEEPS - 1, lam=lam,
                                          resprint=10 ** 9)
        W, G = m.get_factors(b, with_grad=True)
        for a, r in zip(W, W_ref):
            assert relerr(a, r) < 1e-8, (b, relerr(a, r))
        for a, r in zip(G, G_ref):
            assert np.linalg.norm(a - r) < 100 * 1e-8 * (1 + np.linalg.norm(r))
    m.close()
    t.close()


@pytest.mark.parametrize("dtype", [F32, F64])
def test_a_singular_start_leaves_the_others_alone(pp, ctx, dtype):
    """start 1 has two identical columns in every factor: with a small lambda > 0 its S is nearly
    singular and that workgroup alone takes the inverse's fallback route; starts 0 and 2 of the same
    launch match their solo runs"""
    lens, R, K = [12, 10, 9, 11], 4, 3
    V = O.build_V(O.init_factors(lens, R, 1007))
    lam = 1e-10
    t = pp.Tensor(ctx, lens, dtype).upload(V)
    W0, G0 = starts(lens, R, K, seed=9)
    for w in W0[1]:
        w[:, 1] = w[:, 0]
    m = pp.CPMulti(ctx, t, R, K)
    m.set_factors(-1, W0, G0)
    m.sweeps(NSWEEPS, lam)
    for b in (0, 2):
        s = solo(pp, ctx, t, R, W0[b], G0[b], NSWEEPS, lam)
        check_start(m, b, s, FTOL[dtype])
        s.close()
    m.close()
    t.close()


def _scan_profile(ctx, fn):
    ctx.sync()
    ctx.profile_enable(1)
    ctx.profile_reset()
    fn()
    ctx.sync()
    n, _, by = ctx.profile_read(0)
    ctx.profile_enable(0)
    return n, by


def test_the_tensor_is_read_once_for_all_starts(pp, ctx):
    lens, R, K, n = [40, 40, 40, 40], 10, 4, 3
    t = pp.Tensor(ctx, lens, F32).fill_uniform(5)
    W0, G0 = starts(lens, R, K)
    m = pp.CPMulti(ctx, t, R, K)
    m.set_factors(-1, W0, G0)
    wide = pp.CP(ctx, t, R * K)
    wide.set_factors([np.hstack([W0[b][i] for b in range(K)]) for i in range(len(lens))])
    one = pp.CP(ctx, t, R)
    one.set_factors(W0[0], G0[0])
    got = _scan_profile(ctx, lambda: m.sweeps(n))
    kw = dict(tol=0.0, maxiter=n - 1, resprint=10 ** 9)
    want = _scan_profile(ctx, lambda: wide.cpd_als(0, **kw))
    single = _scan_profile(ctx, lambda: one.cpd_als(0, **kw))
    print("scan launches / bytes: multi", got, "R = 40 session", want, "R = 10 session", single)
    assert got[0] > 0 and got == want
    assert got[1] < K * single[1]
    for h in (m, wide, one, t):
        h.close()


def test_one_launch_per_batched_update(pp, ctx):
    """the bracketed non-scan kernels of a sweep (the mttv chain and the mode updates) do not grow with
    the number of starts: every mode update is one launch whatever K is"""
    lens, R, n = [20, 12, 16, 10], 10, 3
    t = pp.Tensor(ctx, lens, F32).fill_uniform(6)
    counts = {}
    for K in (2, 7):
        W0, G0 = starts(lens, R, K)
        m = pp.CPMulti(ctx, t, R, K)
        m.set_factors(-1, W0, G0)
        ctx.sync()
        ctx.profile_enable(2)
        ctx.profile_reset()
        m.sweeps(n)
        ctx.sync()
        counts[K] = ctx.profile_read(1)[0]
        ctx.profile_enable(0)
        m.close()
    print("other bracketed kernels in", n, "sweeps:", counts)
    assert counts[2] >= n * len(lens)          # at least the mode updates themselves
    assert counts[7] <= counts[2]
    t.close()


@pytest.mark.parametrize("dtype", [F32, F64])
def test_tensor_refill_while_a_multi_session_is_alive(pp, ctx, dtype):
    lens, R, K = [12, 10, 8, 6], 3, 3
    V1 = O.build_V(O.init_factors(lens, R, 1004))
    V2 = O.fill_uniform(int(np.prod(lens)), 86, lo=0.5, hi=1.0).reshape(lens, order="F")
    W0, G0 = starts(lens, R, K)
    t = pp.Tensor(ctx, lens, dtype).upload(V1)
    m = pp.CPMulti(ctx, t, R, K)
    m.set_factors(-1, W0, G0)
    m.sweeps(2)                # the second layout and the cached contractions hold V1 now
    t.upload(V2)
    m.set_factors(-1, W0, G0)
    m.sweeps(NSWEEPS)
    t2 = pp.Tensor(ctx, lens, dtype).upload(V2)
    fresh = pp.CPMulti(ctx, t2, R, K)
    fresh.set_factors(-1, W0, G0)
    fresh.sweeps(NSWEEPS)
    for b in range(K):
        for a, r in zip(m.get_factors(b), fresh.get_factors(b)):
            assert relerr(a, r) < FTOL[dtype], (b, relerr(a, r))
    s = solo(pp, ctx, t2, R, W0[1], G0[1], NSWEEPS)
    check_start(m, 1, s, FTOL[dtype])
    for h in (s, fresh, m, t2, t):
        h.close()


def test_take_then_pp_and_model_export():
    """take() into an ordinary session, then run_pp and the model export behave as after set_factors
    with the same values. The export goes through torch, which must be imported before the library is
    loaded: a child process of its own (tests/multistart_cases.py), like tests/test_gpu_model_export.py"""
    e = dict(os.environ, PYTHONNOUSERSITE="1")
    p = subprocess.run([sys.executable, os.path.join(HERE, "multistart_cases.py"), "take"],
                       cwd=os.path.dirname(HERE), env=e, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, f"exit {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-6000:]}"
    assert "multistart case take: ok" in p.stdout
