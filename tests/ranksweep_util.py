"""Helpers shared by the rank-sweep suites (tests/test_ranksweep_hostsim.py, tests/test_gpu_ranksweep.py,
tests/ranksweep_cases.py): a multi-start session whose starts have their own ranks
(ppals_cp_multi_create_ranks) against ordinary sessions of those ranks, start by start."""
import numpy as np

import multistart_nonneg_cases as MC
import nonneg_cases as NC

FIGURES = MC.FIGURES


def relerr(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def starts(init, lens, ranks, seed=0):
    """start b: factors and gradients of rank ranks[b] (init = the binding's or the oracle's init_factors)"""
    W = [init(lens, r, 2000 + 31 * b + seed) for b, r in enumerate(ranks)]
    G = [init(lens, r, 7000 + 29 * b + seed) for b, r in enumerate(ranks)]
    return W, G


def sweep(pp, ctx, t, ranks, W0, G0, n, lam=0.0, schedule="msdt", nonneg=False):
    m = pp.CPMulti.with_ranks(ctx, t, ranks)
    m.set_schedule(schedule)
    if nonneg:
        m.set_nonneg(True)
    m.set_factors(-1, W0, G0)
    m.sweeps(n, lam)
    return m


def solo(pp, ctx, t, R, W, G, n, lam=0.0, schedule="msdt", nonneg=False):
    """an ordinary rank-R session advanced by n sweeps of the class API's Simple optimizer (no Normalize)"""
    s = pp.CP(ctx, t, R)
    s.set_schedule(schedule)
    if nonneg:
        s.set_nonneg(True)
    s.set_factors(W, G)
    if n > 0:
        s.cpd_als(0, tol=0.0, maxiter=n - 1, lam=lam, resprint=10 ** 9)   # maxsweep + 1 sweeps
    return s


def check_start(m, b, s, tol, res=None, gn=None):
    """start b against the ordinary session s, the checks of tests/test_gpu_multistart.py"""
    W_ref, G_ref = s.get_factors(with_grad=True)
    W, G = m.get_factors(b, with_grad=True)
    errs = [relerr(a, r) for a, r in zip(W, W_ref)]
    gerrs = [np.linalg.norm(a - r) / (1 + np.linalg.norm(r)) for a, r in zip(G, G_ref)]
    print("start", b, "rank", m.ranks[b], "factor errors", errs, "gradient errors", gerrs)
    assert [w.shape for w in W] == [(n, m.ranks[b]) for n in m.lens]
    assert max(errs) < tol, (b, errs)
    assert max(gerrs) < 100 * tol, (b, gerrs)
    if res is not None:
        r_ref, g_ref = s.residual(), s.gradnorm()
        print("start", b, "residual", res[b], r_ref, "gradnorm", gn[b], g_ref)
        assert abs(res[b] - r_ref) < tol * r_ref
        assert abs(gn[b] - g_ref) < tol * g_ref + 1e-14


def state(m):
    """everything a run leaves behind, start by start"""
    res, gn = m.residuals(), m.gradnorms()
    out = []
    for b in range(m.nstarts):
        W, G = m.get_factors(b, with_grad=True)
        out.append(W + G + [np.array(gn[b]), np.array(res[b])])
    return out


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def nonneg_problem(lens, ranks, seed):
    """a non-negative tensor and one non-negative start per rank, in the manner of
    multistart_nonneg_cases.inputs: the problem of nonneg_cases at the largest rank; start b is the first
    ranks[b] columns of its starting factors (near the truth's: no column dies) times (1 + p u_b)"""
    V, Wfull = NC.problem(lens, max(ranks), seed)
    p = 0.1 if max(ranks) <= min(lens) else 0.01
    W0 = []
    for b, r in enumerate(ranks):
        rng = np.random.default_rng(9000 + 31 * b + seed)
        W0.append([np.asfortranarray(w[:, :r] * (1 + p * rng.random((w.shape[0], r)))) for w in Wfull])
    return V, W0


def nonneg_pair_deviation(pp, ctx, t, m, W0, lam, schedule, n):
    """multistart_nonneg_cases.pair_deviation for starts of their own ranks: the four figures, the worst
    over the starts, against ordinary non-negative sessions from the same factors"""
    Vnorm = np.linalg.norm(t.download())
    res, gn = m.residuals(), m.gradnorms()
    worst = dict.fromkeys(FIGURES, 0.0)
    for b, r in enumerate(m.ranks):
        s = solo(pp, ctx, t, r, W0[b], None, n, lam, schedule, nonneg=True)
        W_ref, G_ref = s.get_factors(with_grad=True)
        W, G = m.get_factors(b, with_grad=True)
        d = {"factors": max(relerr(a, x) for a, x in zip(W, W_ref)),
             "grad": max(np.linalg.norm(a - x) / (1 + np.linalg.norm(x)) for a, x in zip(G, G_ref)),
             "gradnorm": abs(gn[b] - s.gradnorm()) / (1 + s.gradnorm()),
             "residual": abs(res[b] - s.residual()) / Vnorm}
        s.close()
        for q in FIGURES:
            worst[q] = max(worst[q], d[q]) if np.isfinite(d[q]) else np.inf
    return worst
