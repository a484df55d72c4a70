"""Hold-out rows per start of a multi-start session (ppals_cp_multi_set_holdout): the cases shared by
tests/test_holdout_hostsim.py (the host stand-in) and tests/test_gpu_holdout.py (the HIP engine). `pp` is the
binding either of them loaded. The pairing under test: start b of a hold-out session against an ORDINARY
session of the same library on the reduced tensor (np.compress along the sample mode, uploaded from numpy),
from the same factors, under cpd_als / PPALS_OPT_SIMPLE."""
import numpy as np

import corcondia_ref as CR
import holdout_ref as H

F32, F64, BF16 = 0, 1, 3


def relerr(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def truth(lens, R, seed):
    rng = np.random.default_rng(seed)
    return [rng.random((s, R)) for s in lens], rng


def tensor(lens, R, seed):
    """a non-negative rank-R tensor plus 1 % uniform noise (no exact fit: the gradients stay away from 0)"""
    A, rng = truth(lens, R, seed)
    V = CR.cp_tensor(A)
    return np.asfortranarray(V + 0.01 * V.max() * rng.random(lens))


def keep_table(pp, n, K):
    """start 0 keeps everything, start g leaves out the interleaved segment g - 1 of K"""
    return np.vstack([np.ones((1, n), dtype=bool), pp.holdout_segments(n, K)])


def draw(lens, ranks, seed, around=None):
    """per start: factors and gradients in U(0, 1) (a non-negative session takes them too). around = (R, seed)
    of tensor(): the factors are that tensor's true ones plus 0.1 U(0, 1) instead — see WELL-CONDITIONED below"""
    rng = np.random.default_rng(seed)
    A = truth(lens, *around)[0] if around else None
    W = [[np.asfortranarray((A[i][:, :r] if A else 0.0) + (0.1 if A else 1.0) * rng.random((s, r)))
          for i, s in enumerate(lens)] for r in ranks]
    G = [[np.asfortranarray(rng.random((s, r))) for s in lens] for r in ranks]
    return W, G


# WELL-CONDITIONED. The two sessions of a pairing work on tensors of different extents, so their fp32
# intermediates are rounded in different orders (unlike two sessions on ONE tensor, whose columns see the same
# sums): a difference of a few fp32 ulps per contraction comes back from every solve multiplied by cond(S). The
# bars of that pairing (1e-5 for fp32 / bf16 storage) leave room for cond(S) of the order of 100 over three
# sweeps, not for the 10^3 .. 10^5 that ALS iterates from RANDOM starts pass through at these shapes (numpy,
# tests/holdout_ref.py). So the parity cases start near the tensor's true factors, where cond(S) stays below
# 75 on every case of both suites (also measured in numpy, on the reference's iterates, not on the library's).
def compress(Ws, mode, keep):
    return [np.asfortranarray(w[keep]) if i == mode else w for i, w in enumerate(Ws)]


def session(pp, ctx, t, ranks, schedule="msdt", nonneg=False):
    m = pp.CPMulti(ctx, t, ranks[0], len(ranks)) if len(set(ranks)) == 1 else pp.CPMulti.with_ranks(ctx, t, ranks)
    m.set_schedule(schedule)
    if nonneg:
        m.set_nonneg(True)
    return m


def reduced(pp, ctx, V, dtype, mode, keep, R, W, G, n, lam, schedule, nonneg):
    """(tensor, session): an ordinary session on V without the held-out slices, n sweeps from (W, G) compressed"""
    tr = pp.Tensor(ctx, [int(np.sum(keep)) if i == mode else s for i, s in enumerate(V.shape)], dtype)
    tr.upload(np.compress(keep, V, axis=mode))
    s = pp.CP(ctx, tr, R)
    s.set_schedule(schedule)
    if nonneg:
        s.set_nonneg(True)
    s.set_factors(compress(W, mode, keep), compress(G, mode, keep))
    if n > 0:
        s.cpd_als(0, tol=0.0, maxiter=n - 1, lam=lam, resprint=10 ** 9)   # maxsweep + 1 sweeps
    return tr, s


def check_against(m, b, s, mode, keep, tol, gfac, what):
    """check_start of tests/test_gpu_multistart.py with the sample mode compressed, gradient norms included, and
    the exact conditions of a hold-out start"""
    W_ref, G_ref = s.get_factors(with_grad=True)
    W, G = m.get_factors(b, with_grad=True)
    sc = m.heldout_scores(b)
    assert np.all(W[mode][~keep] == 0.0) and np.all(G[mode][~keep] == 0.0), what
    assert np.all(sc[keep] == 0.0), what
    errs = [relerr(a, r) for a, r in zip(compress(W, mode, keep), W_ref)]
    gerrs = [np.linalg.norm(a - r) / (1 + np.linalg.norm(r)) for a, r in zip(compress(G, mode, keep), G_ref)]
    gn, gn_ref = m.gradnorms()[b], s.gradnorm()
    print(f"[holdout] {what} start {b}: factor errors {errs} gradient errors {gerrs} gradnorm {gn} {gn_ref}")
    assert max(errs) < tol, (what, b, errs)
    assert max(gerrs) < gfac * tol, (what, b, gerrs)
    # The gradient norm. gfac == 1 (the stand-in, fp64 throughout): relative, as tests/test_multistart_hostsim.py
    # has it. On the device the gradient -M + W S is a difference of terms far larger than itself near a
    # solution, which is why check_start bounds a gradient by gfac * tol * (1 + its norm), not relatively; the
    # norm of all N gradients can then differ by no more than the norm of those N bounds (triangle inequality),
    # and that is its bar — nothing narrower follows from the bars of the gradients themselves.
    gn_bar = tol * gn_ref + 1e-14 if gfac == 1.0 else \
        np.sqrt(sum((gfac * tol * (1 + np.linalg.norm(r))) ** 2 for r in G_ref))
    assert abs(gn - gn_ref) < gn_bar, (what, b, gn, gn_ref, gn_bar)
    return W, G, sc


def parity(pp, ctx, dtype, lens, ranks, mode, keep, tol, gfac, schedule="msdt", lam=0.0, nonneg=False, n=3,
           seed=0, against_ref=False, residual_tol=None):
    """every start of a hold-out session against the ordinary session on its reduced tensor — before any sweep
    and after n — plus: take_predicted bitwise W + scores; against_ref: scores, factors and gradients against
    tests/holdout_ref.py (fp64 storage); residual_tol: the kept samples' sample_residuals add up to the reduced
    session's residual()^2"""
    what = f"dtype {dtype} lens {lens} ranks {ranks} mode {mode} {schedule} lam {lam} nonneg {nonneg}"
    V = tensor(lens, max(ranks), 1000 + seed)
    t = pp.Tensor(ctx, lens, dtype).upload(V)
    W0, G0 = draw(lens, ranks, 2000 + seed, around=(max(ranks), 1000 + seed))
    m = session(pp, ctx, t, ranks, schedule, nonneg)
    m.set_holdout(mode, keep)
    got = m.holdout
    assert got[0] == mode and np.array_equal(got[1], keep)
    m.set_factors(-1, W0, G0)
    for sweeps in (0, n):
        if sweeps:
            m.sweeps(sweeps, lam)
        for b, R in enumerate(ranks):
            tr, s = reduced(pp, ctx, V, dtype, mode, keep[b], R, W0[b], G0[b], sweeps, lam, schedule, nonneg)
            W, G, sc = check_against(m, b, s, mode, keep[b], tol, gfac, f"{what} sweeps {sweeps}")
            if sweeps == 0:   # the caller's rows moved, bit for bit
                assert np.array_equal(sc[~keep[b]], W0[b][mode][~keep[b]])
                assert np.array_equal(W[mode][keep[b]], W0[b][mode][keep[b]])
            d = pp.CP(ctx, t, R)
            m.take_predicted(b, d)
            Wd, Gd = d.get_factors(with_grad=True)
            for i in range(len(lens)):
                assert np.array_equal(Wd[i], W[i] + sc if i == mode else W[i]), (what, b, i)
                assert np.array_equal(Gd[i], G[i]), (what, b, i)
            if nonneg and sweeps:   # predicted scores come out of the HALS row update
                assert np.all(sc[~keep[b]] >= 1e-16) and np.all(W[mode][keep[b]] >= 1e-16)
            if residual_tol is not None:
                ss = m.sample_residuals(b, d)
                want = s.residual() ** 2
                assert abs(np.sum(ss[keep[b]]) - want) < residual_tol * want, (what, b, np.sum(ss[keep[b]]), want)
            if against_ref and sweeps:
                Wr, Gr, scr = H.als_holdout(CR.stored(V, dtype), W0[b], G0[b], mode, keep[b], sweeps, lam)
                errs = [relerr(a, r) for a, r in zip(W, Wr)] + [relerr(sc, scr)] if not np.all(keep[b]) else \
                    [relerr(a, r) for a, r in zip(W, Wr)]
                print(f"[holdout] {what} start {b}: against numpy {errs}")
                assert max(errs) < tol, (what, b, errs)
                for a, r in zip(G, Gr):
                    assert np.linalg.norm(a - r) < gfac * tol * (1 + np.linalg.norm(r))
            for h in (d, s, tr):
                h.close()
    m.close()
    t.close()


def untouched_start(pp, ctx, dtype, lens, ranks, mode, nonneg=False, n=3):
    """a start that holds nothing out is bit for bit the same start of a session of the same ranks with no
    hold-out set; repeated reads give identical bits"""
    V = tensor(lens, max(ranks), 1100)
    t = pp.Tensor(ctx, lens, dtype).upload(V)
    W0, G0 = draw(lens, ranks, 2100, around=(max(ranks), 1100))
    keep = np.ones((len(ranks), lens[mode]), dtype=bool)
    keep[1:] = pp.holdout_segments(lens[mode], len(ranks) - 1)
    out = []
    for hold in (True, False):
        m = session(pp, ctx, t, ranks, nonneg=nonneg)
        if hold:
            m.set_holdout(mode, keep)
        m.set_factors(-1, W0, G0)
        m.sweeps(n)
        out.append(m.get_factors(0, with_grad=True) + (m.gradnorms()[0],))
        if hold:
            again = [m.heldout_scores(1), m.heldout_scores(1)]
            assert np.array_equal(again[0], again[1])
            W1, W1b = m.get_factors(1), m.get_factors(1)
            assert all(np.array_equal(a, b) for a, b in zip(W1, W1b))
        m.close()
    (Wa, Ga, gna), (Wb, Gb, gnb) = out
    assert all(np.array_equal(a, b) for a, b in zip(Wa, Wb))
    assert all(np.array_equal(a, b) for a, b in zip(Ga, Gb))
    assert gna == gnb
    t.close()


def same_bits_twice(pp, ctx, dtype, lens, ranks, mode, keep, n=2):
    """the same state gives the same bits: two sessions run alike agree in every bit of every start"""
    V = tensor(lens, max(ranks), 1200)
    t = pp.Tensor(ctx, lens, dtype).upload(V)
    W0, G0 = draw(lens, ranks, 2200, around=(max(ranks), 1200))
    runs = []
    for _ in range(2):
        m = session(pp, ctx, t, ranks)
        m.set_holdout(mode, keep)
        m.set_factors(-1, W0, G0)
        m.sweeps(n)
        runs.append((m.get_factors(-1, with_grad=True), [m.heldout_scores(b) for b in range(len(ranks))],
                     m.gradnorms()))
        m.close()
    (Fa, Sa, ga), (Fb, Sb, gb) = runs
    for Xa, Xb in zip(Fa, Fb):
        for wa, wb in zip(Xa, Xb):
            assert all(np.array_equal(a, b) for a, b in zip(wa, wb))
    assert all(np.array_equal(a, b) for a, b in zip(Sa, Sb)) and np.array_equal(ga, gb)
    t.close()


def core_consistency(pp, ctx, dtype, lens, R, mode, K, n=3):
    """cc of a hold-out start is the cc of its factors on the reduced tensor: the checker and the bars of
    tests/corcondia_ref.py, for the hold-out start and for the ordinary session on the reduced tensor"""
    V = tensor(lens, R, 1300)
    t = pp.Tensor(ctx, lens, dtype).upload(V)
    keep = keep_table(pp, lens[mode], K)
    W0, G0 = draw(lens, [R] * (K + 1), 2300, around=(R, 1300))
    m = session(pp, ctx, t, [R] * (K + 1))
    m.set_holdout(mode, keep)
    m.set_factors(-1, W0, G0)
    m.sweeps(n)
    cc = m.core_consistencies()
    for b in range(K + 1):
        Vr = CR.stored(np.compress(keep[b], V, axis=mode), dtype)
        CR.check(f"hold-out start {b}", Vr, compress(m.get_factors(b), mode, keep[b]), dtype, cc[b])
        tr, s = reduced(pp, ctx, V, dtype, mode, keep[b], R, W0[b], G0[b], n, 0.0, "msdt", False)
        CR.check(f"reduced session {b}", Vr, s.get_factors(), dtype, s.core_consistency())
        s.close()
        tr.close()
    m.close()
    t.close()
