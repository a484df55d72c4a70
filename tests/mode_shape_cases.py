"""Shapes on non-negative modes of CP sessions (ppals_cp_set_mode_shapes, include/ppals.h): a numpy fp64
restatement of a sweep with a kind and a shape per mode, and the cases of tests/test_gpu_mode_shapes.py (one per
process: `python mode_shape_cases.py <case>`, the exit status is the verdict) and tests/test_mode_shapes_hostsim.py
(the same functions, called with the host stand-in's binding: the ops.h default of the update).

The sweep is that of tests/nonneg_cases.py (MTTKRP by einsum on the tensor as download() returns it, grad = -M +
W S with the pre-update W, Normalize as tests/numpy_ref.py) with, per mode, the solve, the HALS pass or the
column loop of tests/shape_cases.py (shape_update: brute force over the split, textbook PAVA).

The bars of `sweeps` are those tests/nonneg_cases.py holds the all-NONNEG session to (NC.BARS: 10 x what the
UNCONSTRAINED session deviates from numpy, per back end and storage type): a projection onto a convex cone is
1-Lipschitz as the clamp is, and the split of a unimodal fit is discrete — a restatement and a session that
disagree on it differ by far more than any bar, so the bar also says that they agree."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import nonneg_cases as NC  # noqa: E402
import numpy_ref as NR  # noqa: E402
import shape_cases as SC  # noqa: E402
from bf16_util import same_values  # noqa: E402

SWEEPS = 5
LAMBDAS = (0.0, 1e-3)
SCHEDULES = ("msdt", "dt")
SHAPE_CODE = {"none": 0, "unimodal": SC.UNIMODAL, "increasing": SC.INCREASING, "decreasing": SC.DECREASING}
# (lens, R, kinds, shapes): order 3 and order 4, one unimodal and one increasing mode, NONNEG everywhere or mixed
TABLE = [
    ((40, 9, 7), 3, ("nonneg", "nonneg", "nonneg"), ("unimodal", "increasing", "none")),
    ((40, 9, 7), 3, ("nonneg", "nonneg", "free"), ("unimodal", "increasing", "none")),
    ((12, 33, 6, 5), 3, ("nonneg", "nonneg", "nonneg", "nonneg"), ("increasing", "unimodal", "none", "none")),
    ((12, 33, 6, 5), 3, ("free", "nonneg", "nonneg", "free"), ("none", "unimodal", "increasing", "none")),
]


def problem(lens, R, shapes, seed, noise=0.05):
    """a tensor of Gaussian-peak (unimodal modes), rising (increasing), falling (decreasing) and non-negative
    random (the rest) factors plus `noise` x its mean of uniform noise, and a positive start 20 % off the truth"""
    rng = np.random.default_rng(seed)
    A = []
    for s, sh in zip(lens, shapes):
        x = np.arange(s, dtype=float)[:, None]
        if sh == "unimodal":
            a = np.exp(-0.5 * ((x - rng.uniform(0.2 * s, 0.8 * s, R)[None, :]) / rng.uniform(0.08 * s, 0.2 * s, R)[None, :]) ** 2)
        elif sh in ("increasing", "decreasing"):
            a = np.cumsum(rng.random((s, R)), axis=0) / s + 0.1 * rng.random(R)[None, :]
            a = a[::-1].copy() if sh == "decreasing" else a
        else:
            a = 0.2 + rng.random((s, R))
        A.append(a)
    V = np.einsum(",".join(NR.LET[j] + "z" for j in range(len(lens))) + "->" + NR.LET[:len(lens)], *A)
    V = V + noise * np.mean(V) * rng.random(lens)
    W0 = [a * (1 + 0.2 * rng.random(a.shape)) + 0.2 * a.mean() * rng.random(a.shape) for a in A]
    return np.asfortranarray(V), W0


def ms_sweep(V, W, G, lam, kinds, shapes, normalize=True):
    """one sweep; returns (W, per-mode scale ||W_old S|| + ||grad||, per-mode factor Normalize applied)"""
    W = [w.copy() for w in W]
    scales = []
    for i, (kind, sh) in enumerate(zip(kinds, shapes)):
        M = NR._mttkrp(V, W, i)
        S = NR._S(W, i, lam)
        WS = W[i] @ S
        G[i] = -M + WS
        scales.append(np.linalg.norm(WS) + np.linalg.norm(G[i]))
        if kind == "free":
            W[i] = M @ NR._svd_inverse(S)
        elif sh == "none":
            W[i], _ = NC.hals_update(M, W[i], S)
        else:
            W[i] = SC.shape_update(M, W[i], S, SHAPE_CODE[sh])
    if not normalize:
        return W, scales, [1.0] * V.ndim
    norms = [np.linalg.norm(w) for w in W]
    gmean = float(np.prod(norms)) ** (1.0 / V.ndim)
    return NR._normalize(W), scales, [gmean / x for x in norms]


def numpy_run(Vh, W0, lam, kinds, shapes, n=SWEEPS):
    W, G, scales, nfac = [w.copy() for w in W0], [np.zeros_like(w) for w in W0], None, None
    for _ in range(n):
        W, scales, nfac = ms_sweep(Vh, W, G, lam, kinds, shapes)
    return W, G, scales, nfac


def shaped_ok(W, kinds, shapes, nfac):
    """every column of a shaped mode has its shape and every entry of a NONNEG mode is >= the floor times the
    factor the sweep's Normalize applied (nonneg_cases.NORM_SLACK)"""
    for w, kind, sh, f in zip(W, kinds, shapes, nfac):
        if kind == "nonneg" and not w.min() >= NC.FLOOR * f * NC.NORM_SLACK:
            return False
        if sh != "none" and not all(SC.has_shape(w[:, r], SHAPE_CODE[sh]) for r in range(w.shape[1])):
            return False
    return True


def session(pp, ctx, lens, R, dtype, V, W0, sched, kinds, shapes):
    t = pp.Tensor(ctx, list(lens), dtype).upload(V)
    s = pp.CP(ctx, t, R)
    s.set_schedule(sched)
    s.set_factors(W0)
    if kinds is not None:
        s.set_mode_constraints(kinds)
    if shapes is not None:
        s.set_mode_shapes(shapes)
        assert s.mode_shapes == list(shapes)
    return t, s


# ---------------------------------------------------------------------------- cases
def case_sweeps(pp, ctx, table=TABLE):
    """five sweeps against numpy on F64 and F32 storage, both schedules, lambda 0 and 1e-3, within NC.BARS"""
    bars = NC.BARS[NC.backend(pp)]
    for k, (lens, R, kinds, shapes) in enumerate(table):
        V, W0 = problem(lens, R, shapes, 700 + k)
        for dtype in (pp.F32, pp.F64):
            bar = bars[int(dtype)]
            for lam in LAMBDAS:
                for sched in SCHEDULES:
                    t, s = session(pp, ctx, lens, R, dtype, V, W0, sched, kinds, shapes)
                    Vh = t.download()
                    W_ref, G_ref, scales, nfac = numpy_run(Vh, W0, lam, kinds, shapes)
                    s.sweeps_dt(SWEEPS, lam)
                    d = NC.deviation(s, Vh, W_ref, G_ref, scales)
                    print(f"  {lens} R={R} {kinds} {shapes} dtype={int(dtype)} {sched} lambda={lam:g}: "
                          + " ".join(f"{q} {d[q]:.3g} (bar {bar[q]:.3g})" for q in d), flush=True)
                    assert shaped_ok(W_ref, kinds, shapes, nfac) and shaped_ok(s.get_factors(), kinds, shapes, nfac)
                    for q in d:
                        assert d[q] <= bar[q], (lens, R, kinds, int(dtype), sched, lam, q, d[q], bar[q])
                    s.close()
                    t.close()


def case_properties(pp, ctx):
    """after every one of 20 sweeps every column of a shaped mode has its shape and is >= the floor (times the
    sweep's Normalize factor); on F64 storage the residual never rises by more than 1e-9 relative from the
    first sweep on (each column step minimises exactly over a set that holds the current column once the
    factor is feasible) — the numpy restatement first"""
    for k, (lens, R, kinds, shapes) in enumerate(TABLE):
        V, W0 = problem(lens, R, shapes, 700 + k)
        W, G = [w.copy() for w in W0], [np.zeros_like(w) for w in W0]
        prev, nfacs = None, []
        for it in range(20):
            W, _, nfac = ms_sweep(V, W, G, 0.0, kinds, shapes)
            cur = NR._residual(V, W)
            assert prev is None or cur <= prev * (1 + 1e-9), ("numpy", lens, it, prev, cur)
            assert shaped_ok(W, kinds, shapes, nfac), ("numpy", lens, it)
            nfacs.append(nfac)
            prev = cur
        for sched in SCHEDULES:
            t, s = session(pp, ctx, lens, R, pp.F64, V, W0, sched, kinds, shapes)
            prev = None
            for it in range(20):
                s.sweeps_dt(1)
                cur = s.residual()
                assert shaped_ok(s.get_factors(), kinds, shapes, nfacs[it]), (lens, sched, it)
                assert prev is None or cur <= prev * (1 + 1e-9), (lens, sched, it, prev, cur)
                prev = cur
            print(f"  {lens} R={R} {kinds} {sched}: residual after 20 sweeps {cur:.6g}", flush=True)
            s.close()
            t.close()


RECOVERS = dict(lens=(40, 9, 7), R=3, seed=741, noise=0.6, sweeps=10)


def unimodal_columns(w):
    return sum(SC.has_shape(w[:, r], SC.UNIMODAL) for r in range(w.shape[1]))


def case_recovers(pp, ctx):
    """on the noisy peaked tensor the unimodal session's loadings of mode 0 are unimodal and the all-NONNEG
    session's, from the same start, are not — in the numpy restatement first"""
    lens, R = RECOVERS["lens"], RECOVERS["R"]
    kinds, shapes = ("nonneg",) * 3, ("unimodal", "none", "none")
    V, W0 = problem(lens, R, shapes, RECOVERS["seed"], RECOVERS["noise"])
    for sh in (shapes, ("none",) * 3):
        W, _, _, _ = numpy_run(V, W0, 0.0, kinds, sh, RECOVERS["sweeps"])
        assert unimodal_columns(W[0]) == (R if sh[0] == "unimodal" else 0), ("numpy", sh, unimodal_columns(W[0]))
    for sched in SCHEDULES:
        for sh in (shapes, ("none",) * 3):
            t, s = session(pp, ctx, lens, R, pp.F64, V, W0, sched, kinds, sh)
            s.sweeps_dt(RECOVERS["sweeps"])
            got = unimodal_columns(s.get_factors()[0])
            print(f"  {sched} shapes {sh}: {got} of {R} loadings of mode 0 are unimodal", flush=True)
            assert got == (R if sh[0] == "unimodal" else 0), (sched, sh, got)
            s.close()
            t.close()


def _counts(ctx, make, body):
    h = make()
    ctx.sync()
    ctx.profile_enable(2)
    ctx.profile_reset()
    body(h)
    ctx.sync()
    out = (ctx.profile_read(0)[0], ctx.profile_read(1)[0])
    ctx.profile_enable(0)
    return h, out


def case_none_is_free(pp, ctx):
    """a session whose shapes are all NONE, and one where a shape was set and cleared, take the same launches
    (profile counters) and give the same bits as an untouched NONNEG session"""
    for k, (lens, R, kinds, shapes) in enumerate(TABLE[:3:2]):
        V, W0 = problem(lens, R, shapes, 700 + k)
        for dtype in (pp.F32, pp.F64):
            for sched in SCHEDULES:
                got = []
                for touch in ("never", "none", "cleared"):
                    def make():
                        t, s = session(pp, ctx, lens, R, dtype, V, W0, sched, kinds, None)
                        if touch == "none":
                            s.set_mode_shapes(["none"] * len(lens))
                        if touch == "cleared":
                            s.set_mode_shapes(shapes)
                            s.set_mode_shapes(["none"] * len(lens))
                        assert s.mode_shapes == ["none"] * len(lens)
                        s._keep = t
                        return s
                    s, booked = _counts(ctx, make, lambda s: s.sweeps_dt(3, 1e-3))
                    W, G = s.get_factors(with_grad=True)
                    got.append((booked, W + G + [np.array(s.gradnorm()), np.array(s.residual())]))
                    s.close()
                    s._keep.close()
                for booked, arrays in got[1:]:
                    assert booked == got[0][0], (lens, int(dtype), sched, booked, got[0][0])
                    assert all(same_values(a, b) for a, b in zip(arrays, got[0][1])), (lens, int(dtype), sched)
                print(f"  {lens} dtype={int(dtype)} {sched}: scans / other launches {got[0][0]} three times over", flush=True)


def case_multi(pp, ctx):
    """start b of a multi-start session (ranks 3, 3, 3) and of a rank sweep (ranks 2, 3, 5) against an ordinary
    session of the same start: factors and gradients bit for bit"""
    lens, kinds, shapes = (40, 9, 7), ("nonneg",) * 3, ("unimodal", "increasing", "none")
    V, _ = problem(lens, 5, shapes, 760)
    for ranks in ((3, 3, 3), (2, 3, 5)):
        starts = [problem(lens, r, shapes, 770 + b)[1] for b, r in enumerate(ranks)]
        for dtype in (pp.F32, pp.F64):
            for sched in SCHEDULES:
                t = pp.Tensor(ctx, list(lens), dtype).upload(V)
                m = (pp.CPMulti(ctx, t, ranks[0], len(ranks)) if len(set(ranks)) == 1
                     else pp.CPMulti.with_ranks(ctx, t, ranks))
                m.set_schedule(sched)
                m.set_factors(-1, starts)
                m.set_mode_constraints(kinds)
                m.set_mode_shapes(shapes)
                assert m.mode_shapes == list(shapes)
                m.sweeps(3, 1e-3)
                for b, r in enumerate(ranks):
                    s = pp.CP(ctx, t, r)
                    s.set_schedule(sched)
                    s.set_factors(starts[b])
                    s.set_mode_constraints(kinds)
                    s.set_mode_shapes(shapes)
                    s.cpd_als(0, maxiter=2, tol=0.0, lam=1e-3, resprint=1 << 20)   # 3 sweeps, no Normalize
                    Wm, Gm = m.get_factors(b, with_grad=True)
                    Ws, Gs = s.get_factors(with_grad=True)
                    worst = max(NC.relerr(a, x) for a, x in zip(Wm + Gm, Ws + Gs))
                    print(f"  ranks {ranks} start {b} dtype={int(dtype)} {sched}: worst relative difference {worst:.3g}",
                          flush=True)
                    assert all(same_values(a, x) for a, x in zip(Wm + Gm, Ws + Gs)), (ranks, b, int(dtype), sched, worst)
                    assert shaped_ok(Wm, kinds, shapes, [1.0] * 3)
                    s.close()
                m.close()
                t.close()


def case_em(pp, ctx):
    """run_em with a 20 % mask and a unimodal mode runs, lowers the observed residual, and the loadings keep
    the shape"""
    import torch
    lens, R, kinds, shapes = (40, 9, 7), 3, ("nonneg", "nonneg", "free"), ("unimodal", "increasing", "none")
    V, W0 = problem(lens, R, shapes, 780)
    g = torch.Generator(device="cpu").manual_seed(3)
    mask = (torch.rand(lens, generator=g) >= 0.2).to(f"cuda:{ctx.device}")
    for dtype in (pp.F32, pp.F64):
        t, s = session(pp, ctx, lens, R, dtype, V, W0, "msdt", kinds, shapes)
        start = s.impute_torch(mask, want_residual=True)
        t.upload(V)
        rc, iters, end = s.run_em(mask, inner_sweeps=2, maxiter=10, resprint=5)
        print(f"  dtype={int(dtype)}: observed residual {start:.6g} -> {end:.6g} in {iters} iterations", flush=True)
        assert iters == 10 and end < start, (start, end, iters)
        W = s.get_factors()
        assert unimodal_columns(W[0]) == R and all(SC.has_shape(W[1][:, r], SC.INCREASING) for r in range(R))
        assert W[0].min() > 0 and W[1].min() > 0
        s.close()
        t.close()


def _refused(pp, code, prefix, fn, *a, **kw):
    try:
        fn(*a, **kw)
    except pp.PpalsError as e:
        assert f"ppals error {code}: {prefix}" in str(e), (code, prefix, str(e))
        return
    raise AssertionError(f"not refused: {fn}")


def case_refusals(pp, ctx):
    """every row of the rules of include/ppals.h: the code, the function's name in front of the message, shapes
    and kinds unchanged afterwards; a kind that leaves NONNEG clears the shape"""
    import ctypes as C
    L = pp.lib()
    lens, R, kinds, shapes = TABLE[1]
    V, W0 = problem(lens, R, shapes, 701)
    t, s = session(pp, ctx, lens, R, pp.F64, V, W0, "msdt", kinds, shapes)
    t2, ref = session(pp, ctx, lens, R, pp.F64, V, W0, "msdt", kinds, shapes)
    fn, mfn = "ppals_cp_set_mode_shapes", "ppals_cp_multi_set_mode_shapes"
    arr = (C.c_int * 3)(0, 0, 0)
    for f in (L.ppals_cp_set_mode_shapes, L.ppals_cp_get_mode_shapes, L.ppals_cp_multi_set_mode_shapes,
              L.ppals_cp_multi_get_mode_shapes):
        assert f(None, arr) == -3
    assert L.ppals_cp_set_mode_shapes(s._h, None) == -3 and L.ppals_cp_get_mode_shapes(s._h, None) == -3
    _refused(pp, -3, fn, s.set_mode_shapes, [1, 4, 0])
    _refused(pp, -3, fn, s.set_mode_shapes, [-1, 0, 0])
    _refused(pp, -3, fn, s.set_mode_shapes, ["unimodal", "none", "increasing"])   # (mode 2 is FREE)
    assert s.mode_shapes == list(shapes) and s.mode_constraints == list(kinds)
    # the kinds stay 0..3: a fifth kind is refused as before, and leaves kinds and shapes
    _refused(pp, -3, "ppals_cp_set_mode_constraints", s.set_mode_constraints, [0, 4, 0])
    assert s.mode_shapes == list(shapes) and s.mode_constraints == list(kinds)
    # everything NONNEG refuses stays refused
    _refused(pp, -5, "ppals_cp_pp", s.run_pp, maxiter=3)
    _refused(pp, -5, "ppals_cp_pp_partupdate", s.run_pp_partupdate, maxiter=3)
    _refused(pp, -5, "ppals_cpd_als_lr", s.cpd_als_lr, 3, 1, maxiter=2)
    # R > 64: no NONNEG mode to put a shape on
    lens65 = (70, 6, 5)
    V65, W65 = NC.problem(lens65, 65, 5)
    t65, s65 = session(pp, ctx, lens65, 65, pp.F64, V65, W65, "msdt", None, None)
    _refused(pp, -5, "ppals_cp_set_mode_constraints", s65.set_mode_constraints, ["nonneg", "free", "free"])
    _refused(pp, -3, fn, s65.set_mode_shapes, ["unimodal", "none", "none"])
    assert s65.mode_shapes == ["none"] * 3
    # the hold-out mode of a multi-start session has no shape, and a shaped mode is not held out
    m = pp.CPMulti(ctx, t, R, 2)
    m.set_factors(-1, [W0, W0])
    m.set_mode_constraints(["nonneg"] * 3)
    keep = np.ones((2, lens[0]), dtype=np.uint8)
    keep[0, 1] = 0
    m.set_holdout(0, keep)
    _refused(pp, -5, mfn, m.set_mode_shapes, ["unimodal", "none", "none"])
    m.set_mode_shapes(["none", "increasing", "none"])
    assert m.mode_shapes == ["none", "increasing", "none"]
    m.set_holdout(0, None)
    m.set_mode_shapes(["unimodal", "increasing", "none"])
    _refused(pp, -5, "ppals_cp_multi_set_holdout", m.set_holdout, 0, keep)
    _refused(pp, -3, mfn, m.set_mode_shapes, [0, 0, 7])
    assert m.mode_shapes == ["unimodal", "increasing", "none"] and m.mode_constraints == ["nonneg"] * 3
    # take copies factors and ignores shapes
    m.sweeps(1)
    m.take(0, s)
    assert s.mode_shapes == list(shapes) and s.mode_constraints == list(kinds)
    for a, b in zip(s.get_factors(), m.get_factors(0)):
        assert same_values(a, b)
    s.set_factors(W0)
    m.close()
    # nothing of the above touched the session: it sweeps exactly as one that never saw the calls
    s.sweeps_dt(2)
    ref.sweeps_dt(2)
    for a, b in zip(s.get_factors(), ref.get_factors()):
        assert same_values(a, b)
    # a kind that leaves NONNEG clears its mode's shape, and only that one; so does set_nonneg(False)
    s.set_mode_constraints(["nonneg", "free", "free"])
    assert s.mode_shapes == ["unimodal", "none", "none"]
    s.set_mode_constraints(["nonneg", "nonneg", "free"])
    assert s.mode_shapes == ["unimodal", "none", "none"]
    s.set_nonneg(False)
    assert s.mode_shapes == ["none"] * 3 and s.mode_constraints == ["free"] * 3
    _refused(pp, -3, fn, s.set_mode_shapes, ["unimodal", "none", "none"])
    s.set_factors(W0)
    s.set_nonneg(True)
    s.set_mode_shapes(["unimodal", "decreasing", "increasing"])
    assert s.mode_shapes == ["unimodal", "decreasing", "increasing"]
    s.sweeps_dt(1)
    assert np.isfinite(s.residual())
    for x in (s, ref, s65, t, t2, t65):
        x.close()


def case_blocked_hook(pp, ctx):
    """under PPALS_TEST_BLOCKED_UPDATE (read when a session is created) no mode becomes NONNEG (-5), so no mode
    takes a shape (-3, the function's name in front); the shapes stay all none and the session sweeps on.
    (The other row NONNEG refuses, more than one rank, needs a communicator: on the host stand-in
    tests/test_mode_shapes_hostsim.py builds one of two ranks from callbacks; on the device it would take a
    second GPU, which a single-GPU test run does not have.)"""
    lens, R, kinds, shapes = TABLE[0]
    V, W0 = problem(lens, R, shapes, 700)
    old = os.environ.get("PPALS_TEST_BLOCKED_UPDATE")
    os.environ["PPALS_TEST_BLOCKED_UPDATE"] = "2"
    try:
        t, s = session(pp, ctx, lens, R, pp.F64, V, W0, "msdt", None, None)
    finally:
        if old is None:
            del os.environ["PPALS_TEST_BLOCKED_UPDATE"]
        else:
            os.environ["PPALS_TEST_BLOCKED_UPDATE"] = old
    try:
        s.set_mode_constraints(kinds)
    except pp.PpalsError as e:
        assert "ppals error -5: ppals_cp_set_mode_constraints: " in str(e) and "PPALS_TEST_BLOCKED_UPDATE" in str(e), str(e)
    else:
        raise AssertionError("NONNEG under the blocked-update hook was not refused")
    _refused(pp, -3, "ppals_cp_set_mode_shapes", s.set_mode_shapes, shapes)
    assert s.mode_shapes == ["none"] * 3 and s.mode_constraints == ["free"] * 3
    s.set_mode_shapes(["none"] * 3)
    s.sweeps_dt(1)
    assert np.isfinite(s.residual())
    s.close()
    t.close()


LAUNCHES_PER_SHAPED_UPDATE = 3  # kernels_shape.hip.h: gradient, column loop, finish


def case_counted(pp, ctx):
    """the launch profile: a shaped update is three launches for 1, 4 and 12 starts, in place of the one bracket
    of the batched NONNEG update, and a sweep with a shaped mode books the scans of the NONNEG one"""
    lens, R = (33, 12, 10, 9), 10
    V, _ = NC.problem(lens, R, 101)
    t = pp.Tensor(ctx, list(lens), pp.F32).upload(V)
    got = {}
    for K in (1, 4, 12):
        def makeK(shape):
            def f():
                m = pp.CPMulti(ctx, t, R, K)
                m.set_factors(-1, [NC.problem(lens, R, 410 + b)[1] for b in range(K)])
                m.set_mode_constraints(["nonneg", "fixed", "fixed", "fixed"])
                m.set_mode_shapes([shape, "none", "none", "none"])
                return m
            return f
        for shape in ("unimodal", "increasing", "decreasing"):
            m, o = _counts(ctx, makeK(shape), lambda m: m.sweeps(1))
            m.close()
            m, n = _counts(ctx, makeK("none"), lambda m: m.sweeps(1))
            m.close()
            got[K, shape] = o[1] - (n[1] - 1)
            print(f"  K={K} {shape}: one sweep books {o} with the shaped update, {n} with the NONNEG one: "
                  f"{got[K, shape]} launches of the shaped update", flush=True)
            assert o[0] == n[0], (K, shape, o, n)
            assert got[K, shape] == LAUNCHES_PER_SHAPED_UPDATE, (K, shape, o, n)
    t.close()


CASES = {"sweeps": case_sweeps, "properties": case_properties, "recovers": case_recovers,
         "none_is_free": case_none_is_free, "multi": case_multi, "em": case_em, "refusals": case_refusals,
         "blocked_hook": case_blocked_hook, "counted": case_counted}


if __name__ == "__main__":
    import torch  # noqa: F401  (before the binding loads libppals: one HIP runtime for both)
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "pairwise-perturbation_amd"))
    import ppals as pp_
    ctx_ = pp_.Context(0)
    CASES[sys.argv[1]](pp_, ctx_)
    ctx_.close()
    print(f"mode shape case {sys.argv[1]}: ok")
