"""Non-negative CP sessions (ppals_cp_set_nonneg, include/ppals.h): a numpy fp64 restatement of the HALS
mode update and of a whole sweep, and the cases of tests/test_gpu_nonneg.py (one per process:
`python nonneg_cases.py <case>`, the exit status is the verdict) and tests/test_nonneg_hostsim.py (the same
functions, called with the host stand-in's binding: the ops.h default of the update).

The sweep: MTTKRP by einsum on the tensor as download() returns it (so an F32 session is compared on the
values it holds), grad = -M + W S with the pre-update W, one HALS pass, Normalize as tests/numpy_ref.py.

The bars (BARS below) are NOT taken from the code under test: they are 10 x what the UNCONSTRAINED session
deviates from tests/numpy_ref.py at the same shapes, storage types, schedules, lambdas and sweeps, measured
with `python nonneg_cases.py measure_bars` (profiles/nonneg_bars.md) — per storage type, the largest over
shapes, schedules and lambdas. max is 1-Lipschitz, so the clamp amplifies nothing; the 10 is for the R
sequential dependent steps that replace one solve. One measurement is left out of that maximum: at
(70, 6, 5), R = 64, lambda = 0 the unconstrained system is singular (S is 64 x 64 of rank <= 30), its solve
amplifies rounding to O(1) and a bar derived from it would say nothing (well_posed below). The non-negative
session is held to the bar there as everywhere: HALS divides by diagonal entries only."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import numpy_ref as NR  # noqa: E402

FLOOR = 1e-16   # PPALS_NN_FLOOR
SWEEPS = 3
LAMBDAS = (0.0, 1e-3)
SCHEDULES = ("msdt", "dt")
# one row tile; order 4; three row tiles with a ragged last one (130 = 2 * 64 + 2); the largest rank
# (the LDS bound of the kernel) over two tiles
SHAPES = [((9, 8, 7), 3), ((33, 12, 10, 9), 10), ((130, 9, 8), 17), ((70, 6, 5), 64)]
# Normalize multiplies a whole factor by one positive number (its own norm against the geometric mean of
# all of them), below 1 for some mode: an entry the update left ON the floor is then FLOOR times that
# number — positive, and back on the floor at the mode's next update. So right after an update, and
# after a sweep of the class API (no Normalize), every entry is >= FLOOR; after a sweep that ends in
# Normalize it is >= FLOOR * that mode's factor, which the numpy run supplies (the session's own differs
# from it by rounding, at most 4e-6 relative on F32 storage: NORM_SLACK).
NORM_SLACK = 1 - 1e-3
FTOL = {0: 1e-5, 1: 1e-8}   # tests/test_gpu_cp.py: both schedules against one reference, F32 / F64 storage


# ---------------------------------------------------------------------------- numpy restatement
def hals_update(M, W, S, floor=FLOOR):
    """w[x,r] <- max(floor, w[x,r] + (M[x,r] - sum_q w[x,q] S[q,r]) / S[r,r]), r ascending, the sum over
    the row as updated so far; rows are independent. Returns (W_new, entries that the max moved)."""
    W = W.copy()
    clamped = 0
    for r in range(W.shape[1]):
        d = S[r, r]
        if not (d > 0 and np.isfinite(d)):
            continue
        v = W[:, r] + (M[:, r] - W @ S[:, r]) / d
        clamped += int(np.sum(v < floor))
        W[:, r] = np.maximum(floor, v)
    return W, clamped


def _sweep(V, W, G, lam, update, normalize=True):
    """one sweep; returns (W, per-mode scale ||W_old S|| + ||grad|| that formed grad_W, clamped entries,
    per-mode factor Normalize applied: 1 without it)"""
    W = [w.copy() for w in W]
    scales, clamped = [], 0
    for i in range(V.ndim):
        M = NR._mttkrp(V, W, i)
        S = NR._S(W, i, lam)
        WS = W[i] @ S
        G[i] = -M + WS
        scales.append(np.linalg.norm(WS) + np.linalg.norm(G[i]))
        W[i], c = update(M, W[i], S)
        clamped += c
    if not normalize:
        return W, scales, clamped, [1.0] * V.ndim
    norms = [np.linalg.norm(w) for w in W]
    gmean = float(np.prod(norms)) ** (1.0 / V.ndim)
    return NR._normalize(W), scales, clamped, [gmean / x for x in norms]


def nn_sweep(V, W, G, lam, normalize=True):
    return _sweep(V, W, G, lam, hals_update, normalize)


def ls_sweep(V, W, G, lam):
    """the unconstrained sweep of tests/numpy_ref.py (_exact_sweep), with the same by-products"""
    return _sweep(V, W, G, lam, lambda M, Wi, S: (M @ NR._svd_inverse(S), 0))


def problem(lens, R, seed):
    """a non-negative tensor of sparse non-negative factors plus uniform noise, and positive starting
    factors: fitting the zeros of the true factors drives entries onto the floor"""
    rng = np.random.default_rng(seed)
    A = [np.maximum(0.0, rng.standard_normal((s, R))) for s in lens]
    for a in A:   # no all-zero column in the truth (a 5-row factor of 64 sparse columns would have some)
        for r in range(R):
            a[r % a.shape[0], r] = max(a[r % a.shape[0], r], 0.5)
    V = np.einsum(",".join(NR.LET[j] + "z" for j in range(len(lens))) + "->" + NR.LET[:len(lens)], *A)
    V = V + 0.05 * np.mean(V) * rng.random(lens)
    # a start near the truth, positive where the truth is zero: those entries are what the fit clamps, and
    # no column dies (a whole column on the floor makes S[r,r] ~ 1e-30 and the next division meaningless:
    # from an arbitrary start HALS does that in its first update here, in numpy as on the device)
    # (more columns than the shortest mode has rows — R = 64 on (70, 6, 5) — is over-parameterised: from
    # 20 % off the truth HALS empties the redundant columns within three sweeps, from 2 % off it does not)
    p = 0.2 if R <= min(lens) else 0.02
    W0 = [a * (1 + p * rng.random(a.shape)) + p * rng.random(a.shape) for a in A]
    return np.asfortranarray(V), W0


def relerr(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def deviation(s, Vh, W_ref, G_ref, scales):
    """what a session deviates from a numpy run: factors (worst relative Frobenius), grad_W (worst mode,
    relative to the scale that formed it), gradnorm (relative to that scale), residual (relative to ||V||)"""
    W_got, G_got = s.get_factors(with_grad=True)
    tot = np.sqrt(sum(x * x for x in scales))
    return {
        "factors": max(relerr(a, b) for a, b in zip(W_got, W_ref)),
        "grad": max(np.linalg.norm(a - b) / sc for a, b, sc in zip(G_got, G_ref, scales)),
        "gradnorm": abs(s.gradnorm() - NR._gradnorm(G_ref)) / tot,
        "residual": abs(s.residual() - NR._residual(Vh, W_ref)) / np.linalg.norm(Vh),
    }


def numpy_run(Vh, W0, lam, sweep, n=SWEEPS):
    W, G = [w.copy() for w in W0], [np.zeros_like(w) for w in W0]
    clamped, scales, nfac = 0, None, None
    for _ in range(n):
        W, scales, c, nfac = sweep(Vh, W, G, lam)
        clamped += c
    return W, G, scales, clamped, nfac


def above_floor(W, nfac):
    """every entry >= FLOOR * the factor the sweep's Normalize applied to its mode (see NORM_SLACK)"""
    return all(w.min() >= FLOOR * f * NORM_SLACK for w, f in zip(W, nfac))


def session(pp, ctx, lens, R, dtype, V, W0, sched, nonneg):
    t = pp.Tensor(ctx, list(lens), dtype).upload(V)
    s = pp.CP(ctx, t, R)
    s.set_schedule(sched)
    if nonneg:
        s.set_nonneg(True)
        assert s.nonneg
    s.set_factors(W0)
    return t, s


# 10 x the deviation of the UNCONSTRAINED session from tests/numpy_ref.py (profiles/nonneg_bars.md holds
# the measured values): BARS[back end][dtype] = the four figures of deviation()
BARS = {
    "hip": {
        0: {'factors': 0.0369, 'grad': 2.12e-05, 'gradnorm': 2.15e-07, 'residual': 1.63e-07},
        1: {'factors': 1.96e-09, 'grad': 5.68e-11, 'gradnorm': 6.17e-13, 'residual': 1.05e-12},
    },
    "hostsim": {
        0: {'factors': 0.019, 'grad': 9.72e-06, 'gradnorm': 6.96e-08, 'residual': 2.63e-07},
        1: {'factors': 2.72e-09, 'grad': 2.46e-10, 'gradnorm': 7.95e-12, 'residual': 1.15e-12},
    },
}


def backend(pp):
    return "hostsim" if b"hostsim" in pp.lib().ppals_version() else "hip"


def well_posed(lens, R, lam):
    """S of every mode can have full rank: R <= the product of the other extents, or lambda > 0"""
    return lam > 0 or all(R <= int(np.prod(lens)) // s for s in lens)


def measure_bars(pp, ctx, shapes=SHAPES):
    """the unconstrained session against ls_sweep: prints the table of profiles/nonneg_bars.md and the
    BARS entries (10 x the largest over the well-posed shapes, schedules and lambdas, per storage type)"""
    print(f"back end {backend(pp)}: measured deviation of the unconstrained session, {SWEEPS} sweeps")
    print("| lens | R | storage | schedule | lambda | factors | grad | gradnorm | residual |")
    print("|---|---|---|---|---|---|---|---|---|")
    out = {}
    for k, (lens, R) in enumerate(shapes):
        V, W0 = problem(lens, R, 100 + k)
        for dtype in (pp.F32, pp.F64):
            worst = out.setdefault(int(dtype), {})
            for lam in LAMBDAS:
                for sched in SCHEDULES:
                    t, s = session(pp, ctx, lens, R, dtype, V, W0, sched, False)
                    Vh = t.download()
                    W_ref, G_ref, scales, _, _ = numpy_run(Vh, W0, lam, ls_sweep)
                    s.sweeps_dt(SWEEPS, lam)
                    d = deviation(s, Vh, W_ref, G_ref, scales)
                    print(f"| {lens} | {R} | {'F32' if dtype == pp.F32 else 'F64'} | {sched} | {lam:g} | "
                          + " | ".join(f"{d[q]:.3g}" for q in ("factors", "grad", "gradnorm", "residual")) + " |")
                    if well_posed(lens, R, lam):
                        for q, v in d.items():
                            worst[q] = max(worst.get(q, 0.0), v)
                    s.close()
                    t.close()
    for key, val in out.items():
        print(f"        {key}: {({q: float(f'{10 * v:.3g}') for q, v in val.items()})},")
    return out


# ---------------------------------------------------------------------------- cases
def case_sweeps(pp, ctx, shapes=SHAPES):
    """1 + 2: three sweeps against numpy on F32 and F64 storage, both schedules, lambda 0 and 1e-3"""
    bars = BARS[backend(pp)]
    for k, (lens, R) in enumerate(shapes):
        V, W0 = problem(lens, R, 100 + k)
        for dtype in (pp.F32, pp.F64):
            bar = bars[int(dtype)]
            for lam in LAMBDAS:
                for sched in SCHEDULES:
                    t, s = session(pp, ctx, lens, R, dtype, V, W0, sched, True)
                    Vh = t.download()
                    W_ref, G_ref, scales, clamped, nfac = numpy_run(Vh, W0, lam, nn_sweep)
                    assert clamped >= 1, (lens, R, "the numpy run clamped nothing: change the seed")
                    s.sweeps_dt(SWEEPS, lam)
                    d = deviation(s, Vh, W_ref, G_ref, scales)
                    print(f"  {lens} R={R} dtype={int(dtype)} {sched} lambda={lam:g} clamped={clamped}: "
                          + " ".join(f"{q} {d[q]:.3g} (bar {bar[q]:.3g})" for q in d), flush=True)
                    assert above_floor(W_ref, nfac) and above_floor(s.get_factors(), nfac)
                    for q in d:
                        assert d[q] <= bar[q], (lens, R, int(dtype), sched, lam, q, d[q], bar[q])
                    s.close()
                    t.close()


def case_properties(pp, ctx):
    """3: entries >= the floor (times the sweep's Normalize factor, NORM_SLACK) after every sweep; on F64
    storage the residual never rises by more than 1e-9 relative over 20 sweeps (HALS is exact
    block-coordinate descent) — the numpy restatement first"""
    for k, (lens, R) in enumerate(SHAPES[:3]):
        V, W0 = problem(lens, R, 100 + k)
        W, G = [w.copy() for w in W0], [np.zeros_like(w) for w in W0]
        prev = NR._residual(V, W)
        nfacs = []
        for _ in range(20):
            W, _, _, nfac = nn_sweep(V, W, G, 0.0)
            cur = NR._residual(V, W)
            assert cur <= prev * (1 + 1e-9), ("numpy", lens, prev, cur)
            assert above_floor(W, nfac)
            nfacs.append(nfac)
            prev = cur
        for sched in SCHEDULES:
            t, s = session(pp, ctx, lens, R, pp.F64, V, W0, sched, True)
            prev = s.residual()
            for it in range(20):
                s.sweeps_dt(1)
                cur = s.residual()
                assert above_floor(s.get_factors(), nfacs[it]), (lens, sched, it)
                assert cur <= prev * (1 + 1e-9), (lens, sched, it, prev, cur)
                prev = cur
            print(f"  {lens} R={R} {sched}: residual after 20 sweeps {cur:.6g}", flush=True)
            s.close()
            t.close()


def case_schedules(pp, ctx):
    """4: dt and msdt give the same iterates (the margin tests/test_gpu_cp.py holds both to)"""
    for k, (lens, R) in enumerate(SHAPES[:3]):
        V, W0 = problem(lens, R, 100 + k)
        for dtype in (pp.F32, pp.F64):
            got = []
            for sched in SCHEDULES:
                t, s = session(pp, ctx, lens, R, dtype, V, W0, sched, True)
                s.sweeps_dt(SWEEPS)
                got.append(s.get_factors())
                s.close()
                t.close()
            worst = max(relerr(a, b) for a, b in zip(*got))
            print(f"  {lens} R={R} dtype={int(dtype)}: msdt vs dt {worst:.3g}", flush=True)
            assert worst < FTOL[int(dtype)], (lens, R, int(dtype), worst)


def case_repeatable(pp, ctx):
    """5: two runs from the same factors: identical factors, gradients and Grams (read through the
    Hadamard products of ppals_cp_gram_system, every mode), bit for bit"""
    for k, (lens, R) in enumerate(SHAPES):
        V, W0 = problem(lens, R, 100 + k)
        for sched in SCHEDULES:
            runs = []
            for _ in range(2):
                t, s = session(pp, ctx, lens, R, pp.F32, V, W0, sched, True)
                s.sweeps_dt(SWEEPS, 1e-3)
                W, G = s.get_factors(with_grad=True)
                runs.append(W + G + [s.gram_system(i)[0] for i in range(len(lens))] + [np.array(s.gradnorm())])
                s.close()
                t.close()
            for a, b in zip(*runs):
                assert np.array_equal(a, b), (lens, R, sched)


def case_em(pp, ctx):
    """6: EM with a 30 % random mask on a non-negative rank-3 tensor: the factors stay non-negative and the
    observed residual ends below where it started"""
    import torch
    lens, R = (12, 10, 8), 3
    rng = np.random.default_rng(7)
    A = [rng.random((s, R)) for s in lens]
    V = np.asfortranarray(np.einsum("az,bz,cz->abc", *A))
    g = torch.Generator(device="cpu").manual_seed(3)
    mask = (torch.rand(lens, generator=g) >= 0.3).to(f"cuda:{ctx.device}")
    W0 = [np.abs(rng.standard_normal((s, R))) for s in lens]
    for dtype in (pp.F32, pp.F64):
        t = pp.Tensor(ctx, list(lens), dtype).upload(V)
        s = pp.CP(ctx, t, R)
        s.set_nonneg(True)
        s.set_factors(W0)
        start = s.impute_torch(mask, want_residual=True)
        t.upload(V)
        rc, iters, end = s.run_em(mask, inner_sweeps=2, maxiter=15, resprint=5)
        print(f"  dtype={int(dtype)}: observed residual {start:.6g} -> {end:.6g} in {iters} iterations", flush=True)
        assert iters == 15 and end < start, (start, end, iters)
        assert min(w.min() for w in s.get_factors()) > 0   # (sweeps that end in Normalize: see NORM_SLACK)
        s.close()
        t.close()


def case_drivers(pp, ctx):
    """7: cpd_als(0) and run_dt drive a non-negative session and stop as they do an unconstrained one"""
    lens, R = SHAPES[1]
    V, W0 = problem(lens, R, 101)
    for kw in (dict(maxiter=4, tol=0.0, resprint=2), dict(maxiter=4, tol=1e30, resprint=1)):
        out = []
        for nonneg in (False, True):
            t, s = session(pp, ctx, lens, R, pp.F64, V, W0, "msdt", nonneg)
            before = s.residual()
            a = s.cpd_als(0, **kw)
            lo_a = min(w.min() for w in s.get_factors())
            mid = s.residual()
            s.set_factors(W0)
            b = s.run_dt(**kw)
            out.append((a, b))
            if nonneg:
                assert lo_a >= (FLOOR if a[1] > 0 else 0.0)
                assert mid <= before and s.residual() <= before
                if b[1] > 0:   # run_dt's sweeps end in Normalize: positive (see NORM_SLACK)
                    assert min(w.min() for w in s.get_factors()) > 0
            s.close()
            t.close()
        print(f"  {kw}: cpd_als (rc, sweeps, iters) / run_dt (rc, iters) off {out[0]} on {out[1]}", flush=True)
        assert out[0] == out[1], (kw, out)
    # the class API runs without Normalize: three sweeps against the numpy restatement without it
    t, s = session(pp, ctx, lens, R, pp.F64, V, W0, "msdt", True)
    s.cpd_als(0, maxiter=2, tol=0.0, resprint=100)   # maxsweep + 1 = 3 sweeps
    W, G = [w.copy() for w in W0], [np.zeros_like(w) for w in W0]
    for _ in range(3):
        W, _, _, _ = nn_sweep(V, W, G, 0.0, normalize=False)
    bar = BARS[backend(pp)][int(pp.F64)]["factors"]
    worst = max(relerr(a, b) for a, b in zip(s.get_factors(), W))
    print(f"  cpd_als(0), 3 sweeps, against numpy: {worst:.3g} (bar {bar:.3g})", flush=True)
    assert worst <= bar
    s.close()
    t.close()


def _refused(pp, code, fn, *a, **kw):
    try:
        fn(*a, **kw)
    except pp.PpalsError as e:
        assert f"ppals error {code}:" in str(e), (code, str(e))
        return
    raise AssertionError(f"not refused: {fn}")


def case_refusals(pp, ctx):
    """8: each refusal returns its error, and the session sweeps on afterwards"""
    lens, R = SHAPES[0]
    V, W0 = problem(lens, R, 100)
    t, s = session(pp, ctx, lens, R, pp.F64, V, W0, "msdt", True)
    t2, ref = session(pp, ctx, lens, R, pp.F64, V, W0, "msdt", True)
    bad = [w.copy() for w in W0]
    bad[1][2, 1] = -1e-300
    _refused(pp, -3, s.set_factors, bad)
    bad[1][2, 1] = np.nan
    _refused(pp, -3, s.set_factors, bad)
    bad[1][2, 1] = np.inf
    _refused(pp, -3, s.set_factors, bad)
    _refused(pp, -5, s.run_pp, maxiter=3)
    _refused(pp, -5, s.run_pp_partupdate, maxiter=3)
    _refused(pp, -5, s.cpd_als_lr, 3, 1, maxiter=2)
    _refused(pp, -5, s.cpd_als_lr, 4, 1, maxiter=2)
    m = pp.CPMulti(ctx, t, R, 2)
    m.set_factors(-1, [W0, W0])
    m.sweeps(1)
    _refused(pp, -5, m.take, 0, s)
    m.close()
    assert pp.lib().ppals_cp_set_nonneg(None, 1) == -3 and pp.lib().ppals_cp_get_nonneg(None) == -3
    # nothing of the above touched the session: it sweeps exactly as one that never saw the calls
    s.sweeps_dt(2)
    ref.sweeps_dt(2)
    for a, b in zip(s.get_factors(), ref.get_factors()):
        assert np.array_equal(a, b)
    assert s.nonneg
    # turning the flag on over negative factors: refused, the flag stays off, ordinary sweeps go on
    neg = [-w for w in W0]
    s.set_nonneg(False)
    s.set_factors(neg)
    _refused(pp, -3, s.set_nonneg, True)
    assert not s.nonneg
    s.sweeps_dt(1)
    assert np.isfinite(s.residual())
    for x in (s, ref, t2):
        x.close()
    # R = 65
    lens65 = (70, 6, 5)
    V65, W65 = problem(lens65, 65, 5)
    t65, s65 = session(pp, ctx, lens65, 65, pp.F64, V65, W65, "msdt", False)
    _refused(pp, -5, s65.set_nonneg, True)
    assert not s65.nonneg
    s65.sweeps_dt(1, 1e-3)
    assert np.isfinite(s65.residual())
    for x in (s65, t65, t):
        x.close()


def case_flag_off(pp, ctx):
    """9: a session that turned the flag on and off again, and one that never touched it, sweep bit for bit alike"""
    for k, (lens, R) in enumerate(SHAPES[:2]):
        V, W0 = problem(lens, R, 100 + k)
        for dtype in (pp.F32, pp.F64):
            got = []
            for touch in (False, True):
                t, s = session(pp, ctx, lens, R, dtype, V, W0, "msdt", False)
                if touch:
                    s.set_nonneg(True)
                    s.set_nonneg(False)
                assert not s.nonneg
                s.sweeps_dt(SWEEPS)
                W, G = s.get_factors(with_grad=True)
                got.append(W + G)
                s.close()
                t.close()
            for a, b in zip(*got):
                assert np.array_equal(a, b), (lens, R, int(dtype))
            assert min(w.min() for w in got[0]) < 0   # the unconstrained fit does go negative here


CASES = {"sweeps": case_sweeps, "properties": case_properties, "schedules": case_schedules,
         "repeatable": case_repeatable, "em": case_em, "drivers": case_drivers, "refusals": case_refusals,
         "flag_off": case_flag_off, "measure_bars": measure_bars}


if __name__ == "__main__":
    import torch  # noqa: F401  (before the binding loads libppals: one HIP runtime for both)
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "pairwise-perturbation_amd"))
    if os.environ.get("PPALS_NONNEG_BACKEND") == "hostsim":   # measure_bars for the stand-in's table
        import hostsim_util
        pp_ = hostsim_util.load()
    else:
        import ppals as pp_
    ctx_ = pp_.Context(0)
    CASES[sys.argv[1]](pp_, ctx_)
    ctx_.close()
    print(f"nonneg case {sys.argv[1]}: ok")
