"""Non-negative multi-start sessions (ppals_cp_multi_set_nonneg, include/ppals.h): the cases of
tests/test_gpu_multistart_nonneg.py (the batched HIP launch of kernels_nn.hip.h) and of
tests/test_multistart_nonneg_hostsim.py (the same functions with the host stand-in's binding: the ops.h
default, a loop of the one-start update). `python multistart_nonneg_cases.py measure_bars` prints the
tables of profiles/multistart_nonneg_bars.md (PPALS_NONNEG_BACKEND=hostsim: the stand-in's).

Inputs: V, W0 = nonneg_cases.problem(lens, R, 100 + k) for row k of ROWS; start b begins from
W0 * (1 + p u_b), u_b uniform from default_rng(9000 + 31 b + k), p = 0.1, or 0.01 where R exceeds the
shortest extent (an over-parameterised model empties its redundant columns from further off).

The reference of every start is the numpy restatement of tests/nonneg_cases.py without Normalize
(a multi-start session has none), computed once per (row, storage type, lambda) and shared by both
schedules and by the cases that need it.

The bars are NOT taken from the code under test. BARS: 10 x what the UNCONSTRAINED multi-start session
deviates from the unconstrained numpy sweep without Normalize on the same inputs — the largest over
rows, schedules, lambdas and starts per storage type and back end, the singular combination
(nonneg_cases.well_posed) left out, exactly as nonneg_cases.measure_bars does. PAIR_BARS: 10 x what the
unconstrained pairing (CPMulti against cpd_als(0) sessions from the same factors) deviates, figures of
pair_deviation below. max is 1-Lipschitz, so the clamp amplifies nothing; the 10 is for the R sequential
dependent steps that replace one solve."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import numpy_ref as NR  # noqa: E402
import nonneg_cases as NC  # noqa: E402

FLOOR = NC.FLOOR
SWEEPS = NC.SWEEPS
LAMBDAS = NC.LAMBDAS
SCHEDULES = NC.SCHEDULES
BF16 = 3
# (lens, R, K): one ragged tile; order 4 and the scan route above 64 columns; three tiles with a ragged
# last one (130 = 2 * 64 + 2); the LDS bound, two tiles, the column limit; the most starts
ROWS = [((9, 8, 7), 3, 2), ((33, 12, 10, 9), 10, 7), ((130, 9, 8), 17, 4), ((70, 6, 5), 64, 2),
        ((20, 9, 8), 3, 32)]
FIGURES = ("factors", "grad", "gradnorm", "residual")

# 10 x the measured deviation of the unconstrained multi-start session (profiles/multistart_nonneg_bars.md
# holds the measured tables): [back end][storage type] = the four figures
BARS = {
    "hip": {
        0: {'factors': 0.0103, 'grad': 5.21e-06, 'gradnorm': 2.63e-07, 'residual': 6.33e-07},
        1: {'factors': 6.97e-10, 'grad': 2.17e-11, 'gradnorm': 4.79e-12, 'residual': 4.68e-13},
    },
    "hostsim": {
        0: {'factors': 0.00524, 'grad': 2.25e-06, 'gradnorm': 7.26e-08, 'residual': 3.71e-07},
        1: {'factors': 7.41e-10, 'grad': 3.62e-11, 'gradnorm': 8.89e-12, 'residual': 4.04e-13},
    },
}
# the same for the pairing with ordinary sessions (pair_deviation), BF16 storage included; case 2 runs on
# the GPU (on the stand-in a multi-start session IS a loop over the one-start update)
PAIR_BARS = {
    "hip": {
        0: {'factors': 0.0131, 'grad': 0.00987, 'gradnorm': 0.000644, 'residual': 7.69e-07},
        1: {'factors': 4.54e-10, 'grad': 9.56e-08, 'gradnorm': 8.78e-09, 'residual': 1.67e-13},
        3: {'factors': 2.3e-06, 'grad': 0.000565, 'gradnorm': 9.34e-05, 'residual': 1.9e-08},
    },
    "hostsim": {
        0: {'factors': 1.62e-06, 'grad': 0.000377, 'gradnorm': 2.79e-05, 'residual': 1.01e-08},
        1: {'factors': 7.02e-14, 'grad': 1.75e-11, 'gradnorm': 2.71e-12, 'residual': 8.08e-16},
    },
}


def dname(dtype):
    return {0: "F32", 1: "F64", 3: "BF16"}[int(dtype)]


# ---------------------------------------------------------------------------- inputs and references
def inputs(k):
    """(lens, R, K, V, [the K starting factor lists]) of row k"""
    lens, R, K = ROWS[k]
    V, W0 = NC.problem(lens, R, 100 + k)
    p = 0.1 if R <= min(lens) else 0.01
    starts = []
    for b in range(K):
        rng = np.random.default_rng(9000 + 31 * b + k)
        starts.append([w * (1 + p * rng.random(w.shape)) for w in W0])
    return lens, R, K, V, starts


def nn_sweep(V, W, G, lam):
    return NC.nn_sweep(V, W, G, lam, normalize=False)


def ls_sweep(V, W, G, lam):
    """the unconstrained sweep without Normalize: what an unconstrained multi-start session runs"""
    return NC._sweep(V, W, G, lam, lambda M, Wi, S: (M @ NR._svd_inverse(S), 0), normalize=False)


_REF = {}


def reference(k, Vh, starts, lam, sweep, key):
    """per start (W, G, scales, clamped) after SWEEPS sweeps, computed once per key"""
    key = (k, key, lam, sweep.__name__)
    if key not in _REF:
        _REF[key] = [NC.numpy_run(Vh, W0, lam, sweep)[:4] for W0 in starts]
    return _REF[key]


def multi(pp, ctx, t, R, K, starts, sched, nonneg):
    m = pp.CPMulti(ctx, t, R, K)
    m.set_schedule(sched)
    if nonneg:
        m.set_nonneg(True)
        assert m.nonneg
    m.set_factors(-1, starts)
    return m


class _Start:
    """start b of a multi-start session with the read-outs nonneg_cases.deviation asks of a session"""

    def __init__(self, m, b, res, gn):
        self.m, self.b, self.res, self.gn = m, b, res, gn

    def get_factors(self, with_grad=False):
        return self.m.get_factors(self.b, with_grad=with_grad)

    def gradnorm(self):
        return self.gn[self.b]

    def residual(self):
        return self.res[self.b]


def deviations(m, K, Vh, ref):
    """the four figures of nonneg_cases.deviation, the worst over the starts"""
    res, gn = m.residuals(), m.gradnorms()
    worst = dict.fromkeys(FIGURES, 0.0)
    for b in range(K):
        W_ref, G_ref, scales, _ = ref[b]
        d = NC.deviation(_Start(m, b, res, gn), Vh, W_ref, G_ref, scales)
        for q in FIGURES:
            worst[q] = max(worst[q], d[q]) if np.isfinite(d[q]) else np.inf
    return worst


def solo(pp, ctx, t, R, W0, sched, lam, nonneg):
    """an ordinary session advanced by SWEEPS sweeps of the class API's Simple optimizer (no Normalize)"""
    s = pp.CP(ctx, t, R)
    s.set_schedule(sched)
    if nonneg:
        s.set_nonneg(True)
    s.set_factors(W0)
    s.cpd_als(0, tol=0.0, maxiter=SWEEPS - 1, lam=lam, resprint=10 ** 9)   # maxsweep + 1 sweeps
    return s


def pair_deviation(m, K, t, Vnorm, pp, ctx, R, starts, sched, lam, nonneg):
    """start by start against ordinary sessions from the same factors, the worst over the starts: factors
    (worst relative Frobenius), grad_W (worst mode, against 1 + its norm, the scale of
    tests/test_gpu_multistart.py), gradnorm (against 1 + it), residual (against ||V||)"""
    res, gn = m.residuals(), m.gradnorms()
    worst = dict.fromkeys(FIGURES, 0.0)
    for b in range(K):
        s = solo(pp, ctx, t, R, starts[b], sched, lam, nonneg)
        W_ref, G_ref = s.get_factors(with_grad=True)
        W, G = m.get_factors(b, with_grad=True)
        d = {"factors": max(NC.relerr(a, r) for a, r in zip(W, W_ref)),
             "grad": max(np.linalg.norm(a - r) / (1 + np.linalg.norm(r)) for a, r in zip(G, G_ref)),
             "gradnorm": abs(gn[b] - s.gradnorm()) / (1 + s.gradnorm()),
             "residual": abs(res[b] - s.residual()) / Vnorm}
        s.close()
        for q in FIGURES:
            worst[q] = max(worst[q], d[q]) if np.isfinite(d[q]) else np.inf
    return worst


def _fmt(d, bar=None):
    if bar is None:
        return " | ".join(f"{d[q]:.3g}" for q in FIGURES)
    return " ".join(f"{q} {d[q]:.3g} (bar {bar[q]:.3g})" for q in FIGURES)


def _constants(out):
    for key, val in out.items():
        print(f"        {key}: {({q: float(f'{10 * v:.3g}') for q, v in val.items()})},")


def measure_bars(pp, ctx, rows=None):
    """the unconstrained multi-start session against ls_sweep, and against unconstrained cpd_als(0)
    sessions: prints the tables of profiles/multistart_nonneg_bars.md and the BARS / PAIR_BARS entries"""
    rows = range(len(ROWS)) if rows is None else rows
    be = NC.backend(pp)
    print(f"back end {be}: measured deviation of the unconstrained multi-start session from numpy, "
          f"{SWEEPS} sweeps, the worst start")
    print("| lens | R | K | storage | schedule | lambda | factors | grad | gradnorm | residual |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    out, pair, pair_rows = {}, {}, []
    for k in rows:
        lens, R, K, V, starts = inputs(k)
        for dtype in (pp.F32, pp.F64, BF16):
            try:
                t = pp.Tensor(ctx, list(lens), dtype).upload(V)
            except pp.PpalsError:
                if dtype != BF16:
                    raise
                continue   # (a back end without bf16 storage)
            Vh = t.download()
            for lam in LAMBDAS:
                ok = NC.well_posed(lens, R, lam)
                for sched in SCHEDULES:
                    m = multi(pp, ctx, t, R, K, starts, sched, False)
                    m.sweeps(SWEEPS, lam)
                    if dtype != BF16:   # (no bf16 case against numpy)
                        ref = reference(k, Vh, starts, lam, ls_sweep, int(dtype))
                        d = deviations(m, K, Vh, ref)
                        print(f"| {lens} | {R} | {K} | {dname(dtype)} | {sched} | {lam:g} | {_fmt(d)} |"
                              + ("" if ok else " (singular: left out)"), flush=True)
                        if ok:
                            w = out.setdefault(int(dtype), {})
                            for q in FIGURES:
                                w[q] = max(w.get(q, 0.0), d[q])
                    d = pair_deviation(m, K, t, np.linalg.norm(Vh), pp, ctx, R, starts, sched, lam, False)
                    pair_rows.append(f"| {lens} | {R} | {K} | {dname(dtype)} | {sched} | {lam:g} | {_fmt(d)} |"
                                     + ("" if ok else " (singular: left out)"))
                    if ok:
                        w = pair.setdefault(int(dtype), {})
                        for q in FIGURES:
                            w[q] = max(w.get(q, 0.0), d[q])
                    m.close()
            t.close()
    print(f"BARS[{be!r}] (10 x the largest, per storage type):")
    _constants(out)
    print(f"\nback end {be}: measured deviation of the unconstrained multi-start session from unconstrained "
          f"cpd_als(0) sessions, {SWEEPS} sweeps, the worst start")
    print("| lens | R | K | storage | schedule | lambda | factors | grad | gradnorm | residual |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    print("\n".join(pair_rows))
    print(f"PAIR_BARS[{be!r}] (10 x the largest, per storage type):")
    _constants(pair)
    return out, pair


# ---------------------------------------------------------------------------- cases
def case_numpy(pp, ctx, rows=None):
    """1: three sweeps of every start against the numpy restatement"""
    bars = BARS[NC.backend(pp)]
    for k in (range(len(ROWS)) if rows is None else rows):
        lens, R, K, V, starts = inputs(k)
        for dtype in (pp.F32, pp.F64):
            bar = bars[int(dtype)]
            t = pp.Tensor(ctx, list(lens), dtype).upload(V)
            Vh = t.download()
            for lam in LAMBDAS:
                ref = reference(k, Vh, starts, lam, nn_sweep, int(dtype))
                for b in range(K):
                    assert ref[b][3] >= 1, (lens, R, b, "the numpy run clamped nothing: change the seed")
                    assert all(w.min() >= FLOOR for w in ref[b][0])
                for sched in SCHEDULES:
                    m = multi(pp, ctx, t, R, K, starts, sched, True)
                    m.sweeps(SWEEPS, lam)
                    d = deviations(m, K, Vh, ref)
                    print(f"  {lens} R={R} K={K} {dname(dtype)} {sched} lambda={lam:g} clamped "
                          f"{min(r[3] for r in ref)}..{max(r[3] for r in ref)}: {_fmt(d, bar)}", flush=True)
                    for b in range(K):
                        assert all(w.min() >= FLOOR for w in m.get_factors(b)), (lens, b)
                    for q in FIGURES:
                        assert d[q] <= bar[q], (lens, R, K, dname(dtype), sched, lam, q, d[q], bar[q])
                    m.close()
            t.close()


def case_pairs(pp, ctx, rows=None):
    """2: every start against an ordinary non-negative session run by cpd_als(0) from the same factors,
    F32, F64 and BF16 storage"""
    bars = PAIR_BARS[NC.backend(pp)]
    for k in (range(len(ROWS)) if rows is None else rows):
        lens, R, K, V, starts = inputs(k)
        for dtype in (pp.F32, pp.F64, BF16):
            bar = bars[int(dtype)]
            t = pp.Tensor(ctx, list(lens), dtype).upload(V)
            Vnorm = np.linalg.norm(t.download())
            for lam in LAMBDAS:
                for sched in SCHEDULES:
                    m = multi(pp, ctx, t, R, K, starts, sched, True)
                    m.sweeps(SWEEPS, lam)
                    d = pair_deviation(m, K, t, Vnorm, pp, ctx, R, starts, sched, lam, True)
                    print(f"  {lens} R={R} K={K} {dname(dtype)} {sched} lambda={lam:g}: {_fmt(d, bar)}",
                          flush=True)
                    for q in FIGURES:
                        assert d[q] <= bar[q], (lens, R, K, dname(dtype), sched, lam, q, d[q], bar[q])
                    m.close()
            t.close()


def _state(m, K):
    """everything a run leaves behind, start by start: factors, gradients, the gradient sum (read through
    gradnorms), the residual"""
    res, gn = m.residuals(), m.gradnorms()
    out = []
    for b in range(K):
        W, G = m.get_factors(b, with_grad=True)
        out.append(W + G + [np.array(gn[b]), np.array(res[b])])
    return out


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def case_uncoupled(pp, ctx):
    """3: two runs that differ in start 1's initial factors only: every other start identical bit for bit
    (a wrong partial-sum or Gram offset would leak one start into another)"""
    for k in (2, 4):
        lens, R, K, V, starts = inputs(k)
        other = [w * (1 + 0.05 * np.random.default_rng(77).random(w.shape)) for w in starts[1]]
        for dtype in (pp.F32, pp.F64):
            t = pp.Tensor(ctx, list(lens), dtype).upload(V)
            for lam in LAMBDAS:
                for sched in SCHEDULES:
                    runs = []
                    for s1 in (starts[1], other):
                        m = multi(pp, ctx, t, R, K, [starts[0], s1] + starts[2:], sched, True)
                        m.sweeps(SWEEPS, lam)
                        runs.append(_state(m, K))
                        m.close()
                    for b in range(K):
                        if b != 1:
                            assert _same(runs[0][b], runs[1][b]), (lens, dname(dtype), lam, sched, b)
                    assert not _same(runs[0][1], runs[1][1])
            t.close()


def case_repeatable(pp, ctx, rows=None):
    """4: two runs from the same state: identical bits"""
    for k in (range(len(ROWS)) if rows is None else rows):
        lens, R, K, V, starts = inputs(k)
        for dtype in (pp.F32, pp.F64):
            t = pp.Tensor(ctx, list(lens), dtype).upload(V)
            for lam in LAMBDAS:
                for sched in SCHEDULES:
                    runs = []
                    for _ in range(2):
                        m = multi(pp, ctx, t, R, K, starts, sched, True)
                        m.sweeps(SWEEPS, lam)
                        runs.append(_state(m, K))
                        m.close()
                    for b in range(K):
                        assert _same(runs[0][b], runs[1][b]), (lens, dname(dtype), lam, sched, b)
            t.close()


PROPERTY_SWEEPS = 20


def case_properties(pp, ctx, rows=None):
    """5: F64 storage, lambda = 0 (the residual is the objective HALS descends exactly), 20 single sweeps:
    every entry of every start >= the floor after each, no start's residual rises by more than 1e-9
    relative — the numpy restatement first"""
    for k in (range(len(ROWS)) if rows is None else rows):
        lens, R, K, V, starts = inputs(k)
        for b in range(K):
            W, G = [w.copy() for w in starts[b]], [np.zeros_like(w) for w in starts[b]]
            prev = NR._residual(V, W)
            for it in range(PROPERTY_SWEEPS):
                W, _, _, _ = nn_sweep(V, W, G, 0.0)
                cur = NR._residual(V, W)
                assert cur <= prev * (1 + 1e-9), ("numpy", lens, b, it, prev, cur)
                assert all(w.min() >= FLOOR for w in W)
                prev = cur
        t = pp.Tensor(ctx, list(lens), pp.F64).upload(V)
        for sched in SCHEDULES:
            m = multi(pp, ctx, t, R, K, starts, sched, True)
            prev = m.residuals()
            for it in range(PROPERTY_SWEEPS):
                m.sweeps(1)
                cur = m.residuals()
                lo = min(w.min() for W in m.get_factors(-1) for w in W)
                assert lo >= FLOOR, (lens, sched, it, lo)
                assert np.all(cur <= prev * (1 + 1e-9)), (lens, sched, it, prev, cur)
                prev = cur
            print(f"  {lens} R={R} K={K} {sched}: residuals after {PROPERTY_SWEEPS} sweeps "
                  f"{cur.min():.6g}..{cur.max():.6g}", flush=True)
            m.close()
        t.close()


def case_launches(pp, ctx):
    """6: the bracketed non-scan launches of three sweeps do not grow with the number of starts and are at
    least the mode updates; the scans are those of the unconstrained multi-start session of the same K"""
    lens, R, n = [20, 12, 16, 10], 10, 3
    t = pp.Tensor(ctx, lens, pp.F32).fill_uniform(6)
    counts = {}
    for K in (2, 7):
        starts = [pp.init_factors(lens, R, 2000 + 31 * b) for b in range(K)]   # uniform in [0, 1)
        scans = {}
        for nonneg in (True, False):
            m = multi(pp, ctx, t, R, K, starts, "msdt", nonneg)
            ctx.sync()
            ctx.profile_enable(2)
            ctx.profile_reset()
            m.sweeps(n)
            ctx.sync()
            nscan, _, nbytes = ctx.profile_read(0)
            if nonneg:
                counts[K] = ctx.profile_read(1)[0]
            scans[nonneg] = (nscan, nbytes)
            ctx.profile_enable(0)
            m.close()
        print(f"  K={K}: other bracketed launches in {n} non-negative sweeps {counts[K]}, scan launches / "
              f"bytes non-negative {scans[True]} unconstrained {scans[False]}", flush=True)
        assert scans[True][0] > 0 and scans[True] == scans[False]
    assert counts[2] >= n * len(lens)
    assert counts[7] <= counts[2]
    t.close()


def _refused(pp, code, fn, *a, **kw):
    try:
        fn(*a, **kw)
    except pp.PpalsError as e:
        assert f"ppals error {code}:" in str(e), (code, str(e))
        return
    raise AssertionError(f"not refused: {fn}")


def case_take(pp, ctx):
    """7: a start of a non-negative multi-start session goes into a non-negative session (which sweeps on
    bit for bit as one given the same factors by set_factors) and into an ordinary one; a start of an
    unconstrained multi-start session is still refused by a non-negative destination"""
    lens, R, K, V, starts = inputs(1)
    for dtype in (pp.F32, pp.F64):
        t = pp.Tensor(ctx, list(lens), dtype).upload(V)
        m = multi(pp, ctx, t, R, K, starts, "msdt", True)
        m.sweeps(2)
        b = int(np.argmin(m.residuals()))
        W, G = m.get_factors(b, with_grad=True)
        d = pp.CP(ctx, t, R)       # (the destination is a session of the same tensor)
        d.set_nonneg(True)
        d.set_factors(starts[0])
        d.sweeps_dt(1)             # caches alive in the destination
        m.take(b, d)
        assert d.nonneg
        r = pp.CP(ctx, t, R)
        r.set_nonneg(True)
        r.set_factors(W, G)
        Wd, Gd = d.get_factors(with_grad=True)
        assert _same(Wd + Gd, W + G)
        d.sweeps_dt(2)
        r.sweeps_dt(2)
        assert _same(sum(d.get_factors(with_grad=True), []), sum(r.get_factors(with_grad=True), []))
        o = pp.CP(ctx, t, R)       # an ordinary destination
        m.take(b, o)
        assert not o.nonneg and _same(o.get_factors(), W)
        u = multi(pp, ctx, t, R, K, starts, "msdt", False)
        u.sweeps(1)
        _refused(pp, -5, u.take, 0, d)
        assert _same(d.get_factors(), r.get_factors())   # the refusal left the destination alone
        for h in (u, o, m, d, r, t):
            h.close()


def case_refusals(pp, ctx):
    """8: each refusal returns its error and leaves the session sweeping exactly as an untouched twin"""
    lens, R, K, V, starts = inputs(0)
    t = pp.Tensor(ctx, list(lens), pp.F64).upload(V)
    m = multi(pp, ctx, t, R, K, starts, "msdt", True)
    twin = multi(pp, ctx, t, R, K, starts, "msdt", True)
    for v in (-1e-300, np.nan, np.inf):
        bad = [w.copy() for w in starts[1]]
        bad[1][2, 1] = v
        _refused(pp, -3, m.set_factors, 1, bad)
        _refused(pp, -3, m.set_factors, -1, [starts[0], bad])
    L = pp.lib()
    assert L.ppals_cp_multi_set_nonneg(None, 1) == -3 and L.ppals_cp_multi_get_nonneg(None) == -3
    m.sweeps(2)
    twin.sweeps(2)
    assert m.nonneg and all(_same(a, b) for a, b in zip(_state(m, K), _state(twin, K)))
    # turning the flag on over a negative start: refused, the flag stays off, unconstrained sweeps go on
    neg = [starts[0], [-w for w in starts[1]]]
    for h in (m, twin):
        h.set_nonneg(False)
        h.set_factors(-1, neg)
    _refused(pp, -3, m.set_nonneg, True)
    assert not m.nonneg
    m.sweeps(1)
    twin.sweeps(1)
    assert all(_same(a, b) for a, b in zip(_state(m, K), _state(twin, K)))
    m.close()
    twin.close()
    # R > 64 is possible at one start only
    one = pp.CPMulti(ctx, t, 65, 1)
    _refused(pp, -5, one.set_nonneg, True)
    assert not one.nonneg
    one.close()
    t.close()


def case_blocked_hook(pp, ctx):
    """8: PPALS_TEST_BLOCKED_UPDATE (read when a session is created) is refused as for ordinary sessions"""
    lens, R, K, V, starts = inputs(0)
    t = pp.Tensor(ctx, list(lens), pp.F64).upload(V)
    twin = multi(pp, ctx, t, R, K, starts, "msdt", False)
    old = os.environ.get("PPALS_TEST_BLOCKED_UPDATE")
    os.environ["PPALS_TEST_BLOCKED_UPDATE"] = "2"
    try:
        m = multi(pp, ctx, t, R, K, starts, "msdt", False)
    finally:
        if old is None:
            del os.environ["PPALS_TEST_BLOCKED_UPDATE"]
        else:
            os.environ["PPALS_TEST_BLOCKED_UPDATE"] = old
    try:
        m.set_nonneg(True)
    except pp.PpalsError as e:
        assert "ppals error -5:" in str(e) and "PPALS_TEST_BLOCKED_UPDATE" in str(e), str(e)
    else:
        raise AssertionError("not refused")
    assert not m.nonneg
    m.sweeps(2)
    twin.sweeps(2)
    assert all(_same(a, b) for a, b in zip(_state(m, K), _state(twin, K)))
    for h in (m, twin, t):
        h.close()


def case_two_ranks(pp):
    """8: a context of two ranks cannot create a multi-start session at all (nothing is launched before the
    refusal: the communicator's callbacks are never reached)"""
    import ctypes as C
    AR = C.CFUNCTYPE(None, C.POINTER(C.c_double), C.c_int64)
    RS = C.CFUNCTYPE(None, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int64)
    calls = []
    cbs = (AR(lambda b, n: calls.append("ar")), RS(lambda a, b, n: calls.append("rs")),
           RS(lambda a, b, n: calls.append("ag")))
    uid = C.create_string_buffer(128)
    for i, cb in enumerate(cbs):
        C.memmove(C.byref(uid, 8 * i), C.byref(C.cast(cb, C.c_void_p)), 8)
    c = pp.Context(0)
    c.init_comm(0, 2, uid)
    assert c.nranks == 2
    t = pp.Tensor(c, [6, 5, 4], pp.F64)
    try:
        pp.CPMulti(c, t, 2, 2)
    except pp.PpalsError as e:
        assert "ppals error -5:" in str(e) and "one rank" in str(e), str(e)
    else:
        raise AssertionError("a two-rank context created a multi-start session")
    assert not calls
    t.close()
    c.close()


def case_flag_off(pp, ctx):
    """9: a session that turned the flag on and off again sweeps bit for bit as one that never touched it"""
    for k in (0, 1):
        lens, R, K, V, starts = inputs(k)
        for dtype in (pp.F32, pp.F64):
            t = pp.Tensor(ctx, list(lens), dtype).upload(V)
            for lam in LAMBDAS:
                got = []
                for touch in (False, True):
                    m = multi(pp, ctx, t, R, K, starts, "msdt", False)
                    if touch:
                        m.set_nonneg(True)
                        m.set_nonneg(False)
                    assert not m.nonneg
                    m.sweeps(SWEEPS, lam)
                    got.append(_state(m, K))
                    m.close()
                assert all(_same(a, b) for a, b in zip(*got)), (lens, dname(dtype), lam)
                # the unconstrained fit does go negative here: the flag is what keeps the sign
                assert min(x.min() for st in got[0] for x in st[:len(lens)]) < 0
            t.close()


def case_run(pp, ctx):
    """10: run() drives a non-negative session as it drives an unconstrained one and names the start with
    the smallest residual"""
    lens, R, K, V, starts = inputs(1)
    t = pp.Tensor(ctx, list(lens), pp.F64).upload(V)
    for kw in (dict(maxiter=4, tol=0.0, resprint=2), dict(maxiter=4, tol=1e30, resprint=1)):
        out = []
        for nonneg in (False, True):
            m = multi(pp, ctx, t, R, K, starts, "msdt", nonneg)
            rc, sweeps, best = m.run(**kw)
            out.append((rc, sweeps))
            assert best == int(np.argmin(m.residuals())), (nonneg, best, m.residuals())
            if nonneg and sweeps:
                assert min(w.min() for W in m.get_factors(-1) for w in W) >= FLOOR
                ref = multi(pp, ctx, t, R, K, starts, "msdt", True)
                ref.sweeps(sweeps)
                assert all(_same(a, b) for a, b in zip(_state(m, K), _state(ref, K)))
                ref.close()
            m.close()
        print(f"  {kw}: (rc, sweeps) unconstrained {out[0]} non-negative {out[1]}", flush=True)
        assert out[0] == out[1], (kw, out)
    t.close()


CASES = {"numpy": case_numpy, "pairs": case_pairs, "uncoupled": case_uncoupled, "repeatable": case_repeatable,
         "properties": case_properties, "launches": case_launches, "take": case_take,
         "refusals": case_refusals, "blocked_hook": case_blocked_hook, "flag_off": case_flag_off,
         "run": case_run, "measure_bars": measure_bars}


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "pairwise-perturbation_amd"))
    if sys.argv[1] == "two_ranks":   # on the GPU: the product's engine over the callback communicator
        import hipsim_util
        case_two_ranks(hipsim_util.load(make=False))
    else:
        if os.environ.get("PPALS_NONNEG_BACKEND") == "hostsim":   # measure_bars for the stand-in's table
            import hostsim_util
            pp_ = hostsim_util.load()
        else:
            import ppals as pp_
        ctx_ = pp_.Context(0)
        CASES[sys.argv[1]](pp_, ctx_)
        ctx_.close()
    print(f"multistart nonneg case {sys.argv[1]}: ok")
