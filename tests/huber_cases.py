"""Cases of tests/test_gpu_huber.py, one per process: `python huber_cases.py <case>`.

ppals_cp_huber_device / ppals_cp_robust / ppals_cp_abs_residual_quantile (include/ppals.h) through the torch
helpers of the binding. torch is imported BEFORE the binding loads libppals (one HIP runtime for both). The
reference is tests/huber_ref.py on numpy's fp64 model built from the factors get_factors returns, and the
tensor downloaded before the call. Exit status 0: passed."""
import math
import os
import sys
import threading

import torch  # noqa: I001  (first: see above)
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "pairwise-perturbation_amd"))
import ppals as pp  # noqa: E402
import huber_ref  # noqa: E402
import wls_ref  # noqa: E402
from model_export_cases import DEV, check_values, cp_model, host  # noqa: E402
from wls_cases import PAIRS, SHAPES, layout, random_weights, session, view_pair  # noqa: E402

DATA_KINDS = ("c_contiguous", "first_index_fastest", "permuted", "box_at_lo")
PS = (0.0, 0.25, 0.5, 0.9, 1.0)
BAR = 1e-13       # check_values' fp64 bar: the model is within BAR x (the magnitude of its terms)


def box_slices(shape, lo, box):
    return tuple(slice(l, l + n) for l, n in zip(lo or [0] * len(shape), box))


def check_step(t, s, V0, M, absM, shape, dt, data, h, lo, c, what):
    """one step with the outputs from the contents V0: stored values, the unclipped h >= 1 elements, outside the
    box, the loss, the clipped count; then the same bits without the outputs"""
    t.upload(V0)
    loss, clipped = s.huber_torch(data, c, weights=h, lo=lo, want_loss=True)
    got = t.download()
    sl = box_slices(shape, lo, data.shape)
    xh = host(data)
    hh = host(h) if h is not None else np.ones(xh.shape)
    on = hh > 0
    xs = np.where(on, xh, 0.0)
    z, want_loss, want_clipped = huber_ref.step(xh, hh, M[sl], c)
    mag = absM[sl] + np.abs(xs)
    check_values(got[sl], z, mag, torch.float64 if dt == pp.F64 else torch.float32, what)
    bar = BAR * mag
    a_ref = np.where(on, np.abs(xs - M[sl]), 0.0)
    kept = (hh >= 1) & (a_ref < c - bar)        # certainly not clipped: the stored value is x rounded once
    stored = xh if dt == pp.F64 else xh.astype(np.float32).astype(np.float64)
    assert np.array_equal(got[sl][kept], stored[kept]), what
    outside = np.ones(shape, dtype=bool)
    outside[sl] = False
    assert np.array_equal(got[outside], V0[outside]), what
    scale = float(np.sum(np.where(on, np.minimum(hh, 1.0), 0.0) * xs ** 2))
    n_lo, n_hi = int(np.count_nonzero(on & (a_ref > c + bar))), int(np.count_nonzero(on & (a_ref > c - bar)))
    print(f"    {what}: loss {loss:.17g} numpy {want_loss:.17g} diff / sum h x^2 "
          f"{abs(loss - want_loss) / scale:.3g}; clipped {clipped} numpy {want_clipped} [{n_lo}, {n_hi}]", flush=True)
    assert np.isfinite(loss) and abs(loss - want_loss) <= 1e-10 * scale, (what, loss, want_loss, scale)
    assert n_lo <= clipped <= n_hi, (what, clipped, n_lo, n_hi)
    t.upload(V0)
    assert s.huber_torch(data, c, weights=h, lo=lo) is None      # without the outputs: the same bits
    assert np.array_equal(t.download(), got), what
    return clipped, int(np.count_nonzero(on))


def median_c(M, shape, data, lo):
    """numpy's median of |x - M| over the box: both branches of the rule are hit about equally"""
    return float(np.median(np.abs(host(data) - M[box_slices(shape, lo, data.shape)])))


def values(which):
    """one of: orders 3, 4, 5 and a box of several tiles per side (`which` indexes wls_cases.SHAPES); R in {1, 3, 10,
    33, 70, 128} cycled, across the four shapes, over F32 / F64 storage and f32 / f64 views; factors from two
    sweeps; every pair of view kinds with weights, every data kind without; c the median absolute residual"""
    ctx = pp.Context(0)
    shape = SHAPES[int(which)]
    k = 6 * int(which)
    for R in (1, 3, 10, 33, 70, 128):
        dt = (pp.F32, pp.F64)[k % 2]
        tdt = (torch.float32, torch.float64)[(k // 2) % 2]
        k += 1
        t = pp.Tensor(ctx, list(shape), dt).fill_uniform(100 + k, lo=0.5, hi=1.5)
        s = pp.CP(ctx, t, R)
        s.set_factors(pp.init_factors(shape, R, 10 * k), pp.init_factors(shape, R, 10 * k + 1))
        s.sweeps_dt(2)
        V0 = t.download()
        W = s.get_factors()
        M, absM = cp_model(W), cp_model(W, True)
        assert np.isfinite(M).all()
        for i, (dkind, wkind) in enumerate(PAIRS):
            data, h, lo, _ = view_pair(shape, dkind, wkind, tdt, 1000 * k + i)
            n, of = check_step(t, s, V0, M, absM, shape, dt, data, h, lo, median_c(M, shape, data, lo),
                               (shape, R, dt, str(tdt), dkind, wkind))
            assert 0.2 * of < n < 0.8 * of, (n, of)
        for i, dkind in enumerate(DATA_KINDS):
            data, _, lo, _ = view_pair(shape, dkind, dkind, tdt, 2000 * k + i)
            n, of = check_step(t, s, V0, M, absM, shape, dt, data, None, lo, median_c(M, shape, data, lo),
                               (shape, R, dt, str(tdt), dkind, None))
            assert 0.4 * of < n < 0.6 * of, (n, of)
        print(f"  shape {shape} R {R} storage {dt} views {tdt}: ok", flush=True)
        s.close()
        t.close()
    ctx.close()


def equals_wls():
    """c = inf: with weights the tensor's bytes and the loss are those of wls_torch from the same state, under
    every pair of views; without weights the tensor equals import_torch(data)"""
    ctx = pp.Context(0)
    shape = (36, 40, 20, 24)
    for R, dt, tdt in ((10, pp.F32, torch.float32), (33, pp.F64, torch.float64), (3, pp.F32, torch.float64),
                       (3, pp.F64, torch.float32)):
        t, s = session(ctx, shape, R, dt)
        V0 = t.download()
        for i, (dkind, wkind) in enumerate(PAIRS):
            data, h, lo, _ = view_pair(shape, dkind, wkind, tdt, i)
            t.upload(V0)
            loss, clipped = s.huber_torch(data, float("inf"), weights=h, lo=lo, want_loss=True)
            a = t.download()
            t.upload(V0)
            want = s.wls_torch(data, h, lo=lo, want_loss=True)
            b = t.download()
            assert np.mean(a != V0) > 0.2
            assert a.tobytes() == b.tobytes(), (R, dt, dkind, wkind, float(np.mean(a != b)))
            assert np.float64(loss).tobytes() == np.float64(want).tobytes(), (R, dt, dkind, wkind, loss, want)
            assert clipped == 0
        for i, dkind in enumerate(DATA_KINDS):
            data, _, lo, _ = view_pair(shape, dkind, dkind, tdt, 50 + i)
            t.upload(V0)
            loss, clipped = s.huber_torch(data, float("inf"), lo=lo, want_loss=True)
            a = t.download()
            t.upload(V0)
            t.import_torch(data, lo=lo)
            torch.cuda.synchronize()
            assert a.tobytes() == t.download().tobytes(), (R, dt, dkind)
            assert clipped == 0 and np.isfinite(loss)
        print(f"  R {R} storage {dt} views {tdt}: the weighted step's bits and loss; an import without weights",
              flush=True)
        s.close()
        t.close()
    ctx.close()


def special():
    """h in {0, -1, NaN, 0.5, 1, 2, inf}; x NaN / +-Inf wherever h is off: nothing propagates; x = +Inf under h = 1
    and a finite c: stored m + c, an infinite loss, counted as clipped; a c so small that everything clips; a
    c so large that nothing does"""
    ctx = pp.Context(0)
    shape, R = (9, 13, 7, 11), 3
    for dt in (pp.F32, pp.F64):
        for tdt in (torch.float32, torch.float64):
            t, s = session(ctx, shape, R, dt)
            V0 = t.download()
            W = s.get_factors()
            M, absM = cp_model(W), cp_model(W, True)
            g = torch.Generator(device="cpu").manual_seed(4)
            u = torch.rand(shape, generator=g)
            h = torch.full(shape, 0.5, dtype=torch.float64)
            for j, val in enumerate((0.0, -1.0, float("nan"), 0.5, 1.0, 2.0, float("inf"))):
                h[(u >= j / 7.0) & (u < (j + 1) / 7.0)] = val
            x = torch.rand(shape, generator=g, dtype=torch.float64) + 0.5
            off = ~(h > 0)
            v = torch.rand(shape, generator=g)
            x[off & (v < 0.3)] = float("inf")
            x[off & (v >= 0.3) & (v < 0.6)] = float("-inf")
            x[off & (v >= 0.6)] = float("nan")
            n_on = int((h > 0).sum())
            c_mid = float(np.median(np.abs(x.numpy() - M)[(h > 0).numpy()]))
            for kind in ("c_contiguous", "first_index_fastest"):
                data, hv = layout(x.to(tdt).to(DEV), kind), layout(h.to(tdt).to(DEV), kind)
                what = ("special", dt, str(tdt), kind)
                check_step(t, s, V0, M, absM, shape, dt, data, hv, None, c_mid, what)
                n, of = check_step(t, s, V0, M, absM, shape, dt, data, hv, None, 1e-6, what + ("all clip",))
                assert of == n_on and n >= 0.999 * of, (n, of)
                n, _ = check_step(t, s, V0, M, absM, shape, dt, data, hv, None, 1e6, what + ("none clips",))
                assert n == 0
                assert np.isfinite(t.download()).all()
            # +Inf under h = 1: m + c, counted, and the loss says so
            xi = x.clone()
            xi[off] = 0.0
            where = (h == 1.0).nonzero()[0]
            xi[tuple(where)] = float("inf")
            t.upload(V0)
            loss, n = s.huber_torch(xi.to(tdt).to(DEV), c_mid, weights=h.to(tdt).to(DEV), want_loss=True)
            got = t.download()
            _, _, want_n = huber_ref.step(xi.numpy(), h.numpy(), M, c_mid)
            idx = tuple(int(i) for i in where)
            want = M[idx] + c_mid
            tol = BAR * absM[idx] + (0.0 if dt == pp.F64 else float(np.spacing(np.float32(want))))
            assert loss == float("inf") and abs(got[idx] - want) <= tol, (dt, tdt, loss, got[idx], want)
            assert abs(n - want_n) <= 0.02 * want_n and np.isfinite(got).all(), (n, want_n)
            s.close()
            t.close()
    ctx.close()


def reproducible():
    """the same step with the outputs twice from the same state: the same bits, tensor, loss and count"""
    ctx = pp.Context(0)
    shape, R = (36, 40, 20, 24), 10
    for dt, tdt in ((pp.F32, torch.float32), (pp.F64, torch.float64)):
        t, s = session(ctx, shape, R, dt)
        V0 = t.download()
        M = cp_model(s.get_factors())
        for i, (dkind, wkind) in enumerate(PAIRS[:3] + PAIRS[6:7] + ((PAIRS[0][0], None), (PAIRS[1][0], None))):
            data, h, lo, _ = view_pair(shape, dkind, wkind or dkind, tdt, i)
            h = h if wkind else None
            c = median_c(M, shape, data, lo)
            runs = []
            for _ in range(2):
                t.upload(V0)
                loss, n = s.huber_torch(data, c, weights=h, lo=lo, want_loss=True)
                runs.append((np.float64(loss).tobytes(), n, t.download().tobytes()))
            assert runs[0][0] == runs[1][0], (dt, dkind, wkind, "loss")
            assert runs[0][1] == runs[1][1] and runs[0][1] > 0, (dt, dkind, wkind, "count")
            assert runs[0][2] == runs[1][2], (dt, dkind, wkind, "tensor")
        s.close()
        t.close()
    ctx.close()


def session_consistent():
    """after a step the session sweeps on the new contents: two sweeps agree to 1e-10 (F64 storage, both
    schedules) with a fresh session on a copy of the rewritten tensor from the same factors; so does a second
    session that existed on the tensor (its layouts and caches built) before the step"""
    ctx = pp.Context(0)
    shape, R = [20, 18, 16, 14], 4
    data, h, _, _ = view_pair(shape, "c_contiguous", "c_contiguous", torch.float64, 3)

    def relerr(a, b):
        return max(np.linalg.norm(x - y) / np.linalg.norm(y) for x, y in zip(a, b))

    for sched, hv in (("dt", h), ("msdt", None)):
        t = pp.Tensor(ctx, shape, pp.F64).fill_uniform(11, lo=0.5, hi=1.5)
        s, other = pp.CP(ctx, t, R), pp.CP(ctx, t, R)
        for x in (s, other):
            x.set_schedule(sched)
            x.set_factors(pp.init_factors(shape, R, 5), pp.init_factors(shape, R, 6))
            x.sweeps_dt(2)
        V0 = t.download()
        s.huber_torch(data, 0.2, weights=hv)
        W, G = s.get_factors(with_grad=True)
        stepped = t.download()
        assert np.mean(stepped != V0) > 0.2
        s.sweeps_dt(2)
        other.set_factors(W, G)
        other.sweeps_dt(2)
        t2 = pp.Tensor(ctx, shape, pp.F64).upload(stepped)
        fresh = pp.CP(ctx, t2, R)
        fresh.set_schedule(sched)
        fresh.set_factors(W, G)
        fresh.sweeps_dt(2)
        Wf = fresh.get_factors()
        e1, e2 = relerr(s.get_factors(), Wf), relerr(other.get_factors(), Wf)
        print(f"  schedule {sched}: stepping session {e1:.3g}, other session {e2:.3g}", flush=True)
        assert e1 <= 1e-10 and e2 <= 1e-10, (sched, e1, e2)
        for x in (s, other, fresh, t, t2):
            x.close()
    ctx.close()


def check_quantile(v, n, a_ref, tol_m, n_want, p, what):
    """the derived acceptance rule: with k the rank asked for, tol_e = the fp64 bar on the model of element e +
    one fp32 step of v, #{a_ref < v - tol} <= k < #{a_ref <= v + tol}: the kernel's keys are
    float32(|x - m'|) with |m' - m| within the bar, so a key lies within tol of a_ref, and v is the k-th key"""
    assert n == n_want, (what, n, n_want)
    k = min(n - 1, max(0, math.ceil(p * n) - 1))
    tol = tol_m + float(np.spacing(np.float32(v)))
    below, upto = int(np.count_nonzero(a_ref < v - tol)), int(np.count_nonzero(a_ref <= v + tol))
    assert below <= k < upto, (what, p, v, k, below, upto)


def quantile():
    """the quantile against numpy under the derived rank rule; an exact case (powers of two, ties, zeros) bit for
    bit; all keys equal; a single element; no element; +inf and NaN; nothing of the session or tensor changes;
    BF16 storage"""
    ctx = pp.Context(0)
    for shape, R, seed in (((23, 17, 30), 3, 1), ((23, 17, 30), 33, 2), ((36, 40, 20, 24), 3, 3),
                           ((36, 40, 20, 24), 33, 4)):
        t, s = session(ctx, shape, R, pp.BF16 if seed == 2 else pp.F32, seed=seed)
        V0, W0 = t.download(), s.get_factors()
        M, absM = cp_model(W0), cp_model(W0, True)
        for tdt in (torch.float32, torch.float64):
            for i, dkind in enumerate(DATA_KINDS):
                data, h, lo, box = view_pair(shape, dkind, dkind, tdt, 10 * seed + i)
                sl = box_slices(shape, lo, box)
                a_all, hh = np.abs(host(data) - M[sl]), host(h)
                for hv in (h, None):
                    on = hh > 0 if hv is not None else np.ones(box, dtype=bool)
                    a_ref, tol_m = a_all[on], BAR * absM[sl][on]
                    for p in PS:
                        v, n = s.abs_residual_quantile_torch(data, p, weights=hv, lo=lo)
                        check_quantile(v, n, a_ref, tol_m, int(on.sum()), p, (shape, R, str(tdt), dkind, hv is None))
        assert np.array_equal(t.download(), V0)
        for a, b in zip(s.get_factors(), W0):
            assert np.array_equal(a, b)
        print(f"  shape {shape} R {R}: ranks within the bar, counts exact, session and tensor untouched", flush=True)
        s.close()
        t.close()
    # exact: R = 1, factors and offsets dyadic, so |x - m| is exact on both sides: the same bits, ties included
    shape = (20, 9, 33)
    g = np.random.default_rng(5)
    W = [np.asfortranarray(2.0 ** g.integers(-2, 3, size=(n, 1))) for n in shape]
    t = pp.Tensor(ctx, list(shape), pp.F32).fill_uniform(1)
    s = pp.CP(ctx, t, 1)
    s.set_factors(W, pp.init_factors(shape, 1, 2))
    assert all(np.array_equal(a, b) for a, b in zip(s.get_factors(), W))
    M = cp_model(W)
    off = g.integers(-6, 7, size=shape) / 8.0
    off[g.uniform(size=shape) < 0.2] = 0.0
    hh = np.where(g.uniform(size=shape) < 0.3, 0.0, 1.0)
    for tdt in (torch.float32, torch.float64):
        for kind in DATA_KINDS[:3]:
            data, hv = layout(torch.from_numpy(M + off).to(tdt).to(DEV), kind), layout(torch.from_numpy(hh).to(tdt).to(DEV), kind)
            for w, wn in ((hv, hh), (None, None)):
                for p in PS + (0.1, 0.37, 0.63):
                    got, want = s.abs_residual_quantile_torch(data, p, weights=w), huber_ref.quantile(M + off, wn, M, p)
                    assert got == want, (str(tdt), kind, p, got, want)
    same = torch.from_numpy(M + 0.25).to(DEV)
    for p in PS:
        assert s.abs_residual_quantile_torch(same, p) == (0.25, M.size), p
    one = torch.from_numpy(M[3:4, 2:3, 5:6] - 1.5).to(DEV)
    for p in PS:
        assert s.abs_residual_quantile_torch(one, p, lo=[3, 2, 5]) == (1.5, 1), p
    v, n = s.abs_residual_quantile_torch(same, 0.5, weights=torch.zeros(shape, dtype=torch.float64, device=DEV))
    assert math.isnan(v) and n == 0
    bad = M + off
    bad[1, 2, 3], bad[7, 1, 30] = np.inf, np.nan
    badt, n_all = torch.from_numpy(bad).to(DEV), M.size
    v, n = s.abs_residual_quantile_torch(badt, 1.0)
    assert math.isnan(v) and n == n_all
    assert s.abs_residual_quantile_torch(badt, (n_all - 1.5) / n_all) == (float("inf"), n_all)
    assert s.abs_residual_quantile_torch(badt, (n_all - 2.5) / n_all) == (0.75, n_all)
    for p in PS:
        got, want = s.abs_residual_quantile_torch(badt, p), huber_ref.quantile(bad, None, M, p)
        assert got == want or (math.isnan(got[0]) and math.isnan(want[0]) and got[1] == want[1]), (p, got, want)
    s.close()
    t.close()
    ctx.close()


def driver():
    """Robust CP recovers a rank-3 tensor through 5 % gross outliers that plain ALS cannot fit through.

    (12, 10, 9, 8), R = 3, data = [[W_true]] (factors U(0, 1)) + 0.01 N(0, 1), and on a random 5 % of the entries
    +- U(0.5, 2); random start, 20 plain sweeps, then two stages of 100 iterations, each at
    c = 1.345 x 1.4826 x median |r| taken at the stage's start. With the numpy reference (tests/huber_ref.py),
    seeds 0-5: relative error against the clean tensor 4.2e-3 ... 5.7e-3, 320 plain sweeps 0.09 ... 0.26; c goes
    from 0.038 ... 0.048 to 0.0142 ... 0.0146; about 19 % of the entries are clipped at the end; the loss at a fixed
    c rises by at most 3e-16 relative between iterations, also with Z rounded to fp32. Asserted with seed 0 for
    F64 and F32 storage, the reference run here on the same data: error <= 2 x the reference's; error <= 0.1 x
    that of the library's own 320 plain sweeps; within each stage every look's loss <= (1 + 1e-9) x the look
    before; run_robust(c=None) returns a c within the quantile case's tolerance of the reference's;
    run_robust(rel_change=1e-6, resprint=10) returns 2; with tol set to a residual already reached it returns 1."""
    ctx = pp.Context(0)
    shape, R, seed = [12, 10, 9, 8], 3, 0
    g = np.random.default_rng(seed)
    Wt = [g.uniform(0.0, 1.0, (n, R)) for n in shape]
    clean = wls_ref.cp_model(Wt)
    xh = clean + 0.01 * g.normal(size=shape)
    bad = g.uniform(size=shape) < 0.05
    xh = xh + bad * g.choice([-1.0, 1.0], size=shape) * g.uniform(0.5, 2.0, size=shape)
    W0 = [np.asfortranarray(g.uniform(0.0, 1.0, (n, R))) for n in shape]
    G0 = pp.init_factors(shape, R, 51)
    nclean = float(np.linalg.norm(clean))
    tune = 1.345 * 1.4826

    def err_of(W):
        return float(np.linalg.norm(wls_ref.cp_model(W) - clean)) / nclean

    Wr = [w.copy() for w in W0]
    for _ in range(20):
        wls_ref.als_sweep(xh, Wr)
    ref_c = []
    for _ in range(2):
        ref_c.append(tune * float(np.median(np.abs(xh - wls_ref.cp_model(Wr)))))
        Wr, _ = huber_ref.mm_als(xh, None, Wr, 100, ref_c[-1])
    ref_err = err_of(Wr)
    ref_clipped = huber_ref.step(xh, None, wls_ref.cp_model(Wr), ref_c[-1])[2] / xh.size
    print(f"  numpy reference: error {ref_err:.3g}, c {ref_c[0]:.4g} then {ref_c[1]:.4g}, clipped {ref_clipped:.3f}",
          flush=True)
    assert ref_err < 0.01
    for dt, tdt in ((pp.F64, torch.float64), (pp.F32, torch.float32)):
        data = torch.from_numpy(xh).to(tdt).to(DEV)
        xd = host(data)
        t = pp.Tensor(ctx, shape, dt).upload(xh)
        s = pp.CP(ctx, t, R)
        s.set_factors(W0, G0)
        s.sweeps_dt(320)
        plain = err_of(s.get_factors())
        t.upload(xh)
        s.set_factors(W0, G0)
        s.sweeps_dt(20)
        W20, G20 = s.get_factors(with_grad=True)
        stages = []
        for stage in range(2):
            W = s.get_factors()
            M, absM = cp_model(W), cp_model(W, True)
            looks, c = [], None
            for _ in range(10):
                rc, it, res, c_used = s.run_robust(data, c=c, inner_sweeps=1, maxiter=10, resprint=10)
                assert (rc, it) == (0, 10), (dt, rc, it)
                if c is None:   # taken once, from the factors the session held: the rank rule of the quantile case
                    check_quantile(c_used / tune, xd.size, np.abs(xd - M).ravel(), BAR * absM.ravel(), xd.size, 0.5,
                                   ("driver c", dt, stage))
                    print(f"    stage {stage}: c {c_used:.6g} (numpy's own run: {ref_c[stage]:.6g})", flush=True)
                c = c_used
                looks.append(res)
            rise = max((b * b - a * a) / (a * a) for a, b in zip(looks, looks[1:]))
            stages.append((c, looks, rise))
            assert rise <= 1e-9, (dt, stage, rise)
        err = err_of(s.get_factors())
        _, n = s.huber_torch(data, stages[1][0], want_loss=True)
        print(f"  storage {dt}: error {err:.3g} (reference {ref_err:.3g}, 320 plain sweeps {plain:.3g}); c "
              f"{stages[0][0]:.4g} then {stages[1][0]:.4g}; clipped {n / xd.size:.3f}; largest relative rise of the "
              f"loss between looks {max(stages[0][2], stages[1][2]):.3g}", flush=True)
        assert err <= 2 * ref_err, (dt, err, ref_err)
        assert err <= 0.1 * plain, (dt, err, plain)
        c1, looks1, _ = stages[0]
        s2 = pp.CP(ctx, t.upload(xh), R)
        s2.set_factors(W20, G20)
        rc, it, res, _ = s2.run_robust(data, c=c1, inner_sweeps=1, rel_change=1e-6, resprint=10, maxiter=2000)
        print(f"    rel_change 1e-6: stopped {rc} after {it} iterations at {res:.6g}", flush=True)
        assert rc == 2, (dt, rc, it)
        t.upload(xh)
        s2.set_factors(W20, G20)
        rc, it, res, _ = s2.run_robust(data, c=c1, inner_sweeps=1, maxiter=200, resprint=10, tol=looks1[2])
        print(f"    tol = the residual at iteration 30: stopped {rc} after {it} iterations", flush=True)
        assert rc == 1 and it < 200 and res <= looks1[2], (dt, rc, it, res, looks1[2])
        for x in (s2, s, t):
            x.close()
    ctx.close()


def stream_order():
    """a step on a side torch stream right behind the kernels that write data and weights there, no host
    synchronisation; both are overwritten on that stream right after the call; then the same without weights"""
    ctx = pp.Context(0)
    shape, R = (64, 256, 1024), 4   # 64 MB of fp32
    t = pp.Tensor(ctx, list(shape), pp.F32).fill_uniform(3)
    s = pp.CP(ctx, t, R)
    s.set_factors(pp.init_factors(shape, R, 1), pp.init_factors(shape, R, 2))
    ref = s.model_to_torch(torch.float64)
    c = 0.5
    for weighted in (True, False):
        data = torch.full(shape, -5.0, dtype=torch.float32, device=DEV)      # stale contents
        h = torch.ones(shape, dtype=torch.float32, device=DEV)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            busy = torch.rand((4096, 4096), device=DEV)
            for _ in range(8):
                busy = busy @ busy / 4096.0   # keep the stream busy ahead of the views' kernels
            real_x = ref.float() + 2.0 * (torch.rand(shape, device=DEV) - 0.5)
            real_h = torch.rand(shape, device=DEV) if weighted else torch.ones(shape, device=DEV)
            data.copy_(real_x)
            h.copy_(real_h)
            assert s.huber_torch(data, c, weights=h if weighted else None) is None
            data.fill_(-5.0)                  # must not reach the step's reads
            h.fill_(0.0)
            out = torch.empty(shape, dtype=torch.float32, device=DEV)
            t.export_torch(out)
            want = ref + real_h.double() * (real_x.double() - ref).clamp(-c, c)
            near = (out.double() - want).abs() <= want.abs() * 2.0 ** -23 + 1e-12
        torch.cuda.synchronize()
        assert bool(near.all()), (weighted, int((~near).sum()))
    s.close()
    t.close()
    ctx.close()


def refusals():
    """for either view a host pointer, a span leaving its allocation, a negative stride, a box outside the
    tensor: PPALS_ERR_ARG with the entry point's name in front and the view named, before anything is launched;
    bad c and p; an integer dtype and mismatched torch dtypes: TypeError; BF16 storage and R = 129:
    PPALS_ERR_UNSUPPORTED (the quantile accepts BF16). The tensor is unchanged"""
    ctx = pp.Context(0)
    lens, R = [20, 12, 9], 3
    t = pp.Tensor(ctx, lens, pp.F32).fill_uniform(1)
    s = pp.CP(ctx, t, R)
    s.set_factors(pp.init_factors(lens, R, 1), pp.init_factors(lens, R, 2))
    V0 = t.download()
    fstr = [1, 20, 240]
    good = torch.full(lens, 0.5, dtype=torch.float32, device=DEV)   # any launch would show
    host_t = torch.full(lens, 0.5, dtype=torch.float32)
    ok = dict(ptr=good.data_ptr(), strides=fstr)
    bad = [("host", dict(ptr=host_t.data_ptr(), strides=fstr)),
           ("span", dict(ptr=good.data_ptr(), strides=[1, 20, 240 * 10 ** 6])),
           ("negative_stride", dict(ptr=good.data_ptr(), strides=[1, -20, 240]))]
    for name, kw in bad:
        for side, view in (("data", "the data view: "), ("weights", "the weights view: ")):
            d, w = (kw, ok) if side == "data" else (ok, kw)
            for want_loss in (False, True):
                try:
                    s.huber_device(d["ptr"], w["ptr"], pp.F32, lens, d["strides"], w["strides"], 0.1,
                                   want_loss=want_loss)
                    raise AssertionError(f"{name} ({side}) accepted")
                except pp.PpalsError as e:
                    assert "ppals error -3: ppals_cp_huber_device: " + view in str(e), (name, side, str(e))
        try:
            s.huber_device(kw["ptr"], None, pp.F32, lens, kw["strides"], None, 0.1)
            raise AssertionError(f"{name} (data, no weights) accepted")
        except pp.PpalsError as e:
            assert "ppals error -3: ppals_cp_huber_device: the data view: " in str(e), (name, str(e))
    for call, fn in ((lambda: s.huber_device(ok["ptr"], ok["ptr"], pp.F32, [10, 12, 9], fstr, fstr, 0.1, lo=[15, 0, 0]),
                      "ppals_cp_huber_device"),
                     (lambda: s.run_robust(good[:10], c=0.1, weights=good[:10], lo=[15, 0, 0], maxiter=2), "ppals_cp_robust"),
                     (lambda: s.abs_residual_quantile_torch(good[:10], lo=[15, 0, 0]),
                      "ppals_cp_abs_residual_quantile")):
        try:
            call()
            raise AssertionError(f"{fn}: box accepted")
        except pp.PpalsError as e:
            assert f"ppals error -3: {fn}: the data view: box mode 0" in str(e), str(e)
    for c in (0.0, -1.0, float("nan")):
        for call in (lambda: s.huber_torch(good, c), lambda: s.run_robust(good, c=c, maxiter=2)):
            try:
                call()
                raise AssertionError(f"c = {c} accepted")
            except pp.PpalsError as e:
                assert "ppals error -3: ppals_cp_" in str(e) and "c must be positive" in str(e), str(e)
    for p in (-0.1, 1.1, float("nan")):
        try:
            s.abs_residual_quantile_torch(good, p)
            raise AssertionError(f"p = {p} accepted")
        except pp.PpalsError as e:
            assert "ppals error -3: ppals_cp_abs_residual_quantile: p must lie in [0, 1]" in str(e), str(e)
    ints = torch.ones(lens, dtype=torch.int32, device=DEV)
    for call in (lambda: s.huber_torch(ints, 0.1, weights=ints), lambda: s.huber_torch(good, 0.1, weights=good.double()),
                 lambda: s.huber_torch(ints, 0.1), lambda: s.run_robust(good.double(), c=0.1, weights=good, maxiter=2),
                 lambda: s.run_robust(ints, maxiter=2), lambda: s.abs_residual_quantile_torch(ints)):
        try:
            call()
            raise AssertionError("bad torch dtypes accepted")
        except TypeError:
            pass
    try:
        s.huber_torch(host_t, 0.1)
        raise AssertionError("a host tensor was accepted")
    except pp.PpalsError as e:
        assert "the context on cuda:" in str(e), str(e)
    torch.cuda.synchronize()
    assert np.array_equal(t.download(), V0)
    for dt, R2, text in ((pp.BF16, 3, "BF16 storage"), (pp.F32, 129, "R > 128")):
        t2 = pp.Tensor(ctx, lens, dt).fill_uniform(1)
        s2 = pp.CP(ctx, t2, R2)
        s2.set_factors(pp.init_factors(lens, R2, 1), pp.init_factors(lens, R2, 2))
        V2 = t2.download()
        for call in (lambda: s2.huber_torch(good, 0.1, weights=good, want_loss=True), lambda: s2.huber_torch(good, 0.1),
                     lambda: s2.run_robust(good, c=0.1, maxiter=2)):
            try:
                call()
                raise AssertionError(f"{text} accepted")
            except pp.PpalsError as e:
                assert "ppals error -5: ppals_cp_" in str(e) and text in str(e), str(e)
        if dt == pp.BF16:
            v, n = s2.abs_residual_quantile_torch(good)
            assert n == good.numel() and np.isfinite(v)
        else:
            try:
                s2.abs_residual_quantile_torch(good)
                raise AssertionError("the quantile accepted R = 129")
            except pp.PpalsError as e:
                assert "ppals error -5: ppals_cp_abs_residual_quantile: R > 128" in str(e), str(e)
        torch.cuda.synchronize()
        assert np.array_equal(t2.download(), V2)
        s2.close()
        t2.close()
    s.close()
    t.close()
    ctx.close()


def shards():
    """P = 2 ranks on the one GPU (hipsim library): each rank rewrites only its own rows, loss and clipped count
    are the global sums on both ranks; the quantile refuses two ranks"""
    import hipsim_util
    hp = hipsim_util.load(make=False)
    lens, R, P = [29, 12, 10, 9], 4, 2
    g = torch.Generator(device="cpu").manual_seed(7)
    Xh = torch.rand(lens, generator=g, dtype=torch.float64)
    X = Xh.to(DEV)
    data, h, _, _ = view_pair(lens, "c_contiguous", "first_index_fastest", torch.float64, 5)
    c = 0.3
    torch.cuda.synchronize()
    W0, G0 = hp.init_factors(lens, R, 20), hp.init_factors(lens, R, 21)
    w = hipsim_util.ThreadWorld(P, timeout=300)
    errors, outs = [], {}

    def rank_main(rank):
        try:
            ctx = hp.Context(0)
            uid, keep = w.comm_uid(rank)
            ctx.init_comm(rank, P, uid)
            t = hp.Tensor(ctx, lens, hp.F64).import_torch(X, stream=0)
            lo, n = t.local_rows()
            s = hp.CP(ctx, t, R)
            s.set_factors(W0, G0)
            s.sweeps_dt(2)
            W = s.get_factors()
            before = t.download()
            refused = ""
            try:
                s.abs_residual_quantile_torch(data, 0.5, stream=0)
            except hp.PpalsError as e:
                refused = str(e)
            loss, clipped = s.huber_torch(data, c, weights=h, stream=0, want_loss=True)
            mid = t.download()
            t.import_torch(X, stream=0)
            loss1, clipped1 = s.huber_torch(data, c, stream=0, want_loss=True)
            outs[rank] = {"rows": (lo, n), "W": W, "before": before, "after": mid, "loss": loss, "clipped": clipped,
                          "after1": t.download(), "loss1": loss1, "clipped1": clipped1, "refused": refused}
            w.barrier()
            s.close()
            t.close()
            ctx.close()
            del keep
        except BaseException as e:  # noqa: BLE001
            errors.append((rank, repr(e)))
            w.abort()

    th = [threading.Thread(target=rank_main, args=(r,)) for r in range(P)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors and not w.failed, (errors, w.failed)
    Vs, xh, hh = Xh.numpy(), host(data), host(h)
    M, absM = cp_model(outs[0]["W"]), cp_model(outs[0]["W"], True)
    bar = BAR * (absM + np.abs(xh))
    for hv, key, lk, ck in ((hh, "after", "loss", "clipped"), (None, "after1", "loss1", "clipped1")):
        z, want_loss, _ = huber_ref.step(xh, hv, M, c)
        on = hv > 0 if hv is not None else np.ones(lens, dtype=bool)
        a_ref = np.abs(xh - M)
        n_lo, n_hi = int(np.count_nonzero(on & (a_ref > c + bar))), int(np.count_nonzero(on & (a_ref > c - bar)))
        scale = float(np.sum((np.minimum(hv, 1.0) if hv is not None else 1.0) * xh * xh))
        union = np.zeros(lens)
        for rank in range(P):
            lo, n = outs[rank]["rows"]
            a, b = outs[rank][key], outs[rank]["before"]
            assert np.array_equal(a[:lo], b[:lo]) and np.array_equal(a[lo + n:], b[lo + n:]), rank
            assert np.array_equal(b[lo:lo + n], Vs[lo:lo + n]), rank
            union[lo:lo + n] = a[lo:lo + n]
            assert abs(outs[rank][lk] - want_loss) <= 1e-10 * scale, (rank, outs[rank][lk], want_loss)
            assert n_lo <= outs[rank][ck] <= n_hi and n_lo > 0, (rank, outs[rank][ck], n_lo, n_hi)
        assert outs[0][lk] == outs[1][lk] and outs[0][ck] == outs[1][ck]
        check_values(union, z, absM + np.abs(xh), torch.float64, "sharded")
    for rank in range(P):
        assert "ppals error -5: ppals_cp_abs_residual_quantile: the residual quantile runs on one rank" in \
            outs[rank]["refused"], outs[rank]["refused"]


def quick():
    """one step with its outputs and one median against numpy (the smallest end-to-end check)"""
    ctx = pp.Context(0)
    shape, R = (12, 10, 8), 3
    t, s = session(ctx, shape, R, pp.F64)
    V0 = t.download()
    W = s.get_factors()
    M, absM = cp_model(W), cp_model(W, True)
    for i, (dkind, wkind) in enumerate(PAIRS[:2]):
        data, h, lo, _ = view_pair(shape, dkind, wkind, torch.float64, i)
        for hv in (h, None):
            check_step(t, s, V0, M, absM, shape, pp.F64, data, hv, lo, median_c(M, shape, data, lo),
                       ("quick", dkind, wkind, hv is None))
        v, n = s.abs_residual_quantile_torch(data, 0.5, lo=lo)
        a = np.abs(host(data) - M[box_slices(shape, lo, data.shape)])
        check_quantile(v, n, a.ravel(), BAR * absM[box_slices(shape, lo, data.shape)].ravel(), a.size, 0.5, "quick")
    s.close()
    t.close()
    ctx.close()


CASES = {f.__name__: f for f in (values, equals_wls, special, reproducible, session_consistent, quantile, driver,
                                 stream_order, refusals, shards, quick)}

if __name__ == "__main__":
    CASES[sys.argv[1]](*sys.argv[2:])
    print(f"huber case {' '.join(sys.argv[1:])}: ok", flush=True)
