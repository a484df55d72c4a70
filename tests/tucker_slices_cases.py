"""The cases of a Tucker session's influence plot (ppals_tucker_residual, ppals_tucker_slice_residuals,
ppals_tucker_leverages, Tucker.explained) shared by tests/test_tucker_slices_hostsim.py (the engine's control
flow and the C ABI over the fp64 host twins of ops.h) and tests/test_gpu_tucker_slices.py (the HIP kernels, one
case per process: `python tucker_slices_cases.py <case>`): each takes the binding `pp` it runs on. This module
does not import torch: the stand-in tests run in the pytest process, which may hold a HIP runtime already, and
torch must come first where the two meet. The GPU child process imports torch before anything else (below), and
only the GPU branches use it. Reference and bars: tests/tucker_slices_ref.py. Every figure is printed before it
is asserted."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tucker_slices_ref as R  # noqa: E402
from tucker_slices_ref import tucker_model  # noqa: E402

F32, F64 = 0, 1

# (shape, the values of r_0, the other ranks): what each covers is in values()
VALUE_CASES = [((70, 12, 9), (1, 4, 16, 17, 20), (3, 5)),
               ((130, 9, 11), (33, 70, 112, 113), (4, 2)),
               ((8, 66, 7, 5), (3, 8), (4, 2, 3)),
               ((64, 1, 65), (2,), (1, 3))]
FITTED = [((70, 12, 9), (4, 3, 5)), ((8, 66, 7, 5), (3, 4, 2, 3))]


def random_model(lens, ranks, seed):
    """factors and a core from a seeded generator (nothing is swept, so any rank is admissible): random_model of
    tucker_impute_cases.py, which imports torch"""
    g = np.random.default_rng(seed)
    W = [np.asfortranarray(g.standard_normal((s, r))) for s, r in zip(lens, ranks)]
    return W, np.asfortranarray(g.standard_normal(ranks))


def given_session(ctx, t, ranks, seed, mod):
    """given_session of tucker_impute_cases.py"""
    k = mod.Tucker(ctx, t, list(ranks))
    W, core = random_model(t.lens, ranks, seed)
    k.set_factors(W)
    k.set_core(core)
    return k


def on_gpu(pp):
    return pp.__name__ == "ppals"


def same_bytes(a, b):
    return len(a) == len(b) and all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


def fitted_session(pp, ctx, lens, ranks, dt, seed=3):
    """_tucker_session of model_export_cases.py — a low multilinear rank tensor plus noise, HOSVD and two
    sweeps — on the GPU; on the stand-in a tensor of the same make from numpy's generator, through upload"""
    if on_gpu(pp):
        from model_export_cases import _tucker_session
        return _tucker_session(ctx, list(lens), list(ranks), dt, seed)
    g = np.random.default_rng(seed)
    W, core = random_model(lens, ranks, seed)
    X = tucker_model(W, core)
    X = X + 0.05 * X.std() * g.standard_normal(lens)
    t = pp.Tensor(ctx, list(lens), dt).upload(np.asfortranarray(X))
    k = pp.Tucker(ctx, t, list(ranks))
    k.hosvd()
    k.sweeps_dt(2)
    return t, k


def pass_launches(k):
    """the pass kernels one slice_residuals launches, counted by name in a torch.profiler trace"""
    import torch
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        k.slice_residuals()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if "k_model_slices" in e.name]
    wide = sum("k_model_slices_wide" in n for n in names)
    return {"wide": wide, "regs": len(names) - wide}


def check_session(pp, t, k, what):
    """every entry of every mode against numpy, the mode sums, the total against residual()**2; returns the
    worst relative entry error"""
    W, core = k.get_factors()
    ss, total = k.slice_residuals(return_total=True)
    worst = R.check_sums(what, ss, total, t.download(), W, core)
    res2 = k.residual() ** 2
    print(f"[tucker slices] {what}: total {total:.17g} residual()^2 {res2:.17g} relative "
          f"{abs(total - res2) / res2:.3e} (bar {R.RESIDUAL_RTOL:.0e})", flush=True)
    assert abs(total - res2) <= R.RESIDUAL_RTOL * res2, what
    assert same_bytes(ss, k.slice_residuals())   # total may be NULL
    return worst


def values(pp, ctx):
    """1. sessions with random factors and core (nothing is swept), storage alternating F32 / F64:
    (70, 12, 9): two row tiles, the second partial; r_0 on both sides of 16 (1, 4, 16 | 17, 20);
    (130, 9, 11): three row tiles, the LDS route to its limit (33, 70, 112) and one past it (113);
    (8, 66, 7, 5): fewer than 16 rows, three modes folded from B;
    (64, 1, 65): a full tile, an extent of 1, one column past a tile.
    On the GPU each case counts the pass kernels of one call by name: 16 < r_0 <= 112 took k_model_slices_wide,
    the others k_model_slices, one launch (one slab)."""
    n, worst = 0, 0.0
    for shape, r0s, rest in VALUE_CASES:
        for r0 in r0s:
            dt = (F32, F64)[n % 2]
            ranks = (r0,) + rest
            t = pp.Tensor(ctx, list(shape), dt).fill_uniform(100 + n, lo=0.5, hi=1.5)
            k = given_session(ctx, t, ranks, 10 * n, mod=pp)
            worst = max(worst, check_session(pp, t, k, f"{shape} ranks {ranks} storage {dt}"))
            if on_gpu(pp):
                route = pass_launches(k)
                wide = 16 < r0 <= 112
                print(f"[tucker slices] {shape} ranks {ranks}: pass kernels of one call, by name: {route}", flush=True)
                assert route == {"wide": 1 if wide else 0, "regs": 0 if wide else 1}, (ranks, route)
            k.close()
            t.close()
            n += 1
    print(f"[tucker slices] values: worst relative entry error of all cases {worst:.3e}", flush=True)


def fitted(pp, ctx):
    """2. HOSVD plus two sweeps, orders 3 and 4, both storage types"""
    for lens, ranks in FITTED:
        for dt in (F32, F64):
            t, k = fitted_session(pp, ctx, lens, ranks, dt)
            check_session(pp, t, k, f"fitted {lens} ranks {ranks} storage {dt}")
            k.close()
            t.close()


def exact_fit(pp, ctx):
    """3. F64, V = tucker_model of the session's own factors: every entry and the total at most
    1e-24 ||tucker_model(|W|, |core|)||^2 (an element's error is a few hundred roundings of its terms'
    magnitudes), and no entry negative"""
    for n, (shape, ranks) in enumerate((((70, 12, 9), (4, 3, 5)), ((70, 12, 9), (20, 3, 5)), ((8, 66, 7, 5), (3, 4, 2, 3)))):
        W, core = random_model(shape, ranks, 60 + n)
        t = pp.Tensor(ctx, list(shape), F64).upload(tucker_model(W, core))
        k = pp.Tucker(ctx, t, list(ranks))
        k.set_factors(W)
        k.set_core(core)
        ss, total = k.slice_residuals(return_total=True)
        bar = 1e-24 * float(np.sum(tucker_model(W, core, True) ** 2))
        worst = max(float(np.max(a)) for a in ss)
        print(f"[tucker slices] exact fit {shape} ranks {ranks}: largest entry {worst:.3e} total {total:.3e} "
              f"bar {bar:.3e}", flush=True)
        assert all(np.all(a >= 0.0) for a in ss) and worst <= bar and 0.0 <= total <= bar
        k.close()
        t.close()


def slabs(pp, ctx):
    """4. (GPU) the two-slab box of the imputation's `slabs` case: (112, 560, 540), ranks (112, 4, 4), F32 — Z
    needs 112 x 560 x 8 B per row of the last mode, so two slabs of 534 + 6 rows (2^25 / (112 x 560) = 534.99, floored): two
    launches in the trace, the values against numpy, and ss of the slab mode across the cut at row 534"""
    shape, ranks = (112, 560, 540), (112, 4, 4)
    t = pp.Tensor(ctx, list(shape), F32).fill_uniform(5, lo=0.5, hi=1.5)
    k = pp.Tucker(ctx, t, list(ranks))
    g = np.random.default_rng(2)
    k.set_factors([np.asfortranarray(g.standard_normal((s, r)) / np.sqrt(r)) for s, r in zip(shape, ranks)])
    k.set_core(np.asfortranarray(g.standard_normal(ranks)))
    W, core = k.get_factors()
    ref = R.slice_sums(t.download(), W, core)
    ss, total = k.slice_residuals(return_total=True)
    R.check_sums("slabs", ss, total, None, W, core, ref=ref)
    cut = np.abs(ss[2][530:] - ref[0][2][530:]) / ref[0][2][530:]
    print(f"[tucker slices] slabs: relative errors of mode 2 at rows 530..539 {[f'{x:.1e}' for x in cut]}", flush=True)
    assert np.all(cut <= R.SS_RTOL)
    route = pass_launches(k)   # one launch per slab
    print(f"[tucker slices] slabs: pass kernels of one call, by name: {route}", flush=True)
    assert route == {"wide": 2, "regs": 0}, route
    k.close()
    t.close()


def reproducible(pp, ctx):
    """5. two calls from the same state give the same bytes: F32 and F64, r_0 = 4 and 20"""
    shape = (70, 40, 30)
    for dt in (F32, F64):
        for r0 in (4, 20):
            t = pp.Tensor(ctx, list(shape), dt).fill_uniform(7, lo=0.5, hi=1.5)
            k = given_session(ctx, t, (r0, 3, 4), 1, mod=pp)
            runs = []
            for _ in range(2):
                ss, total = k.slice_residuals(return_total=True)
                runs.append((ss + k.leverages(), np.float64(total).tobytes(), np.float64(k.residual()).tobytes()))
            assert same_bytes(runs[0][0], runs[1][0]) and runs[0][1:] == runs[1][1:], (dt, r0)
            k.close()
            t.close()


def slab_cap(pp, ctx):
    """a cap of one byte on the partial sums (PPALS_TEST_SLICE_WORK_BYTES): one row tile a launch, the bits of
    the uncapped session; on the GPU three launches at (130, 9, 11)"""
    shape = (130, 9, 11)
    for dt, ranks in ((F32, (4, 4, 2)), (F64, (33, 4, 2))):
        t = pp.Tensor(ctx, list(shape), dt).fill_uniform(9, lo=0.5, hi=1.5)
        out = []
        for cap in (None, "1"):
            old = os.environ.pop("PPALS_TEST_SLICE_WORK_BYTES", None)
            if cap:
                os.environ["PPALS_TEST_SLICE_WORK_BYTES"] = cap
            try:
                k = given_session(ctx, t, ranks, 4, mod=pp)
            finally:
                os.environ.pop("PPALS_TEST_SLICE_WORK_BYTES", None)
                if old is not None:
                    os.environ["PPALS_TEST_SLICE_WORK_BYTES"] = old
            out.append(k.slice_residuals(return_total=True))
            if cap:
                check_session(pp, t, k, f"capped {shape} ranks {ranks} storage {dt}")
                if on_gpu(pp):
                    route = pass_launches(k)
                    assert route["wide"] + route["regs"] == 3, route
            k.close()
        assert same_bytes(out[0][0], out[1][0]) and out[0][1] == out[1][1], (dt, ranks)
        t.close()


def _all(k):
    W, core = k.get_factors()
    return W + [core]


def undisturbed(pp, ctx):
    """6. two sessions from the same factors: one calls the three new entries between sweeps_dt(1) calls, the
    other get_factors() at the same points: factors and core bit-equal after each of three sweeps; the tensor's
    bytes unchanged; a third session created earlier on the tensor, run afterwards like the second, gives its
    bits. Order 3 (the multi-sweep schedule) and order 4."""
    for shape, ranks in (((40, 36, 30), (4, 3, 5)), ((20, 18, 16, 14), (3, 4, 2, 3))):
        for dt in (F64, F32):
            t = pp.Tensor(ctx, list(shape), dt).fill_uniform(11, lo=0.5, hi=1.5)
            g = np.random.default_rng(4)
            W = [np.asfortranarray(np.linalg.qr(g.standard_normal((s, r)))[0]) for s, r in zip(shape, ranks)]
            core = np.asfortranarray(g.standard_normal(ranks))
            third, a, b = (pp.Tucker(ctx, t, list(ranks)) for _ in range(3))
            for k in (third, a, b):
                k.set_factors(W)
                k.set_core(core)
            before = t.download().tobytes()
            want = []
            for sweep in range(3):
                a.residual()
                a.slice_residuals()
                a.leverages()
                b.get_factors()
                a.sweeps_dt(1)
                b.sweeps_dt(1)
                want.append(_all(b))
                assert same_bytes(_all(a), want[-1]), (shape, dt, sweep)
            assert t.download().tobytes() == before, "the tensor changed"
            for sweep in range(3):
                third.get_factors()
                third.sweeps_dt(1)
                assert same_bytes(_all(third), want[sweep]), (shape, dt, sweep, "the third session")
            for k in (third, a, b):
                k.close()
            t.close()


def leverages(pp, ctx):
    """7. fitted sessions: against pinv, within [-1e-12, 1 + 1e-12], each mode summing to r_i within 1e-9, equal
    to the row sums of squares of W_i within 1e-12; standard-normal factors through set_factors at
    (130, 9, 11) with ranks (112, 4, 2) and (70, 5, 3): against pinv; a factor with a repeated column: NaN
    everywhere, PPALS_OK"""
    for lens, ranks in FITTED:
        for dt in (F32, F64):
            t, k = fitted_session(pp, ctx, lens, ranks, dt)
            W, _ = k.get_factors()
            lev = k.leverages()
            R.check_leverages(f"fitted {lens} ranks {ranks} storage {dt}", lev, W)
            lo, hi = min(float(a.min()) for a in lev), max(float(a.max()) for a in lev)
            sums = [float(a.sum()) - r for a, r in zip(lev, ranks)]
            rows = max(float(np.max(np.abs(a - np.sum(w * w, axis=1)))) for a, w in zip(lev, W))
            print(f"[tucker slices] leverages fitted {lens}: range [{lo:.3g}, {hi:.3g}], sums - r_i "
                  f"{[f'{x:.1e}' for x in sums]}, against the rows' sums of squares {rows:.3e}", flush=True)
            assert lo >= -1e-12 and hi <= 1.0 + 1e-12 and all(abs(x) <= 1e-9 for x in sums) and rows <= 1e-12
            k.close()
            t.close()
    shape = (130, 9, 11)
    t = pp.Tensor(ctx, list(shape), F64)
    for n, ranks in enumerate(((112, 4, 2), (70, 5, 3))):
        k = given_session(ctx, t, ranks, 30 + n, mod=pp)
        W, _ = k.get_factors()
        R.check_leverages(f"standard normal {shape} ranks {ranks}", k.leverages(), W)
        k.close()
    ranks = (5, 4, 2)
    W, core = random_model(shape, ranks, 33)
    W[1][:, 3] = W[1][:, 1]
    k = pp.Tucker(ctx, t, list(ranks))
    k.set_factors(W)
    k.set_core(core)
    out = np.full(sum(shape), -1.0)
    assert pp.lib().ppals_tucker_leverages(k._h, pp._dp(out)) == 0
    assert np.all(np.isnan(out)), out
    k.close()
    t.close()


def explained(pp, ctx):
    """8. its sum equals 1 - residual()^2 / ||V||^2 within 1e-9 on a fitted F64 session; shaped like the core"""
    lens, ranks = FITTED[0]
    t, k = fitted_session(pp, ctx, lens, ranks, F64)
    ex = k.explained()
    want = 1.0 - k.residual() ** 2 / t.norm() ** 2
    print(f"[tucker slices] explained: sum {float(ex.sum()):.15g} 1 - residual^2/|V|^2 {want:.15g}", flush=True)
    assert ex.shape == tuple(ranks) == k.get_factors()[1].shape
    assert np.all(ex >= 0.0) and abs(float(ex.sum()) - want) <= 1e-9
    k.close()
    t.close()


def refusals(pp, ctx):
    """9, the NULL half: PPALS_ERR_ARG through raw ctypes, the message starting with the entry's name"""
    L = pp.lib()
    lens, ranks = [8, 6, 5], (3, 2, 4)
    t = pp.Tensor(ctx, lens, F64).fill_uniform(1)
    k = given_session(ctx, t, ranks, 1, mod=pp)
    out, one, tot = np.zeros(sum(lens)), C.c_double(0), C.c_double(0)
    calls = (("ppals_tucker_residual", lambda h, o: L.ppals_tucker_residual(h, o), C.byref(one)),
             ("ppals_tucker_slice_residuals", lambda h, o: L.ppals_tucker_slice_residuals(h, o, C.byref(tot)), pp._dp(out)),
             ("ppals_tucker_leverages", lambda h, o: L.ppals_tucker_leverages(h, o), pp._dp(out)))
    for fn, call, good in calls:
        assert call(None, good) == -3
        assert L.ppals_last_error().decode().startswith(fn + ": "), L.ppals_last_error()
        assert call(k._h, None) == -3
        assert L.ppals_last_error().decode().startswith(fn + ": "), L.ppals_last_error()
        assert call(k._h, good) == 0
    assert L.ppals_tucker_slice_residuals(k._h, pp._dp(out), None) == 0   # total may be NULL
    k.close()
    t.close()


def two_ranks(pp):
    """9, the other half, on a back end with a callback communicator (the host stand-in, or the HIP kernels
    behind it): a context of two ranks gets PPALS_ERR_UNSUPPORTED from the two diagnostics before any launch —
    the communicator's collectives raise when called"""
    AR = C.CFUNCTYPE(None, C.POINTER(C.c_double), C.c_int64)
    RS = C.CFUNCTYPE(None, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int64)

    def never(*a):
        raise AssertionError("a collective was called")
    cbs = (AR(never), RS(never), RS(never))
    uid = C.create_string_buffer(128)
    for i, cb in enumerate(cbs):
        C.memmove(C.byref(uid, 8 * i), C.byref(C.cast(cb, C.c_void_p)), 8)
    c = pp.Context(0)
    c.init_comm(0, 2, uid)
    assert c.nranks == 2
    t = pp.Tensor(c, [6, 5, 4], F64)
    k = pp.Tucker(c, t, [2, 2, 2])
    out = np.zeros(15)
    L = pp.lib()
    for fn, call in (("ppals_tucker_slice_residuals", lambda: L.ppals_tucker_slice_residuals(k._h, pp._dp(out), None)),
                     ("ppals_tucker_leverages", lambda: L.ppals_tucker_leverages(k._h, pp._dp(out)))):
        assert call() == -5
        err = L.ppals_last_error().decode()
        assert err.startswith(fn + ": ") and "one rank" in err, err
    assert not out.any()
    k.close()
    t.close()
    c.close()


def two_ranks_gpu(pp, ctx):
    import hipsim_util
    two_ranks(hipsim_util.load(make=False))


GPU_CASES = {f.__name__: f for f in (values, fitted, exact_fit, slabs, reproducible, slab_cap, undisturbed, leverages,
                                     explained, refusals, two_ranks_gpu)}

if __name__ == "__main__":
    import torch  # noqa: F401  (before the binding loads libppals: one HIP runtime for both)
    import model_export_cases
    _W, _c = random_model((5, 4, 3), (2, 3, 2), 0)
    assert np.array_equal(model_export_cases.tucker_model(_W, _c), tucker_model(_W, _c))
    assert np.array_equal(model_export_cases.tucker_model(_W, _c, True), tucker_model(_W, _c, True))
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "pairwise-perturbation_amd"))
    import ppals  # noqa: E402
    if sys.argv[1] in ("fitted", "leverages", "explained", "values"):
        ppals.preload_eigensolver()   # a swept mode above 64, before anything initialises the HIP runtime
    context = ppals.Context(0)
    GPU_CASES[sys.argv[1]](ppals, context)
    context.close()
    print(f"tucker slices case {sys.argv[1]}: ok", flush=True)
