"""Cases of tests/test_gpu_tucker_impute.py, one per process: `python tucker_impute_cases.py <case>`.

ppals_tucker_impute_device / ppals_tucker_em (include/ppals.h) through the torch helpers of the binding. torch
is imported BEFORE the binding loads libppals (one HIP runtime for both). The reference is numpy's fp64
tucker_model of the factors and core get_factors returns, and the tensor downloaded before the call; the
value bars are check_values of model_export_cases.py. Exit status 0: passed."""
import os
import sys
import threading

import torch  # noqa: I001  (first: see above)
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "pairwise-perturbation_amd"))
import ppals as pp  # noqa: E402
from impute_cases import MISSING, masks  # noqa: E402
from model_export_cases import DEV, _tucker_session, check_values, tucker_model  # noqa: E402


def random_model(lens, ranks, seed):
    """factors and a core from a seeded generator (nothing is swept, so any rank is admissible)"""
    g = np.random.default_rng(seed)
    W = [np.asfortranarray(g.standard_normal((s, r))) for s, r in zip(lens, ranks)]
    return W, np.asfortranarray(g.standard_normal(ranks))


def given_session(ctx, t, ranks, seed, mod=pp):
    k = mod.Tucker(ctx, t, list(ranks))
    W, core = random_model(t.lens, ranks, seed)
    k.set_factors(W)
    k.set_core(core)
    return k


def check_impute(t, k, shape, dt, label, seed=17):
    """the mask kinds of impute_cases.masks, without and with the observed residual, from the same contents"""
    V0 = t.download()
    W, core = k.get_factors()
    M, absM = tucker_model(W, core), tucker_model(W, core, True)
    nv2 = float(np.linalg.norm(V0)) ** 2
    tdt = torch.float64 if dt == pp.F64 else torch.float32
    for name, mask, lo in masks(shape, seed):
        sl = tuple(slice(l, None) for l in lo) if lo else tuple(slice(None) for _ in shape)
        obs = np.ones(shape, dtype=bool)             # outside the box: untouched
        obs[sl] = mask.cpu().numpy() != 0
        want_sq = float(np.sum(((V0 - M) ** 2)[sl][obs[sl]]))
        for want_residual in (False, True):
            what = (label, name, want_residual)
            t.upload(V0)
            res = k.impute_torch(mask, lo=lo, want_residual=want_residual)
            got = t.download()
            assert np.array_equal(got[obs], V0[obs]), what   # bit for bit: both types widen exactly
            if (~obs).any():
                check_values(got[~obs], M[~obs], absM[~obs], tdt, what)
            if want_residual:
                tol = 1e-10 if dt == pp.F64 else 1e-6
                print(f"    {what}: observed_sq {res * res:.17g} numpy {want_sq:.17g} "
                      f"diff/|V|^2 {abs(res * res - want_sq) / nv2:.3g}", flush=True)
                assert abs(res * res - want_sq) <= tol * nv2, (what, res * res, want_sq, nv2)
            else:
                assert res is None
    t.upload(V0)


def launches_by_name(k, mask):
    """the model kernels one impute with the residual launches, counted by name in a torch.profiler trace"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        k.impute_torch(mask, want_residual=True)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if "k_model" in e.name or "k_sum_partials" in e.name]
    return {"wide": sum("k_model_impute_wide" in n for n in names),
            "view": sum("k_model_view" in n for n in names)}


def values():
    """leading extents of 70, 130 (two and three 64-row tiles) and 8, r_0 on both sides of the kernels'
    K = 16 threshold, at 4-step edges (17, 20, 33), at the ends (1, 112) and past the wide kernel's limit
    (113, which set_factors admits and no sweep does); orders 3 and 4; F32 / F64 storage alternating; every
    mask kind, without and with the residual; then a fitted session. Every case counts the model kernels of
    one impute by name in a torch.profiler trace: 16 < r_0 <= 112 took k_model_impute_wide, the others
    k_model_view, one launch each."""
    ctx = pp.Context(0)
    cases = [((70, 12, 9), r0, (3, 5)) for r0 in (1, 4, 16, 17, 20)]
    cases += [((130, 9, 11), r0, (4, 2)) for r0 in (33, 70, 112, 113)]
    cases += [((8, 66, 7, 5), r0, (4, 2, 3)) for r0 in (3, 8)]
    for n, (shape, r0, rest) in enumerate(cases):
        dt = (pp.F32, pp.F64)[n % 2]
        ranks = (r0,) + rest
        t = pp.Tensor(ctx, list(shape), dt).fill_uniform(100 + n, lo=0.5, hi=1.5)
        k = given_session(ctx, t, ranks, 10 * n)
        check_impute(t, k, shape, dt, (shape, ranks, dt))
        route = launches_by_name(k, masks(shape, 17)[0][1])
        wide = 16 < r0 <= 112
        print(f"  shape {shape} ranks {ranks} storage {dt}: ok; model kernels of one impute, by name: {route}",
              flush=True)
        assert route["wide"] == (1 if wide else 0) and route["view"] == (0 if wide else 1), (ranks, route)
        k.close()
        t.close()
    for dt in (pp.F32, pp.F64):
        shape, ranks = (70, 12, 9), (4, 3, 5)
        t, k = _tucker_session(ctx, list(shape), list(ranks), dt, 3)   # hosvd and two sweeps
        check_impute(t, k, shape, dt, ("fitted", dt))
        print(f"  fitted session storage {dt}: ok", flush=True)
        k.close()
        t.close()
    ctx.close()


def slabs():
    """a box whose Z needs more than the 256 MB of a chain buffer: (112, 560, 540), ranks (112, 4, 4), F32:
    112 x 560 x 8 B per row of the last mode, so two slabs of 535 + 5 rows (two launches in the trace); one dense
    mask with the residual"""
    ctx = pp.Context(0)
    shape, ranks = (112, 560, 540), (112, 4, 4)
    t = pp.Tensor(ctx, list(shape), pp.F32).fill_uniform(5, lo=0.5, hi=1.5)
    k = pp.Tucker(ctx, t, list(ranks))
    g = np.random.default_rng(2)
    W = [np.asfortranarray(g.standard_normal((s, r)) / np.sqrt(r)) for s, r in zip(shape, ranks)]
    core = np.asfortranarray(g.standard_normal(ranks))
    k.set_factors(W)
    k.set_core(core)
    V0 = t.download()
    W, core = k.get_factors()
    M, absM = tucker_model(W, core), tucker_model(W, core, True)
    gen = torch.Generator(device="cpu").manual_seed(3)
    mask = (torch.rand(shape, generator=gen) >= MISSING).to(DEV)
    obs = mask.cpu().numpy()
    res = k.impute_torch(mask, want_residual=True)
    got = t.download()
    assert np.array_equal(got[obs], V0[obs])
    check_values(got[~obs], M[~obs], absM[~obs], torch.float32, "slabs")
    # (both slabs were written: the last 5 rows of the last mode too)
    assert np.mean(got[:, :, 535:] != V0[:, :, 535:]) > 0.2 and np.mean(got[:, :, :535] != V0[:, :, :535]) > 0.2
    want_sq, nv2 = float(np.sum(((V0 - M) ** 2)[obs])), float(np.linalg.norm(V0)) ** 2
    print(f"  observed_sq {res * res:.17g} numpy {want_sq:.17g} diff/|V|^2 {abs(res * res - want_sq) / nv2:.3g}",
          flush=True)
    assert abs(res * res - want_sq) <= 1e-6 * nv2, (res * res, want_sq, nv2)
    route = launches_by_name(k, mask)   # one launch per slab
    assert route == {"wide": 2, "view": 0}, route
    k.close()
    t.close()
    ctx.close()


def reproducible():
    """the same impute with the residual twice from the same state: the same bits, tensor and sum"""
    ctx = pp.Context(0)
    shape = (70, 40, 30)
    for dt in (pp.F32, pp.F64):
        for r0 in (4, 20):
            t = pp.Tensor(ctx, list(shape), dt).fill_uniform(7, lo=0.5, hi=1.5)
            k = given_session(ctx, t, (r0, 3, 4), 1)
            V0 = t.download()
            for name, mask, lo in masks(shape, 5)[:3]:
                runs = []
                for _ in range(2):
                    t.upload(V0)
                    res = k.impute_torch(mask, lo=lo, want_residual=True)
                    runs.append((np.float64(res).tobytes(), t.download().tobytes()))
                assert runs[0][0] == runs[1][0], (dt, r0, name, "observed_sq")
                assert runs[0][1] == runs[1][1], (dt, r0, name, "tensor")
            k.close()
            t.close()
    ctx.close()


def session_consistent():
    """a session whose other layouts of the tensor were built BEFORE its impute sweeps, bit for bit, like a
    session created on the tensor AFTER it from the same factors and core (a stale layout would be off by
    O(1)); so does a third session that existed before and did not impute. Order 3 (three resident
    rotations, the multi-sweep schedule) and order 4 (two)."""
    ctx = pp.Context(0)
    for shape, ranks in (((40, 36, 30), (4, 3, 5)), ((20, 18, 16, 14), (3, 4, 2, 3))):
        for dt in (pp.F64, pp.F32):
            t = pp.Tensor(ctx, list(shape), dt).fill_uniform(11, lo=0.5, hi=1.5)
            g = np.random.default_rng(4)
            W = [np.asfortranarray(np.linalg.qr(g.standard_normal((s, r)))[0]) for s, r in zip(shape, ranks)]
            core = np.asfortranarray(g.standard_normal(ranks))
            mask = masks(shape, 3)[0][1]
            sessions = [pp.Tucker(ctx, t, list(ranks)) for _ in range(2)]   # layouts of the old contents
            for k in sessions:
                k.set_factors(W)
                k.set_core(core)
            V0 = t.download()
            sessions[0].impute_torch(mask)
            assert np.mean(t.download() != V0) > 0.2
            sessions.append(pp.Tucker(ctx, t, list(ranks)))                 # layouts of the new contents
            sessions[2].set_factors(W)
            sessions[2].set_core(core)
            out = []
            for k in sessions:
                k.sweeps_dt(2)
                Wk, ck = k.get_factors()
                out.append(Wk + [ck])
            for who, o in zip(("the imputing session", "the other session"), out[:2]):
                for x, y in zip(o, out[2]):
                    assert np.array_equal(x, y), (shape, dt, who)
            for k in sessions:
                k.close()
            t.close()
    ctx.close()


# ---- a numpy fp64 EM for Tucker: SVD-based HOSVD and HOOI, the loop of ppals_tucker_em ----
def _unfold(X, i):
    return np.moveaxis(X, i, 0).reshape(X.shape[i], -1)


def _ttm_t(X, W, skip=None):
    """X x_j W_j^T for every j != skip"""
    for j, w in enumerate(W):
        if j != skip:
            X = np.moveaxis(np.tensordot(w.T, X, axes=([1], [j])), 0, j)
    return X


def _lead(Y, i, r):
    return np.linalg.svd(_unfold(Y, i), full_matrices=False)[0][:, :r]


def numpy_em(V, obs, ranks, iters, looks):
    """X = V where observed, 0 elsewhere; W = hosvd(X); iteration k: residual on the observed entries (kept
    at the looks), X[missing] = model[missing], one HOOI sweep; one more imputation at the end.
    Returns (residuals at the looks, the final X)"""
    X = np.where(obs, V, 0.0)
    W = [_lead(X, i, r) for i, r in enumerate(ranks)]
    core = _ttm_t(X, W)
    res = {}
    for k in range(iters + 1):
        M = tucker_model(W, core)
        if k in looks:
            res[k] = float(np.linalg.norm((V - M)[obs]))
        X = np.where(obs, V, M)
        if k == iters:
            break
        for i, r in enumerate(ranks):
            W[i] = _lead(_ttm_t(X, W, skip=i), i, r)
        core = _ttm_t(X, W)
    return res, X


def em_recovers():
    """(20, 18, 16), ranks (3, 3, 2), 30 % missing at random and zeroed, start hosvd() of the zero-filled
    tensor, inner_sweeps = 1.
    (a) exact low-rank data: after 30 iterations the relative error on the MISSING entries is <= 1e-4 (F64 and
        F32 storage); the numpy loop is below 1e-6 on the same data (measured with numpy default_rng seeds
        1, 2, 3 on the CPU: 1.9e-8, 1.4e-9, 4.8e-9), so the bar has its margin.
    (b) the same plus noise of 0.05 standard deviations, F64: the observed residual at the looks of
        iterations 0, 10, 20, 30 agrees with the numpy loop's within 1e-5 |V_obs| (the loosest F64 projector
        bar of tests/test_gpu_tucker.py).
    (c) run_em with tol = the residual reached at iteration 10 stops on it: returns 1, it < maxiter."""
    ctx = pp.Context(0)
    shape, ranks, iters = (20, 18, 16), (3, 3, 2), 30
    g = np.random.default_rng(1)
    Wt, ct = [g.standard_normal((s, r)) for s, r in zip(shape, ranks)], g.standard_normal(ranks)
    Vt = tucker_model(Wt, ct)
    obs = g.random(shape) >= MISSING
    mask = torch.from_numpy(obs).to(DEV)
    noisy = Vt + 0.05 * Vt.std() * g.standard_normal(shape)

    def miss_err(X):
        return float(np.linalg.norm(X[~obs] - Vt[~obs]) / np.linalg.norm(Vt[~obs]))

    def start(V, dt):
        t = pp.Tensor(ctx, list(shape), dt).upload(np.where(obs, V, 0.0))
        k = pp.Tucker(ctx, t, list(ranks))
        k.hosvd()
        return t, k

    # (a)
    _, Xn = numpy_em(Vt, obs, ranks, iters, ())
    print(f"  exact data: numpy loop {miss_err(Xn):.3g} on the missing entries after {iters} iterations", flush=True)
    assert miss_err(Xn) < 1e-6, miss_err(Xn)
    for dt in (pp.F64, pp.F32):
        t, k = start(Vt, dt)
        rc, it, res = k.run_em(mask, inner_sweeps=1, maxiter=iters, resprint=10)
        err = miss_err(t.download())
        print(f"  exact data, storage {dt}: engine {err:.3g} after {it} iterations, observed residual {res:.3g}",
              flush=True)
        assert (rc, it) == (0, iters), (dt, rc, it)
        assert err <= 1e-4, (dt, err)
        k.close()
        t.close()
    # (b)
    looks = (0, 10, 20, 30)
    want, _ = numpy_em(noisy, obs, ranks, iters, looks)
    nobs = float(np.linalg.norm(noisy[obs]))
    t, k = start(noisy, pp.F64)
    got = {0: k.impute_torch(mask, want_residual=True)}
    for end in looks[1:]:
        rc, it, res = k.run_em(mask, inner_sweeps=1, maxiter=10, resprint=10)
        assert (rc, it) == (0, 10), (rc, it)
        got[end] = res
    for end in looks:
        print(f"  noisy data, iteration {end}: observed residual / |V_obs| engine {got[end] / nobs:.9g} "
              f"numpy {want[end] / nobs:.9g}", flush=True)
    for end in looks:
        assert abs(got[end] - want[end]) <= 1e-5 * nobs, (end, got[end], want[end], nobs)
    k.close()
    t.close()
    # (c)
    t, k = start(noisy, pp.F64)
    rc, it, res = k.run_em(mask, inner_sweeps=1, maxiter=iters, resprint=10, tol=got[10])
    print(f"  tol = the residual at iteration 10: stopped {rc} after {it} iterations", flush=True)
    assert rc == 1 and it < iters and res <= got[10], (rc, it, res, got[10])
    k.close()
    t.close()
    ctx.close()


def stream_order():
    """an impute on a side torch stream right after the kernel that writes the mask there, no host
    synchronisation; the mask is overwritten on that stream right after the call"""
    ctx = pp.Context(0)
    shape, ranks = (64, 256, 1024), (20, 3, 3)   # 64 MB of fp32
    t = pp.Tensor(ctx, list(shape), pp.F32).fill_uniform(3)
    k = given_session(ctx, t, ranks, 1)
    V0 = t.to_torch()
    ref = k.model_to_torch(torch.float64)
    mask = torch.ones(shape, dtype=torch.bool, device=DEV)   # stale contents: everything observed
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        busy = torch.rand((4096, 4096), device=DEV)
        for _ in range(8):
            busy = busy @ busy / 4096.0   # keep the stream busy ahead of the mask's kernel
        real = torch.rand(shape, device=DEV) >= MISSING
        mask.copy_(real)
        assert k.impute_torch(mask) is None
        mask.fill_(True)                  # must not reach the impute's reads
        out = torch.empty_like(V0)
        t.export_torch(out)
        kept = (out == V0) | ~real
        # (one fp32 rounding of the value; 1e-12: the two fp64 sums, which add their terms in other orders)
        near = ((out.double() - ref).abs() <= ref.abs() * 2.0 ** -23 + 1e-12) | real
        moved = (out != V0).sum()
    torch.cuda.synchronize()
    assert bool(kept.all()) and bool(near.all()), (int((~kept).sum()), int((~near).sum()))
    assert int(moved) > 0.25 * V0.numel(), int(moved)
    k.close()
    t.close()
    ctx.close()


def refusals():
    """a host pointer, a span leaving its allocation, a negative stride, a box outside the tensor and
    inner_sweeps = 0: PPALS_ERR_ARG with the entry point's name in front, before anything is launched; a
    mask of another dtype never reaches the library (its ABI takes bytes): the binding raises TypeError.
    The tensor is unchanged"""
    ctx = pp.Context(0)
    lens, ranks = [20, 12, 9], (3, 2, 4)
    t = pp.Tensor(ctx, lens, pp.F32).fill_uniform(1)
    k = given_session(ctx, t, ranks, 1)
    V0 = t.download()
    fstr = [1, 20, 240]
    mask = torch.zeros(lens, dtype=torch.bool, device=DEV)       # all missing: any launch would show
    host_mask = torch.zeros(lens, dtype=torch.bool)
    bad = [("host", dict(ptr=host_mask.data_ptr(), shape=lens, strides=fstr)),
           ("span", dict(ptr=mask.data_ptr(), shape=lens, strides=[1, 20, 240 * 10 ** 6])),
           ("negative_stride", dict(ptr=mask.data_ptr(), shape=lens, strides=[1, -20, 240])),
           ("box", dict(ptr=mask.data_ptr(), shape=[10, 12, 9], strides=fstr, lo=[15, 0, 0])),
           ("null", dict(ptr=0, shape=lens, strides=fstr))]
    for name, kw in bad:
        for want_residual in (False, True):
            try:
                k.impute_device(want_residual=want_residual, **kw)
                raise AssertionError(f"{name} accepted")
            except pp.PpalsError as e:
                assert "ppals error -3: ppals_tucker_impute_device: " in str(e), (name, str(e))
    for call in (lambda: k.impute_torch(torch.zeros(lens, device=DEV)),
                 lambda: k.run_em(torch.zeros(lens, dtype=torch.int16, device=DEV), maxiter=2)):
        try:
            call()
            raise AssertionError("a mask that is neither bool nor uint8 was accepted")
        except TypeError as e:
            assert "torch.bool or torch.uint8" in str(e), str(e)
    for name, call in (("inner_sweeps", lambda: k.run_em(mask, inner_sweeps=0, maxiter=2)),
                       ("em_box", lambda: k.run_em(mask[:10], lo=[15, 0, 0], maxiter=2))):
        try:
            call()
            raise AssertionError(f"{name} accepted")
        except pp.PpalsError as e:
            assert "ppals error -3: ppals_tucker_em: " in str(e), (name, str(e))
    torch.cuda.synchronize()
    assert np.array_equal(t.download(), V0)
    k.close()
    t.close()
    ctx.close()


def shards():
    """P = 2 ranks on the one GPU (hipsim library): each rank rewrites only its own rows, and observed_sq is
    the global sum on both ranks"""
    import hipsim_util
    hp = hipsim_util.load(make=False)
    lens, P = [45, 12, 10, 9], 2
    g = torch.Generator(device="cpu").manual_seed(7)
    Xh = torch.rand(lens, generator=g, dtype=torch.float64)
    X = Xh.to(DEV)
    mask = (torch.rand(lens, generator=g) >= MISSING).to(DEV)
    torch.cuda.synchronize()
    Vs, obs = Xh.numpy(), mask.cpu().numpy()
    for ranks in ((20, 3, 3, 2),):   # (r_0 > 16: the kernel with Q in LDS, at a row offset on rank 1)
        w = hipsim_util.ThreadWorld(P, timeout=300)
        errors, outs = [], {}

        def rank_main(rank):
            try:
                ctx = hp.Context(0)
                uid, keep = w.comm_uid(rank)
                ctx.init_comm(rank, P, uid)
                t = hp.Tensor(ctx, lens, hp.F64).import_torch(X, stream=0)
                lo, n = t.local_rows()
                k = given_session(ctx, t, ranks, 20, mod=hp)
                Wc = k.get_factors()
                before = t.download()
                res = k.impute_torch(mask, stream=0, want_residual=True)
                outs[rank] = {"rows": (lo, n), "W": Wc, "before": before, "after": t.download(), "res": res}
                w.barrier()
                k.close()
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
        W, core = outs[0]["W"]
        M, absM = tucker_model(W, core), tucker_model(W, core, True)
        want_sq = float(np.sum(((Vs - M) ** 2)[obs]))
        union = np.zeros(lens)
        for rank in range(P):
            lo, n = outs[rank]["rows"]
            a, b = outs[rank]["after"], outs[rank]["before"]
            assert np.array_equal(a[:lo], b[:lo]) and np.array_equal(a[lo + n:], b[lo + n:]), rank
            assert np.array_equal(b[lo:lo + n], Vs[lo:lo + n]), rank
            union[lo:lo + n] = a[lo:lo + n]
            sq = outs[rank]["res"] ** 2
            assert abs(sq - want_sq) <= 1e-10 * float(np.linalg.norm(Vs)) ** 2, (rank, sq, want_sq)
        assert outs[0]["res"] == outs[1]["res"]
        assert np.array_equal(union[obs], Vs[obs])
        check_values(union[~obs], M[~obs], absM[~obs], torch.float64, ("sharded", ranks))
        print(f"  ranks {ranks}: ok", flush=True)


CASES = {f.__name__: f for f in (values, slabs, reproducible, session_consistent, em_recovers, stream_order,
                                 refusals, shards)}

if __name__ == "__main__":
    if sys.argv[1] == "values":
        pp.preload_eigensolver()   # a swept mode above 64, before anything initialises the HIP runtime
    CASES[sys.argv[1]]()
    print(f"tucker impute case {sys.argv[1]}: ok", flush=True)
