"""Cases of tests/test_gpu_impute.py, one per process: `python impute_cases.py <case>`.

ppals_cp_impute_device / ppals_cp_em (include/ppals.h) through the torch helpers of the binding. torch is
imported BEFORE the binding loads libppals (one HIP runtime for both). The reference is numpy's fp64 model
built from the factors get_factors returns, and the tensor downloaded before the call. Exit status 0: passed."""
import os
import sys
import threading

import torch  # noqa: I001  (first: see above)
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "pairwise-perturbation_amd"))
import ppals as pp  # noqa: E402
from model_export_cases import DEV, check_values, cp_model  # noqa: E402

MISSING = 0.3


def bf16_round(x):
    """fp64 -> bf16 as the engine stores it (and torch rounds): through fp32, each step to nearest even"""
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.float32).to(torch.bfloat16).to(torch.float64).numpy()


def check_imputed(got, want, scale, dt, what):
    """check_values of model_export_cases.py for F64 / F32 storage; BF16: the same rule with the bf16 step"""
    if got.size == 0:   # nothing missing
        return
    if dt != pp.BF16:
        check_values(got, want, scale, torch.float64 if dt == pp.F64 else torch.float32, what)
        return
    wb = bf16_round(want)
    same = np.mean(got == wb)
    step = np.ldexp(1.0, np.frexp(np.abs(wb))[1] - 8)   # |x| in [2^(e-1), 2^e): 8 significant bits
    err = np.abs(got - want)
    assert same >= 0.999, (what, same)
    assert (err <= step + 1e-13 * scale).all(), (what, float((err / step).max()))


def masks(shape, seed):
    """(name, mask view on the device, box lo or None): False / 0 = missing"""
    N = len(shape)
    g = torch.Generator(device="cpu").manual_seed(seed)
    base = (torch.rand(shape, generator=g) >= MISSING).to(DEV)
    out = [("c_contiguous", base, None)]
    fstr = [int(np.prod(shape[:i])) for i in range(N)]
    m = torch.empty_strided(shape, fstr, dtype=torch.bool, device=DEV)
    m.copy_(base)
    out.append(("first_index_fastest", m, None))
    perm = list(range(N))[1:] + [0]
    inv = [perm.index(i) for i in range(N)]
    m = torch.empty([shape[p] for p in perm], dtype=torch.bool, device=DEV).permute(inv)
    m.copy_(base)
    out.append(("permuted", m, None))
    vals = torch.where(torch.rand(shape, generator=g) < 0.5, 1, 255).to(torch.uint8).to(DEV)
    out.append(("uint8_0_1_255", torch.where(base, vals, torch.zeros_like(vals)), None))
    lo = [min(1, s - 1) for s in shape]
    box = [s - l for s, l in zip(shape, lo)]
    parent = (torch.rand([b + 3 for b in box], generator=g) >= MISSING).to(DEV)
    out.append(("box_at_lo", parent[tuple(slice(2, 2 + b) for b in box)], lo))
    sl = (torch.rand(shape[:-1], generator=g) >= MISSING).to(DEV)
    out.append(("broadcast_last_mode", sl.unsqueeze(-1).expand(*shape), None))
    out.append(("all_observed", torch.ones(shape, dtype=torch.bool, device=DEV), None))
    out.append(("all_missing", torch.zeros(shape, dtype=torch.bool, device=DEV), None))
    return out


def check_impute(t, s, shape, dt, label):
    """every mask kind, without and with the observed residual, from the same tensor contents"""
    V0 = t.download()
    W = s.get_factors()
    M, absM = cp_model(W), cp_model(W, True)
    nv2 = float(np.linalg.norm(V0)) ** 2
    for name, mask, lo in masks(shape, 17):
        sl = tuple(slice(l, None) for l in lo) if lo else tuple(slice(None) for _ in shape)
        obs = np.zeros(shape, dtype=bool)
        obs[...] = True                      # outside the box: untouched
        obs[sl] = mask.cpu().numpy() != 0
        want_sq = float(np.sum(((V0 - M) ** 2)[sl][obs[sl]]))
        for want_residual in (False, True):
            what = (label, name, want_residual)
            t.upload(V0)
            res = s.impute_torch(mask, lo=lo, want_residual=want_residual)
            got = t.download()
            assert np.array_equal(got[obs], V0[obs]), what   # bit for bit: all three types widen exactly
            check_imputed(got[~obs], M[~obs], absM[~obs], dt, what)
            if want_residual:
                tol = 1e-10 if dt == pp.F64 else 1e-6
                print(f"    {what}: observed_sq {res * res:.17g} numpy {want_sq:.17g} "
                      f"diff/|V|^2 {abs(res * res - want_sq) / nv2:.3g}", flush=True)
                assert abs(res * res - want_sq) <= tol * nv2, (what, res * res, want_sq, nv2)
            else:
                assert res is None
    t.upload(V0)


def values():
    """orders 3, 4, 5 and a box of several tiles per side; R in {1, 3, 10, 33, 70} cycled over F32 / F64 /
    BF16 storage as the model export's cp_values; factors from two sweeps; every mask kind"""
    ctx = pp.Context(0)
    shapes = [(23, 17, 30), (9, 13, 7, 11), (5, 6, 4, 7, 3), (36, 40, 20, 24)]
    k = 0
    for shape in shapes:
        for R in (1, 3, 10, 33, 70):
            dt = (pp.F32, pp.F64, pp.BF16)[k % 3]
            k += 1
            t = pp.Tensor(ctx, list(shape), dt).fill_uniform(100 + k, lo=0.5, hi=1.5)
            s = pp.CP(ctx, t, R)
            s.set_factors(pp.init_factors(shape, R, 10 * k), pp.init_factors(shape, R, 10 * k + 1))
            s.sweeps_dt(2)
            check_impute(t, s, shape, dt, (shape, R, dt))
            print(f"  shape {shape} R {R} storage {dt}: ok", flush=True)
            s.close()
            t.close()
    ctx.close()


def reproducible():
    """the same impute with the residual twice from the same state: the same bits, tensor and sum"""
    ctx = pp.Context(0)
    shape, R = (36, 40, 20, 24), 10
    for dt in (pp.F32, pp.F64, pp.BF16):
        t = pp.Tensor(ctx, list(shape), dt).fill_uniform(7, lo=0.5, hi=1.5)
        s = pp.CP(ctx, t, R)
        s.set_factors(pp.init_factors(shape, R, 1), pp.init_factors(shape, R, 2))
        s.sweeps_dt(2)
        V0 = t.download()
        for name, mask, lo in masks(shape, 5)[:3]:
            runs = []
            for _ in range(2):
                t.upload(V0)
                res = s.impute_torch(mask, lo=lo, want_residual=True)
                runs.append((np.float64(res).tobytes(), t.download().tobytes()))
            assert runs[0][0] == runs[1][0], (dt, name, "observed_sq")
            assert runs[0][1] == runs[1][1], (dt, name, "tensor")
        s.close()
        t.close()
    ctx.close()


def session_consistent():
    """after an impute the session sweeps on the new contents: two sweeps agree to 1e-10 (F64 storage, both
    schedules) with a fresh session on a copy of the imputed tensor from the same factors; so does a second
    session that existed on the tensor (its layouts and caches built) before the impute"""
    ctx = pp.Context(0)
    shape, R = [20, 18, 16, 14], 4
    mask = masks(shape, 3)[0][1]

    def relerr(a, b):
        return max(np.linalg.norm(x - y) / np.linalg.norm(y) for x, y in zip(a, b))

    for sched in ("dt", "msdt"):
        t = pp.Tensor(ctx, shape, pp.F64).fill_uniform(11, lo=0.5, hi=1.5)
        s, other = pp.CP(ctx, t, R), pp.CP(ctx, t, R)
        for x in (s, other):
            x.set_schedule(sched)
            x.set_factors(pp.init_factors(shape, R, 5), pp.init_factors(shape, R, 6))
            x.sweeps_dt(2)
        V0 = t.download()
        s.impute_torch(mask)
        W, G = s.get_factors(with_grad=True)
        imputed = t.download()
        assert np.mean(imputed != V0) > 0.2
        s.sweeps_dt(2)
        other.set_factors(W, G)
        other.sweeps_dt(2)
        t2 = pp.Tensor(ctx, shape, pp.F64).upload(imputed)
        fresh = pp.CP(ctx, t2, R)
        fresh.set_schedule(sched)
        fresh.set_factors(W, G)
        fresh.sweeps_dt(2)
        Wf = fresh.get_factors()
        e1, e2 = relerr(s.get_factors(), Wf), relerr(other.get_factors(), Wf)
        print(f"  schedule {sched}: imputing session {e1:.3g}, other session {e2:.3g}", flush=True)
        assert e1 <= 1e-10 and e2 <= 1e-10, (sched, e1, e2)
        # (a session that kept its old second layout or caches would be off by O(1): the stale values)
        for x in (s, other, fresh, t, t2):
            x.close()
    ctx.close()


def em_recovers():
    """EM recovers an exact rank-3 tensor from 70 % of its entries.

    (12, 10, 9, 8), R = 3, V = [[W_true]], 30 % missing at random and zeroed, start from another seed,
    inner_sweeps = 1. After 150 iterations the relative error on the MISSING entries is <= 1e-4 (F64 and F32
    storage; a numpy fp64 EM-ALS reaches ~1e-7 there, and without imputation the zeros stay: O(1)). The
    observed residual at a look (every 10 iterations) never exceeds the one at the look before by more than
    1e-9 of that one. run_em with tol = the residual reached at iteration 100 stops there and returns 1.
    BF16 storage: the loop runs and the missing-entry error falls below its starting value (1: zeros)."""
    ctx = pp.Context(0)
    shape, R = [12, 10, 9, 8], 3
    Vt = cp_model(pp.init_factors(shape, R, 40))
    g = torch.Generator(device="cpu").manual_seed(9)
    mask = (torch.rand(shape, generator=g) >= MISSING).to(DEV)
    obs = mask.cpu().numpy()
    W0, G0 = pp.init_factors(shape, R, 50), pp.init_factors(shape, R, 51)
    nobs = float(np.linalg.norm(Vt[obs]))

    def miss_err(t):
        return float(np.linalg.norm(t.download()[~obs] - Vt[~obs]) / np.linalg.norm(Vt[~obs]))

    for dt in (pp.F64, pp.F32, pp.BF16):
        t = pp.Tensor(ctx, shape, dt).upload(Vt * obs)
        s = pp.CP(ctx, t, R)
        s.set_factors(W0, G0)
        start = miss_err(t)
        looks = []
        for _ in range(15):
            rc, it, res = s.run_em(mask, inner_sweeps=1, maxiter=10, resprint=10)
            assert (rc, it) == (0, 10), (dt, rc, it)
            looks.append(res)
        err = miss_err(t)
        print(f"  storage {dt}: missing-entry error {start:.3g} -> {err:.3g} after 150 iterations; "
              f"observed residual / |V_obs| at the looks: {[f'{r / nobs:.3g}' for r in looks]}", flush=True)
        if dt == pp.BF16:
            assert err < start, (dt, start, err)
        else:
            rise = max((b - a) / a for a, b in zip(looks, looks[1:]))
            print(f"    largest relative rise between looks: {rise:.3g}", flush=True)
            assert err <= 1e-4, (dt, err)
            assert rise <= 1e-9, (dt, rise)
            s2 = pp.CP(ctx, t.upload(Vt * obs), R)
            s2.set_factors(W0, G0)
            rc, it, res = s2.run_em(mask, inner_sweeps=1, maxiter=150, resprint=10, tol=looks[9])
            print(f"    tol = the residual at iteration 100: stopped {rc} after {it} iterations", flush=True)
            assert rc == 1 and it < 150 and res <= looks[9], (dt, rc, it, res, looks[9])
            s2.close()
        s.close()
        t.close()
    ctx.close()


def stream_order():
    """an impute on a side torch stream right after the kernel that writes the mask there, no host
    synchronisation; the mask is overwritten on that stream right after the call"""
    ctx = pp.Context(0)
    shape, R = (64, 256, 1024), 4   # 64 MB of fp32
    t = pp.Tensor(ctx, list(shape), pp.F32).fill_uniform(3)
    s = pp.CP(ctx, t, R)
    s.set_factors(pp.init_factors(shape, R, 1), pp.init_factors(shape, R, 2))
    V0 = t.to_torch()
    ref = s.model_to_torch(torch.float64)
    mask = torch.ones(shape, dtype=torch.bool, device=DEV)   # stale contents: everything observed
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        busy = torch.rand((4096, 4096), device=DEV)
        for _ in range(8):
            busy = busy @ busy / 4096.0   # keep the stream busy ahead of the mask's kernel
        real = torch.rand(shape, device=DEV) >= MISSING
        mask.copy_(real)
        assert s.impute_torch(mask) is None
        mask.fill_(True)                  # must not reach the impute's reads
        out = torch.empty_like(V0)
        t.export_torch(out)
        kept = (out == V0) | ~real
        near = ((out.double() - ref).abs() <= ref.abs() * 2.0 ** -23) | real
        moved = (out != V0).sum()
    torch.cuda.synchronize()
    assert bool(kept.all()) and bool(near.all()), (int((~kept).sum()), int((~near).sum()))
    assert int(moved) > 0.25 * V0.numel(), int(moved)
    s.close()
    t.close()
    ctx.close()


def refusals():
    """a host pointer, a span leaving its allocation, a negative stride, a box outside the tensor and
    inner_sweeps = 0: PPALS_ERR_ARG with the entry point's name in front, before anything is launched; a
    mask of another dtype never reaches the library (its ABI takes bytes): the binding raises TypeError.
    The tensor is unchanged"""
    ctx = pp.Context(0)
    lens, R = [20, 12, 9], 3
    t = pp.Tensor(ctx, lens, pp.F32).fill_uniform(1)
    s = pp.CP(ctx, t, R)
    s.set_factors(pp.init_factors(lens, R, 1), pp.init_factors(lens, R, 2))
    V0 = t.download()
    fstr = [1, 20, 240]
    mask = torch.zeros(lens, dtype=torch.bool, device=DEV)       # all missing: any launch would show
    host_mask = torch.zeros(lens, dtype=torch.bool)
    bad = [("host", dict(ptr=host_mask.data_ptr(), shape=lens, strides=fstr)),
           ("span", dict(ptr=mask.data_ptr(), shape=lens, strides=[1, 20, 240 * 10 ** 6])),
           ("negative_stride", dict(ptr=mask.data_ptr(), shape=lens, strides=[1, -20, 240])),
           ("box", dict(ptr=mask.data_ptr(), shape=[10, 12, 9], strides=fstr, lo=[15, 0, 0]))]
    for name, kw in bad:
        for want_residual in (False, True):
            try:
                s.impute_device(want_residual=want_residual, **kw)
                raise AssertionError(f"{name} accepted")
            except pp.PpalsError as e:
                assert "ppals error -3: ppals_cp_impute_device: " in str(e), (name, str(e))
    for call in (lambda: s.impute_torch(torch.zeros(lens, device=DEV)),
                 lambda: s.run_em(torch.zeros(lens, dtype=torch.int16, device=DEV), maxiter=2)):
        try:
            call()
            raise AssertionError("a mask that is neither bool nor uint8 was accepted")
        except TypeError as e:
            assert "torch.bool or torch.uint8" in str(e), str(e)
    for name, call in (("inner_sweeps", lambda: s.run_em(mask, inner_sweeps=0, maxiter=2)),
                       ("em_box", lambda: s.run_em(mask[:10], lo=[15, 0, 0], maxiter=2))):
        try:
            call()
            raise AssertionError(f"{name} accepted")
        except pp.PpalsError as e:
            assert "ppals error -3: ppals_cp_em: " in str(e), (name, str(e))
    torch.cuda.synchronize()
    assert np.array_equal(t.download(), V0)
    s.close()
    t.close()
    ctx.close()


def shards():
    """P = 2 ranks on the one GPU (hipsim library): each rank rewrites only its own rows, and observed_sq is
    the global sum on both ranks"""
    import hipsim_util
    hp = hipsim_util.load(make=False)
    lens, R, P = [29, 12, 10, 9], 4, 2
    g = torch.Generator(device="cpu").manual_seed(7)
    Xh = torch.rand(lens, generator=g, dtype=torch.float64)
    X = Xh.to(DEV)
    mask = (torch.rand(lens, generator=g) >= MISSING).to(DEV)
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
            res = s.impute_torch(mask, stream=0, want_residual=True)
            outs[rank] = {"rows": (lo, n), "W": W, "before": before, "after": t.download(), "res": res}
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
    Vs, obs = Xh.numpy(), mask.cpu().numpy()
    M, absM = cp_model(outs[0]["W"]), cp_model(outs[0]["W"], True)
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
    check_values(union[~obs], M[~obs], absM[~obs], torch.float64, "sharded")


def quick():
    """one impute with the residual against numpy (the smallest end-to-end check)"""
    ctx = pp.Context(0)
    shape, R = (12, 10, 8), 3
    t = pp.Tensor(ctx, list(shape), pp.F64).fill_uniform(2)
    s = pp.CP(ctx, t, R)
    s.set_factors(pp.init_factors(shape, R, 1), pp.init_factors(shape, R, 2))
    check_impute(t, s, shape, pp.F64, "quick")
    s.close()
    t.close()
    ctx.close()


CASES = {f.__name__: f for f in (values, reproducible, session_consistent, em_recovers, stream_order,
                                 refusals, shards, quick)}

if __name__ == "__main__":
    CASES[sys.argv[1]]()
    print(f"impute case {sys.argv[1]}: ok", flush=True)
