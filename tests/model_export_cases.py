"""Cases of tests/test_gpu_model_export.py, one per process: `python model_export_cases.py <case>`.

ppals_cp_export_model_device / ppals_tucker_export_model_device (include/ppals.h) through the torch helpers
of the binding. torch is imported BEFORE the binding loads libppals (one HIP runtime for both), and the
eigensolver libraries are preloaded before anything initialises the HIP runtime (Tucker modes above 64).
The reference is numpy's fp64 model built from the factors get_factors returns. Exit status 0: passed."""
import os
import sys
import threading

import torch  # noqa: I001  (first: see above)
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "pairwise-perturbation_amd"))
import ppals as pp  # noqa: E402

DEV = torch.device("cuda:0")
LET = "abcdefgh"
CANARY = -7.25


def host(x):
    return x.detach().to("cpu", torch.float64).numpy()


def cp_model(W, absolute=False):
    """sum_r prod_i W_i[j_i, r] as an ndarray indexed like the tensor (and sum_r prod |W_i|)"""
    N = len(W)
    expr = ",".join(f"{LET[i]}z" for i in range(N)) + "->" + LET[:N]
    return np.einsum(expr, *[np.abs(w) if absolute else w for w in W], optimize=True)


def tucker_model(W, core, absolute=False):
    out = np.abs(core) if absolute else core
    for i, w in enumerate(W):
        out = np.moveaxis(np.tensordot(np.abs(w) if absolute else w, out, axes=([1], [i])), 0, i)
    return out


def check_values(got, want, scale, tdt, what):
    """F64: elementwise within 1e-13 of the terms' magnitude; F32: >= 99.9 % the fp64 value rounded once,
    every element within one fp32 step of it"""
    if tdt == torch.float64:
        err = np.abs(got - want)
        assert (err <= 1e-13 * scale + 1e-300).all(), (what, float((err / (scale + 1e-300)).max()))
    else:
        w32 = want.astype(np.float32)
        same = np.mean(got.astype(np.float32) == w32)
        step = np.spacing(np.abs(w32)).astype(np.float64)
        err = np.abs(got - want)
        assert same >= 0.999, (what, same)
        assert (err <= step + 1e-13 * scale).all(), (what, float((err / step).max()))


def views(shape, tdt):
    """(name, destination view, parent whose other elements must stay untouched or None, box lo or None)"""
    N = len(shape)
    out = []
    fstr = [int(np.prod(shape[:i])) for i in range(N)]
    out.append(("dense_first_fastest", torch.empty_strided(shape, fstr, dtype=tdt, device=DEV), None, None))
    out.append(("c_contiguous", torch.empty(shape, dtype=tdt, device=DEV), None, None))
    perm = list(range(N))[1:] + [0]
    inv = [perm.index(i) for i in range(N)]
    out.append(("permuted", torch.empty([shape[p] for p in perm], dtype=tdt, device=DEV).permute(inv), None,
                None))
    # a box at lo != 0 inside a larger canary tensor
    lo = [min(1, s - 1) for s in shape]
    box = [s - l for s, l in zip(shape, lo)]
    parent = torch.full([b + 3 for b in box], CANARY, dtype=tdt, device=DEV)
    out.append(("box_at_lo", parent[tuple(slice(2, 2 + b) for b in box)], parent, lo))
    # padded (non-contiguous) strides, first index fastest
    parent = torch.full([s + 2 for s in reversed(shape)], CANARY, dtype=tdt, device=DEV)
    v = parent[tuple(slice(0, s) for s in reversed(shape))].permute(*reversed(range(N)))
    out.append(("padded", v, parent, None))
    # no unit-stride mode: C order with the last mode stepped by 2
    parent = torch.full(list(shape[:-1]) + [2 * shape[-1]], CANARY, dtype=tdt, device=DEV)
    out.append(("no_unit_stride", parent[..., ::2], parent, None))
    return out


def check_export(sess, M, absM, Vs, residual_norm, shape, label):
    """every view x F32 / F64 x model / residual of one session against the numpy model M"""
    for tdt in (torch.float32, torch.float64):
        for residual in (False, True):
            want_full = (Vs - M) if residual else M
            scale_full = absM + (np.abs(Vs) if residual else 0.0)
            for name, v, parent, lo in views(shape, tdt):
                before = host(parent) if parent is not None else None
                sess.export_model_torch(v, residual=residual, lo=lo)
                torch.cuda.synchronize()
                sl = tuple(slice(l, None) for l in lo) if lo else tuple(slice(None) for _ in shape)
                what = (label, name, str(tdt), "residual" if residual else "model")
                check_values(host(v), want_full[sl], scale_full[sl], tdt, what)
                if parent is not None:  # everything outside the view is untouched
                    after = host(parent)
                    probe = torch.zeros(parent.shape, dtype=torch.bool, device=DEV)
                    probe.as_strided(v.shape, v.stride(), v.storage_offset()).fill_(True)
                    mask = ~probe.cpu().numpy()
                    assert np.array_equal(after[mask], before[mask]), what
                if residual and name == "c_contiguous" and tdt == torch.float64:
                    n = float(v.norm())
                    assert abs(n - residual_norm) <= 1e-10 * residual_norm, (label, n, residual_norm)


def cp_values():
    """orders 3, 4, 5; R in {1, 3, 10, 33, 70}; F32 / F64 / BF16 storage; every view kind"""
    ctx = pp.Context(0)
    shapes = {3: (23, 17, 30), 4: (9, 13, 7, 11), 5: (5, 6, 4, 7, 3)}
    k = 0
    for order, shape in shapes.items():
        for R in (1, 3, 10, 33, 70):
            dt = (pp.F32, pp.F64, pp.BF16)[k % 3]
            k += 1
            t = pp.Tensor(ctx, list(shape), dt).fill_uniform(100 + k, lo=0.5, hi=1.5)
            s = pp.CP(ctx, t, R)
            s.set_factors(pp.init_factors(shape, R, 10 * k), pp.init_factors(shape, R, 10 * k + 1))
            s.sweeps_dt(2)
            W = s.get_factors()
            M, absM = cp_model(W), cp_model(W, True)
            check_export(s, M, absM, t.download(), s.residual(), shape, ("cp", order, R, dt))
            print(f"  cp order {order} R {R} storage {dt}: ok", flush=True)
            s.close()
            t.close()
    # a larger box: several 64 x 64 tiles along both sides, 16-byte stores
    shape, R = (36, 40, 20, 24), 10
    for dt in (pp.F32, pp.BF16):
        t = pp.Tensor(ctx, list(shape), dt).fill_uniform(7, lo=0.5, hi=1.5)
        s = pp.CP(ctx, t, R)
        s.set_factors(pp.init_factors(shape, R, 1), pp.init_factors(shape, R, 2))
        s.sweeps_dt(1)
        W = s.get_factors()
        check_export(s, cp_model(W), cp_model(W, True), t.download(), s.residual(), shape, ("cp-large", dt))
        s.close()
        t.close()
    ctx.close()


def _tucker_session(ctx, lens, ranks, dt, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    # a low multilinear rank tensor plus noise: a fit worth exporting
    core = torch.randn(ranks, generator=g, dtype=torch.float64)
    X = core
    for i, (s, r) in enumerate(zip(lens, ranks)):
        U = torch.randn((s, r), generator=g, dtype=torch.float64)
        X = torch.movedim(torch.tensordot(U, X, dims=([1], [i])), 0, i)
    X = X + 0.05 * X.std() * torch.randn(lens, generator=g, dtype=torch.float64)
    t = pp.Tensor.from_torch(ctx, X.to(DEV), dtype=dt)
    k = pp.Tucker(ctx, t, ranks)
    k.hosvd()
    k.sweeps_dt(2)
    return t, k


def tucker_values():
    """orders 3 (the multi-sweep schedule) and 4, a mode above 64 rows; F32 / F64 storage"""
    ctx = pp.Context(0)
    for lens, ranks in (((70, 12, 9), (4, 3, 5)), ((8, 66, 7, 5), (3, 4, 2, 3))):
        for dt in (pp.F32, pp.F64):
            t, k = _tucker_session(ctx, list(lens), list(ranks), dt, 3)
            W, core = k.get_factors()
            M, absM = tucker_model(W, core), tucker_model(W, core, True)
            Vs = t.download()
            check_export(k, M, absM, Vs, np.linalg.norm(Vs - M), lens, ("tucker", lens, dt))
            res = k.model_to_torch(torch.float64, residual=True)
            lhs = float(res.norm()) ** 2
            rhs = float(np.linalg.norm(Vs)) ** 2 - float(np.linalg.norm(core)) ** 2
            # (fp32 storage: the sweeps' intermediates are held in fp32 — tucker.h, ms3_ — so the
            # core is V x_i W_i^T to ~1e-7 only, and the identity holds to that)
            tol = 1e-10 if dt == pp.F64 else 1e-6
            assert abs(lhs - rhs) <= tol * float(np.linalg.norm(Vs)) ** 2, (lens, dt, lhs, rhs)
            print(f"  tucker {lens} storage {dt}: ok", flush=True)
            k.close()
            t.close()
    ctx.close()


def tucker_deferred():
    """Exports among sweeps whose eigen-steps are checked deferred, with PPALS_EIG_DEFER_FAIL forcing some
    of those checks to fail (the failing step rolled back and repeated). Every sweep entry of the ABI
    settles its checks before it returns, so what an export must get right is the rest of the path of
    get_factors: the pending rotations of the lazy eigenvectors. Two identical sessions on two contexts
    (each has its own failure counter): A exports, B calls get_factors at the same points. Each export
    equals the model of B's factors, and after all sweeps both sessions' factors are bit-identical (an
    export that skipped the rotations would leave A's later sweeps on other bases). The s x s route of the
    eigen-step is the one with deferred checks (PPALS_TUCKER_THIN=0); its step log (PPALS_EIG_DEBUG=1,
    stderr) must show deferred checks and forced failures."""
    assert os.environ.get("PPALS_EIG_DEFER_FAIL") and os.environ.get("PPALS_TUCKER_THIN") == "0"
    assert os.environ.get("PPALS_EIG_DEBUG") == "1"
    import tempfile
    log = tempfile.TemporaryFile()
    saved = os.dup(2)
    os.dup2(log.fileno(), 2)   # the library's step log goes to fd 2
    try:
        lens, ranks = [96, 80, 72], [5, 6, 4]
        ca, cb = pp.Context(0), pp.Context(0)
        ta, ka = _tucker_session(ca, lens, ranks, pp.F64, 5)
        tb, kb = _tucker_session(cb, lens, ranks, pp.F64, 5)
        for _ in range(6):
            ka.sweeps_dt(2)
            kb.sweeps_dt(2)
            out = ka.model_to_torch(torch.float64)
            torch.cuda.synchronize()
            W, core = kb.get_factors()
            check_values(host(out), tucker_model(W, core), tucker_model(W, core, True), torch.float64,
                         "deferred")
        ka.sweeps_dt(2)
        kb.sweeps_dt(2)
        (Wa, ga), (Wb, gb) = ka.get_factors(), kb.get_factors()
        for x, y in zip(Wa + [ga], Wb + [gb]):
            assert np.array_equal(x, y), "an export changed the session's later sweeps"
        for x in (ka, kb, ta, tb, ca, cb):
            x.close()
    finally:
        os.dup2(saved, 2)
        os.close(saved)
    log.seek(0)
    full = log.read().decode(errors="replace")
    nfail = full.count("NOT accepted (deferred check)")
    ndef = full.count("accepted (deferred check)") - nfail
    print(f"  deferred checks: {ndef} accepted, {nfail} forced failures", flush=True)
    assert ndef >= 4 and nfail >= 2, full[-3000:]


def residual_forms():
    """both forms of the residual (PPALS_MODEL_RESIDUAL, read at session creation): fused, and the tensor
    export followed by view -= model; every storage type, every view kind, F32 / F64 destinations"""
    ctx = pp.Context(0)
    for form in ("fused", "two_pass"):
        os.environ["PPALS_MODEL_RESIDUAL"] = form
        shape, R = (9, 13, 7, 11), 10
        for dt in (pp.F32, pp.F64, pp.BF16):
            t = pp.Tensor(ctx, list(shape), dt).fill_uniform(21, lo=0.5, hi=1.5)
            s = pp.CP(ctx, t, R)
            s.set_factors(pp.init_factors(shape, R, 3), pp.init_factors(shape, R, 4))
            s.sweeps_dt(1)
            W = s.get_factors()
            check_export(s, cp_model(W), cp_model(W, True), t.download(), s.residual(), shape,
                         ("cp", form, dt))
            s.close()
            t.close()
        lens, ranks = (20, 18, 16), (4, 3, 5)
        for dt in (pp.F32, pp.F64):
            t, k = _tucker_session(ctx, list(lens), list(ranks), dt, 4)
            W, core = k.get_factors()
            M, Vs = tucker_model(W, core), t.download()
            check_export(k, M, tucker_model(W, core, True), Vs, np.linalg.norm(Vs - M), lens,
                         ("tucker", form, dt))
            k.close()
            t.close()
        print(f"  residual form {form}: ok", flush=True)
    os.environ.pop("PPALS_MODEL_RESIDUAL")
    ctx.close()


def untouched():
    """two sessions from the same inputs, one exporting a model and a residual between sweeps: the
    factors after three more sweeps are bit-identical (CP under both schedules; Tucker, whose control
    session reads its factors where the other exports — the same publication path)"""
    ctx = pp.Context(0)
    lens, R = [30, 26, 22, 18], 6
    for dt in (pp.F32, pp.BF16):
        for sched in ("dt", "msdt"):
            t = pp.Tensor(ctx, lens, dt).fill_uniform(11)
            got = []
            for export in (True, False):
                s = pp.CP(ctx, t, R)
                s.set_schedule(sched)
                s.set_factors(pp.init_factors(lens, R, 5), pp.init_factors(lens, R, 6))
                s.sweeps_dt(2)
                if export:
                    s.model_to_torch()
                    s.model_to_torch(torch.float64, residual=True)
                s.sweeps_dt(3)
                got.append(s.get_factors())
                s.close()
            for a, b in zip(*got):
                assert np.array_equal(a, b), ("cp", dt, sched)
            t.close()
    for lens, ranks in (([20, 18, 16], [4, 3, 5]), ([12, 10, 9, 8], [3, 2, 3, 2])):
        got = []
        for export in (True, False):
            t, k = _tucker_session(ctx, lens, ranks, pp.F64, 9)
            if export:
                k.model_to_torch()
                k.model_to_torch(torch.float64, residual=True)
            else:
                k.get_factors()
            k.sweeps_dt(3)
            W, core = k.get_factors()
            got.append(W + [core])
            k.close()
            t.close()
        for a, b in zip(*got):
            assert np.array_equal(a, b), ("tucker", lens)
    ctx.close()


def stream_order():
    """an export on a side torch stream, no host synchronisation, consumed on that stream"""
    ctx = pp.Context(0)
    shape, R = (64, 256, 1024), 4   # 64 MB of fp32
    t = pp.Tensor(ctx, list(shape), pp.F32).fill_uniform(3)
    s = pp.CP(ctx, t, R)
    s.set_factors(pp.init_factors(shape, R, 1), pp.init_factors(shape, R, 2))
    ref = s.model_to_torch(torch.float64)
    rref = s.model_to_torch(torch.float64, residual=True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        busy = torch.rand((4096, 4096), device=DEV)
        for _ in range(8):
            busy = busy @ busy / 4096.0   # keep the stream busy ahead of the export
        out = torch.full(shape, float("nan"), dtype=torch.float64, device=DEV)
        s.export_model_torch(out)
        d1 = (out - ref).abs().max()
        out.fill_(float("nan"))
        s.export_model_torch(out, residual=True)
        d2 = (out - rref).abs().max()
    torch.cuda.synchronize()
    assert float(d1) == 0.0 and float(d2) == 0.0, (float(d1), float(d2))
    s.close()
    t.close()
    ctx.close()


def refusals():
    """F16 / BF16 destinations, an overlapping view, host memory, a box outside the tensor and a bad
    `what` are refused with PPALS_ERR_ARG and a message before anything is launched: a canary is unchanged"""
    ctx = pp.Context(0)
    lens, R = [20, 12, 9], 3
    t = pp.Tensor(ctx, lens, pp.F32).fill_uniform(1)
    cp = pp.CP(ctx, t, R)
    cp.set_factors(pp.init_factors(lens, R, 1), pp.init_factors(lens, R, 2))
    tk = pp.Tucker(ctx, t, [2, 2, 2])
    tk.hosvd()
    canary = torch.full(lens, CANARY, device=DEV)
    fstr = [1, 20, 240]
    host_buf = torch.full(lens, CANARY)
    bad = [("f16", dict(ptr=canary.data_ptr(), dtype=pp.F16, shape=lens, strides=fstr)),
           ("bf16", dict(ptr=canary.data_ptr(), dtype=pp.BF16, shape=lens, strides=fstr)),
           ("overlap", dict(ptr=canary.data_ptr(), dtype=pp.F32, shape=lens, strides=[1, 0, 20])),
           ("host", dict(ptr=host_buf.data_ptr(), dtype=pp.F32, shape=lens, strides=fstr)),
           ("box", dict(ptr=canary.data_ptr(), dtype=pp.F32, shape=[10, 12, 9], strides=fstr, lo=[15, 0, 0]))]
    for sess in (cp, tk):
        for name, kw in bad:
            for residual in (False, True):
                try:
                    sess.export_model_device(residual=residual, **kw)
                    raise AssertionError(f"{name} accepted")
                except pp.PpalsError as e:
                    assert "ppals error -3" in str(e) and "export_model_device: " in str(e), (name, str(e))
        rc = getattr(pp.lib(), sess._export_fn)(sess._h, 2, pp.C.c_void_p(canary.data_ptr()), pp.F32,
                                                None, None, None, None)
        assert rc == -3 and b"PPALS_MODEL" in pp.lib().ppals_last_error(), rc
    torch.cuda.synchronize()
    assert bool((canary == CANARY).all()) and bool((host_buf == CANARY).all())
    cp.close()
    tk.close()
    t.close()
    ctx.close()


def shards():
    """P = 2 ranks on the one GPU (hipsim library): each rank writes only its own rows; the union is the
    unsharded model and residual"""
    import hipsim_util
    hp = hipsim_util.load(make=False)
    lens, R, ranks, P = [29, 12, 10, 9], 4, [3, 3, 2, 2], 2
    g = torch.Generator(device="cpu").manual_seed(7)
    Xh = torch.rand(lens, generator=g, dtype=torch.float64)
    X = Xh.to(DEV)
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
            k = hp.Tucker(ctx, t, ranks)
            k.hosvd()
            k.sweeps_dt(1)
            res = {"rows": (lo, n), "cpW": s.get_factors(), "tk": k.get_factors()}
            for name, sess in (("cp", s), ("tucker", k)):
                for residual in (False, True):
                    out = torch.full(lens, CANARY, dtype=torch.float64, device=DEV)
                    sess.export_model_torch(out, residual=residual, stream=0)
                    torch.cuda.synchronize()
                    res[(name, residual)] = host(out)
            outs[rank] = res
            w.barrier()
            s.close()
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
    Vs = Xh.numpy()
    for name in ("cp", "tucker"):
        if name == "cp":
            M, absM = cp_model(outs[0]["cpW"]), cp_model(outs[0]["cpW"], True)
        else:
            W, core = outs[0]["tk"]
            M, absM = tucker_model(W, core), tucker_model(W, core, True)
        for residual in (False, True):
            union = np.full(lens, CANARY)
            for rank in range(P):
                lo, n = outs[rank]["rows"]
                got = outs[rank][(name, residual)]
                assert (got[:lo] == CANARY).all() and (got[lo + n:] == CANARY).all(), (name, rank)
                union[lo:lo + n] = got[lo:lo + n]
            want = Vs - M if residual else M
            check_values(union, want, absM + (np.abs(Vs) if residual else 0), torch.float64,
                         (name, residual, "sharded"))


def quick():
    """one CP and one Tucker export against numpy (the smallest end-to-end check)"""
    ctx = pp.Context(0)
    lens, R = [12, 10, 8], 3
    t = pp.Tensor(ctx, lens, pp.F64).fill_uniform(2)
    s = pp.CP(ctx, t, R)
    s.set_factors(pp.init_factors(lens, R, 1), pp.init_factors(lens, R, 2))
    W = s.get_factors()
    check_values(host(s.model_to_torch(torch.float64)), cp_model(W), cp_model(W, True), torch.float64, "cp")
    s.close()
    t.close()
    ctx.close()


CASES = {f.__name__: f for f in (cp_values, tucker_values, tucker_deferred, residual_forms, untouched,
                                 stream_order, refusals, shards, quick)}

if __name__ == "__main__":
    if sys.argv[1] in ("tucker_deferred", "tucker_values"):
        pp.preload_eigensolver()   # modes above 64, before anything initialises the HIP runtime
    CASES[sys.argv[1]]()
    print(f"model_export case {sys.argv[1]}: ok", flush=True)
