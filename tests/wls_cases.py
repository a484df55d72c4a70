"""Cases of tests/test_gpu_wls.py, one per process: `python wls_cases.py <case>`.

ppals_cp_wls_device / ppals_cp_wls (include/ppals.h) through the torch helpers of the binding. torch is
imported BEFORE the binding loads libppals (one HIP runtime for both). The reference is tests/wls_ref.py on
numpy's fp64 model built from the factors get_factors returns, and the tensor downloaded before the call.
Exit status 0: passed."""
import os
import sys
import threading

import torch  # noqa: I001  (first: see above)
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "pairwise-perturbation_amd"))
import ppals as pp  # noqa: E402
import wls_ref  # noqa: E402
from model_export_cases import DEV, check_values, cp_model, host  # noqa: E402

# (data kind, weights kind): every kind on either side, the same and mixed
PAIRS = (("c_contiguous", "c_contiguous"), ("first_index_fastest", "first_index_fastest"),
         ("permuted", "permuted"), ("box_at_lo", "box_at_lo"), ("c_contiguous", "broadcast_last_mode"),
         ("first_index_fastest", "vector"), ("c_contiguous", "first_index_fastest"),
         ("first_index_fastest", "c_contiguous"), ("permuted", "c_contiguous"), ("c_contiguous", "vector"))


def layout(base, kind):
    """a device tensor with the values of `base` (C-contiguous, on the device) in the layout `kind`"""
    shape, N = list(base.shape), base.dim()
    if kind == "c_contiguous":
        return base.clone()
    if kind == "first_index_fastest":
        out = torch.empty_strided(shape, [int(np.prod(shape[:i])) for i in range(N)], dtype=base.dtype, device=DEV)
    elif kind == "permuted":
        perm = list(range(N))[1:] + [0]
        inv = [perm.index(i) for i in range(N)]
        out = torch.empty([shape[p] for p in perm], dtype=base.dtype, device=DEV).permute(inv)
    elif kind == "box_at_lo":   # a view inside a larger parent
        parent = torch.full([s + 3 for s in shape], float("nan"), dtype=base.dtype, device=DEV)
        out = parent[tuple(slice(2, 2 + s) for s in shape)]
    else:
        raise KeyError(kind)
    out.copy_(base)
    return out


def random_weights(shape, g, tdt):
    """uniform in (0, 1) with 10 % exact zeros and 10 % exact ones (C-contiguous, on the host)"""
    h = torch.rand(shape, generator=g, dtype=torch.float64) * 0.98 + 0.01
    u = torch.rand(shape, generator=g)
    h[u < 0.1] = 0.0
    h[u > 0.9] = 1.0
    return h.to(tdt)


def view_pair(shape, dkind, wkind, tdt, seed):
    """(data view, weights view, box lo or None, box shape): the weights view is already expanded"""
    N = len(shape)
    g = torch.Generator(device="cpu").manual_seed(seed)
    lo = None
    box = list(shape)
    if "box_at_lo" in (dkind, wkind):
        lo = [min(1, s - 1) for s in shape]
        box = [s - l for s, l in zip(shape, lo)]
    x = (torch.rand(box, generator=g, dtype=torch.float64) + 0.5).to(tdt).to(DEV)
    data = layout(x, dkind)
    if wkind == "broadcast_last_mode":
        h = random_weights(box[:-1], g, tdt).to(DEV).unsqueeze(-1).expand(*box)
    elif wkind == "vector":
        mode = seed % N
        sh = [1] * N
        sh[mode] = box[mode]
        h = random_weights([box[mode]], g, tdt).to(DEV).reshape(sh).expand(*box)
    else:
        h = layout(random_weights(box, g, tdt).to(DEV), wkind)
    return data, h, lo, box


def check_step(t, s, V0, M, absM, shape, dt, data, h, lo, what):
    """one step with the loss from the contents V0: stored values, the h = 1 elements, outside the box, loss"""
    t.upload(V0)
    loss = s.wls_torch(data, h, lo=lo, want_loss=True)
    got = t.download()
    sl = tuple(slice(l, l + n) for l, n in zip(lo or [0] * len(shape), data.shape))
    xh, hh = host(data), host(h)
    z, want_loss = wls_ref.step(xh, hh, M[sl])
    check_values(got[sl], z, absM[sl] + np.abs(np.where(hh > 0, xh, 0.0)),
                 torch.float64 if dt == pp.F64 else torch.float32, what)
    one = hh >= 1
    stored = xh if dt == pp.F64 else xh.astype(np.float32).astype(np.float64)
    assert np.array_equal(got[sl][one], stored[one]), what
    outside = np.ones(shape, dtype=bool)
    outside[sl] = False
    assert np.array_equal(got[outside], V0[outside]), what
    scale = float(np.sum(np.where(hh > 0, np.minimum(hh, 1.0) * np.where(hh > 0, xh, 0.0) ** 2, 0.0)))
    print(f"    {what}: loss {loss:.17g} numpy {want_loss:.17g} diff / sum h x^2 "
          f"{abs(loss - want_loss) / scale:.3g}", flush=True)
    assert np.isfinite(loss) and abs(loss - want_loss) <= 1e-10 * scale, (what, loss, want_loss, scale)
    t.upload(V0)
    assert s.wls_torch(data, h, lo=lo) is None      # without the loss: the same bits
    assert np.array_equal(t.download(), got), what


SHAPES = [(23, 17, 30), (9, 13, 7, 11), (5, 6, 4, 7, 3), (36, 40, 20, 24)]


def values(which):
    """one of: orders 3, 4, 5 and a box of several tiles per side (`which` indexes SHAPES); R in {1, 3, 10, 33, 70,
    128} cycled, across the four shapes, over F32 / F64 storage and f32 / f64 views; factors from two sweeps;
    every pair of view kinds"""
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
            check_step(t, s, V0, M, absM, shape, dt, data, h, lo, (shape, R, dt, str(tdt), dkind, wkind))
        print(f"  shape {shape} R {R} storage {dt} views {tdt}: ok", flush=True)
        s.close()
        t.close()
    ctx.close()


def session(ctx, shape, R, dt, seed=1, sweeps=2):
    t = pp.Tensor(ctx, list(shape), dt).fill_uniform(7 + seed, lo=0.5, hi=1.5)
    s = pp.CP(ctx, t, R)
    s.set_factors(pp.init_factors(shape, R, seed), pp.init_factors(shape, R, seed + 1))
    if sweeps:
        s.sweeps_dt(sweeps)
    return t, s


def equals_impute():
    """weights in {0, 1}, data = the tensor's own contents with NaN where the weight is 0: the tensor's bytes
    after the step are those after impute_torch(mask) from the same state; the loss is observed_sq"""
    ctx = pp.Context(0)
    for shape in ((23, 17, 30), (36, 40, 20, 24)):
        for R in (3, 33):
            for dt, tdt in ((pp.F32, torch.float32), (pp.F64, torch.float64)):
                t, s = session(ctx, shape, R, dt)
                V0 = t.download()
                g = torch.Generator(device="cpu").manual_seed(R)
                mask = (torch.rand(shape, generator=g) >= 0.3).to(DEV)
                data = t.to_torch(tdt)
                data[~mask] = float("nan")
                loss = s.wls_torch(data, mask.to(tdt), want_loss=True)
                a = t.download()
                t.upload(V0)
                res = s.impute_torch(mask, want_residual=True)
                b = t.download()
                assert np.mean(a != V0) > 0.2
                assert a.tobytes() == b.tobytes(), (shape, R, dt, float(np.mean(a != b)))
                print(f"  shape {shape} R {R} storage {dt}: same bytes; loss {loss:.17g} observed_sq "
                      f"{res * res:.17g}", flush=True)
                assert abs(loss - res * res) <= 1e-12 * res * res, (shape, R, dt, loss, res * res)
                s.close()
                t.close()
    ctx.close()


def special_weights():
    """h of 2, -1, NaN and 1e-300 (f32 views: 1e-30) among ordinary weights, and data of +-Inf / NaN wherever h is off: stored
    values and loss are the reference's, and the loss is finite"""
    ctx = pp.Context(0)
    shape, R = (9, 13, 7, 11), 3
    for dt in (pp.F32, pp.F64):
        for tdt in (torch.float32, torch.float64):
            t, s = session(ctx, shape, R, dt)
            V0 = t.download()
            W = s.get_factors()
            M, absM = cp_model(W), cp_model(W, True)
            g = torch.Generator(device="cpu").manual_seed(4)
            h = random_weights(shape, g, torch.float64)
            u = torch.rand(shape, generator=g)
            for lo_, val in ((0.0, 2.0), (0.1, -1.0), (0.2, float("nan")), (0.3, 1e-300 if tdt == torch.float64
                                                                            else 1e-30)):
                h[(u >= lo_) & (u < lo_ + 0.1)] = val
            x = torch.rand(shape, generator=g, dtype=torch.float64) + 0.5
            off = ~(h > 0)
            v = torch.rand(shape, generator=g)
            x[off & (v < 0.3)] = float("inf")
            x[off & (v >= 0.3) & (v < 0.6)] = float("-inf")
            x[off & (v >= 0.6)] = float("nan")
            for kind in ("c_contiguous", "first_index_fastest"):
                check_step(t, s, V0, M, absM, shape, dt, layout(x.to(tdt).to(DEV), kind),
                           layout(h.to(tdt).to(DEV), kind), None, ("special", dt, str(tdt), kind))
            s.close()
            t.close()
    ctx.close()


def reproducible():
    """the same step with the loss twice from the same state: the same bits, tensor and loss"""
    ctx = pp.Context(0)
    shape, R = (36, 40, 20, 24), 10
    for dt, tdt in ((pp.F32, torch.float32), (pp.F64, torch.float64)):
        t, s = session(ctx, shape, R, dt)
        V0 = t.download()
        for i, (dkind, wkind) in enumerate(PAIRS[:3] + PAIRS[6:7]):
            data, h, lo, _ = view_pair(shape, dkind, wkind, tdt, i)
            runs = []
            for _ in range(2):
                t.upload(V0)
                loss = s.wls_torch(data, h, lo=lo, want_loss=True)
                runs.append((np.float64(loss).tobytes(), t.download().tobytes()))
            assert runs[0][0] == runs[1][0], (dt, dkind, wkind, "loss")
            assert runs[0][1] == runs[1][1], (dt, dkind, wkind, "tensor")
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

    for sched in ("dt", "msdt"):
        t = pp.Tensor(ctx, shape, pp.F64).fill_uniform(11, lo=0.5, hi=1.5)
        s, other = pp.CP(ctx, t, R), pp.CP(ctx, t, R)
        for x in (s, other):
            x.set_schedule(sched)
            x.set_factors(pp.init_factors(shape, R, 5), pp.init_factors(shape, R, 6))
            x.sweeps_dt(2)
        V0 = t.download()
        s.wls_torch(data, h)
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


def driver():
    """Weighted CP recovers a rank-3 tensor under heteroscedastic noise that plain ALS cannot fit through.

    (12, 10, 9, 8), R = 3, data = [[W_true]] (factors U(0, 1)) + noise of sigma = 1 on 30 % of the entries at
    random and sigma = 0.01 on the rest, h = weights_from_std(sigma), random start, inner_sweeps = 1. With the
    numpy reference (tests/wls_ref.py), seeds 0-5: relative error against the noise-free tensor 3.6e-3 ... 5.9e-3
    after 200 iterations, plain ALS on the same data 0.19 ... 0.46; rel_change = 1e-6 with looks every 10
    iterations stops after 90 ... 140 iterations; the loss at successive looks never rose by more than 3e-16
    relative, with Z rounded to fp32 as well. Asserted for F64 and F32 storage, the reference run here on the
    same data: error <= 2 x the reference's; error <= 0.1 x that of 200 plain sweeps of the library; each look's
    loss <= (1 + 1e-9) x the look before; run_wls(rel_change=1e-6, resprint=10, maxiter=1000) returns 2 within
    300 iterations; run_wls with tol set to a residual already reached returns 1."""
    ctx = pp.Context(0)
    shape, R, seed = [12, 10, 9, 8], 3, 0
    g = np.random.default_rng(seed)
    Wt = [g.uniform(0.0, 1.0, (n, R)) for n in shape]
    clean = wls_ref.cp_model(Wt)
    sigma = np.where(g.uniform(size=shape) < 0.3, 1.0, 0.01)
    xh = clean + sigma * g.normal(size=shape)
    hh = pp.weights_from_std(sigma)
    W0 = [np.asfortranarray(g.uniform(0.0, 1.0, (n, R))) for n in shape]
    G0 = pp.init_factors(shape, R, 51)
    nclean = float(np.linalg.norm(clean))

    def err_of(W):
        return float(np.linalg.norm(wls_ref.cp_model(W) - clean)) / nclean

    Wref, _ = wls_ref.mm_als(xh, hh, W0, 200)
    ref_err = err_of(Wref)
    print(f"  numpy reference: error {ref_err:.3g} after 200 iterations", flush=True)
    assert ref_err < 0.01
    for dt, tdt in ((pp.F64, torch.float64), (pp.F32, torch.float32)):
        data, h = torch.from_numpy(xh).to(tdt).to(DEV), torch.from_numpy(hh).to(tdt).to(DEV)
        t = pp.Tensor(ctx, shape, dt).upload(xh)
        s = pp.CP(ctx, t, R)
        s.set_factors(W0, G0)
        s.sweeps_dt(200)
        plain = err_of(s.get_factors())
        s.set_factors(W0, G0)
        looks = []
        for _ in range(20):
            rc, it, res = s.run_wls(data, h, inner_sweeps=1, maxiter=10, resprint=10)
            assert (rc, it) == (0, 10), (dt, rc, it)
            looks.append(res)
        err = err_of(s.get_factors())
        rise = max((b * b - a * a) / (a * a) for a, b in zip(looks, looks[1:]))
        print(f"  storage {dt}: error {err:.3g} (reference {ref_err:.3g}, plain ALS {plain:.3g}); largest relative "
              f"rise of the loss between looks {rise:.3g}", flush=True)
        assert err <= 2 * ref_err, (dt, err, ref_err)
        assert err <= 0.1 * plain, (dt, err, plain)
        assert rise <= 1e-9, (dt, rise)
        s2 = pp.CP(ctx, t.upload(xh), R)
        s2.set_factors(W0, G0)
        rc, it, res = s2.run_wls(data, h, inner_sweeps=1, rel_change=1e-6, resprint=10, maxiter=1000)
        print(f"    rel_change 1e-6: stopped {rc} after {it} iterations at {res:.6g}", flush=True)
        assert rc == 2 and it <= 300, (dt, rc, it)
        s2.set_factors(W0, G0)
        rc, it, res = s2.run_wls(data, h, inner_sweeps=1, maxiter=200, resprint=10, tol=looks[9])
        print(f"    tol = the residual at iteration 100: stopped {rc} after {it} iterations", flush=True)
        assert rc == 1 and it < 200 and res <= looks[9], (dt, rc, it, res, looks[9])
        for x in (s2, s, t):
            x.close()
    ctx.close()


def stream_order():
    """a step on a side torch stream right behind the kernels that write data and weights there, no host
    synchronisation; both are overwritten on that stream right after the call"""
    ctx = pp.Context(0)
    shape, R = (64, 256, 1024), 4   # 64 MB of fp32
    t = pp.Tensor(ctx, list(shape), pp.F32).fill_uniform(3)
    s = pp.CP(ctx, t, R)
    s.set_factors(pp.init_factors(shape, R, 1), pp.init_factors(shape, R, 2))
    ref = s.model_to_torch(torch.float64)
    data = torch.full(shape, -5.0, dtype=torch.float32, device=DEV)      # stale contents
    h = torch.ones(shape, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        busy = torch.rand((4096, 4096), device=DEV)
        for _ in range(8):
            busy = busy @ busy / 4096.0   # keep the stream busy ahead of the views' kernels
        real_x = torch.rand(shape, device=DEV) + 2.0
        real_h = torch.rand(shape, device=DEV)
        data.copy_(real_x)
        h.copy_(real_h)
        assert s.wls_torch(data, h) is None
        data.fill_(-5.0)                  # must not reach the step's reads
        h.fill_(1.0)
        out = torch.empty(shape, dtype=torch.float32, device=DEV)
        t.export_torch(out)
        want = ref + real_h.double() * (real_x.double() - ref)
        near = (out.double() - want).abs() <= want.abs() * 2.0 ** -23 + 1e-12
    torch.cuda.synchronize()
    assert bool(near.all()), int((~near).sum())
    s.close()
    t.close()
    ctx.close()


def refusals():
    """for either view a host pointer, a span leaving its allocation, a negative stride, a box outside the
    tensor: PPALS_ERR_ARG with the entry point's name in front and the view named, before anything is launched;
    an integer dtype and mismatched torch dtypes: TypeError; BF16 storage and R = 129: PPALS_ERR_UNSUPPORTED.
    The tensor is unchanged"""
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
    bad = [("host", dict(ptr=host_t.data_ptr(), strides=fstr), {}),
           ("span", dict(ptr=good.data_ptr(), strides=[1, 20, 240 * 10 ** 6]), {}),
           ("negative_stride", dict(ptr=good.data_ptr(), strides=[1, -20, 240]), {})]
    for name, kw, extra in bad:
        for side, view in (("data", "the data view: "), ("weights", "the weights view: ")):
            d, w = (kw, ok) if side == "data" else (ok, kw)
            for want_loss in (False, True):
                try:
                    s.wls_device(d["ptr"], w["ptr"], pp.F32, lens, d["strides"], w["strides"], want_loss=want_loss)
                    raise AssertionError(f"{name} ({side}) accepted")
                except pp.PpalsError as e:
                    assert "ppals error -3: ppals_cp_wls_device: " + view in str(e), (name, side, str(e))
    try:
        s.wls_device(ok["ptr"], ok["ptr"], pp.F32, [10, 12, 9], fstr, fstr, lo=[15, 0, 0])
        raise AssertionError("box accepted")
    except pp.PpalsError as e:
        assert "ppals error -3: ppals_cp_wls_device: the data view: box mode 0" in str(e), str(e)
    try:
        s.run_wls(good[:10], good[:10], lo=[15, 0, 0], maxiter=2)
        raise AssertionError("driver box accepted")
    except pp.PpalsError as e:
        assert "ppals error -3: ppals_cp_wls: the data view: box mode 0" in str(e), str(e)
    ints = torch.ones(lens, dtype=torch.int32, device=DEV)
    for call in (lambda: s.wls_torch(ints, ints), lambda: s.wls_torch(good, good.double()),
                 lambda: s.run_wls(good.double(), good, maxiter=2), lambda: s.run_wls(ints, ints, maxiter=2)):
        try:
            call()
            raise AssertionError("bad torch dtypes accepted")
        except TypeError:
            pass
    try:
        s.wls_torch(host_t, good)
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
        for call in (lambda: s2.wls_torch(good, good, want_loss=True), lambda: s2.run_wls(good, good, maxiter=2)):
            try:
                call()
                raise AssertionError(f"{text} accepted")
            except pp.PpalsError as e:
                assert "ppals error -5: ppals_cp_wls" in str(e) and text in str(e), str(e)
        torch.cuda.synchronize()
        assert np.array_equal(t2.download(), V2)
        s2.close()
        t2.close()
    s.close()
    t.close()
    ctx.close()


def shards():
    """P = 2 ranks on the one GPU (hipsim library): each rank rewrites only its own rows, and the loss is the
    global sum on both ranks"""
    import hipsim_util
    hp = hipsim_util.load(make=False)
    lens, R, P = [29, 12, 10, 9], 4, 2
    g = torch.Generator(device="cpu").manual_seed(7)
    Xh = torch.rand(lens, generator=g, dtype=torch.float64)
    X = Xh.to(DEV)
    data, h, _, _ = view_pair(lens, "c_contiguous", "first_index_fastest", torch.float64, 5)
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
            loss = s.wls_torch(data, h, stream=0, want_loss=True)
            outs[rank] = {"rows": (lo, n), "W": W, "before": before, "after": t.download(), "loss": loss}
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
    z, want_loss = wls_ref.step(xh, hh, M)
    union = np.zeros(lens)
    for rank in range(P):
        lo, n = outs[rank]["rows"]
        a, b = outs[rank]["after"], outs[rank]["before"]
        assert np.array_equal(a[:lo], b[:lo]) and np.array_equal(a[lo + n:], b[lo + n:]), rank
        assert np.array_equal(b[lo:lo + n], Vs[lo:lo + n]), rank
        union[lo:lo + n] = a[lo:lo + n]
        assert abs(outs[rank]["loss"] - want_loss) <= 1e-10 * float(np.sum(hh * xh * xh)), (rank, outs[rank]["loss"])
    assert outs[0]["loss"] == outs[1]["loss"]
    check_values(union, z, absM + np.abs(xh), torch.float64, "sharded")


def quick():
    """one step with the loss against numpy under two view pairs (the smallest end-to-end check)"""
    ctx = pp.Context(0)
    shape, R = (12, 10, 8), 3
    t, s = session(ctx, shape, R, pp.F64)
    V0 = t.download()
    W = s.get_factors()
    M, absM = cp_model(W), cp_model(W, True)
    for i, (dkind, wkind) in enumerate(PAIRS[:2]):
        data, h, lo, _ = view_pair(shape, dkind, wkind, torch.float64, i)
        check_step(t, s, V0, M, absM, shape, pp.F64, data, h, lo, ("quick", dkind, wkind))
    s.close()
    t.close()
    ctx.close()


CASES = {f.__name__: f for f in (values, equals_impute, special_weights, reproducible, session_consistent, driver,
                                 stream_order, refusals, shards, quick)}

if __name__ == "__main__":
    CASES[sys.argv[1]](*sys.argv[2:])
    print(f"wls case {' '.join(sys.argv[1:])}: ok", flush=True)
