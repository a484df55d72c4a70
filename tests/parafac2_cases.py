"""Cases of tests/test_gpu_parafac2.py, one per process: `python parafac2_cases.py <case> [arg]`.

ppals_parafac2_* (include/ppals.h) through the binding's Parafac2. torch is imported BEFORE the binding loads
libppals (one HIP runtime for both). The reference is tests/parafac2_ref.py in numpy fp64 on the values the view
holds (an f32 view: the rounded values). Exit status 0: passed."""
import ctypes as C
import os
import sys

import torch  # noqa: I001  (first: see above)
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "pairwise-perturbation_amd"))
import ppals as pp  # noqa: E402
import parafac2_ref as ref  # noqa: E402
import parafac2_cases_inputs as inputs  # noqa: E402

DEV = torch.device("cuda", 0)
ERR_ARG, ERR_UNSUPPORTED = -3, -5
NN_FLOOR = 1e-16          # PPALS_NN_FLOOR
COMBOS = ((torch.float32, pp.F32), (torch.float32, pp.F64), (torch.float64, pp.F32), (torch.float64, pp.F64))


def view(X, tdt, padded=False):
    """X (numpy, I x J x K) as a torch tensor on the GPU with unit stride in mode 0; padded: strides[1] > I and
    strides[2] > strides[1] J, the padding NaN. Returns (the view, its values as numpy fp64)."""
    I, J, K = X.shape
    pi, pj = (3, 2) if padded else (0, 0)
    buf = torch.full((K, J + pj, I + pi), float("nan"), dtype=tdt, device=DEV)
    v = buf.permute(2, 1, 0)[:I, :J, :K]
    v.copy_(torch.from_numpy(np.ascontiguousarray(X)).to(DEV))
    torch.cuda.synchronize()
    assert v.stride(0) == 1 and (not padded or (v.stride(1) > I and v.stride(2) > v.stride(1) * J))
    return v, v.cpu().double().numpy()


def model(ctx, shape, dt, B, A, Cm):
    I, J, K, R = shape
    p = pp.Parafac2(ctx, I, J, K, R, dt)
    p.cp.set_factors([B, A, Cm])
    return p


def half_ulp(y, dt):
    a = np.abs(y)
    if dt == pp.F32:
        return 0.5 * np.spacing(a.astype(np.float32)).astype(np.float64) + 2.0 ** -150
    return 0.5 * np.spacing(a)


def check_step(p, v, Xh, B, A, Cm, dt, what, P_prev=None, want_failed=0):
    """one blocking step against the reference: P, orthonormality, Y, lost_sq, failed; then the loss identity"""
    lost, failed = p.step_torch(v)
    P, Y = p.projections(), p.Y.download()
    Pr, Yr, lost_r, failed_r = ref.step(Xh, B, A, Cm, P_prev)
    kap = ref.kappas(Xh, B, A, Cm)
    ok = np.isfinite(kap)
    assert failed == failed_r == want_failed == int(np.count_nonzero(~ok)), (what, failed, failed_r)
    assert kap[ok].max() <= ref.KAPPA_CAP, (what, kap)
    bound = np.where(ok, ref.p_bound(np.where(ok, kap, 1.0)), 0.0)     # a failed slice kept its P: exact
    xx = float(np.sum(Xh * Xh))
    R = p.R
    dP = np.abs(P - Pr).max(axis=(1, 2))
    dO = np.abs(np.einsum("kir,kis->krs", P, P) - np.eye(R)).max(axis=(1, 2))
    colnorm = np.sqrt(np.sum(Xh * Xh, axis=0))                          # J x K
    tolY = bound[None, None, :] * colnorm[None] + np.maximum(half_ulp(Yr, dt), half_ulp(Y, dt))
    dY = np.abs(Y - Yr)
    tolL = 1e-12 * xx + bound.max() * xx
    print(f"    {what}: kappa max {kap[ok].max():.3g}; P err / bound {np.max(dP[ok] / bound[ok]):.3g}, "
          f"orth err / bound {np.max(dO[ok] / bound[ok]):.3g}; Y err / tol {np.max(dY / tolY):.3g}; "
          f"lost_sq {lost:.17g} ref {lost_r:.17g} diff / tol {abs(lost - lost_r) / tolL:.3g}", flush=True)
    assert np.isfinite(P).all() and np.isfinite(Y).all() and np.isfinite(lost)
    assert np.all(dP <= bound) and np.all(dO <= bound), (what, dP, dO, bound)
    assert np.all(dY <= tolY), (what, float(np.max(dY / tolY)))
    assert abs(lost - lost_r) <= tolL, (what, lost, lost_r, tolL)
    # the identity: lost_sq + residual^2 = ||X - model||^2, the right side from the downloads
    res = p.cp.residual()
    Bg, Ag, Cg = p.cp.get_factors()
    total = ref.loss(Xh, P, Bg, Ag, Cg)
    tol = 1e-10 * xx
    if dt == pp.F32:
        tol += 2.0 ** -24 * np.sqrt(xx) * float(np.linalg.norm(Y - ref.cp_model(Bg, Ag, Cg)))
    print(f"    {what}: lost_sq + residual^2 {lost + res * res:.17g} numpy {total:.17g} diff / tol "
          f"{abs(lost + res * res - total) / tol:.3g}", flush=True)
    assert abs(lost + res * res - total) <= tol, (what, lost, res, total, tol)
    return P, Y, lost


def values(which):
    """step values and the identity for one shape: f32 and f64 views, F32 and F64 storage, padded slices for the
    f64 storage. The shapes 5..7 have three and four rank tiles, and their inner CP session (residual, get_factors,
    the loss identity) runs at ranks up to 64 on an R x J x K tensor."""
    i = int(which)
    shape = inputs.ALL_SHAPES[i]      # 0..4: ref.SHAPES; 5..7: ref.SHAPES_WIDE (three and four rank tiles of 16)
    X, B, A, Cm = inputs.values_inputs(i)
    ctx = pp.Context(0)
    for tdt, dt in COMBOS:
        v, Xh = view(X, tdt, padded=dt == pp.F64)
        p = model(ctx, shape, dt, B, A, Cm)
        check_step(p, v, Xh, B, A, Cm, dt, (shape, str(tdt), dt))
        p.close()
    ctx.close()


def truth():
    """noise-free planted data and the planted factors: the step returns the planted P_k and loses nothing"""
    ctx = pp.Context(0)
    for i, shape in enumerate(inputs.ALL_SHAPES):
        X, B, A, Cm, P0 = inputs.truth_inputs(i)
        for dt in (pp.F32, pp.F64):
            v, Xh = view(X, torch.float64, padded=i % 2 == 0)
            p = model(ctx, shape, dt, B, A, Cm)
            lost, failed = p.step_torch(v)
            kap = ref.kappas(Xh, B, A, Cm)
            P = p.projections()
            err = np.abs(P - P0).max(axis=(1, 2))
            xx = float(np.sum(Xh * Xh))
            print(f"    {shape} storage {dt}: kappa max {kap.max():.3g}, P err / bound {np.max(err / ref.p_bound(kap)):.3g}, "
                  f"lost_sq / ||X||^2 {lost / xx:.3g}", flush=True)
            assert failed == 0 and kap.max() <= ref.KAPPA_CAP
            assert np.all(err <= ref.p_bound(kap)), (shape, err, ref.p_bound(kap))
            assert abs(lost) <= 1e-12 * xx, (shape, lost, xx)
            p.close()
    ctx.close()


def zero_slice():
    """one all-zero slice: failed == 1, that slice keeps the identity columns, its Y is zero, nothing is NaN, the
    other slices are the reference's"""
    shape = ref.SHAPES[0]
    I, J, K, R = shape
    X, B, A, Cm = inputs.zero_slice_inputs()
    ctx = pp.Context(0)
    for tdt, dt in COMBOS:
        v, Xh = view(X, tdt, padded=dt == pp.F32)
        p = model(ctx, shape, dt, B, A, Cm)
        P, Y, _ = check_step(p, v, Xh, B, A, Cm, dt, ("zero slice", str(tdt), dt), want_failed=1)
        assert np.array_equal(P[3], ref.identity_projections(I, K, R)[3]) and not Y[:, :, 3].any()
        # a second step from a state in which slice 3 holds something else: it is kept, not reset
        P2, _, _ = check_step(p, v, Xh, B, A, Cm, dt, ("zero slice again", str(tdt), dt), P_prev=P, want_failed=1)
        assert np.array_equal(P2[3], P[3])
        p.close()
    ctx.close()


def reproducible():
    """the same state twice: P, Y and lost_sq bit for bit, with and without the outputs"""
    ctx = pp.Context(0)
    for i in (1, 4):
        shape = ref.SHAPES[i]
        X, B, A, Cm = inputs.values_inputs(i)
        for tdt, dt in COMBOS[::3]:
            v, _ = view(X, tdt, padded=True)
            got = []
            for want in (True, True, False):
                p = model(ctx, shape, dt, B, A, Cm)
                out = p.step_torch(v, want=want)
                ctx.sync()
                got.append((p.projections().tobytes(), p.Y.download().tobytes(), out))
                if want:          # and again on the same object
                    out2 = p.step_torch(v)
                    assert (p.projections().tobytes(), p.Y.download().tobytes(), out2) == got[-1]
                p.close()
            assert got[0] == got[1] and got[0][:2] == got[2][:2] and got[2][2] is None, (shape, dt)
    ctx.close()


def run_looks(p, v, n, xx):
    """n iterations of one inner sweep, one call each: the loss after every iteration; asserts it never rises"""
    losses = [p.loss(v)]
    for _ in range(n):
        rc, it, res = p.run(v, inner_sweeps=1, maxiter=1, resprint=1)
        assert rc == 0 and it == 1
        losses.append(res * res)
    rises = [b - a for a, b in zip(losses, losses[1:])]
    print(f"    losses / ||X||^2: first {losses[0] / xx:.6g}, after 1 {losses[1] / xx:.6g}, last {losses[-1] / xx:.6g}; "
          f"largest rise / ||X||^2 {max(rises) / xx:.3g}", flush=True)
    assert max(rises) <= 1e-12 * xx, (rises, xx)
    return losses


def driver():
    """(30, 20, 12, 3), 5 % noise, F64 storage: 20 iterations of one inner sweep from B = I, C = 1, A uniform"""
    shape = ref.DRIVER
    X, B, A, Cm = inputs.driver_inputs()
    want = ref.fit(X, B, A, Cm, 20)[4]
    ctx = pp.Context(0)
    v, Xh = view(X, torch.float64)
    xx = float(np.sum(Xh * Xh))
    p = model(ctx, shape, pp.F64, B, A, Cm)
    losses = run_looks(p, v, 20, xx)
    p.close()
    # the same in one call, a look at every iteration
    p = model(ctx, shape, pp.F64, B, A, Cm)
    rc, it, res = p.run(v, inner_sweeps=1, maxiter=20, resprint=1)
    print(f"    final loss / ||X||^2: one call {res * res / xx:.12g}, call by call {losses[-1] / xx:.12g}, numpy "
          f"{want[20] / xx:.12g}; relative difference {abs(res * res - want[20]) / want[20]:.3g}", flush=True)
    assert rc == 0 and it == 20
    assert abs(res * res - want[20]) <= 1e-6 * want[20], (res * res, want[20])
    assert abs(losses[-1] - want[20]) <= 1e-6 * want[20], (losses[-1], want[20])
    assert want[20] < 0.5 * want[0] and res * res < 0.5 * losses[0]      # the driver did something
    # the stop rules of the weighted driver: rel_change ends the run early with 2
    rc, it, res2 = p.run(v, inner_sweeps=1, maxiter=50, resprint=1, rel_change=0.5)
    assert rc == 2 and it < 50 and res2 <= res * (1 + 1e-12)
    p.close()
    ctx.close()


def nonneg():
    """the driver's case with (free, non-negative, non-negative) on the inner session"""
    shape = ref.DRIVER
    X, B, A, Cm = inputs.driver_inputs()
    ctx = pp.Context(0)
    v, Xh = view(X, torch.float64)
    xx = float(np.sum(Xh * Xh))
    p = model(ctx, shape, pp.F64, B, A, Cm)
    p.cp.set_mode_constraints(["free", "nonneg", "nonneg"])
    losses = run_looks(p, v, 20, xx)
    _, Ag, Cg = p.cp.get_factors()
    assert Ag.min() >= NN_FLOOR and Cg.min() >= NN_FLOOR, (Ag.min(), Cg.min())
    assert losses[-1] < 0.5 * losses[0]
    p.close()
    ctx.close()


def stream_order():
    """a step on a side stream with NULL outputs, the data written on that stream just before, then a blocking step
    with outputs: the blocking step's bits"""
    i = 2
    shape = ref.SHAPES[i]
    X, B, A, Cm = inputs.values_inputs(i)
    ctx = pp.Context(0)
    v0, _ = view(X, torch.float32)
    p = model(ctx, shape, pp.F64, B, A, Cm)
    want = p.step_torch(v0)
    wantP, wantY = p.projections(), p.Y.download()
    p.close()
    p = model(ctx, shape, pp.F64, B, A, Cm)
    side = torch.cuda.Stream(device=DEV)
    v = torch.zeros_like(v0)
    assert v.stride() == v0.stride()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        big = torch.randn(1 << 24, device=DEV)
        for _ in range(20):
            big = big * 1.0001 + 0.5          # keeps the stream busy ahead of the write
        v.copy_(v0)                           # the data arrives on the side stream only
        assert p.step_torch(v, stream=side, want=False) is None
        v.zero_()                             # queued after the step: must wait for its reads
    side.synchronize()
    ctx.sync()
    assert p.projections().tobytes() == wantP.tobytes() and p.Y.download().tobytes() == wantY.tobytes()
    got = p.step_torch(v0)
    assert got == want and p.projections().tobytes() == wantP.tobytes() and p.Y.download().tobytes() == wantY.tobytes()
    p.close()
    ctx.close()


def refusals():
    """every refusal comes before any launch or allocation and leaves tensor, session and projections unchanged"""
    ctx = pp.Context(0)
    L = pp.lib()
    h = C.c_void_p()

    def create(I, J, K, R, dt):
        rc = L.ppals_parafac2_create(ctx._h, C.c_int64(I), C.c_int64(J), C.c_int64(K), R, dt, C.byref(h))
        assert not h.value
        return rc, L.ppals_last_error()

    free0 = torch.cuda.mem_get_info()[0]
    for args, code, text in (((9, 7, 4, 1, pp.F64), ERR_ARG, b"[2, 64]"), ((90, 70, 4, 65, pp.F64), ERR_ARG, b"[2, 64]"),
                             ((9, 7, 4, 8, pp.F64), ERR_ARG, b"min(I, J)"), ((7, 9, 4, 8, pp.F32), ERR_ARG, b"min(I, J)"),
                             ((9, 7, 0, 3, pp.F64), ERR_ARG, b"positive"), ((9, 7, 4, 3, 7), ERR_ARG, b"dtype"),
                             ((9, 7, 4, 3, pp.BF16), ERR_UNSUPPORTED, b"BF16")):
        rc, err = create(*args)
        assert rc == code and err.startswith(b"ppals_parafac2_create: ") and text in err, (args, rc, err)
    assert torch.cuda.mem_get_info()[0] == free0

    shape = ref.SHAPES[0]
    I, J, K, R = shape
    X, B, A, Cm = inputs.values_inputs(0)
    v, _ = view(X, torch.float64)
    p = model(ctx, shape, pp.F64, B, A, Cm)
    p.step_torch(v)
    state = (p.projections().tobytes(), p.Y.download().tobytes(), [w.tobytes() for w in p.cp.get_factors()])
    v.mul_(2.0)          # a step that ran would change P's Y at least
    torch.cuda.synchronize()
    st = (C.c_int64 * 3)(*v.stride())
    o = pp._opts(maxiter=3)
    lost, failed, it, res = C.c_double(-1.0), C.c_int(-1), C.c_int(-1), C.c_double(-1.0)

    def step(ptr=v.data_ptr(), dt=pp.F64, strides=st):
        return L.ppals_parafac2_step_device(p._h, C.c_void_p(ptr) if ptr else None, dt, strides, None,
                                            C.byref(lost), C.byref(failed))

    def run(ptr=v.data_ptr(), dt=pp.F64, strides=st, inner=1, rel=0.0, opts=o):
        return L.ppals_parafac2_run(p._h, C.c_void_p(ptr) if ptr else None, dt, strides, None,
                                    C.byref(opts) if opts else None, inner, C.c_double(rel), C.byref(it), C.byref(res))

    vc = torch.zeros((I, J, K), dtype=torch.float64, device=DEV)               # C order: the last index fastest
    hostbuf = np.zeros((I, J, K), order="F")
    small = torch.zeros(I * J * K - 1, dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for fn, name in ((step, b"ppals_parafac2_step_device: "), (run, b"ppals_parafac2_run: ")):
        for kw, code, text in ((dict(ptr=0), ERR_ARG, b"the data pointer is NULL"),
                               (dict(ptr=v.data_ptr() + 4), ERR_ARG, b"not aligned"),
                               (dict(dt=pp.BF16), ERR_ARG, b"bad dtype"), (dict(dt=pp.F16), ERR_ARG, b"bad dtype"),
                               (dict(dt=pp.U8), ERR_ARG, b"bad dtype"),
                               (dict(strides=(C.c_int64 * 3)(1, -I, I * J)), ERR_ARG, b"negative stride"),
                               (dict(ptr=hostbuf.ctypes.data), ERR_ARG, b"not device memory"),
                               (dict(ptr=small.data_ptr()), ERR_ARG, b"past the end of its allocation"),
                               (dict(ptr=vc.data_ptr(), strides=(C.c_int64 * 3)(*vc.stride())), ERR_UNSUPPORTED,
                                b"permute"),
                               (dict(strides=(C.c_int64 * 3)(1, I, 0)), ERR_UNSUPPORTED, b"overlap"),
                               (dict(strides=(C.c_int64 * 3)(1, I - 1, I * J)), ERR_UNSUPPORTED, b"overlap")):
            rc = fn(**kw)
            err = L.ppals_last_error()
            assert rc == code and err.startswith(name) and text in err, (name, kw, rc, err)
        # a constrained mode 0
        for kinds in (["fixed", "free", "free"], ["ortho", "nonneg", "free"]):
            p.cp.set_mode_constraints(kinds)
            assert fn() == ERR_ARG and b"mode 0" in L.ppals_last_error(), (name, kinds)
        p.cp.set_mode_constraints(["free", "free", "free"])
    for kw, text in ((dict(inner=0), b"inner_sweeps"), (dict(rel=-1e-3), b"rel_change"), (dict(rel=float("nan")), b"rel_change"),
                     (dict(opts=None), b"NULL options"), (dict(opts=pp._opts(maxiter=-1)), b"maxiter")):
        assert run(**kw) == ERR_ARG and text in L.ppals_last_error(), kw
    assert (lost.value, failed.value, it.value, res.value) == (-1.0, -1, -1, -1.0)
    assert torch.cuda.mem_get_info()[0] == free0
    assert state == (p.projections().tobytes(), p.Y.download().tobytes(), [w.tobytes() for w in p.cp.get_factors()])
    # a non-negative mode 0 (B = I, so that the session takes the constraint); then the order of destruction is free
    q = model(ctx, shape, pp.F32, np.eye(R), A, Cm)
    q.cp.set_mode_constraints(["nonneg", "free", "free"])
    rc = L.ppals_parafac2_step_device(q._h, C.c_void_p(v.data_ptr()), pp.F64, st, None, C.byref(lost), C.byref(failed))
    assert rc == ERR_ARG and b"mode 0" in L.ppals_last_error() and lost.value == -1.0
    assert not q.Y.download().any()
    q.cp.set_mode_constraints(["free", "free", "free"])
    q.step_torch(v)
    p.close()
    ctx.close()          # closes q through the context's children
    assert not q._h


def convenience():
    """ppals.parafac2 on a torch tensor: the reference's losses, profiles = P_k B, and a non-negative fit; a C-order
    tensor is made contiguous along mode 0 first"""
    I, J, K, R = ref.DRIVER
    X, B, A, Cm = inputs.driver_inputs()
    want = ref.fit(X, B, A, Cm, 20)[4]
    x = torch.from_numpy(np.ascontiguousarray(X)).to(DEV)           # C order: stride(0) != 1
    assert x.stride(0) != 1
    out = pp.parafac2(x, R, n_iter=20, A0=A)
    xx = float(np.sum(X * X))
    assert len(out["losses"]) == 21 and out["iterations"] == 20 and out["rc"] == 0
    assert np.allclose(out["losses"], want, rtol=1e-6, atol=0), (out["losses"], want)
    assert out["projections"].shape == (K, I, R) and np.allclose(out["profiles"], out["projections"] @ out["B"])
    assert abs(ref.loss(X, out["projections"], out["B"], out["A"], out["C"]) - out["losses"][-1]) <= 1e-10 * xx
    nn = pp.parafac2(x, R, n_iter=20, nonneg_modes=(1, 2), A0=A)
    assert all(b <= a + 1e-12 * xx for a, b in zip(nn["losses"], nn["losses"][1:]))
    assert nn["A"].min() >= NN_FLOOR and nn["C"].min() >= NN_FLOOR
    early = pp.parafac2(x, R, n_iter=50, rel_change=0.5, A0=A)
    assert early["rc"] == 2 and early["iterations"] < 50


CASES = dict(convenience=convenience, values=values, truth=truth, zero_slice=zero_slice, reproducible=reproducible, driver=driver, nonneg=nonneg,
             stream_order=stream_order, refusals=refusals)

if __name__ == "__main__":
    name, args = sys.argv[1], sys.argv[2:]
    CASES[name](*args)
    print(f"parafac2 case {' '.join(sys.argv[1:])}: ok", flush=True)
