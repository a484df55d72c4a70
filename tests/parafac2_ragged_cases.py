"""Cases of tests/test_gpu_parafac2_ragged.py, one per process: `python parafac2_ragged_cases.py <case> [arg]`.

ppals_parafac2_*_ragged (include/ppals.h) through the binding's Parafac2.ragged. torch is imported BEFORE the
binding loads libppals (one HIP runtime for both). The reference is tests/parafac2_ragged_ref.py in numpy fp64 on
the values the buffer holds (an f32 buffer: the rounded values). Exit status 0: passed."""
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
import parafac2_ragged_ref as rref  # noqa: E402

DEV = torch.device("cuda", 0)
ERR_ARG, ERR_UNSUPPORTED = -3, -5
NN_FLOOR = 1e-16          # PPALS_NN_FLOOR
COMBOS = ((torch.float32, pp.F32), (torch.float32, pp.F64), (torch.float64, pp.F32), (torch.float64, pp.F64))
NPDT = {torch.float32: np.float32, torch.float64: np.float64}


class View:
    """a list of slices in one flat torch buffer on the GPU in one of the reference's layouts; `.host` are the
    values the buffer holds, as fp64"""

    def __init__(self, slices, tdt, layout="packed"):
        buf, self.offsets, self.col_strides = rref.pack(slices, layout, NPDT[tdt])
        self.rows, self.J = [X.shape[0] for X in slices], slices[0].shape[1]
        self.host = rref.unpack(buf, self.offsets, self.col_strides, self.rows, self.J)
        self.buf = torch.from_numpy(buf).to(DEV)
        torch.cuda.synchronize()
        self.args = dict(offsets=None, col_strides=None) if layout == "packed" else \
            dict(offsets=self.offsets, col_strides=self.col_strides)


def model(ctx, rows, J, R, dt, B, A, Cm):
    p = pp.Parafac2.ragged(ctx, rows, J, R, dt)
    assert p.rows == list(rows) and p.is_ragged
    p.cp.set_factors([B, A, Cm])
    return p


def half_ulp(y, dt):
    a = np.abs(y)
    if dt == pp.F32:
        return 0.5 * np.spacing(a.astype(np.float32)).astype(np.float64) + 2.0 ** -150
    return 0.5 * np.spacing(a)


def bars(Xh, B, A, Cm, want_failed):
    """what the reference says of the inputs, before the GPU is looked at: (ok, bound, kappa), the inputs under
    their cap"""
    R = A.shape[1]
    kap = rref.kappas(Xh, B, A, Cm)
    ok = np.isfinite(kap)
    assert int(np.count_nonzero(~ok)) == want_failed, kap
    assert kap[ok].max() <= rref.cap(R), kap
    return ok, np.where(ok, ref.p_bound(np.where(ok, kap, 1.0)), 0.0), kap     # a failed slice kept its P: exact


def check_against(P, Y, lost, Xh, B, A, Cm, dt, what, Pr, Yr, lost_r, ok, bound, kap):
    """check_step's bars of tests/parafac2_cases.py on P (leading rows of each P[k]), orthonormality, Y and
    lost_sq"""
    R = A.shape[1]
    xx = float(sum(np.sum(X * X) for X in Xh))
    dP = np.array([np.abs(P[k][:Pr[k].shape[0]] - Pr[k]).max() for k in range(len(Pr))])
    dO = np.array([np.abs(P[k].T @ P[k] - np.eye(R)).max() for k in range(len(Pr))])
    colnorm = np.stack([np.sqrt(np.sum(X * X, axis=0)) for X in Xh], axis=1)                 # J x K
    tolY = bound[None, None, :] * colnorm[None] + np.maximum(half_ulp(Yr, dt), half_ulp(Y, dt))
    dY = np.abs(Y - Yr)
    tolL = 1e-12 * xx + bound.max() * xx
    print(f"    {what}: kappa max {kap[ok].max():.3g}; P err / bound {np.max(dP[ok] / bound[ok]):.3g}, "
          f"orth err / bound {np.max(dO[ok] / bound[ok]):.3g}; Y err / tol {np.max(dY / tolY):.3g}; "
          f"lost_sq {lost:.17g} ref {lost_r:.17g} diff / tol {abs(lost - lost_r) / tolL:.3g}", flush=True)
    assert all(np.isfinite(p).all() for p in P) and np.isfinite(Y).all() and np.isfinite(lost)
    # (a slice that failed kept its P bit for bit, bound 0; how orthonormal that P is was settled when it was made)
    assert np.all(dP <= bound) and np.all(dO[ok] <= bound[ok]), (what, dP, dO, bound)
    assert np.all(dY <= tolY), (what, float(np.max(dY / tolY)))
    assert abs(lost - lost_r) <= tolL, (what, lost, lost_r, tolL)


def check_step(p, v, B, A, Cm, dt, what, P_prev=None, want_failed=0):
    """check_step of tests/parafac2_cases.py for a list of slices: one blocking step against the reference (P,
    orthonormality, Y, lost_sq, failed), then the loss identity"""
    Xh = v.host
    ok, bound, kap = bars(Xh, B, A, Cm, want_failed)
    Pr, Yr, lost_r, failed_r = rref.step_ragged(Xh, B, A, Cm, P_prev)
    lost, failed = p.step_torch(v.buf, **v.args)
    P, Y = p.projections(), p.Y.download()
    assert [x.shape for x in P] == [(n, p.R) for n in v.rows] and Y.shape == (p.R, p.J, p.K)
    assert failed == failed_r == want_failed, (what, failed, failed_r)
    check_against(P, Y, lost, Xh, B, A, Cm, dt, what, Pr, Yr, lost_r, ok, bound, kap)
    # the identity: lost_sq + residual^2 = ||X - model||^2, the right side from the downloads
    xx = float(sum(np.sum(X * X) for X in Xh))
    res = p.cp.residual()
    Bg, Ag, Cg = p.cp.get_factors()
    total = rref.loss(Xh, P, Bg, Ag, Cg)
    tol = 1e-10 * xx
    if dt == pp.F32:
        tol += 2.0 ** -24 * np.sqrt(xx) * float(np.linalg.norm(Y - ref.cp_model(Bg, Ag, Cg)))
    print(f"    {what}: lost_sq + residual^2 {lost + res * res:.17g} numpy {total:.17g} diff / tol "
          f"{abs(lost + res * res - total) / tol:.3g}", flush=True)
    assert abs(lost + res * res - total) <= tol, (what, lost, res, total, tol)
    return P, Y, lost


def values(which):
    """one table: f32 and f64 buffers, F32 and F64 storage, the three layouts (the padded one with NaN in every
    element no slice owns: every output must be finite, which check_step asserts)"""
    t = int(which)
    rows, J, R = rref.TABLES[t]
    slices, B, A, Cm = rref.values_inputs(t)
    ctx = pp.Context(0)
    for tdt, dt in COMBOS:
        for layout in rref.LAYOUTS:
            v = View(slices, tdt, layout)
            p = model(ctx, rows, J, R, dt, B, A, Cm)
            check_step(p, v, B, A, Cm, dt, (rows, J, R, str(tdt), dt, layout))
            p.close()
    ctx.close()


def equal_bits():
    """equal rows on the dense layout: the bits of the ppals_parafac2_create object on the same buffer, from the
    same factors; and again after one inner sweep of each"""
    ctx = pp.Context(0)
    for t, (rows, J, R) in enumerate(rref.EQUAL):
        I, K = rows[0], len(rows)
        slices, B, A, Cm = rref.equal_inputs(t)
        for tdt, dt in COMBOS:
            v = View(slices, tdt)                                     # packed: the dense I x J x K tensor
            x3 = v.buf.view(K, J, I).permute(2, 1, 0)
            assert x3.stride() == (1, I, I * J) and x3.data_ptr() == v.buf.data_ptr()
            pr = model(ctx, rows, J, R, dt, B, A, Cm)
            pe = pp.Parafac2(ctx, I, J, K, R, dt)
            pe.cp.set_factors([B, A, Cm])
            assert pe.rows == list(rows) and not pe.is_ragged
            for again in (False, True):
                got_r, got_e = pr.step_torch(v.buf), pe.step_torch(x3)
                Pr, Pe = np.stack(pr.projections()), pe.projections()
                assert got_r == got_e, (rows, dt, again, got_r, got_e)
                assert np.array_equal(Pr, Pe) and np.array_equal(pr.Y.download(), pe.Y.download()), (rows, dt, again)
                assert np.isfinite(Pr).all() and Pr.any()
                pr.cp.sweeps_dt(1)
                pe.cp.sweeps_dt(1)
                assert all(np.array_equal(a, b) for a, b in zip(pr.cp.get_factors(), pe.cp.get_factors()))
            print(f"    {rows} J {J} R {R} {tdt} storage {dt}: lost_sq {got_r[0]:.17g} both ways", flush=True)
            pr.close()
            pe.close()
    ctx.close()


def vs_padded():
    """the first table against the same slices zero-padded to 130 rows on the equal-length path: both under
    check_step's bars of the reference (Y, lost_sq, P_k on the leading rows), the padded path's extra rows zero.
    Not bit for bit: the Gram of the polar factor splits the rows differently."""
    rows, J, R = rref.TABLES[0]
    K, I = len(rows), max(rows)
    slices, B, A, Cm = rref.values_inputs(0)
    ctx = pp.Context(0)
    for tdt, dt in COMBOS:
        v = View(slices, tdt)
        p = model(ctx, rows, J, R, dt, B, A, Cm)
        P, Y, lost = check_step(p, v, B, A, Cm, dt, ("ragged", str(tdt), dt))
        p.close()
        ok, bound, kap = bars(v.host, B, A, Cm, 0)
        Pr, Yr, lost_r, _ = rref.step_ragged(v.host, B, A, Cm)
        xp = torch.from_numpy(np.ascontiguousarray(rref.zero_pad(v.host).transpose(2, 1, 0))).to(tdt).to(DEV)
        xp = xp.permute(2, 1, 0)
        assert xp.stride(0) == 1 and tuple(xp.shape) == (I, J, K)
        q = pp.Parafac2(ctx, I, J, K, R, dt)
        q.cp.set_factors([B, A, Cm])
        lost_p, failed_p = q.step_torch(xp)
        Pp, Yp = q.projections(), q.Y.download()
        q.close()
        assert failed_p == 0
        check_against(list(Pp), Yp, lost_p, v.host, B, A, Cm, dt, ("padded", str(tdt), dt), Pr, Yr, lost_r, ok, bound, kap)
        for k, n in enumerate(rows):
            assert not Pp[k][n:].any(), (k, n)
            assert np.abs(Pp[k][:n] - P[k]).max() <= 2 * bound[k]
    ctx.close()


def truth():
    """noise-free planted data and the planted factors: the step returns the planted P_k and loses nothing"""
    ctx = pp.Context(0)
    for t, (rows, J, R) in enumerate(rref.TABLES):
        slices, P0, B, A, Cm = rref.truth_inputs(t)
        for dt in (pp.F32, pp.F64):
            v = View(slices, torch.float64, rref.LAYOUTS[t % 3])
            kap = rref.kappas(v.host, B, A, Cm)
            assert kap.max() <= rref.cap(R)
            p = model(ctx, rows, J, R, dt, B, A, Cm)
            lost, failed = p.step_torch(v.buf, **v.args)
            P = p.projections()
            err = np.array([np.abs(a - b).max() for a, b in zip(P, P0)])
            xx = float(sum(np.sum(X * X) for X in v.host))
            print(f"    {rows} storage {dt}: kappa max {kap.max():.3g}, P err / bound "
                  f"{np.max(err / ref.p_bound(kap)):.3g}, lost_sq / ||X||^2 {lost / xx:.3g}", flush=True)
            assert failed == 0
            assert np.all(err <= ref.p_bound(kap)), (rows, err, ref.p_bound(kap))
            assert abs(lost) <= 1e-12 * xx, (rows, lost, xx)
            p.close()
    ctx.close()


def failed_slices():
    """rows (9, 12, 7): slice 0 all zero, slice 2 of rank R - 1. Each keeps its P_k (the identity columns the first
    time, the previous P_k the second), each counts in failed, nothing is NaN"""
    rows, J, R = rref.FAILED
    slices, B, A, Cm = rref.failed_inputs()
    ident = rref.identity_projections(rows, R)
    ctx = pp.Context(0)
    for tdt, dt in COMBOS:
        v = View(slices, tdt, "padded" if dt == pp.F32 else "stacked")
        p = model(ctx, rows, J, R, dt, B, A, Cm)
        P, Y, _ = check_step(p, v, B, A, Cm, dt, ("failed slices", str(tdt), dt), want_failed=2)
        assert np.array_equal(P[0], ident[0]) and np.array_equal(P[2], ident[2]) and not Y[:, :, 0].any()
        # a second step from a state in which the two slices hold something else: kept, not reset
        rng = np.random.default_rng(7)
        keep = [np.linalg.qr(rng.standard_normal((n, R)))[0] for n in rows]
        q = model(ctx, rows, J, R, dt, B, A, Cm)
        other = [0.5 * X for X in slices]
        other[0], other[2] = keep[0] @ (B * Cm[0]) @ A.T, keep[2] @ (B * Cm[2]) @ A.T      # full rank there
        q.step_torch(View(other, torch.float64).buf)
        Pq = q.projections()
        assert not np.array_equal(Pq[0], ident[0]) and not np.array_equal(Pq[2], ident[2])
        P2, _, _ = check_step(q, v, B, A, Cm, dt, ("failed slices again", str(tdt), dt), P_prev=Pq, want_failed=2)
        assert np.array_equal(P2[0], Pq[0]) and np.array_equal(P2[2], Pq[2])
        p.close()
        q.close()
    ctx.close()


def reproducible():
    """the same state twice: P, Y and lost_sq bit for bit, with and without the outputs"""
    ctx = pp.Context(0)
    for t in (0, 4):
        rows, J, R = rref.TABLES[t]
        slices, B, A, Cm = rref.values_inputs(t)
        for tdt, dt in COMBOS[::3]:
            v = View(slices, tdt, "padded")
            got = []
            for want in (True, True, False):
                p = model(ctx, rows, J, R, dt, B, A, Cm)
                out = p.step_torch(v.buf, want=want, **v.args)
                ctx.sync()
                got.append((b"".join(x.tobytes() for x in p.projections()), p.Y.download().tobytes(), out))
                if want:          # and again on the same object
                    out2 = p.step_torch(v.buf, **v.args)
                    assert (b"".join(x.tobytes() for x in p.projections()), p.Y.download().tobytes(), out2) == got[-1]
                p.close()
            assert got[0] == got[1] and got[0][:2] == got[2][:2] and got[2][2] is None, (rows, dt)
    ctx.close()


def run_looks(p, v, n, xx):
    """n iterations of one inner sweep, one call each: the loss after every iteration; asserts it never rises"""
    losses = [p.loss(v.buf, **v.args)]
    for _ in range(n):
        rc, it, res = p.run(v.buf, inner_sweeps=1, maxiter=1, resprint=1, **v.args)
        assert rc == 0 and it == 1
        losses.append(res * res)
    rises = [b - a for a, b in zip(losses, losses[1:])]
    print(f"    losses / ||X||^2: first {losses[0] / xx:.6g}, after 1 {losses[1] / xx:.6g}, last {losses[-1] / xx:.6g}; "
          f"largest rise / ||X||^2 {max(rises) / xx:.3g}", flush=True)
    assert max(rises) <= 1e-12 * xx, (rises, xx)
    return losses


def driver():
    """rows (30, 22, 41, 30, 18, 35), J = 20, R = 3, 5 % noise, F64 storage: 20 iterations of one inner sweep from
    B = I, C = 1, A uniform, under the tolerance of the equal-length driver case"""
    rows, J, R = rref.DRIVER
    slices, B, A, Cm = rref.driver_inputs()
    want = rref.fit(slices, B, A, Cm, 20)[4]
    ctx = pp.Context(0)
    v = View(slices, torch.float64, "stacked")
    xx = float(sum(np.sum(X * X) for X in v.host))
    p = model(ctx, rows, J, R, pp.F64, B, A, Cm)
    losses = run_looks(p, v, 20, xx)
    p.close()
    p = model(ctx, rows, J, R, pp.F64, B, A, Cm)
    rc, it, res = p.run(v.buf, inner_sweeps=1, maxiter=20, resprint=1, **v.args)
    print(f"    final loss / ||X||^2: one call {res * res / xx:.12g}, call by call {losses[-1] / xx:.12g}, numpy "
          f"{want[20] / xx:.12g}; relative difference {abs(res * res - want[20]) / want[20]:.3g}", flush=True)
    assert rc == 0 and it == 20
    assert abs(res * res - want[20]) <= 1e-6 * want[20], (res * res, want[20])
    assert abs(losses[-1] - want[20]) <= 1e-6 * want[20], (losses[-1], want[20])
    assert want[20] < 0.5 * want[0] and res * res < 0.5 * losses[0]      # the driver did something
    rc, it, res2 = p.run(v.buf, inner_sweeps=1, maxiter=50, resprint=1, rel_change=0.5, **v.args)
    assert rc == 2 and it < 50 and res2 <= res * (1 + 1e-12)
    p.close()
    # the same with (free, non-negative, non-negative) on the inner session: descends and keeps the floor
    p = model(ctx, rows, J, R, pp.F64, B, A, Cm)
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
    rows, J, R = rref.TABLES[0]
    slices, B, A, Cm = rref.values_inputs(0)
    ctx = pp.Context(0)
    v0 = View(slices, torch.float32, "stacked")
    p = model(ctx, rows, J, R, pp.F64, B, A, Cm)
    want = p.step_torch(v0.buf, **v0.args)
    wantP, wantY = b"".join(x.tobytes() for x in p.projections()), p.Y.download().tobytes()
    p.close()
    p = model(ctx, rows, J, R, pp.F64, B, A, Cm)
    side = torch.cuda.Stream(device=DEV)
    buf = torch.zeros_like(v0.buf)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        big = torch.randn(1 << 24, device=DEV)
        for _ in range(20):
            big = big * 1.0001 + 0.5          # keeps the stream busy ahead of the write
        buf.copy_(v0.buf)                     # the data arrives on the side stream only
        assert p.step_torch(buf, stream=side, want=False, **v0.args) is None
        buf.zero_()                           # queued after the step: must wait for its reads
    side.synchronize()
    ctx.sync()
    assert b"".join(x.tobytes() for x in p.projections()) == wantP and p.Y.download().tobytes() == wantY
    got = p.step_torch(v0.buf, **v0.args)
    assert got == want and b"".join(x.tobytes() for x in p.projections()) == wantP
    assert p.Y.download().tobytes() == wantY
    p.close()
    ctx.close()


def convenience():
    """ppals.parafac2 on a list of torch matrices: the reference's losses, lists of the right shapes, profiles =
    P_k B; a list input of the object is packed once and refilled when a tensor changes"""
    rows, J, R = rref.DRIVER
    slices, B, A, Cm = rref.driver_inputs()
    want = rref.fit(slices, B, A, Cm, 20)[4]
    xs = [torch.from_numpy(np.ascontiguousarray(X)).to(DEV) for X in slices]      # C order, as a user has them
    out = pp.parafac2(xs, R, n_iter=20, A0=A)
    xx = float(sum(np.sum(X * X) for X in slices))
    assert len(out["losses"]) == 21 and out["iterations"] == 20 and out["rc"] == 0
    assert np.allclose(out["losses"], want, rtol=1e-6, atol=0), (out["losses"], want)
    assert isinstance(out["projections"], list) and isinstance(out["profiles"], list)
    assert [x.shape for x in out["projections"]] == [(n, R) for n in rows]
    assert [x.shape for x in out["profiles"]] == [(n, R) for n in rows]
    assert all(np.allclose(f, P @ out["B"]) for f, P in zip(out["profiles"], out["projections"]))
    assert abs(rref.loss(slices, out["projections"], out["B"], out["A"], out["C"]) - out["losses"][-1]) <= 1e-10 * xx
    nn = pp.parafac2(tuple(xs), R, n_iter=20, nonneg_modes=(1, 2), A0=A)
    assert all(b <= a + 1e-12 * xx for a, b in zip(nn["losses"], nn["losses"][1:]))
    assert nn["A"].min() >= NN_FLOOR and nn["C"].min() >= NN_FLOOR
    # the object's packed copy: the list and the flat buffer give the same bits; a changed tensor is seen
    ctx = pp.Context(0)
    p = model(ctx, rows, J, R, pp.F64, B, A, Cm)
    v = View(slices, torch.float64)
    a = p.step_torch(xs)
    assert a == p.step_torch(v.buf) == p.step_torch(xs)
    xs[1].mul_(2.0)
    b = p.step_torch(xs)
    slices[1] = 2.0 * slices[1]
    assert b != a and b == p.step_torch(View(slices, torch.float64).buf)
    p.close()
    ctx.close()


def refusals():
    """every refusal comes before any launch or allocation and leaves tensor, session and projections unchanged"""
    ctx = pp.Context(0)
    L = pp.lib()
    h = C.c_void_p()

    def create(rows, J, R, dt, K=None):
        arr = (C.c_int64 * max(len(rows), 1))(*rows) if rows is not None else None
        rc = L.ppals_parafac2_create_ragged(ctx._h, C.c_int64(len(rows) if K is None else K), arr, C.c_int64(J), R, dt,
                                            C.byref(h))
        assert not h.value
        return rc, L.ppals_last_error()

    free0 = torch.cuda.mem_get_info()[0]
    for args, code, text in ((((9, 8), 7, 1, pp.F64), ERR_ARG, b"[2, 64]"), (((90, 80), 70, 65, pp.F64), ERR_ARG, b"[2, 64]"),
                             (((9, 9), 7, 8, pp.F64), ERR_ARG, b"exceed J"), (((9, 5, 4, 9), 7, 5, pp.F32), ERR_ARG, b"slice 2 "),
                             (((), 7, 3, pp.F64), ERR_ARG, b"positive"), (((9, 8), 0, 3, pp.F64), ERR_ARG, b"positive"),
                             ((None, 7, 3, pp.F64, 2), ERR_ARG, b"rows is NULL"), (((9, 8), 7, 3, 7), ERR_ARG, b"dtype"),
                             (((9, 8), 7, 3, pp.BF16), ERR_UNSUPPORTED, b"BF16")):
        rc, err = create(*args)
        assert rc == code and err.startswith(b"ppals_parafac2_create_ragged: ") and text in err, (args, rc, err)
    assert torch.cuda.mem_get_info()[0] == free0

    rows, J, R = rref.TABLES[0]
    K, N = len(rows), sum(rows)
    slices, B, A, Cm = rref.values_inputs(0)
    v = View(slices, torch.float64, "stacked")
    p = model(ctx, rows, J, R, pp.F64, B, A, Cm)
    p.run(v.buf, maxiter=1, resprint=1, **v.args)      # (everything a step and a run allocate is there from here on)
    p.cp.set_factors([B, A, Cm])
    e = pp.Parafac2(ctx, 9, J, K, R, pp.F64)
    ve = torch.ones(9 * J * K, dtype=torch.float64, device=DEV)
    e.step_device(ve.data_ptr(), pp.F64)

    def snap(x):
        P = x.projections()
        return (b"".join(a.tobytes() for a in P), x.Y.download().tobytes(), [w.tobytes() for w in x.cp.get_factors()])

    state_e = snap(e)
    v.buf.mul_(2.0)          # a step that ran would change Y at least
    ve.mul_(2.0)
    torch.cuda.synchronize()
    i64 = C.c_int64 * K
    off, cs = i64(*v.offsets), i64(*v.col_strides)
    o = pp._opts(maxiter=3)
    lost, failed, it, res = C.c_double(-1.0), C.c_int(-1), C.c_int(-1), C.c_double(-1.0)

    def step(h=None, ptr=v.buf.data_ptr(), dt=pp.F64, offsets=off, strides=cs):
        return L.ppals_parafac2_step_ragged_device(h or p._h, C.c_void_p(ptr) if ptr else None, dt, offsets, strides, None,
                                                   C.byref(lost), C.byref(failed))

    def run(h=None, ptr=v.buf.data_ptr(), dt=pp.F64, offsets=off, strides=cs, inner=1, rel=0.0, opts=o):
        return L.ppals_parafac2_run_ragged(h or p._h, C.c_void_p(ptr) if ptr else None, dt, offsets, strides, None,
                                           C.byref(opts) if opts else None, inner, C.c_double(rel), C.byref(it),
                                           C.byref(res))

    def changed(a, k, val):
        b = list(a)
        b[k] = val
        return i64(*b)

    hostbuf = np.zeros(N * J)
    exact = v.buf.clone()                                                # the stacked layout fits exactly ...
    assert exact.numel() == N * J
    past = changed(v.offsets, K - 1, v.offsets[K - 1] + 1)               # ... and one element further does not
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for fn, name in ((step, b"ppals_parafac2_step_ragged_device: "), (run, b"ppals_parafac2_run_ragged: ")):
        for kw, code, text in ((dict(h=e._h), ERR_ARG, b"ppals_parafac2_create"),
                               (dict(ptr=0), ERR_ARG, b"the data pointer is NULL"),
                               (dict(ptr=v.buf.data_ptr() + 4), ERR_ARG, b"not aligned"),
                               (dict(dt=pp.BF16), ERR_ARG, b"bad dtype"), (dict(dt=pp.U8), ERR_ARG, b"bad dtype"),
                               (dict(offsets=changed(v.offsets, 1, -1)), ERR_ARG, b"offsets[1] is negative"),
                               (dict(strides=changed(v.col_strides, 4, rows[4] - 1)), ERR_ARG, b"col_strides[4]"),
                               (dict(ptr=hostbuf.ctypes.data), ERR_ARG, b"not device memory"),
                               (dict(ptr=exact.data_ptr(), offsets=past), ERR_ARG, b"past the end of its allocation")):
            rc = fn(**kw)
            err = L.ppals_last_error()
            assert rc == code and err.startswith(name) and text in err, (name, kw, rc, err)
        for kinds in (["fixed", "free", "free"], ["ortho", "nonneg", "free"]):
            p.cp.set_mode_constraints(kinds)
            assert fn() == ERR_ARG and b"mode 0" in L.ppals_last_error(), (name, kinds)
        p.cp.set_mode_constraints(["free", "free", "free"])
        assert (lost.value, failed.value, it.value, res.value) == (-1.0, -1, -1, -1.0)
        assert fn(ptr=exact.data_ptr()) == 0          # (the span that ends with the allocation is taken)
        assert fn() == 0
        lost.value, failed.value, it.value, res.value = -1.0, -1, -1, -1.0
        p.cp.set_factors([B, A, Cm])
    # the equal-length entry points on a ragged object
    st3 = (C.c_int64 * 3)(1, N, 0)
    assert L.ppals_parafac2_step_device(p._h, C.c_void_p(v.buf.data_ptr()), pp.F64, st3, None, C.byref(lost),
                                        C.byref(failed)) == ERR_ARG
    assert L.ppals_last_error().startswith(b"ppals_parafac2_step_device: ") and b"ragged" in L.ppals_last_error()
    assert L.ppals_parafac2_run(p._h, C.c_void_p(v.buf.data_ptr()), pp.F64, st3, None, C.byref(o), 1, C.c_double(0.0),
                                C.byref(it), C.byref(res)) == ERR_ARG
    assert L.ppals_last_error().startswith(b"ppals_parafac2_run: ")
    for kw, text in ((dict(inner=0), b"inner_sweeps"), (dict(rel=-1e-3), b"rel_change"), (dict(rel=float("nan")), b"rel_change"),
                     (dict(opts=None), b"NULL options"), (dict(opts=pp._opts(maxiter=-1)), b"maxiter")):
        assert run(**kw) == ERR_ARG and text in L.ppals_last_error(), kw
    assert (lost.value, failed.value, it.value, res.value) == (-1.0, -1, -1, -1.0)
    assert torch.cuda.mem_get_info()[0] == free0
    assert state_e == snap(e)
    p.close()
    e.close()
    ctx.close()


def refusals_state():
    """the refusals of a step leave P, Y, the factors and what the inner session derived from the tensor (its
    residual) as they were, and allocate nothing"""
    rows, J, R = rref.TABLES[0]
    K = len(rows)
    slices, B, A, Cm = rref.values_inputs(0)
    ctx = pp.Context(0)
    L = pp.lib()
    v = View(slices, torch.float64, "stacked")
    p = model(ctx, rows, J, R, pp.F64, B, A, Cm)
    p.step_torch(v.buf, **v.args)
    state = (b"".join(a.tobytes() for a in p.projections()), p.Y.download().tobytes(),
             [w.tobytes() for w in p.cp.get_factors()], p.cp.residual())
    v.buf.mul_(2.0)
    torch.cuda.synchronize()
    i64 = C.c_int64 * K
    lost, failed = C.c_double(-1.0), C.c_int(-1)
    free0 = torch.cuda.mem_get_info()[0]
    bad_off, bad_cs = list(v.offsets), list(v.col_strides)
    bad_off[0], bad_cs[2] = -1, rows[2] - 1
    past = list(v.offsets)
    past[K - 1] += 1
    for ptr, off, cs in ((v.buf.data_ptr(), bad_off, v.col_strides), (v.buf.data_ptr(), v.offsets, bad_cs),
                         (v.buf.data_ptr(), past, v.col_strides), (v.buf.data_ptr() + 4, v.offsets, v.col_strides)):
        rc = L.ppals_parafac2_step_ragged_device(p._h, C.c_void_p(ptr), pp.F64, i64(*off), i64(*cs), None,
                                                 C.byref(lost), C.byref(failed))
        assert rc == ERR_ARG, (off, cs, rc, L.ppals_last_error())
    assert (lost.value, failed.value) == (-1.0, -1)
    assert torch.cuda.mem_get_info()[0] == free0
    assert state == (b"".join(a.tobytes() for a in p.projections()), p.Y.download().tobytes(),
                     [w.tobytes() for w in p.cp.get_factors()], p.cp.residual())
    p.close()
    ctx.close()


CASES = dict(values=values, equal_bits=equal_bits, vs_padded=vs_padded, truth=truth, failed_slices=failed_slices,
             reproducible=reproducible, driver=driver, stream_order=stream_order, convenience=convenience,
             refusals=refusals, refusals_state=refusals_state)

if __name__ == "__main__":
    name, args = sys.argv[1], sys.argv[2:]
    CASES[name](*args)
    print(f"parafac2 ragged case {' '.join(sys.argv[1:])}: ok", flush=True)
