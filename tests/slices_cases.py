"""The cases of the influence plot (ppals_cp_slice_residuals, ppals_cp_leverages) shared by
tests/test_slices_hostsim.py (the engine's control flow and the C ABI over the fp64 host twins of ops.h) and
tests/test_gpu_slices.py (the HIP kernels): each takes the binding `pp` it runs on. Reference and bars:
tests/slices_ref.py.

Inputs: the tensor is fill_uniform, the factors uniform on (0,1) from the counter generator
(pp.init_factors), so every residual element is O(1) and no slice sum suffers cancellation."""
import contextlib
import ctypes as C
import os

import numpy as np

import bf16_util
import slices_ref as R

F32, F64, BF16 = 0, 1, 3

# (lens, R): M = the product of the first N/2 extents, K = the rest. The smallest shapes at which each piece
# of the fused kernel (fp32 / fp64 storage, R <= 32, M a multiple of the vector width) and of the general one
# can go wrong:
SHAPES = [
    ([8, 6, 5], 3),          # M 8, K 30: one partly-live wave; K no multiple of 16 (clamped columns excluded)
    ([20, 18, 17], 10),      # M 20, K 306: the two-rank vector-pipe remainder
    ([12, 10, 9, 7], 9),     # M 120, K 63: the one-rank remainder
    ([24, 22, 5, 4], 12),    # M 528, K 20: three row tiles, the last partial; three matrix-core steps
    ([8, 6, 40, 30], 16),    # M 48, K 1200: 75 column blocks, several k-chunks; four steps
    ([6, 4, 4, 3, 7], 20),   # M 24, K 84: order 5, a three-mode column group to fold; eight steps held
    ([16, 9, 11], 32),       # M 16, K 99: the largest fused R
    ([7, 6, 5], 3),          # M 7: odd, the general route on F32 / F64 too
    ([12, 10, 9], 33),       # R above 32: general route
    ([20, 18, 17], 70),      # R above 64: general route, any-rank kernel; leverages refused
    ([12, 10, 9, 7], 13),    # three matrix-core steps and the one-rank remainder
    ([8, 100, 90], 5),       # M 8, K 9000: more than 64 k-chunks on either route, the two-level row fold
]
# under a cap of one byte: one row tile by one k-chunk a slab — by one GROUP of chunks at [8, 100, 90]
SLAB_SHAPES = [([24, 22, 5, 4], 12), ([8, 6, 40, 30], 16), ([8, 100, 90], 5)]
# leverages: well-conditioned factors need R <= s_i (uniform(0,1) columns, cond(W^T W) ~ 1e3)
LEV_SHAPES = [([8, 6, 5], 3), ([20, 18, 17], 10), ([12, 10, 9, 7], 5), ([6, 4, 4, 3, 7], 3), ([96, 80, 72], 48)]
PLANT_LENS, PLANT_RANK, PLANT_AT = [12, 10, 9, 7], 9, [7, 2, 8, 4]


def ident(v):
    if isinstance(v, (list, tuple)):
        return "x".join(map(str, v))
    return {F32: "F32", F64: "F64", BF16: "BF16"}.get(v, str(v)) if isinstance(v, int) else str(v)


@contextlib.contextmanager
def work_cap(nbytes):
    """sessions created inside read PPALS_TEST_SLICE_WORK_BYTES = nbytes (None: the product's 256 MB)"""
    old = os.environ.pop("PPALS_TEST_SLICE_WORK_BYTES", None)
    if nbytes is not None:
        os.environ["PPALS_TEST_SLICE_WORK_BYTES"] = str(nbytes)
    try:
        yield
    finally:
        os.environ.pop("PPALS_TEST_SLICE_WORK_BYTES", None)
        if old is not None:
            os.environ["PPALS_TEST_SLICE_WORK_BYTES"] = old


def session(pp, ctx, t, Ws, nonneg=False, schedule=None, cap=None):
    with work_cap(cap):
        s = pp.CP(ctx, t, Ws[0].shape[1])
    if schedule:
        s.set_schedule(schedule)
    if nonneg:
        s.set_nonneg(True)
    s.set_factors(Ws)
    return s


def _same(a, b):
    return len(a) == len(b) and all(bf16_util.same_values(x, y) for x, y in zip(a, b))


def reference(pp, ctx, lens, rank, dtype, cap=None, seed=3):
    """checks 1 and 2 (and the two-calls half of 6): ss and total against numpy on the downloaded tensor,
    every mode's sum against total, total against residual()**2; returns (ss, total)"""
    t = pp.Tensor(ctx, lens, dtype).fill_uniform(seed)
    Ws = pp.init_factors(lens, rank, seed + 10)
    s = session(pp, ctx, t, Ws, cap=cap)
    ss, total = s.slice_residuals(return_total=True)
    what = f"{ident(lens)} R={rank} {ident(dtype)}" + (f" cap {cap}" if cap is not None else "")
    R.check_sums(what, ss, total, t.download(), Ws)
    res2 = s.residual() ** 2
    print(f"[slices] {what}: total {total:.17g} residual()^2 {res2:.17g} relative {abs(total - res2) / res2:.3e} "
          f"(bar {R.RESIDUAL_RTOL:.0e})")
    assert abs(total - res2) <= R.RESIDUAL_RTOL * res2
    again, total2 = s.slice_residuals(return_total=True)
    assert _same(ss, again) and bf16_util.same_values([total], [total2]), "two calls, different bits"
    assert _same(ss, s.slice_residuals())
    s.close()
    t.close()
    return ss, total


def planted(pp, ctx):
    """check 3: 10 added to one slice of every mode — each mode's argmax is the planted index"""
    lens = PLANT_LENS
    t = pp.Tensor(ctx, lens, F64).fill_uniform(5)
    V = t.download()
    for i, x in enumerate(PLANT_AT):
        idx = [slice(None)] * len(lens)
        idx[i] = x
        V[tuple(idx)] += 10.0
    t.upload(V)
    Ws = pp.init_factors(lens, PLANT_RANK, 17)
    s = session(pp, ctx, t, Ws)
    ss, total = s.slice_residuals(return_total=True)
    R.check_sums("planted slices", ss, total, V, Ws)
    assert [int(np.argmax(a)) for a in ss] == PLANT_AT, [int(np.argmax(a)) for a in ss]
    s.close()
    t.close()


def exact_fit(pp, ctx, lens, rank):
    """check 4: V = [[W]] of the session's own factors, F64 storage: every entry <= 1e-24 ||V||^2"""
    Ws = pp.init_factors(lens, rank, 29)
    t = pp.Tensor(ctx, lens, F64).fill_cp(Ws)
    s = session(pp, ctx, t, Ws)
    ss, total = s.slice_residuals(return_total=True)
    bar = 1e-24 * t.norm() ** 2
    worst = max(float(np.max(a)) for a in ss)
    print(f"[slices] exact fit {ident(lens)} R={rank}: largest entry {worst:.3e} total {total:.3e} bar {bar:.3e}")
    assert all(np.all(a >= 0.0) for a in ss) and worst <= bar and 0.0 <= total <= bar
    s.close()
    t.close()


def _check_lev(what, lev, Ws):
    ref = R.leverages(Ws)
    rank = Ws[0].shape[1]
    err = max(float(np.max(np.abs(a - b))) for a, b in zip(lev, ref))
    lo, hi = min(float(a.min()) for a in lev), max(float(a.max()) for a in lev)
    sums = [float(a.sum()) for a in lev]
    print(f"[slices] leverages {what}: against pinv {err:.3e} (bar {R.LEV_ATOL:.0e}), range [{lo:.3g}, {hi:.3g}], "
          f"sums - R {[f'{x - rank:.1e}' for x in sums]}")
    assert [a.shape for a in lev] == [b.shape for b in ref]
    assert err <= R.LEV_ATOL and lo >= -1e-12 and hi <= 1.0 + 1e-12
    assert all(abs(x - rank) <= 1e-9 for x in sums)


def leverages(pp, ctx, lens, rank, dtype):
    """check 5, first half: against diag(W pinv(W)), in [0, 1], summing to R; the same bits twice"""
    t = pp.Tensor(ctx, lens, dtype)
    Ws = pp.init_factors(lens, rank, 41)
    s = session(pp, ctx, t, Ws)
    lev = s.leverages()
    _check_lev(f"{ident(lens)} R={rank} {ident(dtype)}", lev, Ws)
    assert _same(lev, s.leverages())
    s.close()
    t.close()


def leverages_after_sweeps(pp, ctx, dtype, nonneg=False):
    lens, rank = [12, 10, 9, 7], 3
    t = pp.Tensor(ctx, lens, dtype).fill_uniform(7)
    s = session(pp, ctx, t, pp.init_factors(lens, rank, 43), nonneg=nonneg)
    s.sweeps_dt(3)
    _check_lev(f"after 3 sweeps {ident(dtype)}" + (" nonneg" if nonneg else ""), s.leverages(), s.get_factors())
    s.close()
    t.close()


def leverages_nan_rule(pp, ctx, dtype):
    """a zero column in ONE factor: NaN in every entry of every mode, PPALS_OK all the same"""
    lens, rank = [8, 6, 5], 3
    t = pp.Tensor(ctx, lens, dtype)
    Ws = pp.init_factors(lens, rank, 47)
    Ws[1][:, 2] = 0.0
    s = session(pp, ctx, t, Ws)
    out = np.full(sum(lens), -1.0)
    assert pp.lib().ppals_cp_leverages(s._h, pp._dp(out)) == 0
    assert np.all(np.isnan(out)), out
    s.close()
    t.close()


def rank_70(pp, ctx, dtype):
    """R = 70: the sums work (general route), the leverages are refused by name"""
    lens = [20, 18, 17]
    t = pp.Tensor(ctx, lens, dtype).fill_uniform(3)
    s = session(pp, ctx, t, pp.init_factors(lens, 70, 13))
    out = np.zeros(sum(lens))
    assert pp.lib().ppals_cp_leverages(s._h, pp._dp(out)) == -5
    err = pp.lib().ppals_last_error().decode()
    assert err.startswith("ppals_cp_leverages: ") and "64" in err, err
    assert pp.lib().ppals_cp_slice_residuals(s._h, pp._dp(out), None) == 0   # total may be NULL
    s.close()
    t.close()


def read_only(pp, ctx, dtype, schedule, nonneg=False, seed=51):
    """check 6: sweeps(2), both calls, sweeps(2) against a twin that never made the calls — factors,
    gradients and gradnorm bit for bit; the tensor bit for bit across the calls"""
    lens, rank = [12, 10, 9, 7], 4
    t = pp.Tensor(ctx, lens, dtype).fill_uniform(seed)
    before = t.download()
    out = []
    for call in (True, False):
        s = session(pp, ctx, t, pp.init_factors(lens, rank, seed + 1), nonneg=nonneg, schedule=schedule)
        s.sweeps_dt(2)
        if call:
            ss, lev = s.slice_residuals(), s.leverages()
            assert _same(ss, s.slice_residuals()) and _same(lev, s.leverages())
            assert bf16_util.same_values(before, t.download()), "the tensor changed"
        s.sweeps_dt(2)
        W, G = s.get_factors(with_grad=True)
        out.append((W, G, s.gradnorm()))
        s.close()
    assert _same(out[0][0], out[1][0]), "the factors differ after the influence plot"
    assert _same(out[0][1], out[1][1]), "the gradients differ after the influence plot"
    assert bf16_util.same_values([out[0][2]], [out[1][2]]), "gradnorm differs after the influence plot"
    t.close()


def refusals(pp, ctx):
    """check 9, the NULL half: PPALS_ERR_ARG, the message starting with the function's name"""
    L = pp.lib()
    lens = [8, 6, 5]
    t = pp.Tensor(ctx, lens, F64).fill_uniform(1)
    s = session(pp, ctx, t, pp.init_factors(lens, 3, 1))
    out = np.zeros(sum(lens))
    tot = C.c_double(0)
    for fn, call in (("ppals_cp_slice_residuals", lambda h, o: L.ppals_cp_slice_residuals(h, o, C.byref(tot))),
                     ("ppals_cp_leverages", lambda h, o: L.ppals_cp_leverages(h, o))):
        assert call(None, pp._dp(out)) == -3
        assert L.ppals_last_error().decode().startswith(fn + ": ")
        assert call(s._h, None) == -3
        assert L.ppals_last_error().decode().startswith(fn + ": ")
        assert call(s._h, pp._dp(out)) == 0
    s.close()
    t.close()


def binding(pp, ctx):
    """check 10"""
    lens = [6, 4, 4, 3, 7]
    t = pp.Tensor(ctx, lens, F32).fill_uniform(2)
    s = session(pp, ctx, t, pp.init_factors(lens, 3, 9))
    ss, lev = s.slice_residuals(), s.leverages()
    both = s.slice_residuals(return_total=True)
    assert isinstance(ss, list) and isinstance(lev, list) and isinstance(both, tuple) and isinstance(both[1], float)
    assert [a.shape for a in ss] == [(n,) for n in lens] == [a.shape for a in lev]
    assert all(a.dtype == np.float64 for a in ss + lev)
    assert "ppals_cp_slice_residuals" in pp.EXPORTS and "ppals_cp_leverages" in pp.EXPORTS
    s.close()
    t.close()
