"""The influence plot of a Tucker session (ppals_tucker_slice_residuals, ppals_tucker_leverages) in numpy,
fp64, on V as Tensor.download() returns it (the stored fp32 / fp64 values, widened exactly) — the reference of
tests/test_tucker_slices_hostsim.py and tests/test_gpu_tucker_slices.py — and the bars those tests hold the
library to.

    ss_i[x]  = sum over the slice x of mode i of (V - core x_j W_j)^2     (tucker_model below, that of model_export_cases.py)
    lev_i[x] = (W_i pinv(W_i))[x, x]

The bars are those of tests/slices_ref.py, for its reason: the sums are of non-negative fp64 terms whose dot
products have at most a few hundred terms, so the relative error of a sum stays far below 1e-9 whatever the
summation order, while one dropped or doubled element moves an entry by at least 1 / (elements in the slice),
which is at least 7e-4 in the shapes of tests/tucker_slices_cases.py. Checked on the CPU at (130, 9, 11), ranks
(112, 4, 2): two summation and contraction orders of this reference agree to 2.7e-15, and the Cholesky-QR
leverages of 130 x 112 standard-normal factors (cond(W^T W) about 460) agree with pinv to 1.9e-15."""
import numpy as np

SS_RTOL = 1e-9
SUM_RTOL = 1e-12       # every mode's ss_i sums to total
RESIDUAL_RTOL = 1e-10  # total against residual()**2: two summation orders
LEV_ATOL = 1e-10


def tucker_model(W, core, absolute=False):
    """core x_0 W_0 ... x_{N-1} W_{N-1} (absolute: of |core| and |W_i|): tucker_model of model_export_cases.py,
    restated because that module imports torch, which must not be loaded into a process that already holds a
    HIP runtime (the pytest process of the stand-in tests); the GPU cases check that the two agree"""
    out = np.abs(core) if absolute else core
    for i, w in enumerate(W):
        out = np.moveaxis(np.tensordot(np.abs(w) if absolute else w, out, axes=([1], [i])), 0, i)
    return out


def slice_sums(V, W, core):
    """(list of the N vectors ss_i, total)"""
    E2 = (np.asarray(V, dtype=np.float64) - tucker_model(W, core)) ** 2
    N = E2.ndim
    return [E2.sum(axis=tuple(a for a in range(N) if a != i)) for i in range(N)], float(E2.sum())


def leverages(W):
    return [np.diag(w @ np.linalg.pinv(w)).copy() for w in W]


def sums_errors(ss, total, ref, tot):
    """(worst relative entry error, relative error of the total, worst mode sum against total)"""
    assert len(ss) == len(ref)
    worst = 0.0
    for i, (a, b) in enumerate(zip(ss, ref)):
        assert a.shape == b.shape, (i, a.shape, b.shape)
        worst = max(worst, float(np.max(np.abs(a - b) / b)))
    return worst, abs(total - tot) / tot, max(abs(float(np.sum(a)) - total) / total for a in ss)


def check_sums(what, ss, total, V, W, core, ref=None):
    """the library's figures beside the reference's, each printed before it is asserted; returns the worst
    relative entry error"""
    ref, tot = ref if ref is not None else slice_sums(V, W, core)
    worst, terr, sums = sums_errors(ss, total, ref, tot)
    print(f"[tucker slices] {what}: worst relative entry error {worst:.3e} (bar {SS_RTOL:.0e}), total {terr:.3e}, "
          f"mode sums against total {sums:.3e} (bar {SUM_RTOL:.0e})", flush=True)
    assert all(np.all(np.isfinite(a)) for a in ss) and worst <= SS_RTOL and terr <= SS_RTOL, what
    assert sums <= SUM_RTOL, what
    return worst


def check_leverages(what, lev, W):
    ref = leverages(W)
    assert [a.shape for a in lev] == [b.shape for b in ref]
    err = max(float(np.max(np.abs(a - b))) for a, b in zip(lev, ref))
    print(f"[tucker slices] leverages {what}: against pinv {err:.3e} (bar {LEV_ATOL:.0e})", flush=True)
    assert err <= LEV_ATOL, what
    return err
