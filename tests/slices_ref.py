"""The influence plot (ppals_cp_slice_residuals, ppals_cp_leverages) in numpy, fp64, on V as
Tensor.download() returns it (the stored bf16 / fp32 / fp64 values, widened exactly) — the reference of
tests/test_slices_hostsim.py and tests/test_gpu_slices.py — and the bars those tests hold the library to.

    ss_i[x]  = sum over the slice x of mode i of (V - [[W_0..W_{N-1}]])^2
    lev_i[x] = (W_i pinv(W_i))[x, x]

Bar of the sums: relative 1e-9 per entry. They are sums of non-negative fp64 terms, at most 1.2e5 a slice in
the shapes of tests/slices_cases.py; a term carries a few ulps from an R-term fp64 dot product, R <= 70, so
the relative error of a sum stays below 1e-12 whatever the summation order. One misplaced, dropped or doubled
element (every residual element here is O(1)) changes an entry by about 1 / (elements in the slice) >= 1e-5:
four orders of magnitude above the bar.
Bar of the leverages: 1e-10 absolute against numpy's pinv, for the well-conditioned factors of the cases
(uniform(0,1), R <= s_i: cond(W^T W) ~ 1e3, so an inverse is good to ~1e-13)."""
import numpy as np

SS_RTOL = 1e-9
SUM_RTOL = 1e-12       # every mode's ss_i sums to total
RESIDUAL_RTOL = 1e-10  # total against residual()**2: two summation orders
LEV_ATOL = 1e-10


def model(Ws):
    """[[W_0..W_{N-1}]] as an array of shape lens"""
    N = len(Ws)
    letters = "abcdefgh"[:N]
    return np.einsum(",".join(l + "z" for l in letters) + "->" + letters, *Ws)


def slice_sums(V, Ws):
    """(list of the N vectors ss_i, total)"""
    E2 = (np.asarray(V, dtype=np.float64) - model(Ws)) ** 2
    N = E2.ndim
    return [E2.sum(axis=tuple(a for a in range(N) if a != i)) for i in range(N)], float(E2.sum())


def leverages(Ws):
    return [np.diag(W @ np.linalg.pinv(W)).copy() for W in Ws]


def check_sums(what, ss, total, V, Ws):
    """the library's figures beside the reference's, each printed before it is asserted"""
    ref, tot = slice_sums(V, Ws)
    assert len(ss) == len(ref)
    worst = 0.0
    for i, (a, b) in enumerate(zip(ss, ref)):
        assert a.shape == b.shape, (what, i, a.shape, b.shape)
        worst = max(worst, float(np.max(np.abs(a - b) / b)))
    terr = abs(total - tot) / tot
    sums = max(abs(float(np.sum(a)) - total) / total for a in ss)
    print(f"[slices] {what}: worst relative entry error {worst:.3e} (bar {SS_RTOL:.0e}), total {terr:.3e}, "
          f"mode sums against total {sums:.3e} (bar {SUM_RTOL:.0e})")
    assert all(np.all(np.isfinite(a)) for a in ss) and worst <= SS_RTOL and terr <= SS_RTOL, what
    assert sums <= SUM_RTOL, what
    return ref, tot
