"""Cases, references and bars of N-PLS regression (ppals_npls_fit / _predict, ppals_tensor_contract_mode /
_slice_inner, ppals.NPLS), shared by tests/test_gpu_npls.py (the HIP kernels of kernels_npls.hip.h, through
`import ppals`) and tests/test_npls_hostsim.py (the fp64 host twins of ops.h, through hostsim_util.load()).

The tensor is viewed as [L, I, T] around the sample mode, first index fastest.

The two tensor passes, against numpy long double on V0 = Tensor.download(), u = 2^-53, bars derived, not tuned, and
valid for any order of summation:
* contract:    |Z - ref| <= (I + 1) u sum_i |x| |U|;
* slice_inner: |S - ref| <= (L T + 1) u sum_{l,t} |x| |W|.
C is 1, 3 and NPLS_CW + 1 = 5 (a launch carries NPLS_CW = 4 columns); column c of a multi-column call has the bits of
that column alone, and two calls give the same bits.

The route rule of hip_ops.hip (npls_contract_chunk / npls_si_chunk), restated in route() from DESIGN.md §3, never
copied from a run; every route has a shape:
* contract: L < 64 and L I size <= 32 KiB: `runs` (U in LDS while 4 I doubles fit 16 KiB, I <= 512: [1000, 4] is
  beyond); beyond the run buffer `long` for L == 1; everything else `rows`, vec = (L % VEC == 0), VEC = 4, 2, 4 for
  f32, f64, bf16 (the tensor's base is aligned), i split over the grid where L T gives fewer than 4 blocks a CU and
  I >= 64 ([3, 12000, 2] mode 1 is split, [20000, 3] mode 1 is not);
* slice_inner: L < 64: `flat`; else `rows`, vec = (L % V16 == 0), V16 = 4, 2, 8, four slices a block ([67, 5, 3] and [20000, 3] mode 1 end in a
  partial group; the latter, T = 1, also splits l over the blocks).

Fit and predict, against tests/npls_ref.py (the deflating algorithm of the paper) on the values as stored. The bar on
T, U, the weights, Q, B, Yhat, ssx and ssy is relative to the largest magnitude of the reference array. Measured: the
largest deviation of the host stand-in from npls_ref over FIT_CASES (F64 and F32 storage) on the development machine
is 5.3e-13 (the weights of 12x7x5, M = 1, where npls_ref takes the SVD and the engine power iterations that stop
at 1e-12); the bar is ten times that, BAR = 5.3e-12, and the GPU test uses the same. (The GPU sums in another
order, and the power iterations amplify a perturbation by about 1 / (1 - sigma_2 / sigma_1).)
"""
import numpy as np

import npls_ref

U = 2.0 ** -53
LD = np.longdouble
F32, F64, BF16 = 0, 1, 3
DTNAME = {F32: "f32", F64: "f64", BF16: "bf16"}
SIZE = {F32: 4, F64: 8, BF16: 2}
ROWS_VEC = {F32: 4, F64: 2, BF16: 4}
VEC16 = {F32: 4, F64: 2, BF16: 8}
NPLS_CW = 4
COLUMNS = (1, 3, NPLS_CW + 1)
BAR = 5.3e-12
ERR_ARG, ERR_UNSUPPORTED = -3, -5

SHAPES = [
    [7, 6, 5],          # everything odd
    [40, 30],           # order 2
    [3, 128, 16, 9],    # L = 3 behind mode 0
    [33, 20, 12],       # unaligned rows
    [5, 1, 4],          # I = 1
    [256, 17, 3],       # a vector tile, and the last mode at T = 1
    [20000, 3],         # L == 1 and a sample beyond the run buffer (all three storage types); L = 20000 rows
    [3, 12000, 2],      # L = 3 and one t beyond the run buffer: scalar rows
    [67, 5, 3],         # L = 67: rows that no vector divides
    [1000, 4],          # L == 1, runs with I = 1000: U beyond the 16 KiB that the runs kernel keeps in LDS
]


def ljt(lens, mode):
    return int(np.prod(lens[:mode], dtype=np.int64)), lens[mode], int(np.prod(lens[mode + 1:], dtype=np.int64))


def route(op, dt, lens, mode):
    L, I, _ = ljt(lens, mode)
    if op == "contract":
        if L < 64 and L * I * SIZE[dt] <= 32 * 1024:
            return "runs"
        if L == 1:
            return "long"
        return f"rows vec={int(L % ROWS_VEC[dt] == 0)}"
    if L < 64:
        return "flat"
    return f"rows vec={int(L % VEC16[dt] == 0)}"


ALL_ROUTES = {"contract": {"runs", "long", "rows vec=0", "rows vec=1"}, "slice_inner": {"flat", "rows vec=0", "rows vec=1"}}
ROUTES = {(op, DTNAME[dt], tuple(lens), mode): route(op, dt, lens, mode)
          for op in ALL_ROUTES for dt in (F32, F64, BF16) for lens in SHAPES for mode in range(len(lens))}
assert ROUTES[("contract", "f32", (3, 128, 16, 9), 1)] == "runs" and ROUTES[("contract", "bf16", (20000, 3), 0)] == "long"
assert ROUTES[("contract", "f32", (3, 12000, 2), 1)] == "rows vec=0" and ROUTES[("contract", "f32", (256, 17, 3), 1)] == "rows vec=1"
assert ROUTES[("slice_inner", "f32", (3, 128, 16, 9), 1)] == "flat" and ROUTES[("slice_inner", "f64", (67, 5, 3), 1)] == "rows vec=0"
assert ROUTES[("slice_inner", "bf16", (256, 17, 3), 1)] == "rows vec=1"


def routes_by_dtype(op, dt):
    return {v for (o, d, _, _), v in ROUTES.items() if o == op and d == DTNAME[dt]}


_DATA = {}


def data(lens, seed=0):
    key = (tuple(lens), seed)
    if key not in _DATA:
        rng = np.random.default_rng(4321 + seed + sum(lens))
        x = np.asfortranarray(rng.standard_normal(lens) + 0.25)
        x.setflags(write=False)
        _DATA[key] = x
    return _DATA[key]


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def fbits(a):
    """the bytes in memory order, first index fastest"""
    return np.asarray(a).ravel(order="F").tobytes()


def within(what, got, ref, bar):
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert not np.any(np.isnan(got)), f"{what}: {int(np.sum(np.isnan(got)))} results are NaN"
    err = np.abs(got.astype(LD) - ref)
    ratio = float(np.max(np.where(err == 0, LD(0), err / np.maximum(bar, LD(np.finfo(np.float64).tiny))))) if err.size else 0.0
    print(f"{what}: max err/bar {ratio:.3g}")
    bad = np.argwhere(err > bar)
    assert bad.size == 0, f"{what}: {len(bad)} elements over the bar, first at {tuple(bad[0])}: err/bar up to {ratio:.3g}"


_REFS = {}


def op_refs(V0, lens, mode, C):
    """long-double references and bars of both passes, computed once per (tensor bits, mode, C)"""
    key = (bits(V0), tuple(lens), mode, C)
    if key not in _REFS:
        L, I, T = ljt(lens, mode)
        rng = np.random.default_rng(99 + mode + 7 * C)
        Um = np.asfortranarray(rng.standard_normal((I, C)))
        Wm = np.asfortranarray(rng.standard_normal((L * T, C)))
        X2 = np.moveaxis(V0, mode, 0).reshape(I, L * T, order="F").astype(LD)  # I x (l + L t)
        Zref = X2.T @ Um.astype(LD)
        Zbar = (I + 1) * U * (np.abs(X2).T @ np.abs(Um).astype(LD))
        Sref = X2 @ Wm.astype(LD)
        Sbar = (L * T + 1) * U * (np.abs(X2) @ np.abs(Wm).astype(LD))
        _REFS[key] = (Um, Wm, Zref, Zbar, Sref, Sbar)
    return _REFS[key]


def check_ops(pp, ctx, lens, dt, mode):
    """the two passes at every C: the reference, column c alone, two calls, the tensor untouched"""
    L, I, T = ljt(lens, mode)
    t = pp.Tensor(ctx, lens, dt).upload(data(lens))
    V0 = t.download()
    for C in COLUMNS:
        what = f"{DTNAME[dt]} {lens} mode {mode} C={C}"
        Um, Wm, Zref, Zbar, Sref, Sbar = op_refs(V0, lens, mode, C)
        Z = t.contract_mode(mode, Um).reshape(L * T, C, order="F")
        within(f"contract {what} [{route('contract', dt, lens, mode)}]", Z, Zref, Zbar)
        S = t.slice_inner(mode, Wm)
        within(f"slice_inner {what} [{route('slice_inner', dt, lens, mode)}]", S, Sref, Sbar)
        assert fbits(t.contract_mode(mode, Um)) == fbits(Z) and fbits(t.slice_inner(mode, Wm)) == fbits(S), f"{what}: two calls differ in bits"
        if C > 1:
            for c in range(C):
                assert fbits(t.contract_mode(mode, Um[:, c])) == fbits(Z[:, c]), f"contract {what}: column {c} alone has other bits"
                assert fbits(t.slice_inner(mode, Wm[:, c])) == fbits(S[:, c]), f"slice_inner {what}: column {c} alone has other bits"
    assert bits(t.download()) == bits(V0), "the tensor changed"
    t.close()


# ------------------------------------------------------------------------------------------ fit and predict
def planted(lens, M, seed, noise=0.05, rank=4, extra=0):
    """(X, Y, Xnew): a rank-4 tensor plus 5 % noise with the samples in mode 0, Y from the sample-mode factor, both
    centred over the samples; Xnew: `extra` more samples of the same model, centred with the training means"""
    rng = np.random.default_rng(seed)
    n = lens[0] + extra
    A = rng.standard_normal((n, rank))
    fs = [A] + [rng.standard_normal((k, rank)) for k in lens[1:]]
    letters = "abcdefg"[:len(lens)]
    X = np.einsum(",".join(c + "r" for c in letters) + "->" + letters, *fs)
    X = X + noise * np.std(X) * rng.standard_normal(X.shape)
    Y = A @ rng.standard_normal((rank, M))
    Y = Y + noise * np.std(Y) * rng.standard_normal(Y.shape)
    mx, my = X[:lens[0]].mean(axis=0, keepdims=True), Y[:lens[0]].mean(axis=0, keepdims=True)
    X, Y = X - mx, Y - my
    return np.asfortranarray(X[:lens[0]]), np.asfortranarray(Y[:lens[0]]), np.asfortranarray(X[lens[0]:])


# (name, lens with the samples first, M, F, sample mode first / last)
FIT_CASES = [(f"{'x'.join(map(str, lens))}-M{M}-{'first' if first else 'last'}", lens, M, F, first)
             for lens, M, F in (([12, 7, 5], 1, 3), ([12, 7, 5], 2, 3), ([10, 4, 5, 3], 1, 2), ([10, 4, 5, 3], 3, 2),
                                ([15, 9], 2, 3))
             for first in (True, False) if first or len(lens) > 2] + [("15x9-M2-last", [15, 9], 2, 3, False)]
NEW_SAMPLES = 5


def fit_inputs(case):
    """(X, Y, Xnew, mode): the sample mode moved last where the case says so"""
    name, lens, M, F, first = case
    X, Y, Xnew = planted(lens, M, seed=1000 + 13 * len(lens) + M, extra=NEW_SAMPLES)
    if first:
        return X, Y, Xnew, 0
    return np.asfortranarray(np.moveaxis(X, 0, -1)), Y, np.asfortranarray(np.moveaxis(Xnew, 0, -1)), len(lens) - 1


def deviation(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.all(np.isfinite(got))
    return float(np.max(np.abs(got - ref)) / np.max(np.abs(ref))) if ref.size else 0.0


def model_deviation(m, ref, what=""):
    """the largest relative deviation of a fitted ppals.NPLS from the npls_ref dict"""
    parts = {"T": (m.scores, ref["T"]), "U": (m.y_scores, ref["U"]), "Q": (m.y_loadings, ref["Q"]),
             "B": (m.inner, ref["B"]), "ssx": (m.ssx, ref["ssx"]), "ssy": (m.ssy, ref["ssy"])}
    for k, (a, b) in enumerate(zip(m.weights, ref["W"])):
        parts[f"W{k}"] = (a, b)
    dev = {k: deviation(a, b) for k, (a, b) in parts.items()}
    print(f"{what}: deviation from npls_ref " + " ".join(f"{k} {v:.2e}" for k, v in dev.items()))
    return max(dev.values())


def check_fit(pp, ctx, case, dt):
    """fit and the three prediction checks; returns the largest relative deviation seen (asserted <= BAR)"""
    name, lens, M, F, first = case
    X, Y, Xnew, mode = fit_inputs(case)
    t = pp.Tensor(ctx, list(X.shape), dt).upload(X)
    V0 = t.download()
    ref = npls_ref.fit(V0, Y, F, mode)
    m = pp.NPLS().fit(t, Y, F, mode)
    assert m.ncomp == F == ref["T"].shape[1]
    assert not np.any(m.status) and not np.any(ref["status"]), (m.status, ref["status"])
    for w in m.weights:
        assert np.max(np.abs(np.sum(w * w, axis=0) - 1)) < 1e-14
    worst = model_deviation(m, ref, f"{name} {DTNAME[dt]}")
    # predict on the training tensor: the fit's own T and Y - Y_res
    Yhat, Tn = m.predict(t, return_scores=True)
    worst = max(worst, deviation(Tn, m.scores), deviation(Yhat, Y - ref["Yres"]))
    # predict(ncomp = k) is a fit with F = k
    for k in range(1, F):
        mk = pp.NPLS().fit(t, Y, k, mode)
        worst = max(worst, deviation(m.predict(t, ncomp=k), mk.predict(t)), deviation(mk.scores, m.scores[:, :k]),
                    deviation(mk.inner, m.inner[:k, :k]))
        mk.close()
    # other samples
    tn = pp.Tensor(ctx, list(Xnew.shape), dt).upload(Xnew)
    Yn, Tnn = m.predict(tn, return_scores=True)
    rY, rT = npls_ref.predict(ref, tn.download())
    assert Yn.shape == (NEW_SAMPLES, M)
    worst = max(worst, deviation(Yn, rY), deviation(Tnn, rT))
    assert bits(t.download()) == bits(V0), "the fit changed the tensor"
    print(f"{name} {DTNAME[dt]}: largest relative deviation {worst:.3e} (bar {BAR:.1e})")
    for x in (m, t, tn):
        x.close()
    assert worst <= BAR, f"{name} {DTNAME[dt]}: {worst:.3e} > {BAR:.1e}"
    return worst


def check_ends_early(pp, ctx, dt):
    """Y = 0: Z is zero at the first component, the fit ends with none and says so"""
    t = pp.Tensor(ctx, [8, 4, 2], dt).upload(data([8, 4, 2]))
    m = pp.NPLS().fit(t, np.zeros((8, 1)), 3, 0)
    assert m.ncomp == 0 and m.scores.shape == (8, 0) and m.inner.shape == (0, 0) and m.weights[0].shape == (4, 0)
    m.close()
    t.close()


def flat_factors(W, G=None):
    return np.concatenate([w.ravel(order="F") for w in W] + ([g.ravel(order="F") for g in G] if G else []))


def check_cp_session_stays_live(pp, ctx, dt):
    """sweep, fit N-PLS, sweep: the factors of a session that never saw the fit, bit for bit"""
    lens, R = [12, 10, 9], 3
    X, Y, _ = planted(lens, 2, seed=77)
    W0, G0 = pp.init_factors(lens, R, 5), pp.init_factors(lens, R, 99)
    ts = [pp.Tensor(ctx, lens, dt).upload(X) for _ in range(2)]
    ss = [pp.CP(ctx, t, R) for t in ts]
    for s in ss:
        s.set_factors(W0, G0)
        s.sweeps_dt(2)
    m = pp.NPLS().fit(ts[0], Y, 2, 0)
    m.predict(ts[0])
    ts[0].contract_mode(1, np.ones(lens[1]))
    ts[0].slice_inner(2, np.ones((lens[0], lens[1])))
    for s in ss:
        s.sweeps_dt(2)
    a, b = [flat_factors(*s.get_factors(with_grad=True)) for s in ss]
    assert bits(a) == bits(b), "the fit disturbed the live session"
    assert bits(ts[0].download()) == bits(ts[1].download())
    for x in [m] + ss + ts:
        x.close()


def raw_refusals(pp, t, other_order, other_extent, model, lens):
    """(name, call, code, message prefix) of every refusal, straight at the C ABI. t: [9, 8, 7]; model: fitted on t
    with 2 components, mode 0"""
    import ctypes as C
    lib = pp.lib()
    N, h = len(lens), t._h
    dp = C.POINTER(C.c_double)
    Y = np.zeros((lens[0], 2), order="F")
    Y[:, 0] = np.arange(lens[0]) - 4.0
    Y[:, 1] = (np.arange(lens[0]) - 4.0) ** 2 - 6.0
    Ynan, Yinf = Y.copy(order="F"), Y.copy(order="F")
    Ynan[3, 1], Yinf[0, 0] = np.nan, np.inf
    big = np.zeros(int(np.prod(lens)) * 2)
    p, out = big.ctypes.data_as(dp), C.c_void_p()
    d = lambda a: a.ctypes.data_as(dp)
    fit = lambda hh, mode, y, M, F: lib.ppals_npls_fit(hh, mode, y, M, F, None, C.byref(out))
    res = [("fit NULL tensor", lambda: fit(None, 0, d(Y), 2, 2), ERR_ARG, "ppals_npls_fit"),
           ("fit NULL Y", lambda: fit(h, 0, None, 2, 2), ERR_ARG, "ppals_npls_fit"),
           ("fit NULL out", lambda: lib.ppals_npls_fit(h, 0, d(Y), 2, 2, None, None), ERR_ARG, "ppals_npls_fit"),
           ("fit mode -1", lambda: fit(h, -1, d(Y), 2, 2), ERR_ARG, "ppals_npls_fit"),
           ("fit mode N", lambda: fit(h, N, d(Y), 2, 2), ERR_ARG, "ppals_npls_fit"),
           ("fit M 0", lambda: fit(h, 0, d(Y), 0, 2), ERR_ARG, "ppals_npls_fit"),
           ("fit F 0", lambda: fit(h, 0, d(Y), 2, 0), ERR_ARG, "ppals_npls_fit"),
           ("fit F > I", lambda: fit(h, 0, d(Y), 2, lens[0] + 1), ERR_ARG, "ppals_npls_fit"),
           ("fit Y nan", lambda: fit(h, 0, d(Ynan), 2, 2), ERR_ARG, "ppals_npls_fit"),
           ("fit Y inf", lambda: fit(h, 0, d(Yinf), 2, 2), ERR_ARG, "ppals_npls_fit"),
           ("predict NULL model", lambda: lib.ppals_npls_predict(None, h, 1, p, None), ERR_ARG, "ppals_npls_predict"),
           ("predict NULL tensor", lambda: lib.ppals_npls_predict(model._h, None, 1, p, None), ERR_ARG, "ppals_npls_predict"),
           ("predict NULL Yhat", lambda: lib.ppals_npls_predict(model._h, h, 1, None, None), ERR_ARG, "ppals_npls_predict"),
           ("predict ncomp 0", lambda: lib.ppals_npls_predict(model._h, h, 0, p, None), ERR_ARG, "ppals_npls_predict"),
           ("predict ncomp 3", lambda: lib.ppals_npls_predict(model._h, h, 3, p, None), ERR_ARG, "ppals_npls_predict"),
           ("predict other order", lambda: lib.ppals_npls_predict(model._h, other_order._h, 1, p, None), ERR_ARG, "ppals_npls_predict"),
           ("predict other extent", lambda: lib.ppals_npls_predict(model._h, other_extent._h, 1, p, None), ERR_ARG, "ppals_npls_predict"),
           ("get NULL model", lambda: lib.ppals_npls_get(None, 0, p, None), ERR_ARG, "ppals_npls_get"),
           ("get bad array", lambda: lib.ppals_npls_get(model._h, 16 + N - 1, p, None), ERR_ARG, "ppals_npls_get"),
           ("dims NULL model", lambda: lib.ppals_npls_dims(None, None, None, None, None, None, None), ERR_ARG, "ppals_npls_dims")]
    for fn, name in ((lib.ppals_tensor_contract_mode, "ppals_tensor_contract_mode"), (lib.ppals_tensor_slice_inner, "ppals_tensor_slice_inner")):
        res += [(name + " NULL tensor", lambda f=fn: f(None, 0, p, 1, p), ERR_ARG, name),
                (name + " mode -1", lambda f=fn: f(h, -1, p, 1, p), ERR_ARG, name),
                (name + " mode N", lambda f=fn: f(h, N, p, 1, p), ERR_ARG, name),
                (name + " NULL in", lambda f=fn: f(h, 0, None, 1, p), ERR_ARG, name),
                (name + " NULL out", lambda f=fn: f(h, 0, p, 1, None), ERR_ARG, name),
                (name + " C 0", lambda f=fn: f(h, 0, p, 0, p), ERR_ARG, name)]
    res.append(("keep", lambda: (Y, Ynan, Yinf, big) and 0, 0, ""))  # (the arrays above stay alive while the list does)
    return res, out


def check_refusals(pp, ctx, dt):
    """every refusal: code, message prefix, no model handed out, the tensor's bytes, and — nothing was bumped — the
    next sweep of a live session equal to that of an undisturbed twin"""
    import ctypes as C
    lens, R = [9, 8, 7], 3
    X, Y, _ = planted(lens, 2, seed=5)
    W0, G0 = pp.init_factors(lens, R, 5), pp.init_factors(lens, R, 99)
    ts = [pp.Tensor(ctx, lens, dt).upload(X) for _ in range(2)]
    ss = [pp.CP(ctx, t, R) for t in ts]
    for s in ss:
        s.set_factors(W0, G0)
        s.sweeps_dt(1)
    V0 = ts[0].download()
    model = pp.NPLS().fit(ts[0], Y, 2, 0)
    other_order = pp.Tensor(ctx, [9, 56], dt).upload(np.zeros((9, 56)))
    other_extent = pp.Tensor(ctx, [4, 8, 6], dt).upload(np.zeros((4, 8, 6)))
    calls, out = raw_refusals(pp, ts[0], other_order, other_extent, model, lens)
    for name, call, code, prefix in calls:
        rc = call()
        assert rc == code, (name, rc, pp.lib().ppals_last_error())
        if code:
            assert pp.lib().ppals_last_error().decode().startswith(prefix + ": "), (name, pp.lib().ppals_last_error())
            assert not out.value, f"{name}: a model was handed out"
        assert bits(ts[0].download()) == bits(V0), f"{name}: the tensor changed"
    # a dead handle: the context is gone, the tensor object still there; the model lives on without its context
    ctx2 = pp.Context(0)
    dead = pp.Tensor(ctx2, lens, dt).upload(X)
    m2 = pp.NPLS().fit(dead, Y, 1, 0)
    h, dead._h = dead._h, None
    ctx2.close()
    Yf = np.asfortranarray(Y)
    yh = np.zeros((lens[0], 2), order="F")
    dp = C.POINTER(C.c_double)
    assert pp.lib().ppals_npls_fit(h, 0, Yf.ctypes.data_as(dp), 2, 1, None, C.byref(out)) == ERR_ARG
    assert pp.lib().ppals_last_error().decode().startswith("ppals_npls_fit: ")
    assert pp.lib().ppals_npls_predict(m2._h, h, 1, yh.ctypes.data_as(dp), None) == ERR_ARG
    assert pp.lib().ppals_last_error().decode().startswith("ppals_npls_predict: ")
    assert m2.scores.shape == (lens[0], 1) and m2.predict(ts[0]).shape == (lens[0], 2)
    pp.lib().ppals_tensor_destroy(h)
    for s in ss:
        s.sweeps_dt(1)
    a, b = [flat_factors(*s.get_factors(with_grad=True)) for s in ss]
    assert bits(a) == bits(b), "a refused call disturbed the live session"
    for x in [model, m2, other_order, other_extent] + ss + ts:
        x.close()


# ------------------------------------------------------------------------------------------ the case that needs torch
# `python npls_cases.py torch` (tests/test_gpu_npls.py): torch is imported BEFORE the binding loads libppals, so that
# both share one HIP runtime.
def torch_fit(torch, pp):
    """Y as a device tensor, X imported from a strided torch view; against the same fit from numpy inputs"""
    ctx = pp.Context(0)
    case = FIT_CASES[1]
    X, Y, Xnew, mode = fit_inputs(case)
    big = torch.zeros([2 * n for n in X.shape], dtype=torch.float64, device="cuda:0")
    view = big[::2, 1::2, ::2]
    view.copy_(torch.from_numpy(np.ascontiguousarray(X)).to("cuda:0"))
    assert not view.is_contiguous()
    t = pp.Tensor.from_torch(ctx, view)
    t2 = pp.Tensor(ctx, list(X.shape), F64).upload(X)
    assert bits(t.download()) == bits(t2.download())
    Yd = torch.from_numpy(np.ascontiguousarray(Y)).to("cuda:0")
    m, m2 = pp.npls(t, Yd, case[3], mode), pp.npls(t2, Y, case[3], mode)
    assert bits(m.scores) == bits(m2.scores) and bits(m.inner) == bits(m2.inner)
    ref = npls_ref.fit(t.download(), Y, case[3], mode)
    assert model_deviation(m, ref, "torch inputs") <= BAR
    tn = pp.Tensor.from_torch(ctx, torch.from_numpy(np.ascontiguousarray(Xnew)).to("cuda:0"))
    assert deviation(m.predict(tn), npls_ref.predict(ref, tn.download())[0]) <= BAR
    for x in (m, m2, t, t2, tn):
        x.close()
    ctx.close()


if __name__ == "__main__":
    import os
    import sys
    import torch  # noqa: I001  (first: see above)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pairwise-perturbation_amd"))
    import ppals
    {"torch": torch_fit}[sys.argv[1]](torch, ppals)
    print(f"npls case {sys.argv[1]}: ok", flush=True)
