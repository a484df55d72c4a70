"""Cases, references and bars of the wide-column tensor passes (ppals_tensor_contract_columns /
_slice_inner_columns; Ops::npls_contract_wide / npls_slice_inner_wide, kernels_npls_wide.hip.h) and of N-PLS
cross-validation (ppals_npls_crossval, ppals.npls_crossval), shared by tests/test_gpu_npls_cv.py (the HIP kernels,
through `import ppals`), tests/test_gpu_npls_wide_routes.py (the ops with their route log, tests/npls_wide_shim) and
tests/test_npls_cv_hostsim.py (the host stand-in, through hostsim_util.load()). It imports npls_cases and npls_ref and
changes neither.

The wide ops, against the numpy long double references and the DERIVED bars of npls_cases.op_refs, which hold for any
order of summation: C in WIDE_COLUMNS (5: above NPLS_CW; 9, 33: the first column counts that slice_inner and contract
send to `wide.rows`, 32 the last that contract does not; 16 / 17, 33, 64 / 65: a tile, a tile and a column, three
tiles, the four tiles of a launch, a second chunk), two calls give equal bits, the tensor is untouched. Equal bits
with the narrow ops are not expected and not asserted.

The route rule of hip_ops.hip (npls_contract_wide / npls_slice_inner_wide), restated in wide_route() from DESIGN.md §3
("Cross-validation"), never copied from a run, a formula on (L, I, T, C) alone; its thresholds are where the wide
routes stopped losing to the narrow chunks in profiles/npls_cv_bench.md:
  L == 1:    `wide.lead` for C > NPLS_CW and I >= 32, both ops;
  L >= 16:   `wide.rows` for C > 32 (contract) and for C > 8 (slice_inner);
  otherwise: `narrow` (the narrow op in its chunks of NPLS_CW).
WIDE_SHAPES are the smallest that reach every boundary (L = 16 exactly with I = 33, a 32-chunk plus one; L = 17, 67,
256, 4352 with T = 1; L = 5 and 3: narrow; L = 1 with I = 40, 1000 and, i split over the grid and folded, 20000;
L = 20000 with I = 3; L = 1 with I = 32 exactly and T = 300, where slice_inner splits t over the blocks, and with
I = 31: narrow); every route name has a shape.

Cross-validation, against cv_ref: per segment, reduce, centre on the training means, npls_ref.fit, npls_ref.predict
for 1 .. F components, add the mean back; the inputs are the values as stored (Tensor.download()). The cases are the
`planted` inputs of npls_cases with X offset by 3 standard deviations and Y by +2, so that a wrong centring cannot
pass. Every fit of the reference and of the engine must settle (status 0), asserted, so no comparison is skipped. Ycv
and press are compared relative to the largest magnitude of the reference. Measured: the largest deviation of the host
stand-in from cv_ref over CV_CASES and the group-split case (F64 and F32 storage) on the development machine is
2.3e-12 (Ycv of 12x7x5, M = 1, leave-one-out, centred, where npls_ref takes the SVD and the engine power iterations
that stop at 1e-12); the bar is ten times that, on the stand-in and on the GPU, the rule npls_cases.BAR follows: the
margin covers another order of summation amplified by the power iterations.

The check that the raw tensor and the tensor after Tensor.center(mode) give the same cross-validation runs on F64
storage: centring in place rounds every element to the storage type, which on F32 or BF16 storage is a different
tensor by 2^-24 or 2^-8 of its values, far above a bar of 1e-11.
"""
import ctypes as C
import math
import os
import subprocess

import numpy as np

import npls_cases as NC
import npls_ref

F32, F64, BF16 = NC.F32, NC.F64, NC.BF16
DTNAME = NC.DTNAME
NPLS_CW = NC.NPLS_CW
WIDE_COLS = 64                     # columns a read of X carries (NPLS_WIDE_COLS, kNplsCvColumns)
WIDE_COLUMNS = (5, 9, 16, 17, 32, 33, 64, 65)
MEASURED = 2.3e-12                 # the host stand-in against cv_ref, see above
CV_BAR = 10 * MEASURED
ERR_ARG, ERR_UNSUPPORTED = NC.ERR_ARG, NC.ERR_UNSUPPORTED

# (lens, mode)
WIDE_SHAPES = [
    ([16, 33, 2], 1),       # L = 16 exactly; I = 33, a 32-chunk plus one
    ([17, 4, 5], 1),        # L = 17
    ([67, 5, 3], 1),        # L = 67
    ([256, 17, 3], 1),      # L = 256
    ([256, 17, 3], 2),      # L = 4352, T = 1
    ([5, 1, 4], 1),         # L = 5, I = 1: narrow
    ([40, 30], 0),          # L = 1
    ([40, 30], 1),          # L = 40
    ([20000, 3], 0),        # L = 1, i split over the grid and folded
    ([20000, 3], 1),        # L = 20000, I = 3, T = 1
    ([1000, 4], 0),         # L = 1
    ([3, 128, 16, 9], 1),   # L = 3: narrow
    ([32, 300], 0),         # L = 1, I = 32 exactly, T = 300: slice_inner splits t over the blocks and folds
    ([31, 70], 0),          # L = 1, I = 31: narrow
]
WIDE_IDS = [f"{'x'.join(map(str, lens))}-m{mode}" for lens, mode in WIDE_SHAPES]


def wide_route(op, lens, mode, Cn):
    L, I, _ = NC.ljt(lens, mode)
    if L == 1:
        return "wide.lead" if Cn > NPLS_CW and I >= 32 else "narrow"
    return "wide.rows" if L >= 16 and Cn > (32 if op == "contract" else 8) else "narrow"


OPS = ("contract", "slice_inner")
ALL_WIDE_ROUTES = {"narrow", "wide.rows", "wide.lead"}
for _op in OPS:
    assert {wide_route(_op, lens, mode, Cn) for lens, mode in WIDE_SHAPES for Cn in WIDE_COLUMNS} == ALL_WIDE_ROUTES
assert wide_route("contract", [16, 33, 2], 1, 32) == "narrow" and wide_route("contract", [16, 33, 2], 1, 33) == "wide.rows"
assert wide_route("slice_inner", [16, 33, 2], 1, 5) == "narrow" and wide_route("slice_inner", [16, 33, 2], 1, 9) == "wide.rows"
assert wide_route("contract", [3, 128, 16, 9], 1, 65) == "narrow" and wide_route("slice_inner", [20000, 3], 1, 4) == "narrow"
assert wide_route("contract", [20000, 3], 0, 5) == "wide.lead" and wide_route("slice_inner", [32, 300], 0, 5) == "wide.lead"
assert wide_route("contract", [31, 70], 0, 65) == "narrow" and wide_route("slice_inner", [31, 70], 0, 65) == "narrow"


def check_wide_ops(pp, ctx, lens, dt, mode):
    """both wide passes at every C: the reference, two calls, the tensor untouched"""
    L, I, T = NC.ljt(lens, mode)
    t = pp.Tensor(ctx, lens, dt).upload(NC.data(lens))
    V0 = t.download()
    for Cn in WIDE_COLUMNS:
        what = f"{DTNAME[dt]} {lens} mode {mode} C={Cn}"
        Um, Wm, Zref, Zbar, Sref, Sbar = NC.op_refs(V0, lens, mode, Cn)
        Z = t.contract_columns(mode, Um).reshape(L * T, Cn, order="F")
        NC.within(f"contract_columns {what} [{wide_route('contract', lens, mode, Cn)}]", Z, Zref, Zbar)
        S = t.slice_inner_columns(mode, Wm)
        NC.within(f"slice_inner_columns {what} [{wide_route('slice_inner', lens, mode, Cn)}]", S, Sref, Sbar)
        assert NC.fbits(t.contract_columns(mode, Um)) == NC.fbits(Z), f"contract_columns {what}: two calls differ in bits"
        assert NC.fbits(t.slice_inner_columns(mode, Wm)) == NC.fbits(S), f"slice_inner_columns {what}: two calls differ in bits"
    assert NC.bits(t.download()) == NC.bits(V0), "the tensor changed"
    t.close()


# ------------------------------------------------------------------------------------------ the ops with their route log
SHIM_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "npls_wide_shim")
GUARD = 16


def load_shim(hostsim=False):
    subprocess.check_call(["make", "-s", "-C", SHIM_DIR] + (["hostsim"] if hostsim else []))
    lib = C.CDLL(os.path.join(SHIM_DIR, "build", "libnpls_wide_shim_hostsim.so" if hostsim else "libnpls_wide_shim.so"))
    lib.npls_wide_shim_error.restype = C.c_char_p
    lib.npls_wide_shim_run.restype = C.c_int
    lib.npls_wide_shim_run.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int,
                                       C.c_void_p, C.c_int64, C.c_char_p, C.c_int]
    return lib


def stored(x, dt):
    """(the storage bytes of x in memory order, the values they hold as fp64)"""
    flat = np.asarray(x, dtype=np.float64).ravel(order="F")
    if dt == F64:
        return flat.copy(), flat.reshape(x.shape, order="F")
    f = flat.astype(np.float32)
    if dt == F32:
        return f, f.astype(np.float64).reshape(x.shape, order="F")
    u = f.view(np.uint32).astype(np.uint64)
    b = ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)  # round to nearest even
    v = (b.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return b, v.reshape(x.shape, order="F")


def shim_call(lib, op, dt, buf, L, I, T, inp, Cn):
    """(the result as a flat array, the route tags); the guards around the result must come back untouched"""
    n = (L * T if op == 0 else I) * Cn
    out = np.full(2 * GUARD + n, -12345.0)
    inp = np.ascontiguousarray(np.asarray(inp, dtype=np.float64).ravel(order="F"))
    route = C.create_string_buffer(4096)
    rc = lib.npls_wide_shim_run(op, dt, buf.ctypes.data, L, I, T, inp.ctypes.data, Cn, out.ctypes.data, GUARD, route, 4096)
    assert rc == 0, lib.npls_wide_shim_error()
    assert np.all(out[:GUARD] == -12345.0) and np.all(out[GUARD + n:] == -12345.0), "a guard was written"
    return out[GUARD:GUARD + n], route.value.decode().split("\n") if route.value else []


def check_wide_routes(lib, lens, mode, dt, logged=True):
    """every C of a shape through the shim: the values under the derived bars, and (logged: the HIP back end) the
    route tags the restated rule names: one `wide.<walk>` tag per chunk of 64 columns and nothing else, or the
    `wide.narrow` tag followed by the narrow op's own"""
    L, I, T = NC.ljt(lens, mode)
    buf, V0 = stored(NC.data(lens), dt)
    for Cn in WIDE_COLUMNS:
        Um, Wm, Zref, Zbar, Sref, Sbar = NC.op_refs(V0, lens, mode, Cn)
        for op, name, inp, ref, bar in ((0, "contract", Um, Zref, Zbar), (1, "slice_inner", Wm, Sref, Sbar)):
            want = wide_route(name, lens, mode, Cn)
            got, tags = shim_call(lib, op, dt, buf, L, I, T, inp, Cn)
            what = f"{name} {DTNAME[dt]} {lens} mode {mode} C={Cn} [{want}]"
            NC.within(what, got.reshape(ref.shape, order="F"), ref, bar)
            if not logged:
                continue
            print("   ", tags)
            head = f"npls.{name}.{DTNAME[dt]}.wide."
            if want == "narrow":
                assert tags[0] == head + "narrow" and len(tags) > 1, (what, tags)
                assert all(t.startswith(f"npls.{name}.{DTNAME[dt]}.") and ".wide." not in t for t in tags[1:]), (what, tags)
            else:
                chunks = [min(WIDE_COLS, Cn - c0) for c0 in range(0, Cn, WIDE_COLS)]
                assert len(tags) == len(chunks), (what, tags)
                for t, nc in zip(tags, chunks):
                    assert t.startswith(head + want.split(".")[1] + " ") and f" nt={(nc + 15) // 16}" in t, (what, tags)
                # T = 3 leaves the contraction short of work, I = 32 the slice inner products
                if (op == 0 and lens == [20000, 3] or op == 1 and lens == [32, 300]) and mode == 0:
                    assert all(int(t.split(" ns=")[1]) > 1 for t in tags), f"{what}: the contracted index was not split: {tags}"


# ------------------------------------------------------------------------------------------ cross-validation
# (name, lens with the samples first, M, F, sample mode first / last, S (0: leave-one-out), center)
CV_CASES = [(f"{'x'.join(map(str, lens))}-M{M}-{'first' if first else 'last'}-S{S or 'I'}-c{center}", lens, M, F, first, S or lens[0], center)
            for lens, M, F in (([12, 7, 5], 1, 3), ([12, 7, 5], 2, 3), ([10, 4, 5, 3], 3, 2), ([15, 9], 2, 3), ([16, 6, 5], 1, 4))
            for first in (True, False) for S in (3, 0) for center in (1, 0)]
GROUP_CASE = ("72x5x4-M1-first-SI-c1", [72, 5, 4], 1, 2, True, 72, 1)   # S M > 64: two groups


def cv_inputs(case):
    """(X, Y, mode, segment labels): planted data, X offset by 3 standard deviations and Y by +2"""
    name, lens, M, F, first, S, center = case
    X, Y, _ = NC.planted(lens, M, seed=2000 + 13 * len(lens) + M + lens[0])
    X = np.asfortranarray(X + 3.0 * np.std(X))
    Y = np.asfortranarray(Y + 2.0)
    seg = np.arange(lens[0]) % S
    if first:
        return X, Y, 0, seg
    return np.asfortranarray(np.moveaxis(X, 0, -1)), Y, len(lens) - 1, seg


def group(lens, mode, M, S):
    """G of DESIGN.md §3: the largest count with G M <= 64 columns and G (M + 2) fp64 slices within 2 GiB"""
    LT = int(np.prod(lens, dtype=np.int64)) // lens[mode]
    return min(max(1, WIDE_COLS // M), max(1, (2 << 30) // (8 * LT * (M + 2))), S)


_CV_REFS = {}


def cv_ref(V0, Y, F, mode, seg, S, center):
    """(Ycv, press) of the per-segment route: reduce, centre on the training means, fit, predict, add the mean back"""
    key = (NC.bits(V0), NC.bits(Y), F, mode, NC.bits(seg), S, center)
    if key not in _CV_REFS:
        Xm = np.moveaxis(np.asarray(V0, dtype=np.float64), mode, 0)
        Y = np.asarray(Y, dtype=np.float64).reshape(Xm.shape[0], -1)
        Ycv = np.zeros(Y.shape + (F,))
        for s in range(S):
            tr = seg != s
            mx = Xm[tr].mean(axis=0, keepdims=True) if center else 0.0
            my = Y[tr].mean(axis=0, keepdims=True) if center else 0.0
            model = npls_ref.fit(Xm[tr] - mx, Y[tr] - my, F, 0)
            assert model["T"].shape[1] == F and not np.any(model["status"]), f"the reference fit without segment {s} did not settle"
            for k in range(1, F + 1):
                Ycv[~tr, :, k - 1] = npls_ref.predict(model, Xm[~tr] - mx, ncomp=k)[0] + my
        press = np.sum((Ycv - Y[:, :, None]) ** 2, axis=0).T   # F x M
        _CV_REFS[key] = (Ycv, press)
    return _CV_REFS[key]


def check_cv(pp, ctx, case, dt):
    """one case: settled, Ycv and press under the bar, the pass count, the record's derived fields, the tensor's bytes;
    returns the largest relative deviation"""
    name, lens, M, F, first, S, center = case
    X, Y, mode, seg = cv_inputs(case)
    t = pp.Tensor(ctx, list(X.shape), dt).upload(X)
    V0 = t.download()
    rYcv, rpress = cv_ref(V0, Y, F, mode, seg, S, center)
    r = pp.npls_crossval(t, Y, F, mode=mode, segments=seg, center=bool(center))
    assert r.Ycv.shape == (lens[0], M, F) and r.press.shape == (F, M) and r.status.shape == (S, F)
    assert np.all(r.fitted == F) and not np.any(r.status), (r.fitted, r.status)
    dev = (NC.deviation(r.Ycv, rYcv), NC.deviation(r.press, rpress))
    print(f"{name} {DTNAME[dt]}: deviation from cv_ref Ycv {dev[0]:.2e} press {dev[1]:.2e} (bar {CV_BAR:.1e})")
    G = group(list(X.shape), mode, M, S)
    assert r.x_passes == 2 * F * math.ceil(S / G), (r.x_passes, F, S, G)
    # (two sums of I squares in different orders: each within (I + 1) u of the exact one)
    assert NC.deviation(r.press, np.sum((r.Ycv - Y[:, :, None]) ** 2, axis=0).T) <= 2 * (lens[0] + 2) * NC.U
    assert NC.bits(r.rmsecv) == NC.bits(np.sqrt(r.press / lens[0]))
    tot = r.press.sum(axis=1)
    assert 1 <= r.best_ncomp <= F and tot[r.best_ncomp - 1] == tot.min() and np.all(tot[:r.best_ncomp - 1] > tot.min())
    # a count of segments gives the same labels through holdout_segments
    if S < lens[0]:
        r2 = pp.npls_crossval(t, Y, F, mode=mode, segments=S, center=bool(center))
        assert NC.bits(r2.segments) == NC.bits(seg.astype(np.int64)) and NC.bits(r2.Ycv) == NC.bits(r.Ycv)
    assert NC.bits(t.download()) == NC.bits(V0), "the cross-validation changed the tensor"
    t.close()
    assert max(dev) <= CV_BAR, f"{name} {DTNAME[dt]}: {max(dev):.3e} > {CV_BAR:.1e}"
    return max(dev)


def check_centered_agrees(pp, ctx, dt=F64):
    """the raw tensor and the same tensor after Tensor.center(mode): the same cross-validation within the bar"""
    case = CV_CASES[0]
    name, lens, M, F, first, S, center = case
    X, Y, mode, seg = cv_inputs(case)
    t = pp.Tensor(ctx, list(X.shape), dt).upload(X)
    a = pp.npls_crossval(t, Y, F, mode=mode, segments=seg, center=True)
    t.center(mode)
    b = pp.npls_crossval(t, Y, F, mode=mode, segments=seg, center=True)
    dev = max(NC.deviation(b.Ycv, a.Ycv), NC.deviation(b.press, a.press))
    print(f"raw against centred tensor: {dev:.2e} (bar {CV_BAR:.1e})")
    t.close()
    assert dev <= CV_BAR, dev


def check_constant_segment(pp, ctx, dt):
    """Y is 2 everywhere but in segment 0: the fit without segment 0 has nothing to explain, ends with no component
    and predicts the training mean; the other fits run"""
    lens, F, S = [9, 4, 3], 2, 3
    X, Y, _ = NC.planted(lens, 1, seed=31)
    seg = np.arange(lens[0]) % S
    Y = np.where((seg == 0)[:, None], Y + 5.0, 2.0)
    t = pp.Tensor(ctx, lens, dt).upload(X + 1.0)
    r = pp.npls_crossval(t, Y, F, segments=seg)
    assert r.fitted[0] == 0 and np.all(r.fitted[1:] == F), r.fitted
    assert np.all(r.Ycv[seg == 0] == 2.0), r.Ycv[seg == 0]
    assert not np.any(r.status[0]) and np.all(np.isfinite(r.Ycv))
    r0 = pp.npls_crossval(t, Y, F, segments=seg, center=False)   # uncentred: a constant Y is something to explain
    assert np.all(r0.fitted >= 1)
    t.close()


def check_cp_session_stays_live(pp, ctx, dt):
    """sweep, cross-validate, sweep: the factors of a session that never saw the calls, bit for bit"""
    lens, R = [12, 10, 9], 3
    X, Y, _ = NC.planted(lens, 2, seed=77)
    W0, G0 = pp.init_factors(lens, R, 5), pp.init_factors(lens, R, 99)
    ts = [pp.Tensor(ctx, lens, dt).upload(X) for _ in range(2)]
    ss = [pp.CP(ctx, t, R) for t in ts]
    for s in ss:
        s.set_factors(W0, G0)
        s.sweeps_dt(2)
    pp.npls_crossval(ts[0], Y, 2, segments=4)
    ts[0].contract_columns(1, np.ones((lens[1], 9)))
    ts[0].slice_inner_columns(2, np.ones((lens[0], lens[1], 9)))
    for s in ss:
        s.sweeps_dt(2)
    a, b = [NC.flat_factors(*s.get_factors(with_grad=True)) for s in ss]
    assert NC.bits(a) == NC.bits(b), "the cross-validation disturbed the live session"
    assert NC.bits(ts[0].download()) == NC.bits(ts[1].download())
    for x in ss + ts:
        x.close()


class _Opts(C.Structure):
    _fields_ = [("hopm_tol", C.c_double), ("hopm_max", C.c_int), ("inner_tol", C.c_double), ("inner_max", C.c_int)]


def check_refusals(pp, ctx, dt):
    """every refusal at the raw ABI: code, message prefix, nothing written, the tensor's bytes, and the next sweep of a
    live session equal to that of an undisturbed twin"""
    lib = pp.lib()
    lens, R, M, F, S = [9, 8, 7], 3, 2, 2, 3
    X, Y, _ = NC.planted(lens, M, seed=5)
    W0, G0 = pp.init_factors(lens, R, 5), pp.init_factors(lens, R, 99)
    ts = [pp.Tensor(ctx, lens, dt).upload(X) for _ in range(2)]
    ss = [pp.CP(ctx, t, R) for t in ts]
    for s in ss:
        s.set_factors(W0, G0)
        s.sweeps_dt(1)
    V0 = ts[0].download()
    N, I, h = len(lens), lens[0], ts[0]._h
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    Yf = np.asfortranarray(Y)
    Ynan, Yinf = Yf.copy(order="F"), Yf.copy(order="F")
    Ynan[3, 1], Yinf[0, 0] = np.nan, np.inf
    seg = (np.arange(I) % S).astype(np.int32)
    seg_neg, seg_big, seg_empty, seg_lop = seg.copy(), seg.copy(), seg.copy(), np.zeros(I, dtype=np.int32)
    seg_neg[2], seg_big[4] = -1, S
    seg_empty[seg_empty == 2] = 1
    seg_lop[0], seg_lop[1] = 1, 2      # segment 0 holds I - 2 samples: a training set of 2
    SENT = -777.0
    Ycv = np.full(I * M * 8, SENT)
    press, fitted, status, passes = np.full(8 * M, SENT), np.full(S, -7, dtype=np.int32), np.full(S * 8, -7, dtype=np.int32), C.c_int64(-7)
    d, g = (lambda a: a.ctypes.data_as(dp)), (lambda a: a.ctypes.data_as(ip))
    bad = [_Opts(-1.0, 500, 1e-12, 200), _Opts(float("nan"), 500, 1e-12, 200), _Opts(1e-12, 0, 1e-12, 200),
           _Opts(1e-12, 500, -1e-3, 200), _Opts(1e-12, 500, 1e-12, 0)]

    def cv(hh=h, mode=0, y=None, m=M, f=F, sg=None, s=S, center=1, opts=None, ycv=True):
        return lib.ppals_npls_crossval(hh, mode, d(Yf) if y is None else y, m, f, g(seg) if sg is None else sg, s, center,
                                       opts, d(Ycv) if ycv else None, d(press), fitted.ctypes.data_as(C.POINTER(C.c_int)),
                                       status.ctypes.data_as(C.POINTER(C.c_int)), C.byref(passes))

    name = "ppals_npls_crossval"
    calls = [("NULL tensor", lambda: cv(hh=None)), ("NULL Y", lambda: cv(y=C.cast(None, dp))),
             ("NULL segment", lambda: cv(sg=C.cast(None, ip))), ("NULL Ycv", lambda: cv(ycv=False)),
             ("mode -1", lambda: cv(mode=-1)), ("mode N", lambda: cv(mode=N)), ("M 0", lambda: cv(m=0)),
             ("F 0", lambda: cv(f=0)), ("S 1", lambda: cv(s=1)), ("S I + 1", lambda: cv(s=I + 1)),
             ("label -1", lambda: cv(sg=g(seg_neg))), ("label S", lambda: cv(sg=g(seg_big))),
             ("empty segment", lambda: cv(sg=g(seg_empty))),
             ("F beyond the smallest training set, centred", lambda: cv(sg=g(seg_lop), f=2, center=1)),
             ("F beyond the smallest training set", lambda: cv(sg=g(seg_lop), f=3, center=0)),
             ("center 2", lambda: cv(center=2)), ("center -1", lambda: cv(center=-1)),
             ("Y nan", lambda: cv(y=d(Ynan))), ("Y inf", lambda: cv(y=d(Yinf)))]
    calls += [(f"bad options {k}", lambda o=o: cv(opts=C.byref(o))) for k, o in enumerate(bad)]
    calls = [(n, c, ERR_ARG, name) for n, c in calls]
    p = d(Ycv)
    for fn, nm in ((lib.ppals_tensor_contract_columns, "ppals_tensor_contract_columns"),
                   (lib.ppals_tensor_slice_inner_columns, "ppals_tensor_slice_inner_columns")):
        calls += [(nm + " NULL tensor", lambda f=fn: f(None, 0, p, 1, p), ERR_ARG, nm),
                  (nm + " mode -1", lambda f=fn: f(h, -1, p, 1, p), ERR_ARG, nm),
                  (nm + " mode N", lambda f=fn: f(h, N, p, 1, p), ERR_ARG, nm),
                  (nm + " NULL in", lambda f=fn: f(h, 0, None, 1, p), ERR_ARG, nm),
                  (nm + " NULL out", lambda f=fn: f(h, 0, p, 1, None), ERR_ARG, nm),
                  (nm + " C 0", lambda f=fn: f(h, 0, p, 0, p), ERR_ARG, nm)]
    for what, call, code, prefix in calls:
        rc = call()
        assert rc == code, (what, rc, lib.ppals_last_error())
        assert lib.ppals_last_error().decode().startswith(prefix + ": "), (what, lib.ppals_last_error())
        assert np.all(Ycv == SENT) and np.all(press == SENT) and np.all(fitted == -7) and np.all(status == -7) and passes.value == -7, f"{what}: something was written"
        assert NC.bits(ts[0].download()) == NC.bits(V0), f"{what}: the tensor changed"
    # the two boundary calls next to the refusals pass: F = smallest training set - center
    assert cv(sg=g(seg_lop), f=1, center=1) == 0 and cv(sg=g(seg_lop), f=2, center=0) == 0, lib.ppals_last_error()
    Ycv[:], press[:], fitted[:], status[:] = SENT, SENT, -7, -7
    passes.value = -7
    # a dead handle: the context is gone, the tensor object still there
    ctx2 = pp.Context(0)
    dead = pp.Tensor(ctx2, lens, dt).upload(X)
    hd, dead._h = dead._h, None
    ctx2.close()
    for what, call, prefix in (("crossval", lambda: cv(hh=hd), name),
                               ("contract_columns", lambda: lib.ppals_tensor_contract_columns(hd, 0, p, 1, p), "ppals_tensor_contract_columns"),
                               ("slice_inner_columns", lambda: lib.ppals_tensor_slice_inner_columns(hd, 0, p, 1, p), "ppals_tensor_slice_inner_columns")):
        assert call() == ERR_ARG, what
        assert lib.ppals_last_error().decode().startswith(prefix + ": ")
    assert np.all(Ycv == SENT) and passes.value == -7
    lib.ppals_tensor_destroy(hd)
    for s in ss:
        s.sweeps_dt(1)
    a, b = [NC.flat_factors(*s.get_factors(with_grad=True)) for s in ss]
    assert NC.bits(a) == NC.bits(b), "a refused call disturbed the live session"
    for x in ss + ts:
        x.close()


# ------------------------------------------------------------------------------------------ the case that needs torch
# `python npls_cv_cases.py torch` (tests/test_gpu_npls_cv.py): torch is imported BEFORE the binding loads libppals, so
# that both share one HIP runtime.
def torch_crossval(torch, pp):
    """Y as a device tensor: the bits of the same call with a numpy Y, and cv_ref"""
    ctx = pp.Context(0)
    case = CV_CASES[4]
    name, lens, M, F, first, S, center = case
    X, Y, mode, seg = cv_inputs(case)
    t = pp.Tensor(ctx, list(X.shape), F64).upload(X)
    Yd = torch.from_numpy(np.ascontiguousarray(Y)).to("cuda:0")
    a = pp.npls_crossval(t, Yd, F, mode=mode, segments=seg, center=bool(center))
    b = pp.npls_crossval(t, Y, F, mode=mode, segments=seg, center=bool(center))
    assert NC.bits(a.Ycv) == NC.bits(b.Ycv) and NC.bits(a.press) == NC.bits(b.press)
    rYcv, rpress = cv_ref(t.download(), Y, F, mode, seg, S, center)
    assert max(NC.deviation(a.Ycv, rYcv), NC.deviation(a.press, rpress)) <= CV_BAR
    t.close()
    ctx.close()


if __name__ == "__main__":
    import sys
    import torch  # noqa: I001  (first: see above)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pairwise-perturbation_amd"))
    import ppals
    {"torch": torch_crossval}[sys.argv[1]](torch, ppals)
    print(f"npls_cv case {sys.argv[1]}: ok", flush=True)
