"""Cases, references and bars of the in-place preprocessing (ppals_tensor_center / _shift / _slice_sumsq / _scale /
_rescale, ppals.preprocess), shared by tests/test_gpu_preprocess.py (the HIP kernels, through `import ppals`) and
tests/test_preprocess_hostsim.py (the fp64 host twins of ops.h, through hostsim_util.load()).

The tensor is viewed as [L, J, T] around the mode, first index fastest. References are numpy long double on
V0 = Tensor.download() taken before the call. u = 2^-53; u_dt as in tests/stream_cases.py. Bars, all derived, none
tuned:
* offsets: with m the exact fibre mean, |off - m| <= (J + 1) u max_fibre |V0| =: E0 (J - 1 additions and a division);
* centred value: E = E0 + u (|v - m| + E0), |stored - (v - m)| <= E + u_dt (|v - m| + E);
* shift with a general alpha: E = 2 u (|v| + |alpha o|), |stored - (v + alpha o)| <= E + u_dt (|v + alpha o| + E);
  alpha = -1 with center's own offsets: the bits center stored;
* slice_sumsq: relative (n + 2) u, n = L T; scales (rms): relative ((n + 2) / 2 + 2) u;
* scaled value: with f = 1 / rms, ((n + 2) / 2 + 5) u |v f| + u_dt |v f| (1 + that); a plain rescale by a given
  factor g is one fp64 product and the storage rounding: u |v g| + u_dt |v g| (1 + u).

The route rule of hip_ops.hip (prep_lead / prep_rows_launch), restated in route() below from DESIGN.md §3, never
copied from a run; ROUTES lists what each shape takes and every route has a shape:
* L == 1: `lead.runs` while a fibre fits the run buffer, J * size <= 48 KiB, `lead.long` beyond;
* L > 1: vec = (L % VEC == 0), VEC = 4, 2, 4 for f32, f64, bf16 (the tensor's base is aligned); a tile is
  BL = 16 VEC (vec) or 64 consecutive l; centring keeps it on chip (`rows.lds`) while J * BL * size <= 56 KiB and
  takes two passes (`rows.twopass`) beyond.
"""
import numpy as np

U = 2.0 ** -53
LD = np.longdouble
F32, F64, BF16 = 0, 1, 3
DTNAME = {F32: "f32", F64: "f64", BF16: "bf16"}
UDT = {F64: 0.0, F32: 2.0 ** -24, BF16: 2.0 ** -8 + 2.0 ** -24 + 2.0 ** -32}
SIZE = {F32: 4, F64: 8, BF16: 2}
ROWS_VEC = {F32: 4, F64: 2, BF16: 4}

SHAPES = [
    [7, 6, 5],          # everything odd
    [40, 30],           # order 2
    [3, 128, 16, 9],    # J = 3: contiguous fibres at 12-byte pitch (fp32), runs with unaligned ends
    [33, 20, 12],       # L = 33: unaligned rows
    [5, 1, 4],          # J = 1: the centred mode is all zeros, the offsets equal the data
    [256, 17, 3],       # a full vector tile (L = 256), and the last mode at T = 1
    [3, 300, 2],        # L = 3, J = 300: above the 56 KiB tile at 64 scalar lanes (f32: 224, f64: 112 rows)
]
LONG_F64 = [[2, 24000, 2], [24000, 3, 2]]  # a 192 KB fibre: above the CU's LDS, and above both on-chip budgets


def ljt(lens, mode):
    return int(np.prod(lens[:mode], dtype=np.int64)), lens[mode], int(np.prod(lens[mode + 1:], dtype=np.int64))


def route(dt, lens, mode):
    """the form center takes (hip_ops.hip: prep_lead, prep_rows_launch)"""
    L, J, _ = ljt(lens, mode)
    if L == 1:
        return "lead.runs" if J * SIZE[dt] <= 48 * 1024 else "lead.long"
    vec = L % ROWS_VEC[dt] == 0
    BL = 16 * ROWS_VEC[dt] if vec else 64
    return ("rows.lds" if J * BL * SIZE[dt] <= 56 * 1024 else "rows.twopass") + f" vec={int(vec)}"


def cases(dtypes):
    out = [(lens, dt) for lens in SHAPES for dt in dtypes]
    return out + [(lens, F64) for lens in LONG_F64 if F64 in dtypes]


ALL_ROUTES = {"lead.runs", "lead.long", "rows.lds vec=0", "rows.lds vec=1", "rows.twopass vec=0", "rows.twopass vec=1"}
ROUTES = {(DTNAME[dt], tuple(lens), mode): route(dt, lens, mode)
          for lens, dt in cases((F32, F64, BF16)) for mode in range(len(lens))}
# what the rule gives, for the record of the shapes above:
assert ROUTES[("f32", (3, 128, 16, 9), 0)] == "lead.runs" and ROUTES[("f64", (24000, 3, 2), 0)] == "lead.long"
assert ROUTES[("f32", (33, 20, 12), 1)] == "rows.lds vec=0" and ROUTES[("f32", (256, 17, 3), 1)] == "rows.lds vec=1"
assert ROUTES[("f32", (3, 300, 2), 1)] == "rows.twopass vec=0" and ROUTES[("f64", (2, 24000, 2), 1)] == "rows.twopass vec=1"
assert set(ROUTES.values()) == ALL_ROUTES


# ------------------------------------------------------------------------------------------ data and references
_DATA = {}


def data(lens, seed=0):
    """mixed signs around a fibre-dependent level, so that the means are neither zero nor alike"""
    key = (tuple(lens), seed)
    if key not in _DATA:
        rng = np.random.default_rng(1234 + seed + sum(lens))
        x = rng.standard_normal(lens) + 2.0 * rng.random([n if i % 2 else 1 for i, n in enumerate(lens)]) - 0.5
        x = np.asfortranarray(x)
        x.setflags(write=False)
        _DATA[key] = x
    return _DATA[key]


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def within(what, got, ref, bar):
    got = np.asarray(got, dtype=np.float64)
    assert not np.any(np.isnan(got)), f"{what}: {int(np.sum(np.isnan(got)))} results are NaN"
    err = np.abs(got.astype(LD) - ref)
    bad = np.argwhere(err > bar)
    ratio = float(np.max(np.where(err == 0, LD(0), err / np.maximum(bar, LD(np.finfo(np.float64).tiny))))) if err.size else 0.0
    print(f"{what}: max err/bar {ratio:.3g}")
    assert bad.size == 0, (f"{what}: {len(bad)} elements over the bar, first at {tuple(bad[0])}: err "
                           f"{float(err[tuple(bad[0])]):.3e} bar {float(np.broadcast_to(bar, err.shape)[tuple(bad[0])]):.3e}")


def center_ref(V0, mode, dt):
    """(m, E0, v - m, bar of the stored value)"""
    v = V0.astype(LD)
    J = V0.shape[mode]
    m = np.sum(v, axis=mode, keepdims=True) / LD(J)
    E0 = (J + 1) * U * np.max(np.abs(v), axis=mode, keepdims=True)
    d = v - m
    E = E0 + U * (np.abs(d) + E0)
    return m, E0, d, E + UDT[dt] * (np.abs(d) + E)


def shift_ref(V0, off, alpha, dt):
    v, o = V0.astype(LD), LD(alpha) * np.asarray(off).astype(LD)
    ref = v + o
    E = 2 * U * (np.abs(v) + np.abs(o))
    return ref, E + UDT[dt] * (np.abs(ref) + E)


def slice_axes(V0, mode):
    return tuple(i for i in range(V0.ndim) if i != mode)


def sumsq_ref(V0, mode):
    v = V0.astype(LD)
    ss = np.sum(v * v, axis=slice_axes(V0, mode))
    n = V0.size // V0.shape[mode]
    return ss, (n + 2) * U * ss, n


def scale_ref(V0, mode, dt):
    """(rms, its bar, v f, the bar of the stored value); slices of rms 0 keep f = 1 and a zero bar"""
    ss, _, n = sumsq_ref(V0, mode)
    rms = np.sqrt(ss / LD(n))
    f = np.where(rms > 0, LD(1) / np.where(rms > 0, rms, LD(1)), LD(1))
    sh = [1] * V0.ndim
    sh[mode] = -1
    vf = V0.astype(LD) * f.reshape(sh)
    rel = ((n + 2) / 2 + 5) * U
    bar = np.where((rms > 0).reshape(sh), rel * np.abs(vf) + UDT[dt] * np.abs(vf) * (1 + rel), LD(0))
    return rms, ((n + 2) / 2 + 2) * U * rms, vf, bar


def rescale_ref(V0, mode, g, dt):
    sh = [1] * V0.ndim
    sh[mode] = -1
    vg = V0.astype(LD) * np.asarray(g).astype(LD).reshape(sh)
    return vg, U * np.abs(vg) + UDT[dt] * np.abs(vg) * (1 + U)


def fresh(pp, ctx, lens, dt, V=None, seed=0):
    return pp.Tensor(ctx, lens, dt).upload(data(lens, seed) if V is None else V)


# ------------------------------------------------------------------------------------------ the checks both suites run
def check_center_host(pp, ctx, lens, dt, mode):
    """test 1, host offsets: reference, two runs bit for bit; returns (V0, stored, offsets)"""
    what = f"center {DTNAME[dt]} {lens} mode {mode} [{route(dt, lens, mode)}]"
    runs = []
    for _ in range(2):
        t = fresh(pp, ctx, lens, dt)
        V0 = t.download()
        off = t.center(mode, "numpy")
        runs.append((t.download(), off))
        t.close()
    assert bits(runs[0][0]) == bits(runs[1][0]) and bits(runs[0][1]) == bits(runs[1][1]), f"{what}: two runs differ in bits"
    got, off = runs[1]
    m, E0, d, bar = center_ref(V0, mode, dt)
    assert list(off.shape) == [1 if i == mode else n for i, n in enumerate(lens)]
    within(what + " offsets", off, m, E0)
    within(what + " stored", got, d, bar)
    if lens[mode] == 1:
        assert not np.any(got) and bits(off.ravel(order="F")) == bits(V0.ravel(order="F")), what
    # offsets == None: the same tensor
    t = fresh(pp, ctx, lens, dt)
    assert t.center(mode) is None
    assert bits(t.download()) == bits(got), f"{what}: offsets=None stores other bits"
    t.close()
    return V0, got, off


def check_shift(pp, ctx, lens, dt, mode, V0, centred, off):
    """test 2"""
    what = f"shift {DTNAME[dt]} {lens} mode {mode}"
    t = fresh(pp, ctx, lens, dt)
    t.shift(mode, off, -1.0)
    assert bits(t.download()) == bits(centred), f"{what}: shift(offsets, -1) is not center bit for bit"
    t.shift(mode, off, 1.0)
    ref, bar = shift_ref(centred, off, 1.0, dt)
    back = t.download()
    within(what + " +1 against its reference", back, ref, bar)
    # V0 itself: the centred value carries center's bar, the shift adds its own
    _, _, _, cbar = center_ref(V0, mode, dt)
    within(what + " +1 restores V0", back, V0.astype(LD), cbar + bar)
    t.upload(V0)
    t.shift(mode, off, 0.37)
    ref, bar = shift_ref(V0, off, 0.37, dt)
    within(what + " alpha=0.37", t.download(), ref, bar)
    t.close()


def check_scale(pp, ctx, lens, dt, mode):
    """test 3: slice_sumsq, scale, rescale(rms); a planted all-zero slice"""
    what = f"scale {DTNAME[dt]} {lens} mode {mode}"
    V = np.array(data(lens, seed=1), order="F")
    zero = lens[mode] // 2 if lens[mode] > 1 else None
    if zero is not None:
        idx = [slice(None)] * len(lens)
        idx[mode] = zero
        V[tuple(idx)] = 0.0
    t = fresh(pp, ctx, lens, dt, V)
    V0 = t.download()
    ss = t.slice_sumsq(mode)
    assert bits(t.download()) == bits(V0), f"{what}: slice_sumsq changed the tensor"
    assert bits(t.slice_sumsq(mode)) == bits(ss), f"{what}: two slice_sumsq calls differ in bits"
    ref, bar, n = sumsq_ref(V0, mode)
    within(what + " slice_sumsq", ss, ref, bar)
    rms = t.scale(mode)
    scaled = t.download()
    rref, rbar, vf, vbar = scale_ref(V0, mode, dt)
    within(what + " rms", rms, rref, rbar)
    within(what + " scaled", scaled, vf, vbar)
    if zero is not None:
        assert rms[zero] == 0.0 and bits(scaled[tuple(idx)]) == bits(V0[tuple(idx)]), f"{what}: the zero slice moved"
    g = np.where(rms > 0, rms, 1.0)
    t.rescale(mode, g)
    ref, bar = rescale_ref(scaled, mode, g, dt)
    within(what + " rescale(rms)", t.download(), ref, bar)
    t.close()
    t2 = fresh(pp, ctx, lens, dt, V)  # two runs, bit for bit
    assert bits(t2.scale(mode)) == bits(rms) and bits(t2.download()) == bits(scaled), f"{what}: two runs differ in bits"
    t2.close()


def check_property(pp, ctx, lens, dt, a, b):
    """test 4: centre across a, scale within b != a. With c the centred tensor as stored (|c - d| <= bar1, the
    fibre means of d are zero) and s = the scaled one (|s - c f| <= bar2, f constant along a fibre of a):
    |mean_a s| <= f mean_a bar1 + mean_a bar2, and |rms_b(s) - 1| <= sqrt(mean over the slice of bar2^2)."""
    what = f"property {DTNAME[dt]} {lens} center {a} scale {b}"
    t = fresh(pp, ctx, lens, dt)
    V0 = t.download()
    t.center(a)
    c = t.download()
    t.scale(b)
    s = t.download()
    t.close()
    _, _, _, bar1 = center_ref(V0, a, dt)
    rms, _, _, bar2 = scale_ref(c, b, dt)
    sh = [1] * len(lens)
    sh[b] = -1
    f = (LD(1) / rms).reshape(sh)
    mean_bar = np.mean(bar1 * f + bar2, axis=a, keepdims=True)
    within(what + " fibre means", np.mean(s.astype(LD), axis=a, keepdims=True).astype(np.float64), LD(0) * mean_bar,
           mean_bar + U * np.mean(np.abs(s), axis=a, keepdims=True))
    ax = slice_axes(s, b)
    got = np.sqrt(np.mean(s.astype(LD) ** 2, axis=ax))
    within(what + " slice rms", got.astype(np.float64), np.ones(lens[b], LD), np.sqrt(np.mean(bar2 * bar2, axis=ax)) + 2 * U)


def planted(R=3, lens=(12, 10, 9), seed=5):
    """test 5: V = [[W]] + b[j, k] broadcast over mode 0, b uniform in [1, 2]; formed in long double, rounded once"""
    rng = np.random.default_rng(seed)
    W = [np.asfortranarray(rng.random((n, R))) for n in lens]
    b = 1.0 + rng.random((1,) + tuple(lens[1:]))
    model = np.einsum("ir,jr,kr->ijk", *[w.astype(LD) for w in W])
    V = np.asfortranarray((model + b.astype(LD)).astype(np.float64))
    Wc = [W[0] - W[0].mean(axis=0, keepdims=True), W[1], W[2]]
    absmodel = np.einsum("ir,jr,kr->ijk", *[np.abs(w).astype(LD) for w in W])
    return W, Wc, V, absmodel


def check_planted(pp, ctx):
    R = 3
    W, Wc, V, absmodel = planted(R)
    lens = list(V.shape)
    t = pp.Tensor(ctx, lens, F64).upload(V)
    V0 = t.download()
    s = pp.CP(ctx, t, R)
    s.set_factors(Wc, [np.zeros_like(w) for w in Wc])
    before = s.residual() / t.norm()
    print(f"planted model: residual / norm before centring {before:.3f}")
    assert before >= 0.3
    t.center(0)
    after = s.residual()
    _, _, _, bar = center_ref(V0, 0, F64)
    bound = float(np.sqrt(np.sum((bar + (R + 2) * U * absmodel) ** 2)))
    print(f"planted model: residual after centring {after:.3e}, bound {bound:.3e}")
    assert after <= bound
    s.close()
    t.close()


def flat_factors(W, G=None):
    return np.concatenate([w.ravel(order="F") for w in W] + ([g.ravel(order="F") for g in G] if G else []))


def check_cp_session(pp, ctx, lens, dt, R, schedule, V, packed=None):
    """test 6: a live session across center(0) + scale(1) against a new session on a new tensor holding the
    preprocessed values. packed: None, or the expectation on the packed twin (True: in use before, refused after)."""
    W0, G0 = pp.init_factors(lens, R, 5), pp.init_factors(lens, R, 99)
    t = pp.Tensor(ctx, lens, dt).upload(V)
    s = pp.CP(ctx, t, R)
    s.set_schedule(schedule)
    s.set_factors(W0, G0)
    n0 = s.placement_report()["packed"]["packed_scans"] if packed else 0
    s.sweeps_dt(2)  # (queued, not waited for)
    t.center(0)
    t.scale(1)
    s.set_factors(W0, G0)
    if packed:
        n1 = s.placement_report()["packed"]["packed_scans"]
        assert n1 > n0, "the packed twin was not in use on the raw tensor"
    s.sweeps_dt(3)
    W, G = s.get_factors(with_grad=True)
    res = s.residual()
    if packed:
        rep = s.placement_report()["packed"]
        assert rep["packed_scans"] == n1 and rep["layouts"] and not any(r["packed"] for r in rep["layouts"]), rep
    P = t.download()
    t2 = pp.Tensor(ctx, lens, dt).upload(P)
    assert bits(t2.download()) == bits(P)
    s2 = pp.CP(ctx, t2, R)
    s2.set_schedule(schedule)
    s2.set_factors(W0, G0)
    s2.sweeps_dt(3)
    W2, G2 = s2.get_factors(with_grad=True)
    assert bits(flat_factors(W, G)) == bits(flat_factors(W2, G2)), f"{lens} {schedule}: factors or gradients differ"
    assert bits(np.float64(res)) == bits(np.float64(s2.residual())), f"{lens} {schedule}: residuals differ"
    for x in (s, s2, t, t2):
        x.close()


def check_tucker_session(pp, ctx, lens, dt, ranks, V):
    """test 6 for a Tucker session: hosvd + a sweep on the raw tensor, center(0) + scale(1), then hosvd + 2 HOOI
    sweeps against a new session on a new tensor holding the preprocessed values, factors and core bit for bit.
    A Tucker session carries history — the warm-start basis of its eigen-steps (modes of 16 rows and more) and the
    order-3 multi-sweep schedule, which stays off once the back end refused a leading-mode product (extents below
    16) — and forgets it when the tensor's preprocessing epoch has moved (TuckerEngine::check_prep_epoch); without
    that the F32 cases differ from the new session by roundings (measured: projectors 2.2e-07 at [12, 10, 9],
    3.6e-13 at [16, 16, 16, 16])."""
    t = pp.Tensor(ctx, lens, dt).upload(V)
    k = pp.Tucker(ctx, t, ranks)
    k.hosvd()
    k.sweeps_dt(1)
    t.center(0)
    t.scale(1)
    k.hosvd()
    k.sweeps_dt(2)
    W, core = k.get_factors()
    t2 = pp.Tensor(ctx, lens, dt).upload(t.download())
    k2 = pp.Tucker(ctx, t2, ranks)
    k2.hosvd()
    k2.sweeps_dt(2)
    W2, core2 = k2.get_factors()
    proj = max(float(np.linalg.norm(a @ a.T - b @ b.T) / np.linalg.norm(b @ b.T)) for a, b in zip(W, W2))
    print(f"Tucker {DTNAME[dt]} {lens}: live against new session: projectors differ by {proj:.3e} (relative), "
          f"|core| ratio - 1 = {abs(np.linalg.norm(core) / np.linalg.norm(core2) - 1):.3e}, factors bitwise "
          f"{bits(flat_factors(W)) == bits(flat_factors(W2))}, core bitwise {bits(core) == bits(core2)}")
    assert bits(flat_factors(W)) == bits(flat_factors(W2)) and bits(core) == bits(core2), f"Tucker {lens}: differs"
    for x in (k, k2, t, t2):
        x.close()


ERR_ARG, ERR_UNSUPPORTED = -3, -5


def raw_refusals(pp, t, lens, device_cases=()):
    """test 7: (name, call, code, message prefix) of every refusal that needs no device pointer; device_cases adds
    (name, pointer, where) triples for center and shift. Calls go straight to the C ABI."""
    import ctypes as C
    lib = pp.lib()
    N, h = len(lens), t._h
    buf = np.zeros(int(np.prod(lens)), dtype=np.float64)
    p = buf.ctypes.data_as(C.POINTER(C.c_double))
    nan, inf = np.full(max(lens), np.nan), np.full(max(lens), 1.0)
    inf[0] = np.inf
    one, d = C.c_double(1.0), lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    out = []
    for mode in (-1, N):
        out += [("center mode", lambda m=mode: lib.ppals_tensor_center(h, m, p, 0, None), ERR_ARG, "ppals_tensor_center"),
                ("shift mode", lambda m=mode: lib.ppals_tensor_shift(h, m, p, 0, one, None), ERR_ARG, "ppals_tensor_shift"),
                ("sumsq mode", lambda m=mode: lib.ppals_tensor_slice_sumsq(h, m, p), ERR_ARG, "ppals_tensor_slice_sumsq"),
                ("scale mode", lambda m=mode: lib.ppals_tensor_scale(h, m, p), ERR_ARG, "ppals_tensor_scale"),
                ("rescale mode", lambda m=mode: lib.ppals_tensor_rescale(h, m, p), ERR_ARG, "ppals_tensor_rescale")]
    out += [("center NULL", lambda: lib.ppals_tensor_center(None, 0, p, 0, None), ERR_ARG, "ppals_tensor_center"),
            ("shift NULL", lambda: lib.ppals_tensor_shift(None, 0, p, 0, one, None), ERR_ARG, "ppals_tensor_shift"),
            ("sumsq NULL", lambda: lib.ppals_tensor_slice_sumsq(None, 0, p), ERR_ARG, "ppals_tensor_slice_sumsq"),
            ("scale NULL", lambda: lib.ppals_tensor_scale(None, 0, p), ERR_ARG, "ppals_tensor_scale"),
            ("rescale NULL", lambda: lib.ppals_tensor_rescale(None, 0, p), ERR_ARG, "ppals_tensor_rescale"),
            ("sumsq NULL ss", lambda: lib.ppals_tensor_slice_sumsq(h, 0, None), ERR_ARG, "ppals_tensor_slice_sumsq"),
            ("rescale NULL factors", lambda: lib.ppals_tensor_rescale(h, 0, None), ERR_ARG, "ppals_tensor_rescale"),
            ("shift NULL offsets", lambda: lib.ppals_tensor_shift(h, 0, None, 0, one, None), ERR_ARG, "ppals_tensor_shift"),
            ("center where", lambda: lib.ppals_tensor_center(h, 0, p, 2, None), ERR_ARG, "ppals_tensor_center"),
            ("center where -1", lambda: lib.ppals_tensor_center(h, 0, p, -1, None), ERR_ARG, "ppals_tensor_center"),
            ("shift where", lambda: lib.ppals_tensor_shift(h, 0, p, 2, one, None), ERR_ARG, "ppals_tensor_shift"),
            ("shift alpha nan", lambda: lib.ppals_tensor_shift(h, 0, p, 0, C.c_double(np.nan), None), ERR_ARG, "ppals_tensor_shift"),
            ("shift alpha inf", lambda: lib.ppals_tensor_shift(h, 0, p, 0, C.c_double(np.inf), None), ERR_ARG, "ppals_tensor_shift"),
            ("rescale nan", lambda: lib.ppals_tensor_rescale(h, 0, d(nan)), ERR_ARG, "ppals_tensor_rescale"),
            ("rescale inf", lambda: lib.ppals_tensor_rescale(h, 0, d(inf)), ERR_ARG, "ppals_tensor_rescale")]
    for name, ptr, code in device_cases:
        out += [("center " + name, lambda q=ptr: lib.ppals_tensor_center(h, 0, C.c_void_p(q), 1, None), code, "ppals_tensor_center"),
                ("shift " + name, lambda q=ptr: lib.ppals_tensor_shift(h, 0, C.c_void_p(q), 1, one, None), code, "ppals_tensor_shift")]
    out.append(("keep", lambda: (buf, nan, inf) and 0, 0, ""))  # (the arrays above stay alive while the list does)
    return out


def check_refusals(pp, ctx, dt, device_cases=()):
    """every refusal: code, message prefix, the tensor's bytes, and — the generation was not bumped — the next sweep
    of a live session equal to that of an undisturbed twin"""
    lens, R = [9, 8, 7], 3
    V = data(lens)
    W0, G0 = pp.init_factors(lens, R, 5), pp.init_factors(lens, R, 99)
    ts = [pp.Tensor(ctx, lens, dt).upload(V) for _ in range(2)]
    ss = [pp.CP(ctx, t, R) for t in ts]
    for s in ss:
        s.set_factors(W0, G0)
        s.sweeps_dt(1)
    V0 = ts[0].download()
    for name, call, code, prefix in raw_refusals(pp, ts[0], lens, device_cases):
        rc = call()
        assert rc == code, (name, rc, pp.lib().ppals_last_error())
        if code:
            assert pp.lib().ppals_last_error().decode().startswith(prefix + ": "), (name, pp.lib().ppals_last_error())
        assert bits(ts[0].download()) == bits(V0), f"{name}: the tensor changed"
    # a dead handle: the context is gone, the tensor object still there
    ctx2 = pp.Context(0)
    dead = pp.Tensor(ctx2, lens, dt).upload(V)
    h, dead._h = dead._h, None  # (the binding must not destroy it with the context)
    ctx2.close()
    import ctypes as C
    assert pp.lib().ppals_tensor_scale(h, 0, None) == ERR_ARG
    assert pp.lib().ppals_last_error().decode().startswith("ppals_tensor_scale: ")
    pp.lib().ppals_tensor_destroy(h)
    for s in ss:
        s.sweeps_dt(1)
    a, b = [flat_factors(*s.get_factors(with_grad=True)) for s in ss]
    assert bits(a) == bits(b), "a refused call disturbed the live session: the generation moved"
    for x in ss + ts:
        x.close()


def check_preprocess(pp, ctx, dt):
    """test 8"""
    lens, R = [10, 9, 8], 2
    A, B = data(lens, seed=2), data(lens, seed=3)
    t = fresh(pp, ctx, lens, dt, A)
    V0 = t.download()
    try:
        pp.preprocess(t, center=[0, 1], scale=[1, 2])
        raise AssertionError("overlapping modes accepted")
    except ValueError:
        pass
    assert bits(t.download()) == bits(V0)
    rec = pp.preprocess(t, center=[0], scale=[1, 2])
    assert [(k, m) for k, m, _ in rec.steps] == [("center", 0), ("scale", 1), ("scale", 2)]
    P = t.download()
    # by hand, on a second tensor of the same values
    h = fresh(pp, ctx, lens, dt, A)
    off = h.center(0, "numpy")
    c = h.download()
    r1 = h.scale(1)
    s1 = h.download()
    r2 = h.scale(2)
    assert bits(h.download()) == bits(P) and bits(off) == bits(rec.steps[0][2])
    assert bits(r1) == bits(rec.steps[1][2]) and bits(r2) == bits(rec.steps[2][2])
    # apply on new data equals the calls by hand
    n1, n2 = fresh(pp, ctx, lens, dt, B), fresh(pp, ctx, lens, dt, B)
    rec.apply(n1)
    n2.shift(0, off, -1.0).rescale(1, 1.0 / r1).rescale(2, 1.0 / r2)
    assert bits(n1.download()) == bits(n2.download())
    # undo restores the raw data. Forward, with d = V0 - m: |c - d| <= cbar, |s1 - c / rr1| <= sbar1,
    # |P - s1 / rr2| <= sbar2 (rr the exact rms, the returned r within rbar of it). Backward u2 = P r2, u1 = u2 r1,
    # u0 = u1 + off, each one fp64 operation and a storage rounding (rb2, rb1, shbar):
    #   |u2 - s1| <= sbar2 r2 + |s1| rbar2 / rr2 + rb2
    #   |u1 - c|  <= |u2 - s1| r1 + sbar1 r1 + |c| rbar1 / rr1 + rb1
    #   |u0 - V0| <= |u1 - c| + cbar + E0 + shbar
    rec.undo(t)
    m, E0, _, cbar = center_ref(V0, 0, dt)
    rr1, rbar1, _, sbar1 = scale_ref(c, 1, dt)
    rr2, rbar2, _, sbar2 = scale_ref(s1, 2, dt)
    b1 = lambda a: np.asarray(a).astype(LD)[None, :, None]
    b2 = lambda a: np.asarray(a).astype(LD)[None, None, :]
    u2, rb2 = rescale_ref(P, 2, r2, dt)
    u1, rb1 = rescale_ref(u2.astype(np.float64), 1, r1, dt)
    _, shbar = shift_ref(u1.astype(np.float64), off, 1.0, dt)
    e2 = sbar2 * b2(r2) + np.abs(s1) * b2(rbar2 / rr2) + rb2
    e1 = e2 * b1(r1) + sbar1 * b1(r1) + np.abs(c) * b1(rbar1 / rr1) + rb1
    within(f"undo {DTNAME[dt]}", t.download(), V0.astype(LD), e1 + cbar + E0 + shbar)
    # unscale_factors: a model of the scaled tensor -> the model of the unscaled one
    t.upload(P)
    s = pp.CP(ctx, t, R)
    s.set_factors(pp.init_factors(lens, R, 11), pp.init_factors(lens, R, 12))
    s.sweeps_dt(3)
    W = s.get_factors()
    per_slice_scaled = P.astype(LD) - np.einsum("ir,jr,kr->ijk", *[w.astype(LD) for w in W])
    Wu = rec.unscale_factors(W)
    assert bits(Wu[0]) == bits(W[0])
    unscaled = P.astype(LD) * r1.astype(LD)[None, :, None] * r2.astype(LD)[None, None, :]
    res_u = unscaled - np.einsum("ir,jr,kr->ijk", *[w.astype(LD) for w in Wu])
    want = per_slice_scaled * r1.astype(LD)[None, :, None] * r2.astype(LD)[None, None, :]
    absm = np.einsum("ir,jr,kr->ijk", *[np.abs(w).astype(LD) for w in Wu])
    # (each entry of the two scaled factors carries one rounding; one more u for the long-double arithmetic)
    within(f"unscale_factors {DTNAME[dt]}", res_u.astype(np.float64), want, 3 * U * (np.abs(unscaled) + absm))
    for x in (s, t, h, n1, n2):
        x.close()


# ------------------------------------------------------------------------------------------ the cases that need torch
# One per process: `python preprocess_cases.py <case>` (tests/test_gpu_preprocess.py). torch is imported BEFORE the
# binding loads libppals, so that both share one HIP runtime and the library can query torch's pointers.
GUARD = 512  # doubles of NaN on each side of a device offsets buffer


def _guarded(torch, n):
    return torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float64, device="cuda:0")


def _check_guards(torch, buf, n, what):
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert np.all(np.isnan(h[:GUARD])) and np.all(np.isnan(h[GUARD + n:])), f"{what}: a guard element changed"
    assert not np.any(np.isnan(h[GUARD:GUARD + n])), f"{what}: NaN among the offsets"
    return h[GUARD:GUARD + n]


def torch_device_offsets(torch, pp):
    """test 1, the device target, every case: the offsets land in the interior of a larger NaN-filled torch tensor,
    ordered on torch's stream; the same bits as the host target, and shift reads them from there"""
    import ctypes as C
    ctx = pp.Context(0)
    for lens, dt in cases((F32, F64, BF16)):
        for mode in range(len(lens)):
            what = f"device offsets {DTNAME[dt]} {lens} mode {mode}"
            L, _, T = ljt(lens, mode)
            t = fresh(pp, ctx, lens, dt)
            V0 = t.download()
            off = t.center(mode, "numpy")
            centred = t.download()
            t.upload(V0)
            buf = _guarded(torch, L * T)
            ptr = C.c_void_p(buf.data_ptr() + 8 * GUARD)
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            rc = pp.lib().ppals_tensor_center(t._h, mode, ptr, pp.DEVICE, st)
            assert rc == 0, (what, pp.lib().ppals_last_error())
            dev = _check_guards(torch, buf, L * T, what)
            assert bits(dev) == bits(off.ravel(order="F")) and bits(t.download()) == bits(centred), what
            t.upload(V0)
            rc = pp.lib().ppals_tensor_shift(t._h, mode, ptr, pp.DEVICE, C.c_double(-1.0), st)
            assert rc == 0, (what, pp.lib().ppals_last_error())
            assert bits(t.download()) == bits(centred), f"{what}: shift(-1) from device offsets is not center"
            _check_guards(torch, buf, L * T, what)
            t.close()
    ctx.close()


def torch_offsets(torch, pp):
    """Tensor.center(mode, "torch") and Tensor.shift with a torch tensor: shaped like the numpy offsets, same values"""
    ctx = pp.Context(0)
    lens, mode = [7, 6, 5], 1
    for dt in (F32, F64, BF16):
        t = fresh(pp, ctx, lens, dt)
        V0 = t.download()
        off = t.center(mode, "torch")
        torch.cuda.synchronize()
        centred = t.download()
        t.upload(V0)
        ref = t.center(mode, "numpy")
        assert list(off.shape) == [7, 1, 5] and bits(off.cpu().numpy()) == bits(ref)
        assert bits(t.download()) == bits(centred)
        for o in (off, off.contiguous()):  # (C-contiguous: the binding reorders it)
            t.upload(V0)
            t.shift(mode, o, -1.0)
            assert bits(t.download()) == bits(centred)
        t.close()
    ctx.close()


def torch_refusals(torch, pp):
    """test 7 with the device pointers that fail the checks: host and pinned memory, L*T*8 bytes that leave the
    allocation, a misaligned pointer"""
    import os
    assert os.environ.get("PYTORCH_NO_CUDA_MEMORY_CACHING") == "1"  # (the allocation is the tensor)
    ctx = pp.Context(0)
    n = 8 * 7  # L*T of mode 0 of check_refusals' [9, 8, 7]
    host = np.zeros(n)
    pinned = torch.zeros(n, dtype=torch.float64).pin_memory()
    z = torch.zeros(n, dtype=torch.float64, device="cuda:0")
    for dt in (F32, F64, BF16):
        check_refusals(pp, ctx, dt, device_cases=[("host offsets", host.ctypes.data, ERR_ARG),
                                                  ("pinned offsets", pinned.data_ptr(), ERR_ARG),
                                                  ("offsets past the allocation", z.data_ptr() + 8, ERR_ARG),
                                                  ("misaligned offsets", z.data_ptr() + 4, ERR_ARG)])
    # the same buffer where it fits is taken
    t = fresh(pp, ctx, [9, 8, 7], F64)
    import ctypes as C
    assert pp.lib().ppals_tensor_center(t._h, 0, C.c_void_p(z.data_ptr()), pp.DEVICE, None) == 0
    torch.cuda.synchronize()
    t.close()
    ctx.close()


if __name__ == "__main__":
    import os
    import sys
    import torch  # noqa: I001  (first: see above)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pairwise-perturbation_amd"))
    import ppals
    {"device_offsets": torch_device_offsets, "torch_offsets": torch_offsets, "refusals": torch_refusals}[sys.argv[1]](torch, ppals)
    print(f"preprocess case {sys.argv[1]}: ok", flush=True)
