"""Ops::parafac2_step and Ops::parafac2_init at the op level (tests/parafac2_shim: the op on host arrays, with its
route log): the kernels of kernels_parafac2.hip.h through libppals.so (tests/test_gpu_parafac2_op.py), and the
checker itself on a numpy emulation of the op (tests/test_parafac2_op_cpu.py). numpy and ctypes only.

Every call hands the op Q, P, T, status and Y with GUARD elements in front and behind and a finite sentinel
pattern inside, and reads everything back. check() holds every stage to a bar against a np.longdouble reference
formed from the DOWNLOADED output of the stage before it, so that one stage's error cannot hide in the next
stage's tolerance. With u = 2^-53 (a sum of n products in any order is within gamma_n <= n 2u of the exact one,
relative to the sum of the absolute products; the kernels' products, fused or not, fit that model):
  project   |Q_k - X_k A diag(C[k]) B^T| <= (J + R + 4) 2u (|X_k| |A| diag|C[k]| |B|^T)   elementwise
            (J terms of G = X_k A, one rounding of C[k, r] B[s, r], R terms of G Mk)
  polar     status[k] is the rule's on the singular values of the downloaded Q_k; where it is 1, T_k is symmetric
            to 64 kappa^2 2u max|T_k|, and P_k and P_k^T P_k - I lie within ref.p_bound(kappa) of ref.polar(Q_k)
            and of 0, kappa the 2-norm condition number of the downloaded Q_k; where it is 0, P_k and T_k keep
            the bytes they were handed in with
  apply     |P_k - Q_k T_k| <= (R + 2) 2u (|Q_k| |T_k|)                                     elementwise
  compress  |Y[:, j, k] - P_k^T X_k[:, j]| <= (I + 2) 2u (|P_k|^T |X_k|), plus half an ulp of the storage type
            for F32 storage
  sums      out[0] against sum x^2 over the I x J x K box, I J K 2u relative; out[1] against the sum of squares of
            the F64-storage Y, R J K 2u relative; out[2] == K - sum(status), an integer
and every guard element is untouched. The bars are derived, not measured; check() returns error / bar per stage."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

import parafac2_ref as ref

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "parafac2_shim")
GUARD = 16
U2 = 2.0 ** -52                    # 2u
MIN_RATIO = 2.0 ** -40             # PPALS_ORTHO_MIN_RATIO
F32, F64 = 0, 1                    # DType of ops.h; ViewDType of device_view.h has the same two values
NAME = {F32: "f32", F64: "f64"}
NPT = {F32: np.float32, F64: np.float64}
COMBOS_FULL = ((F32, F32), (F32, F64), (F64, F32), (F64, F64))     # (view type, storage type)
COMBOS_SHORT = ((F32, F64), (F64, F32))
FULL_RANKS = (16, 33, 49, 64)
STAGES = ("project", "symmetry", "polar", "orthonormal", "apply", "compress", "compress_f32", "sum_x", "sum_y")
LD = np.longdouble


def load():
    subprocess.check_call(["make", "-s", "-C", DIR])
    lib = C.CDLL(os.path.join(DIR, "build", "libparafac2_shim.so"))
    lib.parafac2_shim_error.restype = C.c_char_p
    lib.parafac2_shim_run.restype = C.c_int
    lib.parafac2_shim_run.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64,
                                      C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_char_p,
                                      C.c_int]
    lib.parafac2_shim_init.restype = C.c_int
    lib.parafac2_shim_init.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int64]
    return lib


# ---------------------------------------------------------------------------------------------- a call
def guarded(n, dtype, phase):
    """GUARD elements, n of a finite sentinel pattern that no stage can produce (1000 and more), GUARD elements"""
    buf = np.empty(2 * GUARD + n, dtype=dtype)
    buf[:GUARD] = buf[GUARD + n:] = -12345
    buf[GUARD:GUARD + n] = 1000 + (np.arange(n) + phase) % 97
    return buf


def make_call(shape, X, B, A, Cm, vdt, padded):
    """the op's arguments for one view of X (I x J x K values): the view buffer (padding NaN), the values it holds
    as fp64, and the prefilled outputs"""
    I, J, K, R = shape
    s1 = I + 3 if padded else I
    s2 = s1 * (J + 2) if padded else s1 * J
    buf = np.full(s2 * K, np.nan, dtype=NPT[vdt])
    box = np.lib.stride_tricks.as_strided(buf, (I, J, K), tuple(buf.itemsize * s for s in (1, s1, s2)))
    box[...] = X
    return dict(shape=shape, vdt=vdt, padded=padded, s1=s1, s2=s2, buf=buf, Xh=np.array(box, dtype=np.float64),
                B=np.asfortranarray(B, dtype=np.float64), A=np.asfortranarray(A, dtype=np.float64),
                C=np.asfortranarray(Cm, dtype=np.float64))


def prefilled(c, dt):
    I, J, K, R = c["shape"]
    return dict(Q=guarded(I * R * K, np.float64, 0), P=guarded(I * R * K, np.float64, 5),
                T=guarded(R * R * K, np.float64, 11), status=guarded(K, np.int32, 0),
                Y=guarded(R * J * K, NPT[dt], 23), out=np.full(3, -1.0), dt=dt)


def run(lib, c, dt, want_out=True):
    """the op on freshly prefilled buffers: the buffers as downloaded, and the route tags"""
    I, J, K, R = c["shape"]
    o = prefilled(c, dt)
    route = C.create_string_buffer(1024)
    rc = lib.parafac2_shim_run(I, J, K, R, c["vdt"], dt, c["buf"].ctypes.data, c["s1"], c["s2"], c["buf"].size,
                               c["B"].ctypes.data, c["A"].ctypes.data, c["C"].ctypes.data, MIN_RATIO,
                               o["Q"].ctypes.data, o["P"].ctypes.data, o["T"].ctypes.data, o["status"].ctypes.data,
                               o["Y"].ctypes.data, o["out"].ctypes.data if want_out else None, GUARD, route, 1024)
    assert rc == 0, lib.parafac2_shim_error().decode()
    o["tags"] = route.value.decode().split("\n")
    return o


def emulate(c, dt, want_out=True):
    """the op's contract in numpy fp64, Gram route included, in the shim's layout"""
    I, J, K, R = c["shape"]
    o = prefilled(c, dt)
    X = c["Xh"]
    Q, P, T, Y = (inner(o, c, n) for n in "QPTY")
    st = o["status"][GUARD:GUARD + K]
    sy = 0.0
    for k in range(K):
        Q[k] = (X[:, :, k] @ c["A"]) @ (c["C"][k][:, None] * c["B"].T)
        with np.errstate(all="ignore"):
            th, V = np.linalg.eigh(Q[k].T @ Q[k])
        good = bool(np.all(np.isfinite(th)) and np.all(th > 0) and th.min() > th.max() * MIN_RATIO)
        st[k] = 1 if good else 0
        if good:
            T[k] = ((V / np.sqrt(th)) @ V.T).T
            P[k] = Q[k] @ T[k].T
        y = P[k].T @ X[:, :, k]
        sy += float(np.sum(y * y))
        Y[:, :, k] = y
    if want_out:
        o["out"][:] = float(np.sum(X * X)), sy, K - int(st.sum())
    o["tags"] = [route_tag(c, dt)]
    return o


def inner(o, c, name):
    """a writable view of an output without its guards: Q, P as K x I x R, T as K x R x R (T[k][s, q] the entry
    (q, s) of T_k), Y as R x J x K"""
    I, J, K, R = c["shape"]
    if name in "QP":
        return o[name][GUARD:-GUARD].reshape((K, R, I)).transpose(0, 2, 1)
    if name == "T":
        return o["T"][GUARD:-GUARD].reshape((K, R, R))
    return o["Y"][GUARD:-GUARD].reshape((R, J, K), order="F")


def route_tag(c, dt):
    """the tag from the shape alone: nt = ceil(R / 16), rp = 16 nt, the two dynamic LDS sizes in bytes"""
    I, J, K, R = c["shape"]
    nt = (R + 15) // 16
    rp = 16 * nt
    a = 8 * (max(5120, 64 * (rp + 1)) + R * R)
    b = 8 * (64 * 36 + 36 * rp + 17)
    return (f"parafac2.step.{NAME[dt]}.{NAME[c['vdt']]} R={R} nt={nt} tiles={(I + 63) // 64}x{(J + 63) // 64} "
            f"lds={a},{b}")


# ---------------------------------------------------------------------------------------------- the checker
def half_ulp(y, dt):
    a = np.abs(y)
    if dt == F32:
        return 0.5 * np.spacing(a.astype(np.float32)).astype(np.float64) + 2.0 ** -150
    return np.zeros_like(a, dtype=np.float64)


def ratio(err, bar):
    """the largest err / bar; an error under a zero bar counts as infinite, NaN anywhere as infinite"""
    err, bar = np.asarray(err, dtype=LD), np.asarray(bar, dtype=LD)
    with np.errstate(all="ignore"):
        q = np.where(err == 0, 0.0, err / bar)
    q = np.where(np.isfinite(q), q, np.inf)
    return float(np.max(q)) if q.size else 0.0


def check(c, o, y64=None, want_status=None):
    """raises AssertionError on anything the op got wrong; returns {stage: the largest error / bar}. y64: the Y of
    the F64-storage run on the same view (out[1] is the sum over the fp64 values before the rounding); an
    F64-storage run is its own. want_status: the statuses the case is built for."""
    I, J, K, R = c["shape"]
    dt = o["dt"]
    was = prefilled(c, dt)
    for n in ("Q", "P", "T", "status", "Y"):
        assert o[n][:GUARD].tobytes() == was[n][:GUARD].tobytes(), f"{n}: front guard written"
        assert o[n][-GUARD:].tobytes() == was[n][-GUARD:].tobytes(), f"{n}: back guard written"
    assert o["tags"] == [route_tag(c, dt)], (o["tags"], route_tag(c, dt))
    X = c["Xh"].astype(LD)
    Q, P, T, Y = (inner(o, c, n) for n in "QPTY")
    P0, T0 = inner(was, c, "P"), inner(was, c, "T")
    st = o["status"][GUARD:GUARD + K]
    assert np.isfinite(Q).all() and np.isfinite(P).all() and np.isfinite(T).all() and np.isfinite(Y).all(), "not finite"
    A, B, Cm = c["A"].astype(LD), c["B"].astype(LD), c["C"].astype(LD)
    worst = dict.fromkeys(STAGES, 0.0)

    def held(stage, err, bar, what):
        q = ratio(err, bar)
        worst[stage] = max(worst[stage], q)
        assert q <= 1.0, (stage, what, c["shape"], q)

    for k in range(K):
        Xk, Qk, Pk, Tk = X[:, :, k], Q[k].astype(LD), P[k].astype(LD), T[k].T.astype(LD)
        # project
        Qref = ((Xk @ A) * Cm[k]) @ B.T
        held("project", np.abs(Qk - Qref), (J + R + 4) * U2 * (((np.abs(Xk) @ np.abs(A)) * np.abs(Cm[k])) @ np.abs(B).T),
             f"Q_{k}")
        # polar: the rule on the downloaded Q_k
        s = np.linalg.svd(Q[k], compute_uv=False)
        gap = (s[-1] / s[0]) ** 2 if s[0] > 0 else 0.0
        assert not 2.0 ** -45 <= gap <= 2.0 ** -35, (k, gap, "the slice sits on the threshold: change the seed")
        want = 1 if gap > MIN_RATIO else 0
        assert st[k] == want, (f"status[{k}]", int(st[k]), want)
        if not want:
            assert P[k].tobytes() == P0[k].tobytes(), f"P_{k}: a slice without a polar factor was rewritten"
            assert T[k].tobytes() == T0[k].tobytes(), f"T_{k}: a slice without a polar factor was rewritten"
        else:
            kappa = s[0] / s[-1]
            assert kappa <= ref.KAPPA_WIDE_CAP, (k, kappa)
            pb = ref.p_bound(kappa)
            held("symmetry", np.abs(Tk - Tk.T), 64 * kappa ** 2 * U2 * np.abs(T[k]).max(), f"T_{k}")
            held("polar", np.abs(P[k] - ref.polar(Q[k])), pb, f"P_{k}")
            held("orthonormal", np.abs(Pk.T @ Pk - np.eye(R)), pb, f"P_{k}^T P_{k}")
            # apply
            held("apply", np.abs(Pk - Qk @ Tk), (R + 2) * U2 * (np.abs(Qk) @ np.abs(Tk)), f"P_{k}")
        # compress, with P_k as downloaded (the prefilled one where the slice has no polar factor)
        Yref = Pk.T @ Xk
        yk = Y[:, :, k].astype(np.float64)
        hu = np.maximum(half_ulp(Yref.astype(np.float64), dt), half_ulp(yk, dt))
        held("compress" if dt == F64 else "compress_f32", np.abs(yk - Yref),
             (I + 2) * U2 * (np.abs(Pk).T @ np.abs(Xk)) + hu, f"Y_{k}")
    if want_status is not None:
        assert list(st) == list(want_status), (list(st), want_status)
    out = o["out"]
    if out is not None:
        if y64 is None:
            assert dt == F64, "the sum of y^2 of an F32-storage run is checked against the F64-storage Y"
            y64 = Y
        xx, yy = np.sum(X * X), np.sum(y64.astype(LD) ** 2)
        held("sum_x", abs(out[0] - xx), I * J * K * U2 * xx, "out[0]")
        held("sum_y", abs(out[1] - yy), R * J * K * U2 * yy, "out[1]")
        assert out[2] == K - int(st.sum()) and out[2] == math.floor(out[2]), ("out[2]", out[2], list(st))
    return worst


def same_bytes(a, b, names=("Q", "P", "T", "status", "Y", "out")):
    return all(a[n].tobytes() == b[n].tobytes() for n in names)


def merge(into, w):
    for s, v in w.items():
        into[s] = max(into.get(s, 0.0), v)
    return into


# ---------------------------------------------------------------------------------------------- the cases
def combos_of(shape, first_edge=(64, 64, 1, 64)):
    full = shape == first_edge or (shape[:3] == (130, 70, 2) and shape[3] in FULL_RANKS)
    return COMBOS_FULL if full else COMBOS_SHORT


def case_values(step, shape, inputs, want_status=None):
    """every stage bar for one shape, on a contiguous and on a padded view, for the shape's view / storage
    combinations; an F32-storage run is held to the F64-storage run on the same view (exact relation a): the same
    Q, P, T, status, out[0] and out[1], and Y == float32(Y of the F64 run). step(c, dt) runs the op."""
    X, B, A, Cm = inputs
    worst, tags = {}, []
    for padded in (False, True):
        for vdt in (F32, F64):
            dts = [dt for v, dt in combos_of(shape) if v == vdt]
            if not dts:
                continue
            c = make_call(shape, X, B, A, Cm, vdt, padded)
            o64 = step(c, F64)          # (also the reference of out[1] where the shape asks for F32 storage only)
            merge(worst, check(c, o64, want_status=want_status))
            tags += o64["tags"]
            if F32 in dts:
                o32 = step(c, F32)
                merge(worst, check(c, o32, y64=inner(o64, c, "Y"), want_status=want_status))
                assert same_bytes(o32, o64, ("Q", "P", "T", "status", "out")), (shape, vdt, "storage changed more than Y")
                assert inner(o32, c, "Y").tobytes() == inner(o64, c, "Y").astype(np.float32).tobytes(), \
                    (shape, vdt, "the F32 Y is not the F64 Y rounded once")
                tags += o32["tags"]
    return worst, tags


def case_exact(step, shape, inputs):
    """exact relations b and c on a padded view: an f64 view holding f32-representable values gives the bytes of
    the f32 view of the same values in every output, for both storages; a second run gives the same bytes; a run
    that does not ask for the sums gives the same Q, P, T, status and Y and leaves `out` alone.
    step(c, dt, want_out=True) runs the op."""
    X, B, A, Cm = inputs
    Xr = np.asarray(X, dtype=np.float32).astype(np.float64)
    for dt in (F32, F64):
        c32, c64 = (make_call(shape, Xr, B, A, Cm, vdt, True) for vdt in (F32, F64))
        assert c32["Xh"].tobytes() == c64["Xh"].tobytes()
        a, b = step(c32, dt), step(c64, dt)
        assert same_bytes(a, b), (shape, dt, "the f64 view of f32 values differs from the f32 view")
        assert same_bytes(a, step(c32, dt)) and same_bytes(b, step(c64, dt)), (shape, dt, "not reproducible")
        n = step(c64, dt, False)
        assert same_bytes(n, b, ("Q", "P", "T", "status", "Y")) and np.all(n["out"] == -1.0), (shape, dt, "without out")


def case_init(lib, I=65, R=33, K=3):
    P = guarded(I * R * K, np.float64, 0)
    was = P.copy()
    assert lib.parafac2_shim_init(P.ctypes.data, I, R, K, GUARD) == 0, lib.parafac2_shim_error().decode()
    assert P[:GUARD].tobytes() == was[:GUARD].tobytes() and P[-GUARD:].tobytes() == was[-GUARD:].tobytes(), "guard"
    want = np.transpose(ref.identity_projections(I, K, R), (0, 2, 1))           # K x R x I: i fastest
    assert P[GUARD:-GUARD].tobytes() == np.ascontiguousarray(want).tobytes()
