"""Ops::cp_mode_update_ortho_ragged at the op level (tests/polar_shim: the op on host arrays, with its route
log): the HIP kernels of kernels_polar.hip.h through libppals.so (tests/test_gpu_polar_op.py) and the ops.h
default through the host stand-in (tests/test_polar_hostsim.py), against numpy.

Every call hands the op NaN guards in front of and behind W and grad, leading dimensions wider than the rows
(the rows behind `rows` are NaN too), and reads everything back: check() wants every double outside the
rows x columns the op owns untouched. What the op owns is held to
  grad, gradsq, S, the Gram of the new W: 1e-12 relative (sums of at most 64 fp64 products; the Gram of an
      orthonormal W is I, so its bar is absolute),
  |W^T W - I|_max and the asymmetry of W^T M relative to |M|_F: C_ORTHO R 2^-53 kappa_2(M)^2, the bound of
      tests/mode_constraint_cases.py (its C_ORTHO is measured over this grid too: at R = 1 and kappa = 1 the
      bound is C_ORTHO ulps, and a normalised column of 65 entries is 3.6 ulp off unit length), and positive
      eigenvalues of W^T M — which together say W is the polar
      factor (U V^T of numpy's SVD is then only printed beside it),
  a start whose M has no polar factor under the rule (rows < R here): W bit for bit as handed in."""
import ctypes as C
import os
import subprocess

import numpy as np

import mode_constraint_cases as MC
from bf16_util import same_values

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "polar_shim")
GUARD = 16
ROWS = (1, 63, 64, 65, 130)
RANKS = (1, 3, 17, 64)
RTOL = 1e-12


def load(hostsim):
    subprocess.check_call(["make", "-s", "-C", DIR] + (["hostsim"] if hostsim else []))
    lib = C.CDLL(os.path.join(DIR, "build", "libpolar_shim_hostsim.so" if hostsim else "libpolar_shim.so"))
    lib.polar_shim_error.restype = C.c_char_p
    lib.polar_shim_run.restype = C.c_int
    lib.polar_shim_run.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_double, C.c_int64, C.c_int64, C.c_int64,
                                   C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_char_p, C.c_int]
    return lib


def inputs(rows, ranks, N=3, mode=0, seed=11, pad=3):
    """a call: Grams of N modes per start (those of random factors), M, W_old and grad in guarded, padded buffers"""
    rng = np.random.default_rng(seed + 1000 * rows + sum(ranks))
    Cc, ld = sum(ranks), rows + pad
    G = []
    for r in ranks:
        for _ in range(N):
            A = rng.standard_normal((r + 4, r))
            G.append((A.T @ A).ravel(order="F"))
    M = np.full((ld, Cc), np.nan, order="F")
    M[:rows] = rng.standard_normal((rows, Cc))
    W = np.full(2 * GUARD + ld * Cc, np.nan)
    Wv = W[GUARD:GUARD + ld * Cc].reshape((ld, Cc), order="F")
    Wv[:rows] = rng.standard_normal((rows, Cc))
    grad = np.full(2 * GUARD + ld * Cc, np.nan)
    return dict(N=N, mode=mode, ranks=list(ranks), rows=rows, ld=ld, lam=1e-3, G=np.concatenate(G), M=M, W=W, grad=grad)


def run(lib, c, want_S=True):
    """the op on a copy of the call's buffers: (G, W, grad, gradsq, S, route tags)"""
    G, W, grad = c["G"].copy(), c["W"].copy(), c["grad"].copy()
    K = len(c["ranks"])
    ranks = (C.c_int * K)(*c["ranks"])
    gradsq = np.full(K, np.nan)
    S = np.full(sum(r * r for r in c["ranks"]), np.nan) if want_S else None
    route = C.create_string_buffer(1024)
    rc = lib.polar_shim_run(c["N"], c["mode"], K, ranks, c["lam"], c["rows"], c["ld"], c["ld"], c["ld"], GUARD,
                            G.ctypes.data, c["M"].ctypes.data, W.ctypes.data, grad.ctypes.data, gradsq.ctypes.data,
                            S.ctypes.data if want_S else None, route, 1024)
    assert rc == 0, lib.polar_shim_error().decode()
    return G, W, grad, gradsq, S, route.value.decode().split("\n")


def check(c, out, c_ortho=None):
    """raises AssertionError on anything the op got wrong; returns the worst ratio to R 2^-53 kappa_2(M)^2, which
    is held to c_ortho (MC.C_ORTHO; measure() passes infinity). W^T W and W^T M are evaluated in long double, so
    that the check measures W and not its own rounding."""
    c_ortho = MC.C_ORTHO if c_ortho is None else c_ortho
    G, W, grad, gradsq, S, _ = out
    rows, ld, N, mode = c["rows"], c["ld"], c["N"], c["mode"]
    Cc = sum(c["ranks"])
    view = lambda buf: buf[GUARD:GUARD + ld * Cc].reshape((ld, Cc), order="F")
    for name, got, was in (("W", W, c["W"]), ("grad", grad, c["grad"])):
        assert same_values(got[:GUARD], was[:GUARD]) and same_values(got[-GUARD:], was[-GUARD:]), f"{name}: guard written"
        assert same_values(view(got)[rows:], view(was)[rows:]), f"{name}: rows behind the last one written"
    Wn, Wo, gr = view(W)[:rows], view(c["W"])[:rows], view(grad)[:rows]
    worst, col, sq = 0.0, 0, 0
    for b, R in enumerate(c["ranks"]):
        Gb = c["G"][N * sq:N * (sq + R * R)].reshape((N, R, R))
        Sb = np.ones((R, R))
        for j in range(N):
            if j != mode:
                Sb = Sb * Gb[j].T
        Sb = Sb + c["lam"] * np.eye(R)
        Mb, Wb, Wob = c["M"][:rows, col:col + R], Wn[:, col:col + R], Wo[:, col:col + R]
        want_g = -Mb + Wob @ Sb
        scale = np.linalg.norm(Wob @ Sb) + np.linalg.norm(Mb)
        assert np.linalg.norm(gr[:, col:col + R] - want_g) <= RTOL * scale, (b, "grad")
        assert abs(gradsq[b] - np.sum(want_g * want_g)) <= RTOL * scale * scale, (b, "gradsq")
        if S is not None:
            assert np.abs(S[sq:sq + R * R].reshape((R, R), order="F") - Sb).max() <= RTOL * np.abs(Sb).max(), (b, "S")
        got_G = G[N * sq + mode * R * R:N * sq + (mode + 1) * R * R].reshape((R, R), order="F")
        assert np.abs(got_G - Wb.T @ Wb).max() <= RTOL * max(1.0, np.abs(Wb.T @ Wb).max()), (b, "Gram of the new W")
        for j in range(N):   # the other modes' Grams are inputs
            if j != mode:
                o = N * sq + j * R * R
                assert same_values(G[o:o + R * R], c["G"][o:o + R * R]), (b, j, "Gram of another mode written")
        P, kappa, ratio, stays = MC.polar_update(Mb, Wob)
        if stays:
            assert ratio < 2.0 ** -45, "the case sits on the threshold: change the seed"
            assert same_values(Wb, Wob), (b, "the factor of a start without a polar factor changed")
        else:
            assert ratio > 2.0 ** -35, "the case sits on the threshold: change the seed"
            unit = R * 2.0 ** -53 * kappa * kappa
            Wl = Wb.astype(np.longdouble)
            A = Wl.T @ Mb.astype(np.longdouble)
            r1 = float(np.abs(Wl.T @ Wl - np.eye(R)).max()) / unit
            r2 = float(np.abs(A - A.T).max()) / np.linalg.norm(Mb) / unit
            assert r1 <= c_ortho and r2 <= c_ortho, (b, R, rows, kappa, r1, r2, c_ortho)
            A = A.astype(np.float64)
            assert np.linalg.eigvalsh(0.5 * (A + A.T)).min() > 0, (b, "W^T M is not positive definite")
            worst = max(worst, r1, r2)
        col += R
        sq += R * R
    return worst


def measure(lib):
    """the worst ratio over the grid of case_table, for C_ORTHO (profiles/mode_constraints_bars.md)"""
    worst = 0.0
    for rows in ROWS:
        for R in RANKS:
            c = inputs(rows, [R])
            worst = max(worst, check(c, run(lib, c), np.inf))
    return worst


def case_table(lib):
    """rows {1, 63, 64, 65, 130} x R {1, 3, 17, 64}, one start; then 4 starts of different ranks in one call"""
    for rows in ROWS:
        for R in RANKS:
            c = inputs(rows, [R])
            out = run(lib, c)
            w = check(c, out)
            again = run(lib, c)
            assert all(same_values(a, b) for a, b in zip(out[:5], again[:5])), (rows, R, "not reproducible")
            print(f"  rows={rows} R={R}: {'stays' if rows < R else f'worst ratio to the bound {w:.3g}'} {out[5]}", flush=True)
    c = inputs(130, [2, 64, 5, 17])
    out = run(lib, c)
    check(c, out)
    check(c, run(lib, c, want_S=False)[:4] + (None, []))
    c = inputs(10, [2, 17, 5])   # (the middle start has no polar factor: the others are updated)
    check(c, run(lib, c))
    return out[5]


def case_selftest(lib):
    """the checker rejects an un-normalised W, U V^T with two columns swapped, a dropped last row tile and a
    written guard"""
    c = inputs(130, [17])
    good = run(lib, c)
    check(c, good)
    ld = c["ld"]

    def tampered(f):
        G, W, grad, gradsq, S, tags = (x.copy() if isinstance(x, np.ndarray) else x for x in good)
        f(W, W[GUARD:GUARD + ld * 17].reshape((ld, 17), order="F"), G)
        return G, W, grad, gradsq, S, tags

    def scaled(W, v, G):
        v[:130] *= 1 + 1e-9
        G[:] = np.concatenate([(v[:130].T @ v[:130]).ravel(order="F"), G[289:]])

    def swapped(W, v, G):
        v[:130, [3, 4]] = v[:130, [4, 3]]
        G[:289] = (v[:130].T @ v[:130]).ravel(order="F")

    def dropped(W, v, G):
        v[128:130] = c["W"][GUARD:GUARD + ld * 17].reshape((ld, 17), order="F")[128:130]
        G[:289] = (v[:130].T @ v[:130]).ravel(order="F")

    def guard(W, v, G):
        W[-1] = 0.0

    for f in (scaled, swapped, dropped, guard):
        try:
            check(c, tampered(f))
        except AssertionError:
            continue
        raise RuntimeError(f"the checker accepted: {f.__name__}")
