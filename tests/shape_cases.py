"""Ops::cp_mode_update_shape_ragged at the op level (tests/shape_shim: the op on host arrays, with its route
log): the HIP kernels of kernels_shape.hip.h through libppals.so (tests/test_gpu_shape_op.py) and the ops.h
default through the host stand-in (tests/test_shape_hostsim.py), against numpy fp64.

The reference is a brute force: a textbook pool-adjacent-violators run gives the isotonic fit of every prefix
(and, on the reversed column, of every suffix) as an explicit vector, the error of every split p is the explicit
||u_p - v||^2 of the two clipped fits, and the least wins. It keeps no block errors on a stack.

check() goes COLUMN BY COLUMN, GIVEN THE COLUMNS THE OP ITSELF PRODUCED BEFORE: v_r is recomputed from W_old, M, S
and the op's own new columns q < r, so one legitimate tie flip cannot poison later columns. Per column, with
  u    the reference fit of v_r,
  b    the componentwise rounding bound of v_r: gamma_{R+2} (|w| + (|M| + sum_q |w_q| |S_qr|) / d),
  bar  4 (||b||_2 + n 2^-53 ||v||_inf)   (the projection onto a fixed split's cone is non-expansive, so this
       bounds the error when the split agrees; the second term is the rounding of a block mean),
it wants
  feasibility  w has the shape and is >= floor, exactly;
  objective    ||w - v||^2 <= ||u - v||^2 + 2 ||u - v|| bar + bar^2;
  closeness    ||w - u||_2 <= bar whenever the reference's second-best DISTINCT fit (one further than bar from
               the best) is worse than its best by more than 1e-9 ||v||^2 — else the column is reported exempt;
               only the deliberate tie cases may be, a random case with an exempt column fails;
  a column whose S[r,r] is not a positive finite number or whose v has a non-finite entry: its bytes as handed in.
grad, gradsq, S and the Gram of the returned W are held to the 1e-12 relative of tests/polar_cases.py, guards,
rows behind `rows` and the other modes' Grams to their bytes."""
import ctypes as C
import os
import subprocess

import numpy as np

from bf16_util import same_values

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "shape_shim")
GUARD = 16
FLOOR = 1e-16                      # PPALS_NN_FLOOR
UNIMODAL, INCREASING, DECREASING = 1, 2, 3   # PPALS_SHAPE_*
SHAPES = (UNIMODAL, INCREASING, DECREASING)
ROWS = (1, 2, 3, 63, 64, 65, 130)
RANKS = (1, 3, 17, 64)
RTOL = 1e-12
U = 2.0 ** -53
LDS_BYTES = 152 * 1024             # kShapeLdsBytes of ops.h
GAP = 1e-9


def lds_rows(R):
    """the most rows whose work arrays (64 n + 8 bytes) fit in LDS beside S (8 R^2 bytes)"""
    return (LDS_BYTES - 8 * R * R - 8) // 64


def load(hostsim):
    subprocess.check_call(["make", "-s", "-C", DIR] + (["hostsim"] if hostsim else []))
    lib = C.CDLL(os.path.join(DIR, "build", "libshape_shim_hostsim.so" if hostsim else "libshape_shim.so"))
    lib.shape_shim_error.restype = C.c_char_p
    lib.shape_shim_run.restype = C.c_int
    lib.shape_shim_run.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_double, C.c_int64, C.c_int64, C.c_int64,
                                   C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_int, C.c_char_p, C.c_int]
    return lib


# ---------------------------------------------------------------------------------------------- the reference
def prefix_fits(v):
    """textbook pool-adjacent-violators, left to right: yields (k, the non-decreasing least-squares fit of v[:k+1])"""
    means, counts = [], []
    for k, x in enumerate(v):
        m, c = float(x), 1
        while means and means[-1] >= m:
            m = (means[-1] * counts[-1] + m * c) / (counts[-1] + c)
            c += counts[-1]
            means.pop()
            counts.pop()
        means.append(m)
        counts.append(c)
        yield k, np.repeat(means, counts)


def isotonic(v, floor=FLOOR):
    """the non-decreasing fit of v bounded below by floor: the unbounded one, clipped"""
    fit = None
    for _, fit in prefix_fits(v):
        pass
    return np.maximum(fit, floor)


def split_errors(v, floor=FLOOR):
    """e[p] = the squared error of 'rows 0..p rise, rows p+1.. fall', both fits explicit and clipped"""
    n = len(v)
    pre, suf = np.zeros(n), np.zeros(n + 1)
    for k, fit in prefix_fits(v):
        pre[k] = np.sum((np.maximum(fit, floor) - v[:k + 1]) ** 2)
    for k, fit in prefix_fits(v[::-1]):       # the fit of the last k + 1 rows, read backwards
        suf[n - 1 - k] = np.sum((np.maximum(fit, floor) - v[::-1][:k + 1]) ** 2)
    return pre + suf[1:]


def unimodal_fit(v, p, floor=FLOOR):
    return np.concatenate([isotonic(v[:p + 1], floor), isotonic(v[p + 1:][::-1], floor)[::-1] if p + 1 < len(v) else []])


def project(v, shape, bar, floor=FLOOR):
    """(u, gap): the reference fit, and how much worse the second-best distinct fit is (inf when there is none)"""
    if shape == INCREASING:
        return isotonic(v, floor), np.inf
    if shape == DECREASING:
        return isotonic(v[::-1], floor)[::-1], np.inf
    e = split_errors(v, floor)
    p = int(np.argmin(e))
    u = unimodal_fit(v, p, floor)
    gap = np.inf
    for q in np.argsort(e, kind="stable"):
        if e[q] - e[p] > GAP * float(v @ v) or e[q] - e[p] >= gap:
            break
        if q != p and np.linalg.norm(unimodal_fit(v, int(q), floor) - u) > bar:
            gap = e[q] - e[p]
    return u, gap


def shape_update(M, W, S, shape, floor=FLOOR):
    """the whole column loop of the op in numpy: W_new (the restatement tests/mode_shape_cases.py sweeps with)"""
    W = W.copy()
    for r in range(W.shape[1]):
        d = S[r, r]
        if not (d > 0 and np.isfinite(d)):
            continue
        v = W[:, r] + (M[:, r] - W @ S[:, r]) / d
        if np.all(np.isfinite(v)):
            W[:, r] = project(v, shape, np.inf, floor)[0]
    return W


def has_shape(w, shape):
    d = np.diff(w)
    if shape == INCREASING:
        return bool(np.all(d >= 0))
    if shape == DECREASING:
        return bool(np.all(d <= 0))
    p = int(np.argmax(w))
    return bool(np.all(d[:p] >= 0) and np.all(d[p:] <= 0))


# ------------------------------------------------------------------------------------------------- the calls
def inputs(rows, ranks, shape, N=3, mode=0, seed=11, pad=3, lam=1e-3):
    """a call: Grams of N modes per start (those of random factors), M, W_old and grad in guarded, padded buffers"""
    rng = np.random.default_rng(seed + 1000 * rows + sum(ranks) + 7 * shape)
    Cc, ld = sum(ranks), rows + pad
    G = []
    for r in ranks:
        for _ in range(N):
            A = rng.standard_normal((r + 4, r))
            G.append((A.T @ A).ravel(order="F"))
    M = np.full((ld, Cc), np.nan, order="F")
    M[:rows] = 3.0 * rng.standard_normal((rows, Cc))
    W = np.full(2 * GUARD + ld * Cc, np.nan)
    Wv = W[GUARD:GUARD + ld * Cc].reshape((ld, Cc), order="F")
    Wv[:rows] = rng.random((rows, Cc))
    grad = np.full(2 * GUARD + ld * Cc, np.nan)
    return dict(N=N, mode=mode, ranks=list(ranks), rows=rows, ld=ld, lam=lam, G=np.concatenate(G), M=M, W=W, grad=grad,
                shape=shape)


def views(c):
    """(M rows, W rows) of a call's buffers, writable"""
    Cc, ld, rows = sum(c["ranks"]), c["ld"], c["rows"]
    return c["M"][:rows], c["W"][GUARD:GUARD + ld * Cc].reshape((ld, Cc), order="F")[:rows]


def systems(c):
    """S per start, as the op forms it"""
    N, mode, out, sq = c["N"], c["mode"], [], 0
    for R in c["ranks"]:
        Gb = c["G"][N * sq:N * (sq + R * R)].reshape((N, R, R))
        Sb = np.ones((R, R))
        for j in range(N):
            if j != mode:
                Sb = Sb * Gb[j].T
        out.append(Sb + c["lam"] * np.eye(R))
        sq += R * R
    return out


def with_targets(c, T):
    """M such that, in exact arithmetic, v_r = T[:, r] for a call whose starts all have rank 1"""
    assert all(r == 1 for r in c["ranks"])
    M, _ = views(c)
    for b, Sb in enumerate(systems(c)):
        M[:, b] = T[:, b] * Sb[0, 0]
    return c


def run(lib, c, want_S=True):
    """the op on a copy of the call's buffers: (G, W, grad, gradsq, S, route tags)"""
    G, W, grad = c["G"].copy(), c["W"].copy(), c["grad"].copy()
    K = len(c["ranks"])
    ranks = (C.c_int * K)(*c["ranks"])
    gradsq = np.full(K, np.nan)
    S = np.full(sum(r * r for r in c["ranks"]), np.nan) if want_S else None
    route = C.create_string_buffer(1024)
    rc = lib.shape_shim_run(c["N"], c["mode"], K, ranks, c["lam"], c["rows"], c["ld"], c["ld"], c["ld"], GUARD,
                            G.ctypes.data, c["M"].ctypes.data, W.ctypes.data, grad.ctypes.data, gradsq.ctypes.data,
                            S.ctypes.data if want_S else None, c["shape"], route, 1024)
    assert rc == 0, lib.shape_shim_error().decode()
    return G, W, grad, gradsq, S, route.value.decode().split("\n")


def check(c, out):
    """raises AssertionError on anything the op got wrong; returns the columns exempt from the closeness check
    and the columns that had to stay, as (start, r)"""
    G, W, grad, gradsq, S, _ = out
    rows, ld, N, mode, shape = c["rows"], c["ld"], c["N"], c["mode"], c["shape"]
    Cc = sum(c["ranks"])
    view = lambda buf: buf[GUARD:GUARD + ld * Cc].reshape((ld, Cc), order="F")
    for name, got, was in (("W", W, c["W"]), ("grad", grad, c["grad"])):
        assert same_values(got[:GUARD], was[:GUARD]) and same_values(got[-GUARD:], was[-GUARD:]), f"{name}: guard written"
        assert same_values(view(got)[rows:], view(was)[rows:]), f"{name}: rows behind the last one written"
    Wn, Wo, gr = view(W)[:rows], view(c["W"])[:rows], view(grad)[:rows]
    exempt, stayed, col, sq = [], [], 0, 0
    for b, (R, Sb) in enumerate(zip(c["ranks"], systems(c))):
        Mb, Wb, Wob = c["M"][:rows, col:col + R], Wn[:, col:col + R], Wo[:, col:col + R]
        with np.errstate(invalid="ignore"):
            want_g = -Mb + Wob @ Sb
            scale = np.linalg.norm(np.nan_to_num(Wob @ Sb)) + np.linalg.norm(np.nan_to_num(Mb))
        fin = np.isfinite(want_g)
        assert np.all(np.isfinite(gr[:, col:col + R]) == fin), (b, "grad: non-finite entries elsewhere than the reference's")
        assert np.linalg.norm((gr[:, col:col + R] - want_g)[fin]) <= RTOL * scale, (b, "grad")
        if fin.all():
            assert abs(gradsq[b] - np.sum(want_g * want_g)) <= RTOL * scale * scale, (b, "gradsq")
        else:
            assert not np.isfinite(gradsq[b]), (b, "gradsq of a gradient with non-finite entries")
        if S is not None:
            Sg = S[sq:sq + R * R].reshape((R, R), order="F")
            assert np.all(np.isfinite(Sg) == np.isfinite(Sb)), (b, "S")
            assert np.nanmax(np.abs(Sg - Sb), initial=0.0) <= RTOL * np.nanmax(np.abs(Sb)), (b, "S")
        got_G = G[N * sq + mode * R * R:N * sq + (mode + 1) * R * R].reshape((R, R), order="F")
        assert np.all(np.isfinite(Wb)), (b, "a non-finite entry in W")
        assert np.abs(got_G - Wb.T @ Wb).max() <= RTOL * max(1.0, np.abs(Wb.T @ Wb).max()), (b, "Gram of the new W")
        for j in range(N):   # the other modes' Grams are inputs
            if j != mode:
                o = N * sq + j * R * R
                assert same_values(G[o:o + R * R], c["G"][o:o + R * R]), (b, j, "Gram of another mode written")
        cur = Wob.copy()
        gam = (R + 2) * U / (1 - (R + 2) * U)
        for r in range(R):
            d = Sb[r, r]
            w = Wb[:, r]
            with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                v = cur[:, r] + (Mb[:, r] - cur @ Sb[:, r]) / d if d > 0 and np.isfinite(d) else np.full(rows, np.nan)
            if not np.all(np.isfinite(v)):
                assert same_values(w, Wob[:, r]), (b, r, "a column that had to stay changed")
                stayed.append((b, r))
                continue
            bnd = gam * (np.abs(cur[:, r]) + (np.abs(Mb[:, r]) + np.abs(cur) @ np.abs(Sb[:, r])) / d)
            bar = 4 * (np.linalg.norm(bnd) + rows * U * np.abs(v).max())
            u, gap = project(v, shape, bar)
            assert np.all(w >= FLOOR) and has_shape(w, shape), (b, r, "not feasible")
            eu, ew = np.linalg.norm(u - v), np.linalg.norm(w - v)
            assert ew * ew <= eu * eu + 2 * eu * bar + bar * bar, (b, r, "objective", ew, eu, bar)
            if gap > GAP * float(v @ v):
                assert np.linalg.norm(w - u) <= bar, (b, r, "not the reference's fit", np.linalg.norm(w - u), bar)
            else:
                exempt.append((b, r))
            cur[:, r] = w
        col += R
        sq += R * R
    return exempt, stayed


def same_outputs(a, b):
    return all(same_values(x, y) for x, y in zip(a[:5], b[:5]) if x is not None)


# -------------------------------------------------------------------------------------------------- the cases
def case_table(lib, shape):
    """rows {1, 2, 3, 63, 64, 65, 130} x R {1, 3, 17, 64}, one start, random columns (no column may be exempt,
    none may stay), two runs bit for bit; 4 starts of ranks [2, 64, 5, 17] in one call, with and without S"""
    for rows in ROWS:
        for R in RANKS:
            c = inputs(rows, [R], shape)
            out = run(lib, c)
            exempt, stayed = check(c, out)
            assert not exempt and not stayed, (rows, R, exempt, stayed)
            assert same_outputs(out, run(lib, c)), (rows, R, "not reproducible")
            print(f"  shape={shape} rows={rows} R={R}: {out[5]}", flush=True)
    c = inputs(130, [2, 64, 5, 17], shape)
    out = run(lib, c)
    assert check(c, out) == ([], [])
    noS = run(lib, c, want_S=False)
    assert same_outputs(out[:4], noS[:4]), "S == nullptr changes the bits"
    return out[5]


def case_lds_boundary(lib, shape):
    """R = 2 at the last row counts whose work arrays fit in LDS and the first that do not: the route tags"""
    n, tags = lds_rows(2), {}
    for rows in (n - 1, n, n + 1, n + 2):
        c = inputs(rows, [2], shape)
        out = run(lib, c)
        assert check(c, out) == ([], []), rows
        tags[rows] = out[5]
    return n, tags


def contents(n, rng):
    """name -> target column v, and the names that are deliberate ties"""
    x = np.arange(n, dtype=float)
    peak = lambda m, s: np.exp(-0.5 * ((x - m) / s) ** 2)
    two = np.zeros(n)
    two[n // 4], two[3 * n // 4] = 1.0, 1.0
    T = {
        "random": rng.standard_normal(n),
        "rising": 0.5 + 0.25 * x + 0.1 * rng.random(n),
        "falling": 0.5 + 0.25 * x[::-1] + 0.1 * rng.random(n),
        "constant": np.full(n, 0.75),
        "negative": -1.0 - rng.random(n),
        "peak_first": 2.0 * peak(0, n / 6) + 0.01 * rng.standard_normal(n),
        "peak_last": 2.0 * peak(n - 1, n / 6) + 0.01 * rng.standard_normal(n),
        "two_peaks": two,
        "double_gauss": peak(0.3 * n, n / 12) + 0.8 * peak(0.7 * n, n / 10) + 0.05 * rng.standard_normal(n),
        # one block per row for most of the column, then entries low enough to pool all of them again, from
        # either end: a stack as deep as the column, taken down in one step
        # (the spike in front of the cliff makes the split unambiguous at any length)
        "cliff": np.concatenate([0.5 + 0.25 * x[:n - n // 4 - 1], [1.0 * n], np.full(n // 4, -1.0 * n)]),
    }
    T["cliff_rev"] = T["cliff"][::-1].copy()
    return T, {"two_peaks"}


def case_contents(lib, shape, n=65):
    """one start of rank 1 per column content; only the deliberate tie may be exempt; all negative gives all floor"""
    rng = np.random.default_rng(5 + shape)
    T, ties = contents(n, rng)
    names = list(T)
    c = with_targets(inputs(n, [1] * len(names), shape, seed=23), np.stack([T[k] for k in names], axis=1))
    out = run(lib, c)
    exempt, stayed = check(c, out)
    assert not stayed and {names[b] for b, _ in exempt} <= ties, [names[b] for b, _ in exempt]
    Wn = out[1][GUARD:GUARD + c["ld"] * len(names)].reshape((c["ld"], len(names)), order="F")[:n]
    assert np.all(Wn[:, names.index("negative")] == FLOOR), "all negative must give all floor"
    return [names[b] for b, _ in exempt]


def case_deep_global(lib, shape):
    """the `cliff` contents at a row count whose work arrays lie in global memory: a stack of about 1900 blocks,
    spilled 64 at a time, and taken down again in one step (from either end); returns the route tags"""
    n = lds_rows(1) + 70
    T, _ = contents(n, np.random.default_rng(9 + shape))
    names = ["cliff", "cliff_rev"]
    c = with_targets(inputs(n, [1] * len(names), shape, seed=29), np.stack([T[k] for k in names], axis=1))
    out = run(lib, c)
    assert check(c, out) == ([], [])
    return n, out[5]


def case_feasible(lib, shape, n=65, R=5):
    """a factor that has the shape with M = W S: v = w, and every column comes back within its bar of itself"""
    c = inputs(n, [R], shape, seed=31)
    M, W = views(c)
    x = np.arange(n, dtype=float)[:, None]
    if shape == UNIMODAL:
        W[:] = np.exp(-0.5 * ((x - np.linspace(5, n - 5, R)[None, :]) / 6.0) ** 2) + 0.01
    else:
        W[:] = 0.1 + (x if shape == INCREASING else x[::-1]) * np.linspace(0.01, 0.05, R)[None, :]
    Sb = systems(c)[0]
    M[:] = W @ Sb
    out = run(lib, c)
    assert check(c, out) == ([], [])
    Wn = out[1][GUARD:GUARD + c["ld"] * R].reshape((c["ld"], R), order="F")[:n]
    gam = (R + 2) * U / (1 - (R + 2) * U)
    for r in range(R):
        bnd = gam * (np.abs(W[:, r]) + (np.abs(M[:, r]) + np.abs(W) @ np.abs(Sb[:, r])) / Sb[r, r])
        bar = 4 * (np.linalg.norm(bnd) + n * U * np.abs(W[:, r]).max())
        assert np.linalg.norm(Wn[:, r] - W[:, r]) <= bar, (r, np.linalg.norm(Wn[:, r] - W[:, r]), bar)


def case_robust(lib, shape):
    """S[r,r] = 0 in one column and a NaN in another column of M: those two keep their bytes, the others are
    updated; two runs on fresh buffers agree bit for bit; a third with one start's inputs replaced by NaN
    leaves every other start's bytes as they were"""
    ranks, rows, N = [3, 5, 2], 37, 3
    c = inputs(rows, ranks, shape, seed=41, lam=0.0)
    M, _ = views(c)
    Gs = c["G"][N * 9:N * (9 + 25)].reshape((N, 5, 5))   # start 1
    Gs[1][2, 2] = 0.0                                     # (a mode other than `mode`: S[2,2] = 0)
    M[7, 3 + 4] = np.nan                                  # start 1, column 4
    out = run(lib, c)
    exempt, stayed = check(c, out)
    assert not exempt and stayed == [(1, 2), (1, 4)], (exempt, stayed)
    assert same_outputs(out, run(lib, c)), "not reproducible"
    d = {k: (v.copy(order="K") if isinstance(v, np.ndarray) else v) for k, v in c.items()}   # (M stays column-major)
    M2, W2 = views(d)
    M2[:, 3:8] = np.nan
    W2[:, 3:8] = np.nan
    d["G"][N * 9:N * (9 + 25)] = np.nan
    bad = run(lib, d)
    ld, Cc = c["ld"], sum(ranks)
    view = lambda buf: buf[GUARD:GUARD + ld * Cc].reshape((ld, Cc), order="F")
    for cols, sqs, b in (((0, 3), (0, 9), 0), ((8, 10), (34, 38), 2)):
        for k in (1, 2):
            assert same_values(view(out[k])[:, cols[0]:cols[1]], view(bad[k])[:, cols[0]:cols[1]]), (b, "W / grad")
        assert same_values(out[3][b:b + 1], bad[3][b:b + 1]), (b, "gradsq")
        assert same_values(out[4][sqs[0]:sqs[1]], bad[4][sqs[0]:sqs[1]]), (b, "S")
        assert same_values(out[0][N * sqs[0]:N * sqs[1]], bad[0][N * sqs[0]:N * sqs[1]]), (b, "Grams")


def case_selftest(lib):
    """the checker rejects a column without the shape, the second-best split, an entry below the floor, a
    written guard and a stale Gram"""
    c = inputs(65, [3], UNIMODAL)
    good = run(lib, c)
    assert check(c, good) == ([], [])
    ld = c["ld"]
    M, Wo = views(c)
    Sb = systems(c)[0]
    cur = Wo.copy()   # (the last column's target, given the op's own first two)
    cur[:, :2] = good[1][GUARD:GUARD + ld * 3].reshape((ld, 3), order="F")[:65, :2]
    v2 = cur[:, 2] + (M[:, 2] - cur @ Sb[:, 2]) / Sb[2, 2]
    far = unimodal_fit(v2, (int(np.argmin(split_errors(v2))) + 30) % 65)   # feasible, but a worse split

    def tampered(f):
        G, W, grad, gradsq, S, tags = (x.copy() if isinstance(x, np.ndarray) else x for x in good)
        v = W[GUARD:GUARD + ld * 3].reshape((ld, 3), order="F")
        f(W, v)
        G[:9] = (v[:65].T @ v[:65]).ravel(order="F")
        return G, W, grad, gradsq, S, tags

    def dented(W, v):
        p = int(np.argmax(v[:65, 2]))
        v[(p + 32) % 65, 2] = v[p, 2] * 2

    def other_split(W, v):
        v[:65, 2] = far

    def below_floor(W, v):
        v[0 if np.argmax(v[:65, 2]) > 0 else 64, 2] = 0.0

    def guard(W, v):
        W[-1] = 0.0

    for f in (dented, other_split, below_floor, guard):
        try:
            check(c, tampered(f))
        except AssertionError:
            continue
        raise RuntimeError(f"the checker accepted: {f.__name__}")
    G = good[0].copy()
    G[4] *= 1 + 1e-9
    try:
        check(c, (G,) + good[1:])
    except AssertionError:
        return
    raise RuntimeError("the checker accepted: a stale Gram")
