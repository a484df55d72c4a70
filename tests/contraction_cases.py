"""Op-level cases of the contraction kernels and their one checker (tests/test_gpu_contractions.py on the HIP
kernels, tests/test_contractions_hostsim.py on the host stand-in, both through tests/opshim).

A case is a plain dict: the op, its argument values, `route` (regular expressions every one of which must
match a tag of the call's route log, ops.h) and `why` in a few words. `dev=True` marks a case whose route
rests on the device (CU count, occupancy): sized for 256 CUs, skipped with a message elsewhere.

The checker, per case:
* inputs from a seed, exact in their storage type; value class "pos" = uniform[0.5, 1) (the project's), "mix" =
  uniform[-1, 1);
* every input buffer ends in 4 KiB of NaN inside its allocation, every output buffer lies between two 4 KiB
  NaN guards and holds NaN wherever the call must not write (the gaps of a stride larger than packed); after
  the call every byte outside the result is unchanged and no result element is NaN;
* the reference is numpy: the formula of ops.h as an einsum, padded rows / accumulate / out_scale / strides
  written out from the comments there. In fp64 where the bar is 2^-24, in long double where it is 2^-53;
* componentwise bar (forward bound of a length-J inner product summed in any order):
      |got - ref| <= (J + 3) u (|V| . |B|)   [+ u |out_before| with accumulate]
  u = 2^-24 where the tensor / cached X is fp32 or bf16 or the result is stored as fp32, else 2^-53; the +3:
  rounding the Khatri-Rao operand to the working precision, the fp32 store, out_scale. mttv and pp_correct
  promise fp64 arithmetic (ops.h), so an fp32 X is held to 2^-53 there unless the case pins `u24` with a reason;
* on the "pos" class also the project's Frobenius bars (KTOL of tests/test_gpu_cp.py);
* the route log matches `route` (HIP only).
"""
import re

import numpy as np

from bf16_util import bf16_bits, bf16_round
from opshim_util import BF16, F32, F64

GUARD = 4096
U24, U53 = 2.0 ** -24, 2.0 ** -53
KTOL = {U24: 2e-6, U53: 1e-10}  # tests/test_gpu_cp.py
DT = {"f32": F32, "f64": F64, "bf16": BF16}
VEC = {"f32": 4, "f64": 2, "bf16": 8}
MAX_J = 4096


class Skip(Exception):
    pass


# ------------------------------------------------------------------------------------------ values
def _values(rng, cls, shape):
    x = rng.random(shape)
    return 0.5 + 0.5 * x if cls == "pos" else 2.0 * x - 1.0


def _stored(x, dt):
    """(exact fp64 value, storage image) of x rounded to the storage type dt"""
    if dt == "f32":
        s = x.astype(np.float32)
        return s.astype(np.float64), s
    if dt == "bf16":
        return bf16_round(x), bf16_bits(x).reshape(x.shape)
    return x, x


def _wide(u):
    return np.longdouble if u == U53 else np.float64


def _krp(Ws, dtype):
    """B[j, r] = prod_f W_f[j_f, r], the first factor's index fastest (ops.h: krp)"""
    B = Ws[0].astype(dtype)
    for W in Ws[1:]:
        B = (W.astype(dtype)[:, None, :] * B[None, :, :]).reshape(-1, B.shape[1])
    return B


def _contract(A, B, spec):
    """einsum in A's dtype; through BLAS for fp64 (tensordot), plainly for long double"""
    return np.einsum(spec, A, B, optimize=(A.dtype == np.float64))


# ------------------------------------------------------------------------------------------ buffers
class _In:
    """an input: [lead elements of NaN][payload][4 KiB of NaN], one allocation; ptr at the payload"""

    def __init__(self, sh, payload, lead=0):
        raw = np.ascontiguousarray(payload).reshape(-1).view(np.uint8)
        self.off = lead * payload.dtype.itemsize
        self.img = np.full(self.off + raw.size + GUARD, 0xFF, np.uint8)
        self.img[self.off:self.off + raw.size] = raw
        self.sh, self.base = sh, sh.alloc(self.img.size)
        sh.h2d(self.base, self.img)
        self.ptr = self.base + self.off

    def check(self, what):
        tail = self.sh.d2h(self.base + self.img.size - GUARD, GUARD)
        assert np.array_equal(tail, self.img[-GUARD:]), f"{what}: the NaN tail of an input was written"

    def free(self):
        self.sh.free(self.base)


class _Out:
    """an output of `nelem` elements of numpy type `t`: [4 KiB NaN][nelem, NaN unless init][4 KiB NaN]"""

    def __init__(self, sh, nelem, t, idx=None, init=None):
        self.t, self.nelem = np.dtype(t), nelem
        body = np.full(nelem, np.nan, self.t)
        if init is not None:
            body[idx] = init
        self.img = np.full(2 * GUARD + body.nbytes, 0xFF, np.uint8)
        self.img[GUARD:GUARD + body.nbytes] = body.view(np.uint8)
        self.sh, self.base = sh, sh.alloc(self.img.size)
        sh.h2d(self.base, self.img)
        self.ptr = self.base + GUARD

    def download(self):
        return self.sh.d2h(self.base, self.img.size)

    def free(self):
        self.sh.free(self.base)


def check_image(what, pre, post, t, idx):
    """the result elements of an output image `post` (taken at idx); every other byte must equal `pre`"""
    t = np.dtype(t)
    a = pre[GUARD:-GUARD].view(t).copy()
    b = post[GUARD:-GUARD].view(t).copy()
    got = b[idx].astype(np.float64)
    a[idx] = 0
    b[idx] = 0
    assert np.array_equal(pre[:GUARD], post[:GUARD]), f"{what}: the guard in front of the result was written"
    assert np.array_equal(pre[-GUARD:], post[-GUARD:]), f"{what}: the guard behind the result was written"
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{what}: a gap between result elements was written"
    assert not np.any(np.isnan(got)), f"{what}: {int(np.sum(np.isnan(got)))} result elements are NaN"
    return got


def check_values(what, got, ref, absprod, J, u, cls, before=None, log=None):
    """the componentwise bar and, on the positive class, the Frobenius bar; ref / absprod may be long double"""
    bar = (J + 3) * u * absprod
    if before is not None:
        bar = bar + u * np.abs(before)
    err = np.abs(got.astype(ref.dtype) - ref)
    worst = float(np.max(err / np.maximum(bar, np.finfo(np.float64).tiny)))
    frob = float(np.linalg.norm((got.astype(ref.dtype) - ref).astype(np.float64)) /
                 max(np.linalg.norm(ref.astype(np.float64)), 1e-300))
    if log is not None:
        log.append(f"{what}: max err/bar {worst:.3g} (u=2^{int(np.log2(u))}, J={J}), rel Frobenius {frob:.3g}")
    bad = np.argwhere(err > bar)
    assert bad.size == 0, (f"{what}: {len(bad)} elements over the bar (J+3) u |V|.|B|, u=2^{int(np.log2(u))}: first at "
                           f"{tuple(bad[0])}, err {float(err[tuple(bad[0])]):.3e} bar {float(bar[tuple(bad[0])]):.3e}, "
                           f"worst err/bar {worst:.3g}")
    if cls == "pos":
        assert frob <= KTOL[u], f"{what}: relative Frobenius error {frob:.3e} over {KTOL[u]}"


def check_route(what, case, tags):
    for pat in case["route"]:
        assert any(re.match(pat + r"(?!\d)", t) for t in tags), \
            f"{what}: route {pat!r} expected, the log says {tags}"


# ------------------------------------------------------------------------------------------ the ops
class Run:
    """What one case left behind: pre / post output images and what verify() needs. perturbations of `post`
    are what the checker's self-test feeds back in."""


def _factor_mats(rng, c, J, R):
    """the Khatri-Rao factors of a case: `fac` = list of rows (product J); ld = rows + fld"""
    rows = c.get("fac") or [J]
    assert int(np.prod(rows)) == J and J <= MAX_J, c["name"]
    Ws = [_values(rng, c["cls"], (r, R)) for r in rows]
    return rows, Ws


def _upload_factors(sh, Ws, extra_ld, keep):
    refs = []
    for W in Ws:
        ld = W.shape[0] + extra_ld
        full = np.full((ld, W.shape[1]), np.nan)
        full[:W.shape[0]] = W
        b = _In(sh, np.asfortranarray(full).reshape(-1, order="F"))
        keep.append(b)
        refs.append((b.ptr, W.shape[0], ld))
    return refs


def _gram_inputs(rng, sh, R, keep):
    """Grams of three well-conditioned factors for arm_gram_system (mode 1 of N = 3, lambda = 0.25)"""
    N, mode, lam = 3, 1, 0.25
    Gs = []
    for _ in range(N):
        W = rng.random((4 * R + 8, R)) * 2 - 1
        Gs.append(W.T @ W)
    Gall = _In(sh, np.concatenate([np.asfortranarray(G).reshape(-1, order="F") for G in Gs]))
    S, Si = _Out(sh, R * R, np.float64), _Out(sh, R * R, np.float64)
    keep += [Gall, S, Si]
    want = np.ones((R, R))
    for i, G in enumerate(Gs):
        if i != mode:
            want = want * G
    want = want + lam * np.eye(R)
    sh.arm_gram_system(Gall.ptr, N, mode, R, lam, S.ptr, Si.ptr)
    return S, Si, want


def _check_system(what, S, Si, want, R):
    """S and S^-1 written by the extra workgroup: the bars of tests/test_gpu_normal_equations.py"""
    idx = np.arange(R * R)
    s = check_image(what + " S", S.img, S.download(), np.float64, idx).reshape((R, R), order="F")
    si = check_image(what + " Sinv", Si.img, Si.download(), np.float64, idx).reshape((R, R), order="F")
    rel = lambda a, b: np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)
    cond = np.linalg.cond(want)
    assert rel(s, want) < 1e-13, (what, rel(s, want))
    assert rel(si, np.linalg.inv(want)) < 1e-10 * cond, (what, rel(si, np.linalg.inv(want)), cond)
    assert rel(s @ si, np.eye(R)) < 1e-10 * cond, what
    assert rel(si, si.T) < 1e-13, what


def run_case(sh, c, hip, log=None, perturb=None, posts=None):
    """Runs one case on the shim `sh` and checks it. hip: the routes are checked and S / S^-1 of an armed call too
    (the host stand-in logs nothing and prepares no system). perturb(run): the self-test's hook, called on the
    outcome before it is verified. Returns the route tags."""
    rng = np.random.default_rng(c["seed"])
    keep = []
    try:
        r = _run(sh, c, hip, rng, keep, log)
        if perturb:
            perturb(r)
        if posts is not None:
            posts.append(r.post)
        got = check_image(c["name"], r.pre, r.post, r.t, r.idx).reshape(r.ref.shape)
        check_values(c["name"], got, r.ref, r.absprod, r.J, r.u, c["cls"], r.before, log)
        if hip:
            check_route(c["name"], c, r.tags)
        return r.tags
    finally:
        for b in keep:
            b.free()


def _run(sh, c, hip, rng, keep, log):
    op, R = c["op"], c.get("R")
    r = Run()
    r.before = None
    sh.route_take()
    if op == "scan":
        dt, L, J, T = c["dt"], c["L"], c["J"], c["T"]
        out32 = c.get("out", "f64") == "f32"
        u = U24 if (dt != "f64" or out32) else U53
        wd = _wide(u)
        Vx, Vs = _stored(_values(rng, c["cls"], (L, J, T)), dt)
        pad = c.get("pad") or (0, 0)
        rowsel = np.arange(L)
        if pad[0]:
            Vx[np.arange(L) % pad[0] >= pad[1]] = 0  # pad rows are zero (pad_layout)
            Vs = _stored(Vx, dt)[1]
            rowsel = rowsel[rowsel % pad[0] < pad[1]]
        rows, Ws = _factor_mats(rng, c, J, R)
        B = _krp(Ws, wd)
        Vv = (Vx[rowsel] if pad[0] else Vx).astype(wd, copy=False)
        r.ref = _contract(Vv, B, "ljt,jr->ltr")
        r.absprod = _contract(np.abs(Vv), np.abs(B), "ljt,jr->ltr")
        Lc = len(rowsel)
        # the three stride forms of ops.h; tgap / rgap widen the inner / outer stride beyond packed
        tg, rg = c.get("tgap", 0), c.get("rgap", 0)
        if c.get("form", "suffix") == "inplace":  # tstride = L*R, rstride = L
            rs = Lc + tg
            ts = rs * R + rg
        else:  # suffix (T = 1) and rank-index-last TTM: tstride = L, rstride = L*T; prefix: L = 1
            ts = Lc + tg
            rs = ts * T + rg
        r.idx = (np.arange(Lc)[:, None, None] + ts * np.arange(T)[None, :, None] +
                 rs * np.arange(R)[None, None, :]).reshape(-1)
        r.t = np.float32 if out32 else np.float64
        vin = _In(sh, Vs.reshape(-1, order="F"), lead=c.get("voff", 0))
        out = _Out(sh, int(r.idx.max()) + 1, r.t)
        keep += [vin, out]
        f = _upload_factors(sh, Ws, c.get("fld", 0), keep)
        r.ref, r.absprod = r.ref.reshape(-1), r.absprod.reshape(-1)
        sh.scan_store_mode(c.get("store", -1))
        try:
            sh.scan_contract(vin.ptr, DT[dt], L, J, T, f, R, out.ptr, F32 if out32 else F64, ts, rs, pad)
        finally:
            sh.scan_store_mode(-1)
    elif op == "mttv":
        xdt, L, J, T = c["dt"], c["L"], c["J"], c["T"]
        u = U24 if (xdt == "f32" and c.get("u24")) else U53
        wd = _wide(u)
        Xx, Xs = _stored(_values(rng, c["cls"], (L, J, T, R)), xdt)
        rows, Ws = _factor_mats(rng, c, J, R)
        B = _krp(Ws, wd)
        scale = c.get("scale")
        sc = 1.0 if scale is None else scale
        r.ref = sc * _contract(Xx.astype(wd), B, "ljtr,jr->ltr")
        r.absprod = abs(sc) * _contract(np.abs(Xx).astype(wd), np.abs(B), "ljtr,jr->ltr")
        rs = L * T + c.get("rgap", 0)
        r.idx = (np.arange(L)[:, None, None] + L * np.arange(T)[None, :, None] +
                 rs * np.arange(R)[None, None, :]).reshape(-1)
        r.ref, r.absprod = r.ref.reshape(-1), r.absprod.reshape(-1)
        if c.get("acc"):
            r.before = _values(rng, c["cls"], r.ref.shape)
            r.ref = r.ref + r.before.astype(wd)
        r.t = np.float64
        xin = _In(sh, Xs.reshape(-1, order="F"))
        out = _Out(sh, int(r.idx.max()) + 1, r.t, r.idx, r.before)
        keep += [xin, out]
        f = _upload_factors(sh, Ws, c.get("fld", 0), keep)
        scp = 0
        if scale is not None:
            scb = _In(sh, np.array([scale]))
            keep.append(scb)
            scp = scb.ptr
        call = lambda o: sh.mttv(xin.ptr, DT[xdt], L, J, T, f, R, o.ptr, rs, 1 if c.get("acc") else 0, scp)
        armed = None
        if c.get("arm") and hip:  # the unarmed call first: the armed one must give the same bits
            plain = _Out(sh, int(r.idx.max()) + 1, r.t, r.idx, r.before)
            keep.append(plain)
            call(plain)
            sh.sync()
            sh.route_take()
            armed = _gram_inputs(rng, sh, R, keep)
        call(out)
    elif op in ("ttm_keep", "ttm_lead"):
        dt, L, J, T, Kc = c["dt"], c["L"], c["J"], c["T"], c["Kc"]
        u = U24 if dt == "f32" else U53
        wd = _wide(u)
        assert J <= MAX_J
        shape, spec = ((L, J, T), "ljt,jk->lkt") if op == "ttm_keep" else ((J, L, T), "jst,jk->skt")
        Xx, Xs = _stored(_values(rng, c["cls"], shape), dt)
        W = _values(rng, c["cls"], (J, Kc))
        r.ref = _contract(Xx.astype(wd), W.astype(wd), spec).reshape(-1, order="F")
        r.absprod = _contract(np.abs(Xx).astype(wd), np.abs(W).astype(wd), spec).reshape(-1, order="F")
        r.idx = np.arange(L * Kc * T)
        r.t = np.float64
        xin = _In(sh, Xs.reshape(-1, order="F"))
        out = _Out(sh, L * Kc * T, r.t)
        keep += [xin, out]
        (wp, _, ldw), = _upload_factors(sh, [W], c.get("fld", 0), keep)
        if op == "ttm_keep":
            sh.ttm_keep(xin.ptr, DT[dt], L, J, T, wp, ldw, Kc, out.ptr)
        else:
            taken = sh.ttm_lead_front(xin.ptr, DT[dt], J, L, T, wp, ldw, Kc, out.ptr)
            if not taken:  # the refusal: nothing may have been written, and there is no result to check
                r.tags = sh.route_take()
                post = out.download()
                assert np.array_equal(post, out.img), f"{c['name']}: a refused call wrote to its result"
                assert c.get("refused"), f"{c['name']}: ttm_lead_front returned false"
                if hip:
                    check_route(c["name"], c, r.tags)
                raise _Refused(r.tags)
            assert not (hip and c.get("refused")), f"{c['name']}: ttm_lead_front took a shape it must refuse"
    elif op == "pp":
        rows_, terms = c["rows"], c["terms"]  # terms: list of (ny, keep_first, extra lddw)
        u = U53
        wd = _wide(u)
        M0 = _values(rng, c["cls"], (rows_, R))
        ref = M0.astype(wd)
        ab = np.abs(M0).astype(wd)
        tl = []
        for ny, kf, xld in terms:
            Tt = _values(rng, c["cls"], (rows_, ny, R) if kf else (ny, rows_, R))
            dW = _values(rng, c["cls"], (ny, R))
            spec = "xyr,yr->xr" if kf else "yxr,yr->xr"
            ref = ref + _contract(Tt.astype(wd), dW.astype(wd), spec)
            ab = ab + _contract(np.abs(Tt).astype(wd), np.abs(dW).astype(wd), spec)
            tb = _In(sh, Tt.reshape(-1, order="F"))
            keep.append(tb)
            (dp, _, ld), = _upload_factors(sh, [dW], xld, keep)
            tl.append((tb.ptr, ny, kf, dp, ld))
        J = sum(t[0] for t in terms)
        r.ref, r.absprod = ref.reshape(-1, order="F"), ab.reshape(-1, order="F")
        r.idx = np.arange(rows_ * R)
        r.t = np.float64
        m0 = _In(sh, M0.reshape(-1, order="F"))
        out = _Out(sh, rows_ * R, r.t)
        keep += [m0, out]
        armed = None
        if c.get("arm") and hip:
            plain = _Out(sh, rows_ * R, r.t)
            keep.append(plain)
            sh.pp_correct(m0.ptr, rows_, R, tl, plain.ptr)
            sh.sync()
            sh.route_take()
            armed = _gram_inputs(rng, sh, R, keep)
        sh.pp_correct(m0.ptr, rows_, R, tl, out.ptr)
    else:
        raise ValueError(op)
    sh.sync()
    r.tags = sh.route_take()
    r.J = c["J"] if op != "pp" else J
    r.u = u
    r.pre, r.post = out.img, out.download()
    for b in keep:
        if isinstance(b, _In):
            b.check(c["name"])
    if op in ("mttv", "pp") and armed:
        assert np.array_equal(plain.download(), r.post), f"{c['name']}: the armed call's result differs in bits"
        _check_system(c["name"], *armed, R)
    return r


class _Refused(Exception):
    def __init__(self, tags):
        self.tags = tags


def run_checked(sh, c, hip, ncu=None, log=None):
    """run_case with the table's conventions: device-bound cases skip (Skip) off 256 CUs, a refused
    ttm_lead_front that the case expects counts as passed. Returns the tags."""
    if hip and c.get("dev") and ncu != 256:
        raise Skip(f"{c['name']}: sized for 256 CUs, this device has {ncu}")
    try:
        return run_case(sh, c, hip, log)
    except _Refused as e:
        return e.tags


# ------------------------------------------------------------------------------------------ the table
CASES = []
_seed = [1000]


def _add(op, name, route, why, **kw):
    _seed[0] += 1
    kw.setdefault("cls", "pos" if _seed[0] % 2 else "mix")
    c = dict(op=op, name=f"{op}:{name}", route=route if isinstance(route, list) else [route], why=why,
             seed=_seed[0], **kw)
    CASES.append(c)
    return c


def scan(name, dt, L, J, T, R, route, why, **kw):
    return _add("scan", name, route, why, dt=dt, L=L, J=J, T=T, R=R, family=kw.pop("family", "scan_" + (
        "prefix" if L == 1 and dt != "bf16" else "bf16" if dt == "bf16" else "suffix")), **kw)


SUF = r"scan\.%s\.suffix\.%s nt=%d nsplit=%s nts=%d pad=%d out32=%d"
GEN = r"scan\.%s\.suffix\.generic al=0 nt=%d nsplit=%s pad=%d out32=%d"

# ---- suffix / batched, every kernel -------------------------------------------------------------
for dt in ("f32", "f64"):
    v = VEC[dt]
    tile = 64 * v
    # generic: rows no multiple of the vector, and aligned extents on a base pointer one element off
    scan(f"{dt} generic L%VEC", dt, tile + v + 1, 37, 1, 17, GEN % (dt, 2, "1", 0, 0), "rows not vector multiple")
    scan(f"{dt} generic base+1", dt, 2 * tile, 33, 1, 16, GEN % (dt, 1, "1", 0, 0), "misaligned base, aligned extents",
         voff=1)
    for L in (2, 3):  # (two rows of an fp64 tensor are one whole vector: the buffer kernel's smallest shape)
        scan(f"{dt} M<VEC L={L}", dt, L, 40, 5 if L == 3 else 1, 3,
             SUF % (dt, "buf", 1, "1", 0, 0, 0) if (dt, L) == ("f64", 2) else GEN % (dt, 1, r"\d+", 0, 0),
             "fewer rows than a vector", form="ttm")
    # R: ragged n-tiles, a second column pass, three n-tiles
    for R in (1, 3, 16, 17, 33, 40, 48, 49, 64, 70, 100):
        nt = lambda n: 1 if n <= 16 else 2 if n <= 32 else 3 if n <= 48 else 4
        first = nt(min(R, 64))
        kern = "buf" if (dt == "f64" or first == 1) else "fast"
        pats = [SUF % (dt, kern, first, "1", 0, 0, 0)]
        if R > 64:
            n2 = nt(R - 64)
            pats.append(SUF % (dt, "buf" if (dt == "f64" or n2 == 1) else "fast", n2, "1", 0, 0, 0))
        scan(f"{dt} {kern} R={R}", dt, tile + 2 * v, 19, 1, R, pats, "ragged n-tiles, column passes")
    # L one below / above a tile edge (rows stay a vector multiple: the aligned kernels)
    scan(f"{dt} buf L=tile-VEC", dt, tile - v, 21, 1, 5, SUF % (dt, "buf", 1, "1", 0, 0, 0), "row tile edge below")
    scan(f"{dt} buf L=tile+VEC", dt, tile + v, 21, 1, 5, SUF % (dt, "buf", 1, "1", 0, 0, 0), "row tile edge above")
    scan(f"{dt} generic L=tile-1", dt, tile - 1, 21, 1, 20, GEN % (dt, 2, "1", 0, 0), "row tile edge, unaligned")
    scan(f"{dt} generic L=tile+1", dt, tile + 1, 21, 1, 20, GEN % (dt, 2, "1", 0, 0), "row tile edge, unaligned")
    # T = 1 with k-split (nblk >= 64): J with a shorter last split; through the slab, out32 and not
    Jk = 64 * 4 * v + 4 * 4 * v + 3  # 69 k-blocks, the last one ragged: splits of 35 and 34
    kern = "fast"
    scan(f"{dt} ksplit T=1", dt, tile + v, Jk, 1, 20, SUF % (dt, kern, 2, "2", 0, 0, 0), "ragged last k-split",
         dev=True)
    scan(f"{dt} ksplit T=1 out32", dt, 2 * tile, Jk, 1, 7, SUF % (dt, "buf" if dt == "f32" else "fast", 1, "2", 0, 0, 1),
         "slab then fp32 store", out="f32", dev=True)
    # T > 1 without and with the small-tensor k-split (nblk >= 8 and fewer tiles than CUs)
    scan(f"{dt} batched", dt, tile + v, 5 * 4 * v, 3, 18, SUF % (dt, "buf" if dt == "f64" else "fast", 2, "1", 0, 0, 0),
         "batched, no split", form="ttm")
    scan(f"{dt} batched ksplit", dt, tile + v, 9 * 4 * v + 1, 3, 18, SUF % (dt, "fast", 2, r"[2-9]", 0, 0, 0),
         "batched small-tensor k-split", form="ttm", dev=True)
    # the stride forms: mode in place, and strides larger than packed (odd: the scalar-store epilogue)
    scan(f"{dt} inplace", dt, tile + v, 23, 4, 6, SUF % (dt, "buf", 1, "1", 0, 0, 0), "mode-in-place strides",
         form="inplace")
    scan(f"{dt} inplace gaps", dt, 3 * v, 23, 4, 20, SUF % (dt, "buf" if dt == "f64" else "fast", 2, "1", 0, 0, 0),
         "in-place, both strides wide", form="inplace", tgap=3, rgap=5)
    scan(f"{dt} ttm gaps", dt, tile + v, 23, 3, 6, SUF % (dt, "buf", 1, "1", 0, 0, 0), "rank-last, both strides wide",
         form="ttm", tgap=v, rgap=1)
    scan(f"{dt} out32", dt, tile + v, 50, 1, 40, SUF % (dt, "buf" if dt == "f64" else "fast", 3, "1", 0, 0, 1),
         "fp32 result store", out="f32")
    scan(f"{dt} two factors", dt, 2 * v, 6 * 7, 2, 5, SUF % (dt, "buf", 1, "1", 0, 0, 0), "Khatri-Rao of two, ld > rows",
         fac=[6, 7], fld=3, form="ttm")
    # padded rows (valid < ld) on buf, fast, generic and through the slab
    ld = 8 * v
    scan(f"{dt} pad buf", dt, 9 * ld, 21, 1, 9, SUF % (dt, "buf", 1, "1", 0, 1, 0), "padded rows compacted",
         pad=(ld, ld - 3))
    scan(f"{dt} pad {'buf4' if dt == 'f64' else 'fast'}", dt, 9 * ld, 21, 2, 50,
         SUF % (dt, "buf" if dt == "f64" else "fast", 4, "1", 0, 1, 0), "padded rows, four n-tiles", pad=(ld, ld - 1),
         form="ttm")
    scan(f"{dt} pad generic", dt, 9 * ld, 21, 1, 9, GEN % (dt, 1, "1", 1, 0), "padded rows, unaligned base",
         pad=(ld, ld - 3), voff=1)
    scan(f"{dt} pad slab", dt, 9 * ld, Jk, 1, 9, SUF % (dt, "buf" if dt == "f32" else "fast", 1, "2", 0, 1, 0),
         "padding compacted by combine", pad=(ld, ld - 2), dev=True)
    scan(f"{dt} pad slab out32", dt, 9 * ld, Jk, 1, 9, SUF % (dt, "buf" if dt == "f32" else "fast", 1, "2", 0, 1, 1),
         "out32 + k-split + padding", pad=(ld, ld - 2), out="f32", dev=True)
    # forced non-temporal stores
    scan(f"{dt} buf nts", dt, tile + v, 21, 1, 5, SUF % (dt, "buf", 1, "1", 1, 0, 0), "forced non-temporal stores",
         store=1)
# fp64: buf with 1..4 n-tiles is covered by R above; fp32 fast with 2..4 n-tiles likewise
scan("f32 fast nts", "f32", 260, 21, 1, 40, SUF % ("f32", "fast", 3, "1", 1, 0, 0), "forced non-temporal stores", store=1)
scan("f64 fast ksplit nts", "f64", 130, 64 * 8, 1, 5, SUF % ("f64", "fast", 1, "2", 0, 0, 0),
     "k-split never non-temporal", store=1, dev=True)
# tail mode (fp32, two n-tiles, a round and a bit of resident workgroups: 586 / 520 tiles on 512 slots).
# J = 160 needs 85 MB of tensor: the tail mode exists only past 512 row tiles of 256 rows.
TAIL = r"scan\.f32\.suffix\.tail nt=2 from=512"
for J, L in ((1, 586 * 256), (17, 586 * 256), (160, 520 * 256)):
    scan(f"f32 tail J={J}", "f32", L, J, 1, 20, TAIL, "tail mode quarter items", dev=True, tail=True)

# ---- wide (fp32, more than 64 columns, L*J*T >= 1e6) ---------------------------------------------
WIDE = r"scan\.f32\.wide nt=%d nsplit=\d+ pad=%d out32=%d"
for R, pats in ((65, [WIDE % (5, 0, 0)]), (100, [WIDE % (7, 0, 0)]), (128, [WIDE % (8, 0, 0)]),
                (129, [WIDE % (8, 0, 0), SUF % ("f32", "buf", 1, r"\d+", 0, 0, 0)]),
                (200, [WIDE % (8, 0, 0), WIDE % (5, 0, 0)])):
    scan(f"wide R={R}", "f32", 1000, 1000, 1, R, pats, "wide pass, ragged columns", family="scan_wide")
scan("wide batched", "f32", 100, 100, 100, 100, WIDE % (7, 0, 0), "wide, batched", family="scan_wide", form="ttm")
scan("wide padded", "f32", 8 * 128, 1000, 1, 70, WIDE % (5, 1, 0), "wide, padded rows", family="scan_wide",
     pad=(128, 125))
scan("wide out32", "f32", 1000, 1000, 1, 100, WIDE % (7, 0, 1), "wide, fp32 result", family="scan_wide", out="f32")
scan("wide fallback L%4", "f32", 1001, 1000, 1, 100, [GEN % ("f32", 4, r"\d+", 0, 0), GEN % ("f32", 3, r"\d+", 0, 0)],
     "unaligned rows: passes of 64", family="scan_wide")

# ---- prefix (L = 1) ------------------------------------------------------------------------------
PFAST = r"scan\.%s\.prefix\.fast nt=%d nsplit=%s out32=%d"
PGEN = r"scan\.%s\.prefix\.generic al=0 nt=%d nsplit=%s out32=%d"
for dt in ("f32", "f64"):
    v = VEC[dt]
    scan(f"{dt} prefix fast", dt, 1, 9 * 4 * v, 70, 20, PFAST % (dt, 2, "1", 0), "T off 16 and 64")
    scan(f"{dt} prefix fast T=13", dt, 1, 5 * v, 13, 3, PFAST % (dt, 1, "1", 0), "fewer columns than a group")
    scan(f"{dt} prefix fast R=100", dt, 1, 7 * v, 130, 100, [PFAST % (dt, 4, "1", 0), PFAST % (dt, 3, "1", 0)],
         "two column passes")
    scan(f"{dt} prefix generic J%VEC", dt, 1, 9 * 4 * v + 1, 70, 20, PGEN % (dt, 2, "1", 0), "rows not vector multiple")
    scan(f"{dt} prefix generic base+1", dt, 1, 8 * v, 33, 5, PGEN % (dt, 1, "1", 0), "misaligned base", voff=1)
    scan(f"{dt} prefix J<VEC", dt, 1, v - 1, 100, 17, PGEN % (dt, 2, "1", 0), "reduction shorter than vector")
    scan(f"{dt} prefix ksplit out32", dt, 1, 128 * 4 * v + 4 * v + 2 * v, 50, 20, PFAST % (dt, 2, "2", 1),
         "slab then fp32 store", out="f32", dev=True)
    scan(f"{dt} prefix ksplit gaps", dt, 1, 128 * 4 * v + 3, 50, 5, PGEN % (dt, 1, "2", 0), "generic split, wide strides",
         rgap=7, dev=True)

# ---- bf16 ----------------------------------------------------------------------------------------
MF = r"scan\.bf16\.mfma nsplit=%s nts=0 pad=%d out32=%d"
for L, J, R in ((8, 1, 1), (504, 31, 16), (512, 32, 17), (520, 33, 40), (512, 95, 16), (8, 95, 3)):
    scan(f"bf16 mfma L={L} J={J} R={R}", "bf16", L, J, 1, R, MF % ("1", 0, 0), "ragged k-block, flush parity")
scan("bf16 ksplit", "bf16", 520, 32 * 32 + 40, 1, 17, MF % ("2", 0, 0), "k-split, ragged last", dev=True)
scan("bf16 batched", "bf16", 520, 95, 3, 5, MF % ("1", 0, 0), "batched", form="ttm")
scan("bf16 batched ksplit", "bf16", 24, 8 * 32 + 1, 3, 5, MF % (r"[2-9]", 0, 0), "batched k-split", form="ttm", dev=True)
scan("bf16 padded", "bf16", 9 * 64, 33, 1, 17, MF % ("1", 1, 0), "padded rows", pad=(64, 61))
scan("bf16 out32 inplace", "bf16", 520, 33, 2, 17, MF % ("1", 0, 1), "fp32 result, in place", out="f32", form="inplace")
scan("bf16 padded ksplit out32", "bf16", 9 * 64, 32 * 32 + 40, 1, 5, MF % ("2", 1, 1), "out32 + k-split + padding",
     pad=(64, 61), out="f32", dev=True)
scan("bf16 rows L%8", "bf16", 516, 33, 2, 17, r"scan\.bf16\.rows", "rows no multiple of 8", form="ttm")
scan("bf16 rows base", "bf16", 512, 33, 1, 5, r"scan\.bf16\.rows", "misaligned base", voff=1)
scan("bf16 prefix", "bf16", 1, 95, 70, 17, r"scan\.bf16\.prefix", "prefix fallback")


# ---- mttv: six routes x fp32 / fp64 X ------------------------------------------------------------
def mttv(name, dt, L, J, T, R, route, why, **kw):
    return _add("mttv", name, route, why, dt=dt, L=L, J=J, T=T, R=R, family="mttv", **kw)


for dt in ("f32", "f64"):
    vl = 16 // (4 if dt == "f32" else 8)
    shapes = {
        "1": (1, 35, 50, 5, [5, 7], rf"mttv\.{dt}\.1"),
        "vec": (16 * vl, 6, 32, 32, [2, 3], rf"mttv\.{dt}\.vec"),
        "s": (6, 6, 64, 32, [3, 2], rf"mttv\.{dt}\.s"),
        "l4": (30, 6, 16, 16, [2, 3], rf"mttv\.{dt}\.l4 jsplit=1"),
        "l16": (30, 40, 2, 3, [5, 8], rf"mttv\.{dt}\.l16 jsplit=1"),
        # 60 blocks -> 17 chunks of 65 columns, the last one of 60: 1100 = 16 * 65 + 60
        "jsplit": (70, 1100, 2, 15, [25, 44], rf"mttv\.{dt}\.l4 jsplit=17"),
    }
    for rt, (L, J, T, R, fac, pat) in shapes.items():
        for acc in (0, 1):
            for scale in (None, -0.75):
                mttv(f"{dt} {rt} acc={acc} scale={scale}", dt, L, J, T, R, pat + " extra=0", "accumulate x out_scale",
                     acc=acc, scale=scale)
        mttv(f"{dt} {rt} rstride", dt, L, J, T, R, pat + " extra=0", "rstride above L*T", rgap=3, acc=1)
        mttv(f"{dt} {rt} krp", dt, L, J, T, R, pat + " extra=0", "two-factor Khatri-Rao", fac=fac)
        mttv(f"{dt} {rt} ld>J", dt, L, J, T, R, pat + " extra=0", "factor ld above J", fld=3, scale=1.5)
        mttv(f"{dt} {rt} armed", dt, L, J, T, R, pat + " extra=1", "extra workgroup prepares S", arm=True)


# ---- ttm_keep / ttm_lead_front ---------------------------------------------------------------------
def ttm(op, name, dt, L, J, T, Kc, route, why, **kw):
    return _add(op, name, route, why, dt=dt, L=L, J=J, T=T, Kc=Kc, family=op, **kw)


for op, tag in (("ttm_keep", "ttm_keep"), ("ttm_lead", "ttm_lead")):
    for dt in ("f32", "f64"):
        combos = [(16, 16, 1, 1), (17, 17, 16, 3), (31, 50, 17, 1), (16, 50, 32, 3), (17, 16, 33, 1), (31, 17, 48, 3),
                  (17, 50, 64, 1)]
        for L, J, Kc, T in combos:
            nt = 1 if Kc <= 16 else 2 if Kc <= 32 else 4
            ttm(op, f"{dt} L={L} J={J} Kc={Kc} T={T}", dt, L, J, T, Kc, rf"{tag}\.gemm nt={nt}", "ragged GEMM tiles",
                fld=(5 if Kc in (17, 48) else 0))
        for L, J, Kc, what in ((15, 16, 16, "L"), (16, 15, 16, "J"), (16, 16, 65, "Kc")):
            if op == "ttm_keep":
                ttm(op, f"{dt} fallback {what}", dt, L, J, 2, Kc, [r"ttm_keep\.scan", rf"scan\.{dt}\.suffix\.\w+"],
                    "GEMM condition fails: scan")
            else:
                ttm(op, f"{dt} refused {what}", dt, L, J, 2, Kc, r"ttm_lead\.refused", "GEMM condition fails: false",
                    refused=True)


# ---- pp_correct ------------------------------------------------------------------------------------
def pp(name, rows, R, terms, why, **kw):
    return _add("pp", name, rf"pp_correct terms={len(terms)} extra={1 if kw.get('arm') else 0}", why, rows=rows, R=R,
                terms=terms, family="pp_correct", **kw)


_T7 = [(5, 1, 0), (16, 0, 0), (17, 1, 2), (64, 0, 3), (65, 1, 0), (130, 0, 1), (49, 1, 0)]
for i, (rows, R) in enumerate(((1, 1), (15, 10), (16, 33), (17, 10), (200, 33), (200, 1), (17, 33))):
    n = i + 1
    pp(f"rows={rows} R={R} terms={n}", rows, R, _T7[:n], "mixed keep_first, lddw > ny")
    if R <= 32:
        pp(f"rows={rows} R={R} terms={n} armed", rows, R, _T7[7 - n:], "extra column prepares S", arm=True)

FAMILIES = sorted({c["family"] for c in CASES})

# Every tag family the launchers can log (the test collects the tags of all cases and compares). The aligned
# instantiations of the generic suffix / prefix kernels (al=1) are not here: the launchers send every aligned shape
# with M >= VEC to the fast or buffer kernels, and an aligned M < VEC does not exist.
EXPECTED_TAGS = sorted(
    [f"scan.{dt}.suffix.{k}" for dt in ("f32", "f64") for k in ("generic", "fast", "buf")] + ["scan.f32.suffix.tail"] +
    [f"scan.{dt}.prefix.{k}" for dt in ("f32", "f64") for k in ("generic", "fast")] +
    ["scan.f32.wide", "scan.bf16.mfma", "scan.bf16.rows", "scan.bf16.prefix"] +
    [f"mttv.{dt}.{k}" for dt in ("f32", "f64") for k in ("1", "vec", "s", "l4", "l16")] +
    ["mttv.f32.l4+jsplit", "mttv.f64.l4+jsplit", "ttm_keep.gemm", "ttm_keep.scan", "ttm_lead.gemm", "ttm_lead.refused",
     "pp_correct"])


def tag_family(tag):
    """`scan.f32.suffix.fast nt=2 ...` -> `scan.f32.suffix.fast`; a j-split mttv is a route of its own"""
    head = tag.split(" ")[0]
    m = re.search(r"jsplit=(\d+)", tag)
    return head + "+jsplit" if (m and int(m.group(1)) > 1) else head
