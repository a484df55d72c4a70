"""Op-level cases of the mode-update, Normalize and factor-side kernels and their one checker
(tests/test_gpu_updates.py on the HIP kernels, tests/test_updates_hostsim.py on the host stand-in, both through
tests/opshim), in the style of tests/contraction_cases.py, whose buffers and image checker are used here.

A case is a plain dict: the op, its arguments, `route` (regular expressions each of which must match a tag of the
calls' route log; computed from the launchers' own formulas below, not copied from a run) and `why`.

Per case: inputs from a seed ("pos" = uniform[0.5, 1), "mix" = uniform[-1, 1)), every input followed by 4 KiB of NaN,
every output between two 4 KiB NaN guards with NaN in every leading-dimension gap; after the calls every byte outside
the results is unchanged and no result is NaN. Every case runs TWICE on fresh buffers and the two sets of output
images must be equal bit for bit (the kernels' summation orders are fixed).

References are numpy in long double; u = 2^-53. The bars are componentwise and derived:
* S against the Hadamard product of the input Grams + lambda I: N u (|H| + |lambda|) (N - 2 products, one sum);
* S^-1 only through ||S^-1 S_ref - I||_F / ||I||_F < 1e-10 cond and symmetry to 1e-13 (test_gpu_normal_equations.py);
  the systems are crafted with cond <= 1e3 (asserted by the builder), the indefinite ones with one negative
  eigenvalue and cond <= 16 (asserted);
* grad against W_old S_dev - M with the S the device wrote: (R + 3) u (|W_old| |S_dev| + |M|); W against M Sinv_dev:
  (R + 3) u |M| |Sinv_dev| — the conditioning of S never enters;
* with Winit: b = fl(M Sinv) carries E_b = (R + 3) u |M||Sinv|; d = fl(ratio fl(b - wi)) is two roundings on top:
      |d - ratio (b_ref - wi)| <= |ratio| (E_b + 2u (|b_ref - wi| + E_b))                  =: E_d
  and w = fl(wi + d) (possibly contracted into one fma, which only drops a rounding) one more:
      |w - (wi + d_ref)| <= E_d + u (|wi| + |d_ref| + E_d);
* S / Sinv passed as null: W under 1e-10 cond in Frobenius norm against M inv(S_ref), grad against W_old S_ref with
  (R + 3 + N) u (|W_old||S_ref| + |M|) (the N u |S| error of the S nobody saw, times |W_old|);
* sums of squares (gradsq, dwsq, sumsq, diff_norms) against the long-double sum of the squares of the values the
  device wrote: n u relative, n the number of terms (each square rounds once, n - 1 additions in any order);
* Gram against W_dev^T W_dev: (rows + 3) u |W|^T |W|, and G == G.T bit for bit;
* pack / unpack: exact; scale_update: popcount(mask) u relative, untouched entries bit for bit;
* Normalize: f_i = (prod_j n_j)^(1/N) / n_i, n_i = sqrt(trace G_i). Derived: the trace is R positive terms,
  (R - 1) u; the root halves that and rounds, e_n = ((R - 1) / 2 + 1) u; the product of N roots N e_n + N u, of which
  the N-th root keeps 1/N, plus u |ln prod| / N for the rounded exponent 1.0 / N, plus the error of pow itself;
  the division e_n + u:   rel(f_i) <= 2 e_n + 2u + u |ln prod| / N + POW_ALLOW   =: E_f.
  Factors f_i w: E_f + u. Grams G f^2: 2 E_f + 2u. ms_dst: popcount (E_f + u). wsq[2i] = (n_i f_i)^2 from the
  trace (the fused kernels): 2 (e_n + E_f + u) + u. Only where wsq is the sum over the scaled factor's entries
  (Ops::normalize_ms through sumsq: the normalize.grid route and the stand-in) that sum's n_i u and the
  (rows_i + R) u between the Gram's trace and the exact ||W_i||^2 come on top.
  POW_ALLOW is measured, not guessed: profiles/update_ops_bars.md.
"""
import re

import numpy as np

import contraction_cases as CC
from contraction_cases import check_image, check_route

U = 2.0 ** -53
LD = np.longdouble
TINY = np.finfo(np.float64).tiny
# 4 x the largest deviation of the device's scales from the long-double reference on the unfused route
# (normalize.grid), in units of u: profiles/update_ops_bars.md
POW_ALLOW = 4 * 3.73 * U
WORST = {}  # family -> largest err / bar seen (profiles/update_ops_bars.md)
SCALE_DEV = []  # |f_dev / f_ref - 1| / u of every Normalize on the grid route (the measurement behind POW_ALLOW)


def lds_bytes(R):
    return 8 * (4 * R * R + 2 * R + 96) + 256


def staged(rows, R):
    """the launchers' limit of the staged launch (hip_ops.hip, R x R side)"""
    return lds_bytes(R) + 16 * rows * R <= 150 * 1024


def update_route(rows, R, jacobi=False):
    if R > 64:
        return "unfused why=R"
    if jacobi:
        return "unfused why=jacobi"
    if staged(rows, R):
        return "staged"
    return "unfused why=rows" if rows * R > 6144 else "unstaged"


# ------------------------------------------------------------------------------------------ helpers
def vals(rng, cls, shape):
    x = rng.random(shape)
    return 0.5 + 0.5 * x if cls == "pos" else 2.0 * x - 1.0


def colmajor(A, ld):
    """rows x cols -> the flat column-major image with leading dimension ld, NaN in the gap"""
    full = np.full((ld, A.shape[1]), np.nan)
    full[:A.shape[0]] = A
    return full.reshape(-1, order="F")


def midx(rows, cols, ld, col0=0):
    return (np.arange(rows)[:, None] + ld * (col0 + np.arange(cols))[None, :]).reshape(-1, order="F")


def mat(v, rows, cols):
    return np.asarray(v).reshape((rows, cols), order="F")


def within(st, what, got, ref, bar):
    got, ref, bar = np.asarray(got), np.asarray(ref, dtype=LD), np.asarray(bar, dtype=LD)
    if got.size == 0:
        return
    err = np.abs(got.astype(LD) - ref)
    ratio = float(np.max(err / np.maximum(bar, TINY)))
    fam = st.c["family"]
    WORST[fam] = max(WORST.get(fam, 0.0), ratio)
    if st.log is not None:
        st.log.append(f"{st.c['name']} {what}: max err/bar {ratio:.3g}")
    bad = np.argwhere(err > bar)
    assert bad.size == 0, (f"{st.c['name']} {what}: {len(bad)} elements over the bar, first at {tuple(bad[0])}: err "
                           f"{float(err[tuple(bad[0])]):.3e} bar {float(bar[tuple(bad[0])]):.3e}, worst err/bar {ratio:.3g}")


def sumsq_check(st, what, got, terms):
    t = np.asarray(terms, dtype=LD).reshape(-1)
    ref = np.sum(t * t)
    within(st, what, np.array([got]), np.array([ref]), np.array([t.size * U * ref]))


class St:
    """the buffers and the outcome of one run of a case"""

    def __init__(self, sh, c, hip, log):
        self.sh, self.c, self.hip, self.log = sh, c, hip, log
        self.rng = np.random.default_rng(c["seed"])
        self.keep, self.outs, self.posts, self.tags, self.verify = [], {}, {}, [], None

    def inp(self, flat):
        b = CC._In(self.sh, np.ascontiguousarray(flat, dtype=np.float64))
        self.keep.append(b)
        return b

    def out(self, name, n, res=None, idx=None, init=None, raw=False):
        """an output of n doubles; res: the elements the calls must write (default all), idx / init: elements that
        hold values beforehand; raw: contents unspecified, only the guards are checked"""
        o = CC._Out(self.sh, n, np.float64, idx, init)
        self.keep.append(o)
        self.outs[name] = (o, np.arange(n) if res is None else np.asarray(res, dtype=np.int64), raw)
        return o

    def finish(self):
        self.sh.sync()
        self.tags += self.sh.route_take()
        for name, (o, _, _) in self.outs.items():
            self.posts[name] = o.download()
        for b in self.keep:
            if isinstance(b, CC._In):
                b.check(self.c["name"])

    def got(self, name):
        o, res, raw = self.outs[name]
        what = f"{self.c['name']} {name}"
        if raw:
            post = self.posts[name]
            assert np.array_equal(post[:CC.GUARD], o.img[:CC.GUARD]) and \
                np.array_equal(post[-CC.GUARD:], o.img[-CC.GUARD:]), f"{what}: a guard was written"
            return post[CC.GUARD:-CC.GUARD].view(np.float64)
        return check_image(what, o.img, self.posts[name], np.float64, res)

    def free(self):
        for b in self.keep:
            b.free()


def run_case(sh, c, hip, log=None, perturb=None):
    """Runs a case twice on the shim `sh`, compares the two runs bit for bit and checks the second. perturb(st): the
    self-test's hook on the outcome before it is verified. Returns the route tags."""
    first = None
    for rep in (0, 1):
        st = St(sh, c, hip, log if rep else None)
        try:
            sh.route_take()
            OPS[c["op"]](st)
            if rep == 0:
                first = st.posts
                continue
            assert first.keys() == st.posts.keys()
            for k in first:
                assert np.array_equal(first[k], st.posts[k]), f"{c['name']} {k}: two runs differ in bits"
            if perturb:
                perturb(st)
            if st.verify:
                st.verify()
            for k in st.outs:  # (every output's guards and gaps, also those verify() did not read)
                st.got(k)
            if hip:
                check_route(c["name"], c, st.tags)
                for pat in c.get("not_route", []):
                    assert not any(re.match(pat, t) for t in st.tags), f"{c['name']}: route {pat!r} in {st.tags}"
            return st.tags
        finally:
            st.free()


# ------------------------------------------------------------------------------------------ systems
def make_grams(rng, N, mode, R, lam, indef):
    """Grams of the modes other than `mode` whose Hadamard product + lam I has cond <= 1e3, or (indef) the
    `one_negative` spectrum of test_gpu_normal_equations.py. Returns (list of N matrices, the mode's all NaN; lam;
    S_ref long double; |H|; cond)"""
    others = [j for j in range(N) if j != mode]
    Q, _ = np.linalg.qr(rng.standard_normal((R, R)))
    if indef:
        d, lam = np.concatenate([[1.0], np.linspace(3.0, 10.0, R - 1)]), -2.0
    else:
        d = np.logspace(0.0, 2.0, R) if R > 1 else np.array([1.5])
    A = (Q * d) @ Q.T
    Gs = [np.full((R, R), np.nan) for _ in range(N)]
    Gs[others[0]] = 0.5 * (A + A.T)
    for j in others[1:]:
        if indef:
            Gs[j] = np.ones((R, R))
        else:
            F = vals(rng, "mix", (4 * R + 8, R))
            Gs[j] = 3.0 * (F.T @ F) / (4 * R + 8)
    H = np.ones((R, R), dtype=LD)
    for j in others:
        H = H * Gs[j].astype(LD)
    S = H + LD(lam) * np.eye(R, dtype=LD)
    e = np.linalg.eigvalsh(S.astype(np.float64))
    cond = float(np.max(np.abs(e)) / np.min(np.abs(e)))
    if indef:
        assert np.sum(e < 0) == 1 and cond <= 16, (e, cond)
    else:
        assert e[0] > 0 and cond <= 1e3, (e[0], cond)
    return Gs, lam, S, np.abs(H), cond


def gall_flat(Gs):
    return np.concatenate([G.reshape(-1, order="F") for G in Gs])


def check_system(st, what, S, Si, S_ref, absH, lam, N, cond):
    R = S_ref.shape[0]
    within(st, what + "S", S, S_ref, N * U * (absH + abs(lam) * np.eye(R)))
    s64 = S_ref.astype(np.float64)
    res = np.linalg.norm(Si @ s64 - np.eye(R)) / np.sqrt(R)
    assert res < 1e-10 * cond, f"{st.c['name']} {what}Sinv: residual {res:.3e} over 1e-10 * cond {cond:.3g}"
    asym = np.linalg.norm(Si - Si.T) / np.linalg.norm(Si)
    assert asym < 1e-13, f"{st.c['name']} {what}Sinv: asymmetry {asym:.3e}"


def check_gram(st, what, G, W, rows):
    Wl = W.astype(LD)
    within(st, what, G, Wl.T @ Wl, (rows + 3) * U * (np.abs(W).T @ np.abs(W)))
    assert np.array_equal(G, G.T), f"{st.c['name']} {what}: not symmetric bit for bit"


def check_solve(st, what, c, M, Wold, S, Si, grad, Wnew, Winit, dW, gradsq, S_exact, extra=0):
    """grad, W (and dW) of one update against the S / S^-1 it used (module docstring). S_exact: S is the long-double
    reference (the device's was not returned): Si is then inv(S_ref) and W is held in Frobenius norm by the caller."""
    R = S.shape[0]
    Ml, Wl = M.astype(LD), Wold.astype(LD)
    within(st, what + "grad", grad, Wl @ S.astype(LD) - Ml, (R + 3 + extra) * U * (np.abs(Wold) @ np.abs(S).astype(np.float64) + np.abs(M)))
    sumsq_check(st, what + "gradsq", gradsq, grad)
    if S_exact:
        return
    b = Ml @ Si.astype(LD)
    Eb = (R + 3) * U * (np.abs(M) @ np.abs(Si))
    if Winit is None:
        within(st, what + "W", Wnew, b, Eb)
        return
    ratio, wi = c.get("ratio", 1.0), Winit.astype(LD)
    d = LD(ratio) * (b - wi)
    Ed = abs(ratio) * (Eb + 2 * U * (np.abs(b - wi) + Eb))
    within(st, what + "dW", dW, d, Ed)
    if ratio == 1.0:
        within(st, what + "W", Wnew, b, Eb)
    else:
        within(st, what + "W", Wnew, wi + d, Ed + U * (np.abs(wi) + np.abs(d) + Ed))


# ------------------------------------------------------------------------------------------ gram, gram_system
def op_gram(st):
    c, sh = st.c, st.sh
    rows, R, nb = c["rows"], c["R"], c.get("nstarts", 0)
    K, ld, gs = max(nb, 1), rows + c.get("xld", 0), c.get("gstride", R * R)
    W = vals(st.rng, c["cls"], (rows, R * K))
    w = st.inp(colmajor(W, ld))
    res = np.concatenate([b * gs + np.arange(R * R) for b in range(K)])
    g = st.out("G", gs * (K - 1) + R * R, res=res)
    if nb:
        sh.gram_batched(w.ptr, rows, ld, R, nb, g.ptr, gs)
    else:
        sh.gram(w.ptr, rows, ld, R, g.ptr)
    st.finish()

    def verify():
        G = st.got("G").reshape(K, R * R)
        for b in range(K):
            check_gram(st, f"G[{b}]", mat(G[b], R, R), W[:, b * R:(b + 1) * R], rows)
    st.verify = verify


def _pp_dummy(st, R):
    """one small pp_correct: the launch an armed system rides on (its own result is checked by the contraction tests)"""
    rows, ny = 4, 3
    m0 = st.inp(vals(st.rng, "mix", rows * R))
    T = st.inp(vals(st.rng, "mix", rows * ny * R))
    dW = st.inp(vals(st.rng, "mix", ny * R))
    o = st.out("pp.M", rows * R)
    st.sh.pp_correct(m0.ptr, rows, R, [(T.ptr, ny, 1, dW.ptr, ny)], o.ptr)


def op_gram_system(st):
    c, sh = st.c, st.sh
    N, mode, R = c["N"], c["mode"], c["R"]
    Gs, lam, S_ref, absH, cond = make_grams(st.rng, N, mode, R, c.get("lam", 0.0), c.get("indef", False))
    gall = st.inp(gall_flat(Gs))
    S, Si = st.out("S", R * R), st.out("Sinv", R * R)
    if c.get("armed"):  # hazard e: prepared by the contraction, consumed by gram_system, then computed again
        sh.arm_gram_system(gall.ptr, N, mode, R, lam, S.ptr, Si.ptr)
        _pp_dummy(st, R)
        sh.gram_system(gall.ptr, N, mode, R, lam, S.ptr, Si.ptr)
    sh.gram_system(gall.ptr, N, mode, R, lam, S.ptr, Si.ptr)
    st.finish()
    st.verify = lambda: check_system(st, "", mat(st.got("S"), R, R), mat(st.got("Sinv"), R, R), S_ref, absH, lam, N,
                                     cond)


# ------------------------------------------------------------------------------------------ cp_update
def cp_update_route(c):
    rows, R = c["rows"], c["R"]
    if rows == 0:
        return r"cp_update\.empty"
    packed = not (c.get("xg") or c.get("xn") or (c.get("alias", True) and c.get("xw")))
    if R > 64 and packed and (not c.get("winit") or c.get("ratio", 1.0) == 1.0):
        return rf"cp_update\.gemm tail={1 if c.get('winit') else 0}"
    return r"cp_update\.rows" if (R > 64 or rows * R > 6144) else r"cp_update\.one"


def op_cp_update(st):
    c, sh, rng = st.c, st.sh, st.rng
    rows, R, alias = c["rows"], c["R"], c.get("alias", True)
    ldm, ldw, ldg = rows + c.get("xm", 0), rows + c.get("xw", 0), rows + c.get("xg", 0)
    ldn = ldw if alias else rows + c.get("xn", 0)
    ldi, ldd = rows + c.get("xi", 0), rows + c.get("xd", 0)
    Q, _ = np.linalg.qr(rng.standard_normal((R, R)))
    S = (Q * np.logspace(0.0, 2.0, R)) @ Q.T
    S = 0.5 * (S + S.T)
    Si = np.linalg.inv(S)
    Si = 0.5 * (Si + Si.T)
    assert np.linalg.cond(S) <= 1e3
    M, Wold = vals(rng, c["cls"], (rows, R)), vals(rng, c["cls"], (rows, R))
    Winit = vals(rng, c["cls"], (rows, R)) if c.get("winit") else None
    m, s, si = st.inp(colmajor(M, ldm)), st.inp(S.reshape(-1, order="F")), st.inp(Si.reshape(-1, order="F"))
    iw = midx(rows, R, ldw)
    if alias:
        wn = wo = st.out("W", ldw * R, res=iw, idx=iw, init=Wold.reshape(-1, order="F"))
    else:
        wo, wn = st.inp(colmajor(Wold, ldw)), st.out("W", ldn * R, res=midx(rows, R, ldn))
    g, gq = st.out("grad", ldg * R, res=midx(rows, R, ldg)), st.out("gradsq", 1)
    wi = dw = None
    if Winit is not None:
        wi, dw = st.inp(colmajor(Winit, ldi)), st.out("dW", ldd * R, res=midx(rows, R, ldd))
    try:
        sh.cp_update(m.ptr, ldm, wo.ptr, ldw, wn.ptr, ldn, g.ptr, ldg, rows, R, s.ptr, si.ptr, gq.ptr,
                     wi.ptr if wi else 0, ldi, dw.ptr if dw else 0, ldd, c.get("ratio", 1.0))
    except Exception as e:  # (ShimError: the launcher's refusal)
        assert c.get("raises") and c["raises"] in str(e), f"{c['name']}: {e}"
        sh.sync()
        st.tags += sh.route_take()
        st.outs.clear()  # (what a refused call wrote before it noticed is unspecified)
        return
    assert not (c.get("raises") and st.hip), f"{c['name']}: the call was not refused"
    st.finish()

    def verify():
        gq_ = st.got("gradsq")[0]
        if rows == 0:
            assert gq_ == 0.0, gq_
            return
        check_solve(st, "", c, M, Wold, S, Si, mat(st.got("grad"), rows, R), mat(st.got("W"), rows, R), Winit,
                    mat(st.got("dW"), rows, R) if Winit is not None else None, gq_, False)
    st.verify = verify


# ------------------------------------------------------------------------------------------ mode updates
def op_update(st):
    """cp_mode_update (kind plain), _batched, _blocked; the state hazards (`pre`) and the armed Normalize (`norm`)"""
    c, sh, rng = st.c, st.sh, st.rng
    kind, N, mode, R, rows = c.get("kind", "plain"), c["N"], c["mode"], c["R"], c["rows"]
    K = c.get("nstarts", 1)
    ldm, ldw, ldg = rows + c.get("xm", 0), rows + c.get("xw", 0), rows + c.get("xg", 0)
    ldi, ldd = rows + c.get("xi", 0), rows + c.get("xd", 0)
    null, pre, norm = c.get("null", False), c.get("pre"), c.get("norm")
    RR = R * R
    sysb = [make_grams(rng, N, mode, R, c.get("lam", 0.0), b in c.get("indef", ())) for b in range(K)]
    assert len({s[1] for s in sysb}) == 1 or kind == "batched"
    lam = c.get("lam", 0.0) if (kind == "batched" and K > 1) else sysb[0][1]
    if kind == "batched" and K > 1 and c.get("indef"):  # one lambda for all starts: the indefinite start's
        lam = -2.0
        sysb = [s if b in c["indef"] else _shift(s, lam) for b, s in enumerate(sysb)]
    M, W0 = vals(rng, c["cls"], (rows, R * K)), vals(rng, c["cls"], (rows, R * K))
    Winit = vals(rng, c["cls"], (rows, R)) if c.get("winit") else None
    pad = 1 if kind == "batched" else 0  # an unused start's worth behind the last one: must stay NaN
    nrm_in = None
    if norm:
        assert ldw == rows and K == 1
        nrows = [r + R for r in norm["rows"]]
        nrows[mode] = rows
        # the other modes' factors are built to HAVE the crafted Grams (W = Q L^T with G = L L^T, at least R rows), so
        # that trace(G_i) is ||W_i||^2 as Normalize assumes while S keeps its cond (asserted again)
        nrm_in = [None] * N
        for i in range(N):
            if i != mode:
                Qr, _ = np.linalg.qr(rng.standard_normal((nrows[i], R)))
                nrm_in[i] = Qr @ np.linalg.cholesky(sysb[0][0][i]).T
                sysb[0][0][i] = nrm_in[i].T @ nrm_in[i]
        sysb[0] = _resystem(sysb[0], N, mode, R, lam)

    def launch(tag, armed):
        """one whole run on a fresh set of buffers, named with the prefix `tag`"""
        o = {}
        gflat = np.concatenate([gall_flat(s[0]) for s in sysb])
        keepi = np.flatnonzero(~np.isnan(gflat))
        gres = np.concatenate([(b * N + mode) * RR + np.arange(RR) for b in range(K)])
        if armed:
            gres = np.arange(N * RR)
        o["G"] = st.out(tag + "G", (K + pad) * N * RR, res=gres, idx=keepi, init=gflat[keepi])
        if kind == "blocked":
            blk, P = c["blk"], c["P"]
            Mb = np.zeros((blk * P, R))
            Mb[:rows] = M
            mflat = np.concatenate([Mb[p * blk:(p + 1) * blk].reshape(-1, order="F") for p in range(P)])
            o["M"] = st.inp(mflat)
            o["scratch"] = st.out(tag + "scratch", rows * R, raw=True)
        else:
            o["M"] = st.inp(colmajor(M, ldm))
        iw = midx(rows, R * K, ldw)
        o["W"] = st.out(tag + "W", ldw * R * (K + pad), res=iw, idx=iw, init=W0.reshape(-1, order="F"))
        o["grad"] = st.out(tag + "grad", ldg * R * (K + pad), res=midx(rows, R * K, ldg))
        o["gradsq"] = st.out(tag + "gradsq", K + pad, res=np.arange(K))
        if not null:
            o["S"] = st.out(tag + "S", (K + pad) * RR, res=np.arange(K * RR))
            o["Sinv"] = st.out(tag + "Sinv", (K + pad) * RR, res=np.arange(K * RR))
        S, Si = (0, 0) if null else (o["S"].ptr, o["Sinv"].ptr)
        wi = dw = dq = 0
        if Winit is not None:
            o["Winit"] = st.inp(colmajor(Winit, ldi))
            o["dW"] = st.out(tag + "dW", ldd * R, res=midx(rows, R, ldd))
            wi, dw = o["Winit"].ptr, o["dW"].ptr
            if c.get("dwsq"):
                o["dwsq"] = st.out(tag + "dwsq", 1)
                dq = o["dwsq"].ptr
        G = o["G"].ptr
        if pre:  # the state hazards a-d, f: a system armed and prepared in front of this update
            alam, amode, aS, aSi = lam, mode, S, Si
            if pre == "lambda":
                alam = lam + 0.5
            elif pre == "mode":
                amode = (mode + 1) % N
            elif pre == "pointers":
                aS, aSi = st.out(tag + "S2", RR, raw=True).ptr, st.out(tag + "Sinv2", RR, raw=True).ptr
            if pre == "mode":  # (the other mode's system reads this mode's Gram: give it one)
                g2 = gflat.copy()
                g2[np.isnan(g2)] = 1.0
                G2 = st.inp(g2)
                sh.arm_gram_system(G2.ptr, N, amode, R, alam, aS, aSi)
            else:
                sh.arm_gram_system(G, N, amode, R, alam, aS, aSi)
            _pp_dummy(st, R)
            st.outs[tag + "pp.M"] = st.outs.pop("pp.M")
        taken = None
        if armed:
            wp = []
            for i in range(N):
                if i == mode:
                    wp.append(o["W"].ptr)
                else:
                    o[f"W{i}"] = st.out(tag + f"W{i}", nrows[i] * R, idx=np.arange(nrows[i] * R),
                                        init=nrm_in[i].reshape(-1, order="F"))
                    wp.append(o[f"W{i}"].ptr)
            ms = norm.get("ms")
            if norm.get("wsq"):
                o["wsq"] = st.out(tag + "wsq", 2 * N, res=2 * np.arange(N))
            if ms:
                o["ms"] = st.out(tag + "ms", 32, res=[k for k in range(32) if (ms[1] >> k) & 1], idx=np.arange(32),
                                 init=1.5 + np.arange(32) / 64.0)
            wsq, msd = o["wsq"].ptr if "wsq" in o else 0, o["ms"].ptr if ms else 0
            if norm.get("wrong_first") and st.hip:  # hazard g: armed for this mode, an update of another follows
                sh.arm_normalize(wp, nrows, R, G, mode, wsq, msd, ms[0] if ms else None, ms[1] if ms else 0,
                                 ms[2] if ms else 0)
                om = (mode + 1) % N
                try:
                    sh.cp_mode_update(G, N, om, R, lam, o["M"].ptr, ldm, o["W"].ptr, ldw, o["grad"].ptr, ldg, rows,
                                      o["gradsq"].ptr, 0, ldi, 0, ldd, 1.0, S, Si, 0)
                    raise AssertionError(f"{c['name']}: the mismatched update was not refused")
                except Exception as e:
                    assert "armed Normalize does not match" in str(e), str(e)
            taken = sh.arm_normalize(wp, nrows, R, G, mode, wsq, msd, ms[0] if ms else None, ms[1] if ms else 0,
                                     ms[2] if ms else 0)
            if st.hip:
                assert taken == c["norm_taken"], f"{c['name']}: arm_normalize returned {taken}"
        ratio = c.get("ratio", 1.0)
        if kind == "plain":
            sh.cp_mode_update(G, N, mode, R, lam, o["M"].ptr, ldm, o["W"].ptr, ldw, o["grad"].ptr, ldg, rows,
                              o["gradsq"].ptr, wi, ldi, dw, ldd, ratio, S, Si, dq)
        elif kind == "batched":
            sh.cp_mode_update_batched(G, N, mode, R, K, lam, o["M"].ptr, ldm, o["W"].ptr, ldw, o["grad"].ptr, ldg,
                                      rows, o["gradsq"].ptr, S, Si)
        else:
            sh.cp_mode_update_blocked(G, N, mode, R, lam, o["M"].ptr, c["blk"], c["P"], o["scratch"].ptr, o["W"].ptr,
                                      ldw, o["grad"].ptr, ldg, rows, o["gradsq"].ptr, wi, ldi, dw, ldd, ratio, S, Si)
        if armed and not taken:  # the caller's own Normalize (ops.h: arm_normalize)
            sh.normalize_ms(wp, nrows, R, G, msd, ms[0] if ms else None, ms[1] if ms else 0, ms[2] if ms else 0, wsq)
        if armed:
            o["scales"] = sh.normalize_scales()
        return o

    plain = launch("plain." if norm else "", False)
    armed = None
    if norm:
        sh.sync()
        armed = launch("", True)
        sh.sync()
        st.scales = sh.d2h(armed["scales"], 8 * N).view(np.float64).copy()
        st.route_norm = [t for t in sh.route_take()]
        st.tags += st.route_norm
    st.finish()

    def verify():
        p = "plain." if norm else ""
        gflat_post = st.posts[p + "G"][CC.GUARD:-CC.GUARD].view(np.float64)
        st.got(p + "G")
        Wd, gd, gq = st.got(p + "W"), st.got(p + "grad"), st.got(p + "gradsq")
        Wd, gd = mat(Wd, rows, R * K), mat(gd, rows, R * K)
        for b in range(K):
            _, _, S_ref, absH, cond = sysb[b]
            cs = slice(b * R, (b + 1) * R)
            what = f"[{b}] " if K > 1 else ""
            dWd = mat(st.got(p + "dW"), rows, R) if Winit is not None else None
            if null:
                s64 = S_ref.astype(np.float64)
                check_solve(st, what, c, M[:, cs], W0[:, cs], S_ref, None, gd[:, cs], None, None, None, gq[b], True,
                            extra=N)
                want = M[:, cs] @ np.linalg.inv(s64)
                if Winit is not None:
                    want = Winit + c.get("ratio", 1.0) * (want - Winit)
                fro = np.linalg.norm(Wd[:, cs] - want) / np.linalg.norm(want)
                assert fro < 1e-10 * cond, f"{c['name']} {what}W: {fro:.3e} over 1e-10 * cond {cond:.3g}"
            else:
                Sd = mat(st.got(p + "S")[b * RR:(b + 1) * RR], R, R)
                Sid = mat(st.got(p + "Sinv")[b * RR:(b + 1) * RR], R, R)
                check_system(st, what, Sd, Sid, S_ref, absH, lam, N, cond)
                check_solve(st, what, c, M[:, cs], W0[:, cs], Sd, Sid, gd[:, cs], Wd[:, cs], Winit, dWd, gq[b], False)
            if "dwsq" in plain:
                sumsq_check(st, what + "dwsq", st.got(p + "dwsq")[0], dWd)
            Gm = mat(gflat_post[(b * N + mode) * RR:(b * N + mode + 1) * RR], R, R)
            check_gram(st, what + "G", Gm, Wd[:, cs], rows)
        if not norm:
            return
        # the armed run: everything in front of the Normalize equal in bits to the plain run, then f_i times it
        for k in ("grad", "gradsq", "S", "Sinv", "dW", "dwsq"):
            if k in plain:
                assert np.array_equal(st.posts["plain." + k], st.posts[k]), f"{c['name']} {k}: armed differs from plain"
        Gin = [sysb[0][0][i] for i in range(N)]
        Gin[mode] = mat(gflat_post[mode * RR:(mode + 1) * RR], R, R)
        fac_in = [Wd if i == mode else nrm_in[i] for i in range(N)]
        fac_out = [mat(st.got("W" if i == mode else f"W{i}"), nrows[i], R) for i in range(N)]
        check_normalize(st, N, R, Gin, fac_in, fac_out, st.got("G").reshape(N, RR), st.scales,
                        st.got("wsq") if norm.get("wsq") else None, norm.get("ms"),
                        st.got("ms") if norm.get("ms") else None, st.route_norm)
    st.verify = verify


def _resystem(s, N, mode, R, lam):
    Gs = s[0]
    H = np.ones((R, R), dtype=LD)
    for j in range(N):
        if j != mode:
            H = H * Gs[j].astype(LD)
    S = H + LD(lam) * np.eye(R, dtype=LD)
    e = np.linalg.eigvalsh(S.astype(np.float64))
    cond = float(np.max(np.abs(e)) / np.min(np.abs(e)))
    assert e[0] > 0 and cond <= 1e3, (e[0], cond)
    return (Gs, lam, S, np.abs(H), cond)


def _shift(s, lam):
    """an SPD system of a batch whose one lambda is the indefinite start's (-2): its first Gram + 3 I, so that S stays
    positive definite with cond <= 1e3 (asserted)"""
    Gs, _, S, absH, _ = s
    R = S.shape[0]
    j0 = next(j for j, G in enumerate(Gs) if not np.isnan(G[0, 0]))
    Gs = list(Gs)
    Gs[j0] = Gs[j0] + 30.0 * np.eye(R)
    N = len(Gs)
    mode = next(j for j, G in enumerate(Gs) if np.isnan(G[0, 0]))
    return _resystem((Gs,), N, mode, R, lam)


# ------------------------------------------------------------------------------------------ Normalize
def norm_bars(N, R, traces):
    nr = np.sqrt(np.asarray(traces, dtype=LD))
    prod = np.prod(nr)
    f = prod ** (LD(1) / N) / nr
    e_n = ((R - 1) / 2.0 + 1) * U
    Ef = 2 * e_n + 2 * U + U * abs(float(np.log(prod))) / N + POW_ALLOW
    return nr, f, e_n, Ef


def check_normalize(st, N, R, Gin, fac_in, fac_out, Gout, scales, wsq, ms, ms_out, tags):
    traces = [np.sum(np.diag(G).astype(LD)) for G in Gin]
    nr, f, e_n, Ef = norm_bars(N, R, traces)
    dev = np.abs(scales.astype(LD) / f - 1) / U
    if any(t.startswith("normalize.grid") for t in tags):
        SCALE_DEV.append(float(np.max(dev)))
    if st.log is not None:
        st.log.append(f"{st.c['name']} scales: max |f_dev / f_ref - 1| = {float(np.max(dev)):.3g} u, bar {float(Ef / U):.3g} u")
    within(st, "scales", scales, f, Ef * f)
    for i in range(N):
        within(st, f"W{i}", fac_out[i], f[i] * fac_in[i].astype(LD), (Ef + U) * np.abs(f[i] * fac_in[i]))
        g = Gin[i].astype(LD) * f[i] * f[i]
        within(st, f"G{i}", mat(Gout[i], R, R), g, (2 * Ef + 2 * U) * np.abs(g))
    if wsq is not None:
        w = (nr * f) ** 2
        bar = 2 * (e_n + Ef + U) + U  # (n_i f_i)^2 from the trace: the fused kernels
        if not st.hip or any(t.startswith("normalize.grid") for t in tags):
            # summed over the scaled factor's n_i entries instead: the sum's n_i u and the (rows_i + R) u between
            # the Gram's trace and the exact ||W_i||^2 on top
            bar = bar + np.array([fac_in[i].size + fac_in[i].shape[0] + R for i in range(N)]) * U
        within(st, "wsq", wsq, w, bar * w)
    if ms:
        masks, active, fresh = ms
        start = 1.5 + np.arange(32) / 64.0
        ks = [k for k in range(32) if (active >> k) & 1]
        ref = np.array([(LD(1) if (fresh >> k) & 1 else LD(start[k])) * np.prod([f[m] for m in range(8) if masks[k] >> m & 1] + [LD(1)])
                        for k in ks], dtype=LD)
        pc = np.array([bin(masks[k] & 0xFF).count("1") for k in ks])
        within(st, "ms_dst", ms_out, ref, pc * (Ef + U) * np.abs(ref))


def op_normalize(st):
    c, sh, rng = st.c, st.sh, st.rng
    N, R, rows, form = len(c["rows"]), c["R"], c["rows"], c["form"]
    Ws = [vals(rng, c["cls"], (rows[i], R)) for i in range(N)]
    Gin = [W.T @ W for W in Ws]
    bufs = [st.out(f"W{i}", rows[i] * R, idx=np.arange(rows[i] * R), init=Ws[i].reshape(-1, order="F")) for i in range(N)]
    g = st.out("G", N * R * R, idx=np.arange(N * R * R), init=gall_flat(Gin))
    ms, wsq, msd = c.get("ms"), None, None
    wp = [b.ptr for b in bufs]
    if form == "normalize":
        sh.normalize(wp, rows, R, g.ptr)
    else:
        if c.get("wsq"):
            wsq = st.out("wsq", 2 * N, res=2 * np.arange(N))
        if ms:
            msd = st.out("ms", 32, res=[k for k in range(32) if (ms[1] >> k) & 1], idx=np.arange(32),
                         init=1.5 + np.arange(32) / 64.0)
        sh.normalize_ms(wp, rows, R, g.ptr, msd.ptr if msd else 0, ms[0] if ms else None, ms[1] if ms else 0,
                        ms[2] if ms else 0, wsq.ptr if wsq else 0)
    sh.sync()
    st.scales = sh.d2h(sh.normalize_scales(), 8 * N).view(np.float64).copy()
    st.finish()
    st.verify = lambda: check_normalize(
        st, N, R, Gin, Ws, [mat(st.got(f"W{i}"), rows[i], R) for i in range(N)], st.got("G").reshape(N, R * R), st.scales,
        st.got("wsq") if wsq else None, ms, st.got("ms") if msd else None, st.tags)


# ------------------------------------------------------------------------------------------ the factor side
def op_diff_norms(st):
    c, sh, rng = st.c, st.sh, st.rng
    ns, hasB, sd, up = c["n"], c["B"], c.get("store_diff", 0), c.get("update_prev", 0)
    N = len(ns)
    A = [vals(rng, c["cls"], n) for n in ns]
    B = [vals(rng, c["cls"], n) for n in ns]
    Dg = [vals(rng, c["cls"], n) for n in ns]  # (B == nullptr: D is given)
    a = [st.inp(x) for x in A]
    b = d = None
    if hasB:
        b = [st.out(f"B{i}", ns[i], res=np.arange(ns[i]) if up else [], idx=np.arange(ns[i]), init=B[i]) for i in range(N)]
        if sd:
            d = [st.out(f"D{i}", ns[i]) for i in range(N)]
    else:
        d = [st.inp(x) for x in Dg]
    o = st.out("out", 2 * N)
    sh.diff_norms([x.ptr for x in a], [x.ptr for x in b] if b else None, ns, sd, [x.ptr for x in d] if d else None, up,
                  o.ptr)
    st.finish()

    def verify():
        out = st.got("out")
        for i in range(N):
            diff = A[i] - B[i] if hasB else Dg[i]
            if hasB and sd:
                assert np.array_equal(st.got(f"D{i}"), diff), f"{c['name']}: D{i} is not fl(A - B)"
            if hasB:
                Bp = st.got(f"B{i}") if up else B[i]
                assert not up or np.array_equal(Bp, A[i]), f"{c['name']}: B{i} was not updated to A"
            sumsq_check(st, f"out[{2 * i}]", out[2 * i], diff)
            sumsq_check(st, f"out[{2 * i + 1}]", out[2 * i + 1], A[i])
    st.verify = verify


def op_blocks(st):
    c, sh, rng = st.c, st.sh, st.rng
    rows, R, blk, P, ld = c["rows"], c["R"], c["blk"], c["P"], c["rows"] + c.get("xld", 0)
    nat = vals(rng, c["cls"], (rows, R))
    full = np.zeros((blk * P, R))
    full[:rows] = nat
    blocked = np.concatenate([full[p * blk:(p + 1) * blk].reshape(-1, order="F") for p in range(P)])
    n_in = st.inp(colmajor(nat, ld))
    b_out = st.out("blocked", blk * R * P)
    sh.pack_blocks(n_in.ptr, rows, ld, R, blk, P, b_out.ptr)
    # (the pad rows of a gathered buffer are the sender's business: give unpack garbage there, it must not land)
    junk = blocked.copy()
    padfull = np.repeat((np.arange(blk * P) >= rows)[:, None], R, axis=1)
    junk[np.concatenate([padfull[p * blk:(p + 1) * blk].reshape(-1, order="F") for p in range(P)])] = 7.0
    b_in = st.inp(junk)
    n_out = st.out("nat", ld * R, res=midx(rows, R, ld))
    sh.unpack_blocks(b_in.ptr, rows, ld, R, blk, P, n_out.ptr)
    n_rt = st.out("roundtrip", ld * R, res=midx(rows, R, ld))
    sh.unpack_blocks(b_out.ptr, rows, ld, R, blk, P, n_rt.ptr)
    st.finish()

    def verify():
        got = st.got("blocked")
        assert np.array_equal(got, blocked), f"{c['name']}: pack_blocks is not exact (padding rows exactly 0)"
        for k in ("nat", "roundtrip"):
            assert np.array_equal(mat(st.got(k), rows, R), nat), f"{c['name']}: {k} differs"
    st.verify = verify


def op_sumsq(st):
    c, sh = st.c, st.sh
    x = vals(st.rng, c["cls"], c["n"])
    xin, o = st.inp(x), st.out("out", 1)
    sh.sumsq(xin.ptr, c["n"], o.ptr)
    st.finish()

    def verify():
        got = st.got("out")[0]
        if c["n"] == 0:
            assert got == 0.0
        else:
            sumsq_check(st, "sumsq", got, x)
    st.verify = verify


def op_scale(st):
    c, sh, rng = st.c, st.sh, st.rng
    scales = vals(rng, "pos", 8) * 2.0
    s = st.inp(scales)
    start = vals(rng, c["cls"], 32)
    if c["form"] == "one":
        masks, active, fresh = [c["mask"]], 1, c["set_one"]
        d = st.out("dst", 1, idx=[0], init=start[:1])
        sh.scale_update(d.ptr, s.ptr, c["mask"], c["set_one"])
    else:
        masks, active, fresh = c["masks"], c["active"], c["fresh"]
        d = st.out("dst", 32, res=[k for k in range(32) if (active >> k) & 1], idx=np.arange(32), init=start)
        sh.scale_update_many(d.ptr, s.ptr, masks, active, fresh)
    st.finish()

    def verify():
        ks = [k for k in range(len(masks)) if (active >> k) & 1]
        ref = np.array([(LD(1) if (fresh >> k) & 1 else LD(start[k])) *
                        np.prod([LD(scales[m]) for m in range(8) if masks[k] >> m & 1] + [LD(1)]) for k in ks], dtype=LD)
        pc = np.array([bin(masks[k] & 0xFF).count("1") for k in ks])
        within(st, "dst", st.got("dst"), ref, pc * U * np.abs(ref))
    st.verify = verify


OPS = {"gram": op_gram, "gram_system": op_gram_system, "cp_update": op_cp_update, "update": op_update,
       "normalize": op_normalize, "diff_norms": op_diff_norms, "blocks": op_blocks, "sumsq": op_sumsq,
       "scale": op_scale}

# ------------------------------------------------------------------------------------------ the table
CASES = []
_seed = [5000]


def _add(op, family, name, route, why, **kw):
    _seed[0] += 1
    kw.setdefault("cls", "pos" if _seed[0] % 2 else "mix")
    c = dict(op=op, family=family, name=f"{family}:{name}", route=route if isinstance(route, list) else [route],
             why=why, seed=_seed[0], **kw)
    CASES.append(c)
    return c


# ---- gram: rows straddling the 64-lane stride and the four-chain loop (i + 192 < rows), R with more pairs than waves
for rows in (1, 63, 64, 65, 255, 256, 257, 449, 1000):
    for R in (10, 45):
        _add("gram", "gram", f"rows={rows} R={R}", [], "row loop edges", rows=rows, R=R, xld=5 * (rows % 2))
for R in (1, 33, 64, 65, 150):
    for rows in (257, 449):
        _add("gram", "gram", f"rows={rows} R={R}", [], "pair count edges", rows=rows, R=R, xld=5 * (R % 2))
_add("gram", "gram", "batched gstride", [], "gstride above R*R", rows=65, R=10, nstarts=3, gstride=107, xld=5)

# ---- gram_system: every kernel, the early return and the recomputation behind it (hazard e)
for R, pats in ((10, [r"gram_system\.wave"]), (64, [r"gram_system\.wave"]), (65, [r"gram_system\.mfma"]),
                (128, [r"gram_system\.mfma"]), (130, [r"gram_system\.lds", r"gram_system\.host_fallback"]),
                (150, [r"gram_system\.big", r"gram_system\.host_fallback"])):
    _add("gram_system", "gram_system", f"R={R}", pats, "kernel by rank", N=3, mode=R % 3, R=R, lam=0.125)
_add("gram_system", "gram_system", "indefinite R=10", r"gram_system\.wave", "Jacobi inside the wave", N=3, mode=0, R=10,
     indef=True)
_add("gram_system", "gram_system", "armed consumed recomputed", [r"pp_correct terms=1 extra=1", r"gram_system\.ready",
                                                                  r"gram_system\.wave"],
     "hazard e: ready once", N=4, mode=2, R=10, lam=0.125, armed=True)
_add("gram_system", "gram_system", "GJ scalar R=65", r"gram_system\.lds", "forced scalar sweeps", N=3, mode=1, R=65,
     env={"PPALS_GJ_SCALAR": "1"})


# ---- cp_update
def cpu(name, why, **kw):
    return _add("cp_update", "cp_update", name, cp_update_route(kw), why, **kw)


for rows in (1, 64, 614):
    cpu(f"one rows={rows}", "one workgroup", rows=rows, R=10, xm=rows % 3, xg=2)
cpu("rows R=10 rows=615", "first row-parallel size", rows=615, R=10, xw=3)
cpu("rows R=7 rows=1000", "R%4, rows%64", rows=1000, R=7, xm=1, xg=1)
cpu("rows R=65 ldg", "gemm fallback: ldg", rows=130, R=65, xg=3)
cpu("rows R=100 winit 0.5", "gemm fallback: ratio", rows=17, R=100, winit=True, ratio=0.5)
for R in (65, 100, 128):
    for rows in (17, 130):
        cpu(f"gemm R={R} rows={rows}", "matrix-core products", rows=rows, R=R)
        cpu(f"gemm R={R} rows={rows} winit", "diff_norms tail", rows=rows, R=R, winit=True, ratio=1.0)
cpu("one not aliased", "Wnew apart, ldn", rows=64, R=10, alias=False, xn=2, winit=True, ratio=0.5, xi=1, xd=2)
cpu("rows not aliased", "Wnew apart, ldn", rows=130, R=65, alias=False, xn=2)
cpu("empty", "no rows", rows=0, R=10)
cpu("gemm ldi refused", "packed Winit only", rows=17, R=65, winit=True, ratio=1.0, xi=2,
    raises="cp_update expects packed factors")


# ---- cp_mode_update
def upd(family, name, why, **kw):
    rows, R = kw["rows"], kw["R"]
    rt = update_route(rows, R, jacobi=bool(kw.get("env", {}).get("PPALS_FORCE_JACOBI")))
    ps = 1 if kw.get("pre") == "match" else 0
    if rt == "staged":
        pat = rf"update\.staged presolved={ps} norm={1 if kw.get('norm_taken') else 0} mblk=0 dwsq={1 if kw.get('dwsq') else 0}"
    elif rt == "unstaged":
        pat = rf"update\.unstaged presolved={ps}"
    else:
        pat = r"update\." + rt
    pats = [pat] + kw.pop("also", [])
    assert kw.pop("expect", rt.split(" ")[0]) == rt.split(" ")[0], (name, rt)
    return _add("update", family, name, pats, why, **kw)


NM = [(3, 0), (3, 1), (3, 2), (4, 0), (4, 1), (4, 2), (4, 3)]
# the staged Gram refresh: pair loop (rows 1, 3, 25), partial tiles with nks = 1 (26, 27: rows % 4), nks = 16 and
# an odd spw (410: 103 k-steps, 7 a wave, the last wave short), the last staged row count (932)
for rows in (1, 3, 25, 26, 27, 410, 932):
    for N, mode in NM:
        upd("update_staged", f"R=10 rows={rows} N={N} mode={mode}", "Gram refresh splits", rows=rows, R=10, N=N,
            mode=mode, lam=0.125 * ((N + mode) % 2), expect="staged")
for R, rr in ((20, (38, 39)), (16, (15, 16)), (17, (45, 46)), (33, (46, 47)), (64, (20,))):
    for i, rows in enumerate(rr):  # either side of rows * R / (ntile * 256) = 1
        upd("update_staged", f"R={R} rows={rows}", "partial-tile boundary", rows=rows, R=R, N=3 + i, mode=1 + i,
            lam=0.125 * i, expect="staged")
for k, x in enumerate(({"xm": 3}, {"xw": 2}, {"xg": 5}, {"xm": 1, "xw": 2, "xg": 3})):
    upd("update_staged", f"ld {x}", "wide leading dimensions", rows=27, R=10, N=3, mode=k % 3, expect="staged", **x)
for ratio in (1.0, 0.5):
    for dq in (False, True):
        upd("update_staged", f"winit ratio={ratio} dwsq={dq}", "SVD_solve_mod tail", rows=27, R=10, N=3, mode=1,
            winit=True, ratio=ratio, dwsq=dq, lam=0.125, expect="staged")
upd("update_staged", "winit ldi", "ldi above rows", rows=27, R=10, N=4, mode=0, winit=True, ratio=0.5, xi=3, expect="staged")
upd("update_staged", "null S", "S, Sinv not returned", rows=27, R=10, N=3, mode=2, null=True, lam=0.125, expect="staged")
upd("update_staged", "indefinite", "Jacobi inside the launch", rows=27, R=10, N=3, mode=0, indef=(0,), expect="staged")
# unstaged: only R of about 42 .. 64 gets there
for R, rows in ((64, 21), (64, 96), (48, 102), (48, 128)):
    upd("update_unstaged", f"R={R} rows={rows}", "unstaged range ends", rows=rows, R=R, N=3, mode=rows % 3,
        lam=0.125 * (rows % 2), expect="unstaged")
upd("update_unstaged", "winit 0.5 dwsq", "SVD_solve_mod tail", rows=21, R=64, N=3, mode=1, winit=True, ratio=0.5,
    dwsq=True, xd=0, expect="unstaged")
upd("update_unstaged", "indefinite", "Jacobi inside the launch", rows=96, R=64, N=3, mode=2, indef=(0,),
    expect="unstaged")
upd("update_unstaged", "null S", "S, Sinv not returned", rows=102, R=48, N=4, mode=3, null=True, expect="unstaged")
# unfused
for R, rows, also in ((10, 933, [r"gram_system\.wave", r"cp_update\.rows"]), (64, 97, [r"cp_update\.rows"]),
                      (65, 17, [r"gram_system\.mfma", r"cp_update\.gemm tail=0"]), (65, 130, [r"cp_update\.gemm"]),
                      (100, 33, [r"cp_update\.gemm"]), (150, 40, [r"gram_system\.big", r"cp_update\.gemm"])):
    upd("update_unfused", f"R={R} rows={rows}", "separate launches", rows=rows, R=R, N=3, mode=R % 3, lam=0.125,
        also=also, expect="unfused")
upd("update_unfused", "R=65 winit 0.5 dwsq", "dwsq by sumsq", rows=17, R=65, N=3, mode=0, winit=True, ratio=0.5, dwsq=True,
    also=[r"cp_update\.rows"], expect="unfused")
upd("update_unfused", "R=10 rows=933 null S", "null S, separate launches", rows=933, R=10, N=3, mode=1, null=True,
    expect="unfused")
upd("update_unfused", "forced Jacobi R=10", "A/B path", rows=27, R=10, N=3, mode=1, env={"PPALS_FORCE_JACOBI": "1"},
    also=[r"gram_system\.wave", r"cp_update\.one"], expect="unfused")
# the state the launchers keep between calls (hazards a-d, f; e is a gram_system case; g, h below)
PP1, PP0 = r"pp_correct terms=1 extra=1", r"pp_correct terms=1 extra=0"
STALE = r"update\.\w+ presolved=1"  # (not_route: a prepared system taken by an update it was not armed for)
upd("update_state", "a presolved", "armed, prepared, consumed", rows=27, R=10, N=3, mode=1, lam=0.125, pre="match",
    also=[PP1], expect="staged")
# (no such case for the unstaged launch: it needs R >= 42 and arm_gram_system arms nothing above R = 32, so
# k_cp_mode_update<false, false> never runs with presolved = 1 — DESIGN.md section 5)
upd("update_state", "b other lambda", "stale system: lambda", rows=27, R=10, N=3, mode=1, lam=0.125, pre="lambda",
    also=[PP1], not_route=[STALE], expect="staged")
upd("update_state", "c other mode", "stale system: mode", rows=27, R=10, N=3, mode=1, lam=0.125, pre="mode", also=[PP1],
    not_route=[STALE], expect="staged")
upd("update_state", "d other pointers", "stale system: pointers", rows=27, R=10, N=3, mode=1, lam=0.125, pre="pointers",
    also=[PP1], not_route=[STALE], expect="staged")
upd("update_state", "f R=33 arms nothing", "arm limit R <= 32", rows=27, R=33, N=3, mode=1, lam=0.125, pre="none33",
    also=[PP0], expect="staged")
# the armed Normalize tail; g: a mismatched update is refused, a fresh arm works; h: the three refusals
MS = ([0b011, 0b101, 0b110, 0b111] + [0] * 27 + [0b1], 0x80000001 | 0b1110, 0b0100)
for N, mode, R, rows, nrows, extra in ((3, 2, 10, 27, (5, 1, 0), {}), (4, 0, 10, 26, (0, 7, 9, 3), {"wsq": True}),
                                       (3, 1, 64, 20, (4, 0, 6), {"wsq": True, "ms": MS}),
                                       (8, 7, 1, 3, (2, 3, 4, 5, 1, 2, 3, 0), {"ms": MS})):
    upd("update_norm", f"armed N={N} R={R}", "Normalize in the launch", rows=rows, R=R, N=N, mode=mode, lam=0.125,
        norm=dict(rows=nrows, **extra), norm_taken=True, also=[r"arm_normalize\.taken"], expect="staged")
upd("update_norm", "g mismatch then fresh arm", "refused, then works", rows=27, R=10, N=3, mode=0,
    norm=dict(rows=(0, 6, 4), wsq=True, wrong_first=True), norm_taken=True, also=[r"arm_normalize\.taken"], expect="staged")
upd("update_norm", "h sum rows*R over 65536", "refused: total", rows=27, R=10, N=3, mode=0,
    norm=dict(rows=(0, 6527, 1), wsq=True), norm_taken=False,
    also=[r"arm_normalize\.refused", r"normalize\.grid"], expect="staged")
upd("update_norm", "h mode not staged", "refused: mode too long", rows=21, R=64, N=3, mode=0,
    norm=dict(rows=(0, 3, 2)), norm_taken=False, also=[r"arm_normalize\.refused", r"normalize\.fused"], expect="unstaged")
upd("update_norm", "h R=65", "refused: rank", rows=17, R=65, N=3, mode=2, norm=dict(rows=(3, 2, 0)), norm_taken=False,
    also=[r"arm_normalize\.refused", r"normalize\.fused"], expect="unfused")


# ---- cp_mode_update_batched
def bat(name, why, **kw):
    rows, R = kw["rows"], kw["R"]
    rt = update_route(rows, R).split(" ")[0]
    pat = r"update_batched\." + ("loop" if rt == "unfused" else rt)
    return _add("update", "update_batched", name, [pat] + kw.pop("also", []), why, kind="batched", **kw)


for K in (1, 3, 32):
    bat(f"staged K={K}", "one workgroup per start", rows=26, R=10, N=3, mode=K % 3, nstarts=K, lam=0.125, xw=K % 2)
    bat(f"unstaged K={K}", "one workgroup per start", rows=21, R=64, N=3, mode=K % 3, nstarts=K, xg=1)
bat("loop rows K=3", "start by start", rows=933, R=10, N=3, mode=0, nstarts=3, lam=0.125, also=[r"update\.unfused why=rows"])
bat("loop R=65 K=3", "start by start", rows=17, R=65, N=4, mode=1, nstarts=3, also=[r"update\.unfused why=R"])
bat("staged indefinite start", "Jacobi in one start only", rows=26, R=10, N=3, mode=1, nstarts=3, indef=(1,))
bat("unstaged indefinite start", "Jacobi in one start only", rows=21, R=64, N=3, mode=1, nstarts=3, indef=(2,))
bat("staged null S", "S, Sinv not returned", rows=26, R=10, N=3, mode=2, nstarts=3, null=True, lam=0.125)
bat("loop null S", "null S, start by start", rows=933, R=10, N=3, mode=2, nstarts=2, null=True, lam=0.125)


# ---- cp_mode_update_blocked: M in the row blocks an all-gather leaves
def blkd(name, direct, why, **kw):
    rows, R = kw["rows"], kw["R"]
    rt = update_route(rows, R)
    if direct:
        pats = [r"update_blocked\.direct", r"update\.staged presolved=0 norm=0 mblk=1 dwsq=0"]
    else:
        pats = [r"update_blocked\.unpack", r"update\." + rt.split(" ")[0]]
    return _add("update", "update_blocked", name, pats, why, kind="blocked", **kw)


blkd("direct P=3", True, "blocks read in place", rows=21, R=10, N=3, mode=1, blk=7, P=3, lam=0.125)
blkd("direct P=1", True, "one block", rows=21, R=10, N=4, mode=3, blk=21, P=1)
blkd("direct winit", True, "blocks + SVD_solve_mod", rows=21, R=10, N=3, mode=0, blk=7, P=3, winit=True, ratio=0.5)
blkd("unpack rows<blk*P", False, "padded last block", rows=20, R=10, N=3, mode=1, blk=7, P=3)
blkd("unpack R=65", False, "rank above 64", rows=21, R=65, N=3, mode=2, blk=7, P=3)
blkd("unpack long mode", False, "not staged", rows=936, R=10, N=3, mode=0, blk=312, P=3, lam=0.125)

# ---- normalize / normalize_ms: fused up to sum rows * R == 65536, the grid route above
for form in ("normalize", "normalize_ms"):
    rt = r"normalize\.grid" if form == "normalize" else r"normalize\.fused"
    for N, R, rows in ((3, 10, (5, 1, 7)), (4, 1, (3, 1, 2, 9)), (8, 64, (1, 2, 3, 4, 5, 6, 7, 8)), (3, 64, (700, 300, 24))):
        _add("normalize", "normalize", f"{form} N={N} R={R} rows={rows[0]}..", rt, "forms by N, R", form=form, R=R,
             rows=rows, wsq=(N % 2 == 0), ms=MS if N != 3 else None)
_add("normalize", "normalize", "ms grid 65600", r"normalize\.grid", "first grid size", form="normalize_ms", R=64,
     rows=(700, 300, 25), wsq=True, ms=MS)
_add("normalize", "normalize", "ms grid no wsq", r"normalize\.grid", "grid, nothing pending", form="normalize_ms", R=64,
     rows=(700, 300, 25))
_add("normalize", "normalize", "ms fresh none", r"normalize\.fused", "fresh bits clear", form="normalize_ms", R=10,
     rows=(5, 6, 7), ms=(MS[0], MS[1], 0))

# ---- diff_norms
_N8 = (1, 1023, 1025, 5000, 1, 1023, 1025, 64)
for ns in ((5000,), _N8):
    for sd in (0, 1):
        for up in (0, 1):
            _add("diff_norms", "diff_norms", f"N={len(ns)} B store={sd} prev={up}", [], "B given", n=ns, B=True,
                 store_diff=sd, update_prev=up)
    _add("diff_norms", "diff_norms", f"N={len(ns)} B null", [], "D given, B null", n=ns, B=False)
_add("diff_norms", "diff_norms", "N=1 n=1", [], "one element", n=(1,), B=True, store_diff=1, update_prev=1)

# ---- pack_blocks / unpack_blocks
for P in (1, 3, 8):
    for R in (1, 10):
        _add("blocks", "blocks", f"P={P} R={R} full", [], "rows == blk * P", rows=5 * P, R=R, blk=5, P=P, xld=P % 2)
        _add("blocks", "blocks", f"P={P} R={R} short", [], "zero padding rows", rows=5 * P - 2, R=R, blk=5, P=P,
             xld=3 * (R % 2))

# ---- sumsq, scale_update(_many)
for n in (0, 1, 1023, 100000):
    _add("sumsq", "sumsq", f"n={n}", [], "partial sums", n=n)
for set_one in (0, 1):
    for mask in (0, 0b100, 0xFF):
        _add("scale", "scale_update", f"one mask={mask:#x} set_one={set_one}", [], "mask, set_one", form="one", mask=mask,
             set_one=set_one)
_add("scale", "scale_update", "many", [], "active 0x80000001", form="many",
     masks=[0b1, 0] + [0xFF] * 29 + [0b11000000], active=0x80000001, fresh=0)
_add("scale", "scale_update", "many fresh", [], "fresh starts from 1", form="many",
     masks=[0b1, 0b10, 0xFF, 0] + [0b101] * 28, active=0x8000000F, fresh=0x80000005)

FAMILIES = sorted({c["family"] for c in CASES})

# Every tag family these launchers can log. update_batched.loop, update_blocked.unpack and the unfused update log the
# tags of the launchers they go through as well.
EXPECTED_TAGS = sorted(
    ["update.staged", "update.unstaged", "update.unfused", "update_batched.staged", "update_batched.unstaged",
     "update_batched.loop", "update_blocked.direct", "update_blocked.unpack", "cp_update.one", "cp_update.rows",
     "cp_update.gemm", "cp_update.empty", "gram_system.wave", "gram_system.mfma", "gram_system.lds", "gram_system.big",
     "gram_system.ready", "gram_system.host_fallback", "normalize.fused", "normalize.grid", "arm_normalize.taken",
     "arm_normalize.refused", "pp_correct"])


def tag_family(tag):
    return tag.split(" ")[0]


def run_with_env(kind, c, hip, log=None):
    """a case with `env`: the switches are read when an Ops is made, so it gets a Shim of its own"""
    import os

    import opshim_util
    old = {k: os.environ.get(k) for k in c["env"]}
    os.environ.update(c["env"])
    try:
        sh = opshim_util.Shim(kind)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    try:
        return run_case(sh, c, hip, log)
    finally:
        sh.close()
