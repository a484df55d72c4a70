"""Op-level cases of the Tucker eigen side — unfold_gram, top_eigvecs, top_eigvecs_warm with its lazy / deferred
hand-overs, orthonormalize — and of the small factor-side ops next to them (sign_align, rows_times_small,
lowrank_accumulate, add_inplace, the transposes), with their one checker (tests/test_gpu_tucker_ops.py on the HIP
kernels, tests/test_tucker_ops_hostsim.py on the host stand-in, both through tests/opshim), in the style of
tests/update_cases.py; the buffers and the image checker are those of tests/contraction_cases.py.

A case is a plain dict: the op, its arguments, `route` (regular expressions each of which must match a tag of the
calls' route log, computed from the launchers' own formulas below, not copied from a run) and `why`. A warm
sequence carries `routes`: one list of expressions per call.

Per case: inputs from a seed, every input followed by 4 KiB of NaN, every output between two 4 KiB NaN guards; after
the calls every byte outside the results is unchanged and no result is NaN. Every case except the warm sequences
(which own a slot's state) runs TWICE on fresh buffers and the two sets of output images must agree bit for bit:
none of these ops uses atomics, every summation order is fixed.

References are numpy in long double (Grams, products, residuals, orthogonality); u = 2^-53.

unfold_gram: G against A A^T, A[p, c] = X[l, p, t], componentwise (C + 3) u |A||A|^T for BOTH storage types (the
kernels widen fp32 before they multiply, which is exact); G == G.T bit for bit on the SYRK and symmetric-product routes,
within the bar on the others.

top_eigvecs / top_eigvecs_warm: G = Q diag(lam) Q^T formed in long double, rounded to fp64 and symmetrised; all checks
are backward checks on THAT matrix, in long double:
  1. orthonormality  max |U^T U - I|;
  2. residual        ||G U - U diag(theta)||_F, theta_k = u_k^T G u_k;
  3. theta descending (inside a declared cluster of eigenvalues only the subspace is checked);
  4. the largest principal-angle sine between span(U) and the span of numpy eigh's leading vectors of the same G.
The same two quantities 1 and 2 are computed for numpy eigh's vectors; the bars are
      bar = min(cap, MULT[family] x max(reference value, floor)),
floor = J u (orthonormality: normalising one column) resp. J u lam_1 (residual: forming G U at all), MULT = 4 x the
worst device / reference ratio measured on the MI355X per route family — full solvers, projector (warm steps), cold
routes — (profiles/tucker_ops_bars.md; None = not yet measured: the cap alone). A call belongs to the family of the
step that produced its U. The caps are conditions, not measurements:
  * residual: what check_step / cold_bisect promise — max(1e-9 gap, 1e-14 lam_1) sqrt(rank) for a warm step,
    1e-13 lam_1 sqrt(rank) for a strict / cold one (cold_subspace included) and, no looser, for the full solvers;
  * sine <= residual bar / gap (Davis-Kahan), the residual bar being the one enforced, min(cap, MULT x ...);
  * orthonormality, projector and cold routes: 6 (J rank + rank (rank + 1)) u, the published CholeskyQR2 bound, which
    every tail of those routes ends in;
  * orthonormality, full solvers: 240 J u. Their U is a product of plane rotations, (J - 1) per column and sweep, each
    orthogonal to 6 u (c and s rounded once each: |c^2 + s^2 - 1| <= 4 u, two rounded products per entry), and both
    Jacobi kernels stop after 40 sweeps at the latest: 6 x 40 x J u whatever the rank (the CholeskyQR2 expression
    shrinks with the rank, which the error of a product of rotations does not). The vendor solver is held to the same.
Every spectrum has gap / lam_1 >= 1e-3 at the cut (asserted by the builder). The one exception is the spectrum with
lam_1 = 1e6 x the rest, which the issue names: no cut below lam_1 can have such a gap, so a case that declares
`dominant=1` is held to the condition on the largest eigenvalue below the dominant one — the launchers deflate it
before anything depends on the gap — while the caps go on using the true lam_1.

orthonormalize: ||Q^T Q - I||_max <= 6 (rows r + r (r + 1)) u (CholeskyQR2, valid for cond <= u^-1/2 / 8; the cases
stay at or below 1e6); M = Q^T U_in upper triangular with a positive diagonal; ||U_in - Q triu(M)||_F / ||U_in||_F.
The last two against numpy's Householder QR (sign-fixed) in the same arithmetic: MULT x max(reference, floor), floor
= r u; the strictly lower triangle is measured relative to ||U_in||_2.
"""
import os
import re

import numpy as np

import contraction_cases as CC
import opshim_util
from bf16_util import bf16_bits
from contraction_cases import check_image, check_route
from opshim_util import BF16, F32, F64

U = 2.0 ** -53
U24 = 2.0 ** -24
LD = np.longdouble
TINY = np.finfo(np.float64).tiny
NCU = opshim_util.compute_units() or 256
SYM_LDS_MIN = 768   # hip_ops.hip: sym_lds_min_
K_EV_MAX = 128      # kernels_eig.hip.h: kEigEvMax, kJacobiBigMax

# 4 x the worst device / reference ratio per route family, measured on the MI355X: profiles/tucker_ops_bars.md.
# None: not yet measured, the caps alone hold. (A ratio below 1: the device beat max(reference, floor).)
MULT = {
    "full": {"orth": 4 * 7.95, "res": 4 * 20.1},       # in-LDS Jacobi (cold and on Q^T G Q), one-sided Jacobi, dsyevd
    "projector": {"orth": 4 * 1.25, "res": 4 * 4.73},  # warm projector steps, lazy and deferred ones included
    "cold": {"orth": 4 * 0.32, "res": 4 * 11.4},       # strict projector steps, cold_subspace, cold_bisect
    "qr": {"tri": 4 * 0.479, "rec": 4 * 0.664},        # orthonormalize against Householder QR
}
WORST = {}   # family -> largest err / bar seen
RATIOS = {}  # (route family, quantity) -> largest device / reference ratio seen


def _ratio(fam, what, dev, ref):
    RATIOS[(fam, what)] = max(RATIOS.get((fam, what), 0.0), float(dev) / float(ref))


def _worst(fam, r):
    WORST[fam] = max(WORST.get(fam, 0.0), float(r))


# ------------------------------------------------------------------------------------------ buffers
class St:
    """the buffers and the outcome of one run of a case"""

    def __init__(self, sh, c, hip, log):
        self.sh, self.c, self.hip, self.log = sh, c, hip, log
        self.rng = np.random.default_rng(c["seed"])
        self.keep, self.outs, self.posts, self.tags, self.verify = [], {}, {}, [], None

    def say(self, msg):
        if self.log is not None:
            self.log.append(f"{self.c['name']}: {msg}")

    def inp(self, flat, t=np.float64):
        b = CC._In(self.sh, np.ascontiguousarray(flat, dtype=t))
        self.keep.append(b)
        return b

    def out(self, name, n, t=np.float64, res=None, init=None, raw=False):
        """an output of n elements of type t; res: the elements the calls must write (default all); init: the values
        all n elements hold beforehand (in / out buffers); raw: contents unspecified, only the guards are checked"""
        o = CC._Out(self.sh, n, t, np.arange(n) if init is not None else None, init)
        self.keep.append(o)
        self.outs[name] = (o, np.arange(n) if res is None else np.asarray(res, dtype=np.int64), raw)
        return o

    def fetch(self, name):
        self.posts[name] = self.outs[name][0].download()

    def finish(self):
        self.sh.sync()
        self.tags += self.sh.route_take()
        for name in self.outs:
            if name not in self.posts:
                self.fetch(name)
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
            return post[CC.GUARD:-CC.GUARD].view(o.t)
        return check_image(what, o.img, self.posts[name], o.t, res)

    def put(self, name, arr):
        """(the self-test) writes result values back into the downloaded image"""
        o, res, _ = self.outs[name]
        body = self.posts[name][CC.GUARD:-CC.GUARD].view(o.t)
        body[res] = np.asarray(arr, dtype=o.t).reshape(-1)

    def free(self):
        for b in self.keep:
            b.free()
        self.keep = []


def within(st, what, got, ref, bar):
    got, ref, bar = np.asarray(got), np.asarray(ref, dtype=LD), np.asarray(bar, dtype=LD)
    if got.size == 0:
        return
    err = np.abs(got.astype(LD) - ref)
    ratio = float(np.max(err / np.maximum(bar, TINY)))
    _worst(st.c["family"], ratio)
    st.say(f"{what}: max err/bar {ratio:.3g}")
    bad = np.argwhere(err > bar)
    assert bad.size == 0, (f"{st.c['name']} {what}: {len(bad)} elements over the bar, first at {tuple(bad[0])}: err "
                           f"{float(err[tuple(bad[0])]):.3e} bar {float(bar[tuple(bad[0])]):.3e}, worst err/bar {ratio:.3g}")


def scalar_within(st, what, val, bar):
    r = float(val) / max(float(bar), TINY)
    _worst(st.c["family"], r)
    st.say(f"{what}: {float(val):.3e} (bar {float(bar):.3e}, ratio {r:.3g})")
    assert val <= bar, f"{st.c['name']} {what}: {float(val):.3e} over the bar {float(bar):.3e}"


def run_case(sh, c, hip, log=None, perturb=None):
    """Runs a case (twice on fresh buffers unless it is a warm sequence, comparing the two runs bit for bit) and checks
    the last run. perturb(st): the self-test's hook on the outcome before it is verified. Returns the route tags."""
    first = None
    reps = (1,) if c.get("once") else (0, 1)
    for rep in reps:
        st = St(sh, c, hip, log if rep else None)
        try:
            sh.route_take()
            OPS[c["op"]](st)
            if rep == 0:
                first = st.posts
                continue
            if first is not None:
                assert first.keys() == st.posts.keys()
                for k in first:
                    if not st.outs[k][2]:
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


def run_with_env(kind, c, hip, log=None):
    """a case with `env`: the switches are read when an Ops is made, so it gets a Shim of its own"""
    env = dict(c["env"])
    if not hip:  # (the stand-in's own switch for the deferred hand-over)
        env = {k: v for k, v in env.items() if not k.startswith("PPALS_EIG")}
        if c["op"] == "eig_defer":
            env["PPALS_HOSTSIM_DEFER"] = "1"
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
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


# ------------------------------------------------------------------------------------------ unfold_gram
def k_split(n, want, min_per=1, align=1):
    want = max(want, 1)
    per = max((n + want - 1) // want, min_per)
    per = (per + align - 1) // align * align
    return (n + per - 1) // per, per


def gram_route(dt, L, J, T, sym_lds_min=SYM_LDS_MIN, ncu=NCU):
    """HipOps::unfold_gram's decision, restated: (tag, bitwise symmetric)"""
    C = L * T
    if dt == "f64" and 64 <= J <= 8192 and 16 <= C <= 4096 and J * C * 8.0 <= 64e6:
        return f"unfold_gram.sym transposed={int(L > 1)} lds={int(J >= sym_lds_min)}", True
    if dt == "f32" and J >= 64 and C >= 4096 and ((L == 1 and J % 4 == 0) or (L > 1 and L % 4 == 0)):
        nt = (J + 63) // 64
        ntri = nt * (nt + 1) // 2
        want = min(max(1, (ncu * 3) // ntri), max(1, C // 1024))
        return f"unfold_gram.syrk nsplit={k_split(C, min(want, 512), 1, 32)[0]}", True
    tiles = (J + 31) // 32
    want, target = 1, ncu * 4
    if tiles * tiles < target:
        want = min((target + tiles * tiles - 1) // (tiles * tiles), max(1, C // 256))
    nsplit = k_split(C, min(want, 1024), 1, 32)[0]
    return f"unfold_gram.{'mfma' if J >= 16 else 'valu'}.{dt} nsplit={nsplit}", False


def gram_values(rng, cls, shape):
    mix = 2.0 * rng.random(shape) - 1.0
    return 1.0 + 1e-3 * mix if cls == "mean" else mix


def op_unfold_gram(st):
    c = st.c
    dt, L, J, T = c["dt"], c["L"], c["J"], c["T"]
    Xx, Xs = CC._stored(gram_values(st.rng, c["cls"], L * J * T), dt)
    xin = st.inp(Xs, Xs.dtype)
    g = st.out("G", J * J)
    st.sh.unfold_gram(xin.ptr, CC.DT[dt], L, J, T, g.ptr)
    st.finish()
    A = Xx.reshape((L, J, T), order="F").transpose(1, 0, 2).reshape((J, L * T), order="F")
    st.A = A

    def verify():
        G = st.got("G").reshape((J, J), order="F")
        Al = A.astype(LD)
        ref = Al @ Al.T
        absp = np.abs(A) @ np.abs(A).T
        bar = (L * T + 3) * U * absp
        within(st, "G", G, ref, bar)
        bitsym = np.array_equal(G, G.T)
        if c.get("bitsym"):
            assert bitsym, f"{c['name']}: G != G.T in bits on a route that promises it"
        else:
            st.say(f"symmetric bit for bit: {bitsym}")
            assert np.all(np.abs(G - G.T) <= 2 * bar.astype(np.float64)), f"{c['name']}: G - G.T beyond the bar"
    st.verify = verify


# ------------------------------------------------------------------------------------------ eigenvectors
def craft(rng, lam, Q=None):
    """G = Q diag(lam) Q^T in long double, rounded to fp64 and symmetrised; returns (G, Q)"""
    J = len(lam)
    if Q is None:
        Q, _ = np.linalg.qr(rng.standard_normal((J, J)))
    Ql = Q.astype(LD)
    G = ((Ql * np.asarray(lam, dtype=LD)[None, :]) @ Ql.T).astype(np.float64)
    return 0.5 * (G + G.T), Q


def perturbed(rng, G, eps):
    """(I + eps S) G (I + eps S)^T, S symmetric with ||S||_2 = 1: a congruence, so a Gram stays a Gram"""
    J = G.shape[0]
    S = rng.standard_normal((J, J))
    S = 0.5 * (S + S.T)
    S /= np.linalg.norm(S, 2)
    B = (np.eye(J) + eps * S).astype(LD)
    Gn = (B @ G.astype(LD) @ B.T).astype(np.float64)
    return 0.5 * (Gn + Gn.T)


class Ref:
    """what numpy eigh says about one matrix: leading vectors, gap, and its own values of checks 1 and 2"""

    def __init__(self, G, rank, name, dominant=0):
        J = G.shape[0]
        w, V = np.linalg.eigh(G)
        w, V = w[::-1], V[:, ::-1]
        self.G, self.J, self.rank, self.w, self.V = G, J, rank, w, V[:, :rank].copy()
        self.lam1 = float(max(abs(w[0]), abs(w[-1])))
        self.gap = float(w[rank - 1] - w[rank]) if rank < J else np.inf
        # (dominant=1, the lam_1 = 1e6 x the rest spectrum only: the condition is on what is left below lam_1)
        top = float(abs(w[min(dominant, J - 1)])) if dominant < rank else self.lam1
        assert self.gap / top >= 1e-3, f"{name}: gap / lam = {self.gap / top:.2e} < 1e-3 at the cut"
        self.orth, self.res, _ = eig_quantities(G, self.V)


def eig_quantities(G, Um):
    """(max |U^T U - I|, ||G U - U diag(theta)||_F, theta), in long double"""
    Ul, Gl = Um.astype(LD), G.astype(LD)
    orth = float(np.max(np.abs(Ul.T @ Ul - np.eye(Um.shape[1], dtype=LD)))) if Um.shape[1] else 0.0
    GU = Gl @ Ul
    theta = np.sum(Ul * GU, axis=0)
    res = float(np.sqrt(np.sum((GU - Ul * theta[None, :]) ** 2)))
    return orth, res, theta.astype(np.float64)


def sine(Um, V):
    """the largest principal-angle sine between span(Um) (orthonormal to rounding) and span(V)"""
    if V.shape[1] == V.shape[0]:
        return 0.0
    Ul, Vl = Um.astype(LD), V.astype(LD)
    R = Ul - Vl @ (Vl.T @ Ul)
    return float(np.linalg.norm(R.astype(np.float64), 2))


def eig_caps(ref, fam):
    """(orthonormality, residual, sine) caps of a route family: conditions of the project's own acceptance rule
    (module docstring)"""
    J, r = ref.J, ref.rank
    res = 1e-13 * ref.lam1
    if np.isfinite(ref.gap) and fam == "projector":
        res = max(1e-9 * ref.gap, 1e-14 * ref.lam1)
    res *= np.sqrt(r)
    orth = 240.0 * J * U if fam == "full" else 6.0 * (J * r + r * (r + 1)) * U
    return orth, res, (res / ref.gap if np.isfinite(ref.gap) else np.inf)


def check_eig(st, what, Um, ref, fam, order=True, residual=True, clusters=()):
    """checks 1-4 of the module docstring on the J x rank result Um"""
    assert Um.shape == (ref.J, ref.rank)
    cap_o, cap_r, cap_s = eig_caps(ref, fam)
    orth, res, theta = eig_quantities(ref.G, Um)
    fl_o, fl_r = ref.J * U, ref.J * U * ref.lam1
    m = MULT[fam]
    bar_o = cap_o if m["orth"] is None else min(cap_o, m["orth"] * max(ref.orth, fl_o))
    bar_r = cap_r if m["res"] is None else min(cap_r, m["res"] * max(ref.res, fl_r))
    if st.hip:
        _ratio(fam, "orth", orth, max(ref.orth, fl_o))
        if residual:
            _ratio(fam, "res", res, max(ref.res, fl_r))
    scalar_within(st, f"{what} [{fam}] max|U^T U - I|", orth, bar_o)
    if residual:
        scalar_within(st, f"{what} [{fam}] residual", res, bar_r)
    if order:
        skip = {k for a, b in clusters for k in range(a, b)}  # (pairs k, k + 1 inside a cluster)
        for k in range(ref.rank - 1):
            assert k in skip or theta[k] > theta[k + 1], \
                f"{st.c['name']} {what}: theta not descending at {k}: {theta[k]!r} <= {theta[k + 1]!r}"
    if ref.rank < ref.J:
        scalar_within(st, f"{what} [{fam}] subspace sine", sine(Um, ref.V), min(bar_r, cap_r) / ref.gap)


def numpy_within_caps(c):
    """the CPU-side condition of the table: numpy eigh's own vectors pass every cap with room (a quarter), on every
    matrix of the case; check 4 against the crafted eigenvectors where the case has them"""
    rng = np.random.default_rng(c["seed"])
    out = []
    for G, Qtrue, rank, _ in eig_matrices(rng, c):
        ref = Ref(G, rank, c["name"], c.get("dominant", 0))
        for fam in ("full", "projector", "cold"):
            cap_o, cap_r, cap_s = eig_caps(ref, fam)
            assert ref.orth <= cap_o / 4 and ref.res <= cap_r / 4, (c["name"], ref.orth, cap_o, ref.res, cap_r)
            if Qtrue is not None and rank < ref.J:
                s = sine(ref.V, Qtrue[:, :rank])
                assert s <= cap_s / 4, (c["name"], s, cap_s)
        out.append((ref.orth / cap_o, ref.res / cap_r))
    return out


# spectra: name -> lam(J, rank), descending
def spectrum(kind, J, rank, rng):
    k = np.arange(J, dtype=np.float64)
    if kind == "geo":  # wanted: 10 .. 3 spread linearly; the rest decays from 1
        lam = np.where(k < rank, 10.0 - 7.0 * k / max(rank - 1, 1), 0.8 ** (k - rank))
    elif kind == "pair":  # a repeated eigenvalue inside the wanted set (indices 1, 2)
        lam = spectrum("geo", J, rank, rng)
        lam[2] = lam[1]
    elif kind == "dom1":  # lam_1 = 1e6 x the rest
        lam = spectrum("geo", J, rank, rng)
        lam[0] = 1e6 * lam[1] if J > 1 else lam[0]
    elif kind == "dom2":  # two dominant eigenvalues, both >= 20 x the third
        lam = spectrum("geo", J, rank, rng)
        lam[0], lam[1] = 30.0 * lam[2], 24.0 * lam[2]
    elif kind == "deficient":  # PSD of numerical rank `rank`
        lam = np.where(k < rank, 10.0 - 7.0 * k / max(rank - 1, 1), 0.0)
    elif kind == "low_shift":  # 0.4 x lam_{rank+1} lies below two further eigenvalues
        lam = spectrum("geo", J, rank, rng)
        lam[rank:rank + 3] = [2.5, 1.8, 1.3]
        lam[rank + 3:] = 0.9 * 0.8 ** np.arange(J - rank - 3)
    elif kind == "slow":  # lam_{rank+17} / lam_rank close to 1: block subspace iteration crawls
        lam = np.where(k < rank, 10.0 - 6.0 * k / max(rank - 1, 1), 2.9 - 0.4 * (k - rank) / (J - rank))
    else:
        raise KeyError(kind)
    return lam


def eig_matrices(rng, c):
    """the calls of a case in order: (matrix, its crafted eigenvector matrix or None, rank, action); action "free":
    the slot's session block is freed before the call, "lazy_off": eig_lazy(slot, false) before the call"""
    J, rank, kind = c["J"], c.get("rank", 1), c.get("spec", "geo")
    if kind == "diag":
        return [(np.diag(spectrum("geo", J, rank, rng)), np.eye(J), rank, None)]
    if kind == "noise":  # the Gram of a noise matrix: no gap the Ritz values can see
        # (256 J columns: lam_rank / lam_rank+5 = 1.013, inside the 2 % the cold start asks of its Ritz values)
        N = np.random.default_rng(c["noise_seed"]).standard_normal((J, 256 * J))
        G0 = (N @ N.T) / (256 * J)
        G0, Q0 = 0.5 * (G0 + G0.T), None
    else:
        G0, Q0 = craft(rng, spectrum(kind, J, rank, rng))
    out = [(G0, Q0, rank, None)]
    for step in c.get("steps", []):
        G, _, rk, _ = out[-1]
        if step[0] == "perturb":
            out.append((perturbed(rng, G, step[1]), None, rk, step[2] if len(step) > 2 else None))
        elif step[0] == "scale":
            out.append((G * step[1], None, rk, None))
        elif step[0] == "cross":  # lam_rank and lam_rank+1 cross: their eigenvectors trade places
            lam = spectrum(kind, J, rank, rng)
            lam[rank - 1], lam[rank] = lam[rank], lam[rank - 1]
            out.append((craft(rng, lam, Q0)[0], None, rk, None))
        elif step[0] == "newJ":  # the same slot goes on with a matrix of another size
            G2, Q2 = craft(rng, spectrum("geo", step[1], step[2], rng))
            out.append((G2, Q2, step[2], None))
        elif step[0] in ("same", "free"):
            out.append((G.copy(), None, rk, "free" if step[0] == "free" else None))
        else:
            raise KeyError(step[0])
    return out


def route_family(tags):
    """the family of the step that produced U: the last tag of the call that names a producer (a projector step
    that was not accepted, a Ritz block, a retry produce nothing)"""
    fam = "full"
    for t in tags:
        if t.startswith("eig.projector") and t.endswith(" ok=1"):
            fam = "cold" if " strict=1" in t else "projector"
        elif t.startswith(("eig.cold.subspace", "eig.cold.bisect")):
            fam = "cold"
        elif t.startswith(("eig.full", "eig.small")):
            fam = "full"
    return fam


def full_route(J):
    return "eig.full.lds_jacobi" if J <= 64 else "eig.full.onesided_jacobi" if J <= K_EV_MAX else "eig.full.dsyevd"


def _call_eig(st, i, G, rank, slot, fn):
    """one eigenvector call on a fresh (raw, in / out) copy of G and a fresh U; returns (U, the call's tags)"""
    J = G.shape[0]
    g = st.out(f"G{i}", J * J, init=G.reshape(-1, order="F"), raw=True)
    u = st.out(f"U{i}", J * rank)
    gp = g.ptr
    own = st.sh.eig_gram(slot, J) if (slot is not None and slot >= 0 and st.c.get("own_gram")) else None
    if own:
        st.sh.d2d(own, g.ptr, 8 * J * J)
        gp = own
    fn(gp, u.ptr)
    st.sh.sync()
    tags = st.sh.route_take()
    st.tags += tags
    st.fetch(f"U{i}")
    return u, tags


def op_eig_full(st):
    c = st.c
    G = eig_matrices(st.rng, c)[0][0]
    J, rank = c["J"], c["rank"]
    _call_eig(st, 0, G, rank, None, lambda g, u: st.sh.top_eigvecs(g, J, rank, u))
    st.finish()
    st.ref = Ref(G, rank, c["name"], c.get("dominant", 0))

    def verify():
        Um = st.got("U0").reshape((J, rank), order="F")
        check_eig(st, "U", Um, st.ref, "full", clusters=c.get("clusters", ()))
    st.verify = verify


def op_eig_warm(st):
    """a sequence of top_eigvecs_warm calls on one slot (c['slot']: absent = a slot of a fresh session, -1 as it is)"""
    c, sh = st.c, st.sh
    calls = eig_matrices(st.rng, c)
    base = sh.eig_session_new()
    slot = c.get("slot", base + 3)
    lazy = bool(c.get("lazy"))
    checks = []
    try:
        if lazy:
            sh.eig_lazy(slot, True)
        for i, (G, _, ri, action) in enumerate(calls):
            if action == "free":
                # (the block's number is drawn afresh: the SAME slot number is reused to show that its state is gone)
                sh.eig_session_free(base)
                if lazy:
                    sh.eig_lazy(slot, True)
            if action == "lazy_off":
                sh.eig_lazy(slot, False)
            Ji = G.shape[0]
            _, tags = _call_eig(st, i, G, ri, slot, lambda g, u: sh.top_eigvecs_warm(g, Ji, ri, u, slot))
            Y = None
            if lazy:
                yp = sh.eig_pending_rotation(slot)
                lazy_step = any(" lazy=1" in t for t in tags)
                if st.hip:
                    assert bool(yp) == lazy_step, f"{c['name']} call {i}: pending rotation {yp} but tags {tags}"
                if yp:
                    Y = sh.d2h(yp, 8 * ri * ri).view(np.float64).reshape((ri, ri), order="F").copy()
                    sh.eig_rotation_done(slot)
                    assert not sh.eig_pending_rotation(slot), f"{c['name']} call {i}: rotation still pending"
            checks.append((i, G, ri, tags, Y))
    finally:
        sh.eig_session_free(base)
    st.finish()
    st.calls = checks

    def verify():
        for i, G, ri, tags, Y in st.calls:
            ref = Ref(G, ri, f"{c['name']} call {i}", c.get("dominant", 0))
            Um = st.got(f"U{i}").reshape((G.shape[0], ri), order="F")
            fam = route_family(tags) if st.hip else "full"
            if Y is not None:
                check_eig(st, f"call {i} lazy U", Um, ref, fam, order=False, residual=False)
                UY = (Um.astype(LD) @ Y.astype(LD)).astype(np.float64)
                check_eig(st, f"call {i} U Y", UY, ref, fam)
            else:
                check_eig(st, f"call {i} U", Um, ref, fam)
            if st.hip and c.get("routes"):
                for pat in c["routes"][i]:
                    assert any(re.match(pat, t) for t in tags), f"{c['name']} call {i}: route {pat!r} expected in {tags}"
                for pat in c.get("not_routes", [[]] * (i + 1))[i]:
                    assert not any(re.match(pat, t) for t in tags), f"{c['name']} call {i}: route {pat!r} in {tags}"
    st.verify = verify


def op_eig_defer(st):
    """lazy + deferred: the sequence goes on until a step defers, then eig_deferred / eig_verify and the basis;
    c['expect']: what eig_verify must say (0 accepted, 1 under PPALS_EIG_DEFER_FAIL=1 or with discard)"""
    c, sh = st.c, st.sh
    J, rank = c["J"], c["rank"]
    G0, _ = craft(st.rng, spectrum(c["spec"], J, rank, st.rng))
    base = sh.eig_session_new()
    slot = base + 1
    st.calls, st.deferred_at = [], None
    try:
        assert sh.eig_verify(slot) == -1, f"{c['name']}: eig_verify on an idle slot"
        assert not sh.eig_deferred(slot)
        sh.eig_lazy(slot, True)
        sh.eig_defer(slot, True)
        G = G0
        for i in range(10):
            _, tags = _call_eig(st, i, G, rank, slot, lambda g, u: sh.top_eigvecs_warm(g, J, rank, u, slot))
            if sh.eig_deferred(slot):
                if st.hip:
                    assert any(" defer_now=1" in t for t in tags), f"{c['name']}: deferred without its tag: {tags}"
                v = sh.eig_verify(slot, bool(c.get("discard")))
                st.tags += sh.route_take()
                assert v == c["expect"], f"{c['name']}: eig_verify returned {v}, expected {c['expect']}"
                assert sh.eig_verify(slot) == -1 and not sh.eig_deferred(slot)
                st.deferred_at = i
                if v == 0:
                    yp = sh.eig_pending_rotation(slot)
                    Y = None
                    if yp:
                        Y = sh.d2h(yp, 8 * rank * rank).view(np.float64).reshape((rank, rank), order="F").copy()
                        sh.eig_rotation_done(slot)
                    st.calls.append((i, G, tags, Y, "projector" if st.hip else "full"))
                else:  # the factor is thrown away; the next call of the slot takes the checked route
                    _, tags2 = _call_eig(st, i + 1, G, rank, slot,
                                         lambda g, u: sh.top_eigvecs_warm(g, J, rank, u, slot))
                    if st.hip:
                        assert not any(" defer_now=1" in t for t in tags2), (c["name"], tags2)
                    yp = sh.eig_pending_rotation(slot)
                    Y = None
                    if yp:
                        Y = sh.d2h(yp, 8 * rank * rank).view(np.float64).reshape((rank, rank), order="F").copy()
                        sh.eig_rotation_done(slot)
                    st.calls.append((i + 1, G, tags2, Y, route_family(tags2) if st.hip else "full"))
                break
            yp = sh.eig_pending_rotation(slot)
            if yp:
                sh.eig_rotation_done(slot)
            G = perturbed(st.rng, G, 0.01)
    finally:
        sh.eig_session_free(base)
    st.finish()

    def verify():
        assert st.deferred_at is not None, f"{c['name']}: no step deferred in 10 calls: {st.tags}"
        for i, G, tags, Y, fam in st.calls:
            ref = Ref(G, rank, c["name"])
            Um = st.got(f"U{i}").reshape((J, rank), order="F")
            if Y is not None:
                check_eig(st, f"call {i} deferred U", Um, ref, fam, order=False, residual=False)
                Um = (Um.astype(LD) @ Y.astype(LD)).astype(np.float64)
            check_eig(st, f"call {i} U Y", Um, ref, fam)
    st.verify = verify


# ------------------------------------------------------------------------------------------ orthonormalize
def qr_input(rng, rows, r, cond):
    """rows x r with singular values 1 .. 1 / cond (geometric), cond asserted"""
    P, _ = np.linalg.qr(rng.standard_normal((rows, r)))
    V, _ = np.linalg.qr(rng.standard_normal((r, r)))
    s = cond ** (-np.arange(r) / max(r - 1, 1)) if r > 1 else np.ones(1)
    A = ((P.astype(LD) * s[None, :].astype(LD)) @ V.T.astype(LD)).astype(np.float64)
    sv = np.linalg.svd(A, compute_uv=False)
    assert abs(sv[0] / sv[-1] / (cond if r > 1 else 1.0) - 1) < 1e-3 and cond <= 2.0 ** 26.5 / 8 * 1.0001, (rows, r, cond)
    return A


def qr_quantities(Uin, Q):
    """(max |Q^T Q - I|, max strictly-lower |Q^T U_in| / ||U_in||_2, min diagonal of Q^T U_in,
    ||U_in - Q triu(Q^T U_in)||_F / ||U_in||_F), in long double"""
    Ql, Al = Q.astype(LD), Uin.astype(LD)
    r = Q.shape[1]
    orth = float(np.max(np.abs(Ql.T @ Ql - np.eye(r, dtype=LD))))
    M = Ql.T @ Al
    n2 = np.linalg.norm(Uin, 2)
    low = float(np.max(np.abs(np.tril(M, -1)))) / n2 if r > 1 else 0.0
    rec = float(np.sqrt(np.sum((Al - Ql @ np.triu(M)) ** 2)) / np.sqrt(np.sum(Al ** 2)))
    return orth, low, float(np.min(np.diag(M))), rec


def check_qr(st, Uin, Q):
    rows, r = Uin.shape
    orth, low, dmin, rec = qr_quantities(Uin, Q)
    Qh, Rh = np.linalg.qr(Uin)
    Qh = Qh * np.where(np.diag(Rh) < 0, -1.0, 1.0)[None, :]
    _, low_h, dmin_h, rec_h = qr_quantities(Uin, Qh)
    assert dmin_h > 0
    bar_o = 6.0 * (rows * r + r * (r + 1)) * U
    scalar_within(st, "max|Q^T Q - I|", orth, bar_o)
    assert dmin > 0, f"{st.c['name']}: diagonal of Q^T U_in not positive ({dmin:.3e})"
    fl = r * U
    if st.hip:
        _ratio("qr", "tri", low, max(low_h, fl))
        _ratio("qr", "rec", rec, max(rec_h, fl))
    m = MULT["qr"]
    # (not yet measured: Q^T U_in = (I + d) R + Q^T E with |d| <= the orthogonality bar and ||E|| the reconstruction
    # error, itself of the order of the orthogonality bar for CholeskyQR2 — both relative to ||U_in||)
    scalar_within(st, "strictly lower part of Q^T U_in / ||U_in||", low,
                  2 * bar_o if m["tri"] is None else min(2 * bar_o, m["tri"] * max(low_h, fl)))
    scalar_within(st, "||U_in - Q triu(Q^T U_in)|| / ||U_in||", rec,
                  2 * bar_o * np.sqrt(r) if m["rec"] is None else min(2 * bar_o * np.sqrt(r), m["rec"] * max(rec_h, fl)))


def op_orthonormalize(st):
    c = st.c
    rows, r = c["rows"], c["r"]
    if r == 0:
        u = st.out("U", 4, init=np.arange(4.0), res=np.arange(0))
        ok = st.sh.orthonormalize(u.ptr, rows, 0)
        st.finish()
        st.verify = lambda: _assert(ok is True, f"{c['name']}: r = 0 must return true")
        return
    A = qr_input(st.rng, rows, r, c["cond"])
    bad = c.get("bad")
    if bad:  # an exactly rank-deficient input: a duplicated / zero column
        kind, col = bad
        A[:, col] = A[:, col - 1] if kind == "dup" else 0.0
    u = st.out("U", rows * r, init=A.reshape(-1, order="F"), raw=bool(bad))
    ok = st.sh.orthonormalize(u.ptr, rows, r)
    st.finish()

    def verify():
        if bad:
            assert ok is False, f"{c['name']}: a rank-deficient input was accepted"
            return
        assert ok is True, f"{c['name']}: refused at cond {c['cond']:g}"
        check_qr(st, A, st.got("U").reshape((rows, r), order="F"))
    st.verify = verify
    st.A = A


def _assert(cond, msg):
    assert cond, msg


# ------------------------------------------------------------------------------------------ the small ops
def mix(rng, shape):
    return 2.0 * rng.random(shape) - 1.0


def op_sign_align(st):
    c = st.c
    rows, r = c["rows"], c["r"]
    W, Wr = mix(st.rng, (rows, r)), mix(st.rng, (rows, r))
    flip = np.array([np.sum(W[:, k].astype(LD) * Wr[:, k].astype(LD)) for k in range(r)])
    # (a sign decided by rounding is not a case: keep the dot products clear of zero)
    for k in range(r):
        if abs(flip[k]) < 1e-3 * rows:
            Wr[:, k] = W[:, k] * (1 if k % 2 else -1)
    expect = np.array([not (np.sum(W[:, k].astype(LD) * Wr[:, k].astype(LD)) > 0) for k in range(r)])
    if c.get("zero") is not None and rows >= 2:  # disjoint supports: the dot product is exactly 0 -> flips
        k = c["zero"]
        W[0::2, k], Wr[1::2, k] = 0.0, 0.0
        Wr[0::2, k] = 1.0
        expect[k] = True
    elif c.get("zero") is not None:
        Wr[:, c["zero"]] = 0.0
        expect[c["zero"]] = True
    if c.get("nan") is not None:  # a NaN dot product flips too: !(c > 0)
        Wr[0, c["nan"]] = np.nan
        expect[c["nan"]] = True
    w = st.out("W", rows * r, init=W.reshape(-1, order="F"))
    wr = st.inp(Wr.reshape(-1, order="F"))
    st.sh.sign_align(w.ptr, wr.ptr, rows, r)
    st.finish()

    def verify():
        got = st.got("W").reshape((rows, r), order="F")
        want = W * np.where(expect, -1.0, 1.0)[None, :]
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), \
            f"{c['name']}: columns {np.nonzero(np.any(got != want, axis=0))[0]} are not +-1 x the input, bit for bit"
    st.verify = verify


def op_rows_times_small(st):
    c = st.c
    rows, K, Cc, form = c["rows"], c["K"], c["C"], c["form"]
    A, B = mix(st.rng, (rows, K)), mix(st.rng, (K, Cc))
    D = mix(st.rng, (rows, Cc)) if form in ("D", "Dalias") else None
    b = st.inp(B.reshape(-1, order="F"))
    res = np.arange(rows * Cc)
    if form == "inplace":  # out == A: the workspace route
        init = np.full(rows * max(K, Cc), np.nan)
        init[:rows * K] = A.reshape(-1, order="F")
        o = st.out("out", rows * max(K, Cc), res=res, init=init)
        ap, dp = o.ptr, 0
    else:
        ap = st.inp(A.reshape(-1, order="F")).ptr
        if form == "Dalias":
            o = st.out("out", rows * Cc, init=D.reshape(-1, order="F"))
            dp = o.ptr
        else:
            o = st.out("out", rows * Cc)
            dp = st.inp(D.reshape(-1, order="F")).ptr if D is not None else 0
    if c.get("refused"):
        try:
            st.sh.rows_times_small(ap, rows, K, b.ptr, Cc, dp, o.ptr)
            refused = False
        except opshim_util.ShimError:
            refused = True
        st.finish()
        st.verify = lambda: _assert(refused or not st.hip, f"{c['name']}: K C 8 > 60 KiB was not refused")
        st.outs["out"] = (o, np.arange(0) if refused else res, not refused)
        return
    st.sh.rows_times_small(ap, rows, K, b.ptr, Cc, dp, o.ptr)
    st.finish()

    def verify():
        got = st.got("out").reshape((rows, Cc), order="F")
        ref = A.astype(LD) @ B.astype(LD) + (D.astype(LD) if D is not None else 0)
        bar = (K + 3) * U * (np.abs(A) @ np.abs(B) + (np.abs(D) if D is not None else 0))
        within(st, "out", got, ref, bar)
    st.verify = verify


def op_lowrank(st):
    c = st.c
    n, R, r, dt = c["n"], c["R"], c["r"], c["dt"]
    Xx, Xs = CC._stored(mix(st.rng, (n, R)), dt)
    T, VT = mix(st.rng, (n, r)), mix(st.rng, (r, R))
    x = st.out("X", n * R, t=Xs.dtype, init=Xs.reshape(-1, order="F"))
    t, v = st.inp(T.reshape(-1, order="F")), st.inp(VT.reshape(-1, order="F"))
    st.sh.lowrank_accumulate(x.ptr, CC.DT[dt], n, R, t.ptr, r, v.ptr)
    st.finish()

    def verify():
        got = st.got("X").reshape((n, R), order="F")
        ref = Xx.astype(LD) + T.astype(LD) @ VT.astype(LD)
        bar = (r + 3) * U * (np.abs(T) @ np.abs(VT)) + (U24 if dt == "f32" else U) * np.abs(ref)
        within(st, "X", got, ref, bar)
    st.verify = verify


def op_add_inplace(st):
    n = st.c["n"]
    a, b = mix(st.rng, n), mix(st.rng, n) * 10.0 ** st.rng.integers(-3, 4, n)
    d = st.out("dst", n, init=a)
    s = st.inp(b)
    st.sh.add_inplace(d.ptr, s.ptr, n)
    st.finish()

    def verify():
        ref = a.astype(LD) + b.astype(LD)
        within(st, "dst", st.got("dst"), ref, U * np.abs(ref))
    st.verify = verify


def op_transpose(st):
    c = st.c
    rows, cols, batch, dt = c["rows"], c["cols"], c["batch"], c["dt"]
    x = mix(st.rng, (batch, cols, rows))  # [b][c][r]: src[r + rows * (c + cols * b)]
    if dt == "bf16":
        # (bit patterns, handled as float16 images: no bf16 value of [-1, 1) reads as a float16 NaN)
        src = bf16_bits(x).reshape(x.shape).astype(np.uint16).view(np.float16)
        t = np.float16
    else:
        src = x.astype(np.float32 if dt == "f32" else np.float64)
        t = src.dtype
    s = st.inp(src.reshape(-1), t)
    d = st.out("dst", rows * cols * batch, t=t)
    if c.get("batched", True):
        st.sh.transpose_batched(s.ptr, CC.DT[dt], rows, cols, batch, d.ptr)
    else:
        st.sh.transpose2d(s.ptr, CC.DT[dt], rows, cols, d.ptr)
    st.finish()

    def verify():
        o, res, _ = st.outs["dst"]
        st.got("dst")  # (guards, NaN)
        got = st.posts["dst"][CC.GUARD:-CC.GUARD].view(t).reshape((batch, rows, cols))  # dst[c + cols * (r + rows * b)]
        assert np.array_equal(np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(src.transpose(0, 2, 1)).view(np.uint8)), \
            f"{c['name']}: the transpose is not exact"
    st.verify = verify


OPS = {"unfold_gram": op_unfold_gram, "eig_full": op_eig_full, "eig_warm": op_eig_warm, "eig_defer": op_eig_defer,
       "orthonormalize": op_orthonormalize, "sign_align": op_sign_align, "rows_times_small": op_rows_times_small,
       "lowrank": op_lowrank, "add_inplace": op_add_inplace, "transpose": op_transpose}

# ------------------------------------------------------------------------------------------ the table
CASES = []


def _add(op, family, name, route, why, **kw):
    c = dict(op=op, family=family, name=f"{family}/{name}", route=route, why=why, seed=1000 + len(CASES), **kw)
    CASES.append(c)
    return c


# ---- unfold_gram
def gram(name, why, dt, L, J, T, cls="mix", env=None, near=None):
    lds_min = int(env["PPALS_SYM_LDS_MIN"]) if env else SYM_LDS_MIN
    tag, bitsym = gram_route(dt, L, J, T, lds_min)
    if near:
        assert not tag.startswith(near), (name, tag)
    kw = dict(env=env) if env else {}
    _add("unfold_gram", "unfold_gram", f"{name} {dt} L{L} J{J} T{T} {cls}", [re.escape(tag)], why, dt=dt, L=L, J=J, T=T,
         cls=cls, bitsym=bitsym, **kw)


for dt in ("f32", "f64"):
    for J in (1, 7, 15):
        for L in (1, 3):
            gram("valu", "tiny mode, C no multiple of 32", dt, L, J, 37)
    for J in (16, 33, 63):
        gram("mfma", "partial edge tiles, the p-fast load", dt, 1, J, 33)
        gram("mfma", "partial edge tiles, the c-fast load", dt, 5, J, 7)
    for C in (1, 31, 32):
        gram("mfma", "C around one chunk", dt, 1, 33, C)
    # k_split with 256 CUs at J = 33 (4 tiles): want = min(256, C / 256); C = 1000 -> 3 slabs of 352, the last ragged
    gram("mfma", "nsplit > 1 with a ragged last slab", dt, 1, 33, 1000)
    gram("mfma", "nsplit > 1, c-fast", dt, 5, 16, 203)
gram("mfma", "a mean component: cancellation-free sums", "f32", 1, 33, 1000, cls="mean")
gram("mfma", "fp64, J >= 64 below the symmetric route's window", "f64", 1, 64, 15, near="unfold_gram.sym")
gram("mfma", "fp64, J >= 64 above the symmetric route's window", "f64", 1, 64, 4097, near="unfold_gram.sym")
for J in (64, 80, 100):
    for C in (16, 17, 100):
        gram("sym", "the 16-tile symmetric product", "f64", 1, J, C)
gram("sym", "through transpose_batched into the workspace", "f64", 3, 80, 7)
gram("sym", "through transpose_batched, ragged", "f64", 3, 100, 7, cls="mean")
for J in (64, 100):
    gram("sym.lds", "k_dgemm_nt_sym_lds<32> at small J", "f64", 1, J, 17, env={"PPALS_SYM_LDS_MIN": "64"})
    gram("sym.lds", "the same behind a transpose", "f64", 3, J, 7, env={"PPALS_SYM_LDS_MIN": "64"})
for J in (64, 68, 132):
    gram("syrk", "one / ragged second / three tiles, C = 4096 exactly", "f32", 1, J, 4096)
gram("syrk", "C = 4096 + 32", "f32", 1, 68, 4128)
gram("syrk", "C = 4096 + 32, a mean component", "f32", 1, 132, 4128, cls="mean")
gram("syrk", "the c-fast load", "f32", 4, 68, 1024)
gram("mfma", "near miss of the SYRK: J % 4 != 0", "f32", 1, 66, 4096, near="unfold_gram.syrk")
gram("mfma", "near miss of the SYRK: L % 4 != 0", "f32", 6, 64, 683, near="unfold_gram.syrk")


# ---- the full solvers
def full(name, J, rank, spec, why, **kw):
    _add("eig_full", "eig_full", f"{name} J{J} r{rank} {spec}", [re.escape(full_route(J))], why, J=J, rank=rank,
         spec=spec, **kw)


for J in (1, 2, 17, 50, 64):
    for rank in sorted({1, max(1, J // 2), J}):
        full("lds", J, rank, "geo", "in-LDS Jacobi")
full("lds", 17, 8, "pair", "a repeated eigenvalue inside the wanted set", clusters=[(1, 2)])
full("lds", 50, 25, "diag", "a diagonal matrix: no rotation needed")
full("lds", 50, 5, "deficient", "PSD of numerical rank 5")
for J in (65, 96, 128):
    for rank in (1, 20, J):
        full("onesided", J, rank, "geo", "one-sided Jacobi, one workgroup")
full("onesided", 96, 20, "dom1", "lam_1 = 1e6 x the rest", dominant=1)
full("onesided", 96, 20, "deficient", "PSD of rank 20: rounding-level negative eigenvalues below")
for J in (129, 200):
    for rank in (1, 30):
        full("dsyevd", J, rank, "geo", "the vendor solver, ascending -> descending in k_take_top")

# ---- warm sequences
P_OK = r"eig\.projector m=%d strict=0 fused_scale=%d fused_tail=%d wide=0 lazy=%d defer_now=0 ok=1"
COLD = [r"eig\.cold\.ritz ok=1", r"eig\.projector m=\d strict=1 fused_scale=0 fused_tail=\d wide=\d lazy=\d defer_now=0 ok=1"]
STEPS4 = [("perturb", 0.01), ("perturb", 0.02), ("perturb", 0.03), ("perturb", 0.01)]


def warm(name, J, rank, spec, steps, routes, why, **kw):
    _add("eig_warm", "eig_warm", f"{name} J{J} r{rank} {spec}", [], why, J=J, rank=rank, spec=spec, steps=steps,
         routes=routes, once=True, **kw)


for J in (16, 50, 64):
    warm("small", J, max(1, J // 3), "geo", [("perturb", 0.02), ("perturb", 0.02)],
         [[r"eig\.small cold=1"], [r"eig\.small cold=0"], [r"eig\.small cold=0"]], "small modes: Jacobi on Q^T G Q")
warm("small.J", 32, 8, "geo", [("perturb", 0.02), ("newJ", 48, 8), ("same",)],
     [[r"eig\.small cold=1"], [r"eig\.small cold=0"], [r"eig\.small cold=1"], [r"eig\.small cold=0"]],
     "a J change on the same slot resets it")
warm("small.free", 32, 8, "geo", [("perturb", 0.02), ("free",), ("same",)],
     [[r"eig\.small cold=1"], [r"eig\.small cold=0"], [r"eig\.small cold=1"], [r"eig\.small cold=0"]],
     "a slot reused after eig_session_free starts cold")
warm("proj", 96, 8, "geo", STEPS4, [COLD] + [[P_OK % (0, 1, 1, 0)]] * 4, "fused scale and fused tail")
warm("proj", 96, 56, "geo", STEPS4, [COLD + [r"chol_qr2\.blocks r=72", r"orthonormalize nblk=2"]] +
     [[P_OK % (0, 1, 0, 0)]] * 4, "plain tail: rank + 16 > 64")
warm("proj", 160, 100, "geo", STEPS4[:3], [COLD + [r"chol_qr2\.blocks r=116"]] + [[P_OK % (0, 1, 0, 0)]] * 3,
     "Rayleigh-Ritz above 64 columns through the one-sided Jacobi")
warm("proj.free", 96, 8, "geo", [("perturb", 0.01), ("free",), ("same",)],
     [COLD, [P_OK % (0, 1, 1, 0)], COLD, [P_OK % (0, 1, 1, 0)]], "a freed slot starts cold")
warm("proj.m1", 96, 8, "dom1", STEPS4, [[r"eig\.cold\.ritz ok=0", r"eig\.warm\.bootstrap", re.escape(full_route(96))]] +
     [[P_OK % (1, 1, 1, 0)]] * 4, "one dominant eigenpair: power steps, deflation",
     dominant=1)
warm("proj.m2", 96, 8, "dom2", STEPS4, [[]] + [[P_OK % (2, 0, 0, 0)]] * 4, "two dominant eigenpairs: block deflation")
warm("proj.jump", 96, 8, "geo", [("perturb", 0.01), ("scale", 40.0), ("perturb", 0.01)],
     [COLD, [P_OK % (0, 1, 1, 0)], [r"eig\.warm\.frob_retry"], []], "a jump that outruns the spectral bound")
warm("proj.cross", 96, 8, "geo", [("perturb", 0.0), ("cross",), ("perturb", 0.01)],
     [COLD, [P_OK % (0, 1, 1, 0)], [r"eig\.projector .* ok=0|eig\.cold|eig\.warm\.bootstrap"], []],
     "lam_rank and lam_rank+1 cross between calls: the route falls back")
warm("proj.lowshift", 96, 8, "low_shift", [("perturb", 0.01), ("perturb", 0.01)],
     [[]] + [[r"eig\.projector m=0 strict=0 fused_scale=0 fused_tail=1 wide=1 lazy=0 defer_now=0 ok=1"]] * 2,
     "a shift two eigenvalues too low: the wide tail delivers exactly rank vectors", env={"PPALS_EIG_SIGMA_SCALE": "0.4"})
warm("cold.bisect", 96, 8, "noise", [("perturb", 0.01)], [[r"eig\.cold\.ritz", r"eig\.cold\.bisect"], []],
     "a flat spectrum: the shift is placed by counting", noise_seed=1)
warm("cold.subspace", 96, 8, "geo", [("perturb", 0.01)], [[r"eig\.cold\.ritz ok=1", r"eig\.cold\.subspace"], [P_OK % (0, 1, 1, 0)]],
     "block subspace iteration converges", env={"PPALS_COLD_SUBSPACE_FROM": "65"})
warm("cold.subspace.slow", 96, 8, "slow", [("perturb", 0.01)],
     [[r"eig\.cold\.ritz ok=1", r"eig\.projector m=\d strict=1"], []],
     "lam_{rank+17} / lam_rank near 1: it gives up and hands over to the projector",
     env={"PPALS_COLD_SUBSPACE_FROM": "65"}, not_routes=[[r"eig\.cold\.subspace"], []])
warm("fast0", 96, 8, "geo", [("perturb", 0.01)], [[r"eig\.warm\.direct why=fast", re.escape(full_route(96))]] * 2,
     "PPALS_EIG_FAST=0: the full solver everywhere", env={"PPALS_EIG_FAST": "0"})
warm("fast2", 160, 100, "geo", [("perturb", 0.01)], [[r"eig\.warm\.bootstrap", r"eig\.full\.dsyevd"], [P_OK % (0, 1, 0, 0)]],
     "PPALS_EIG_FAST=2: cold starts by the full solver (bootstrap through dsyevd)", env={"PPALS_EIG_FAST": "2"})
warm("direct.slot", 96, 8, "geo", [("perturb", 0.01)], [[r"eig\.warm\.direct why=slot"]] * 2, "slot = -1", slot=-1)
warm("direct.rank", 96, 80, "geo", [("perturb", 0.01)], [[r"eig\.warm\.direct why=rank_J"]] * 2, "rank + 16 >= J")
warm("direct.rankmax", 200, 120, "geo", [], [[r"eig\.warm\.direct why=rank_max", r"eig\.full\.dsyevd"]],
     "rank + 16 > 128")
warm("direct.J", 50, 8, "geo", [], [[r"eig\.warm\.direct why=J", r"eig\.full\.lds_jacobi"]], "a small mode without a slot",
     slot=-1)
warm("lazy", 96, 8, "geo", STEPS4 + [("perturb", 0.01, "lazy_off")], [COLD] + [[P_OK % (0, 1, 1, 1)]] * 4 +
     [[P_OK % (0, 1, 1, 0)]], "the lazy contract: basis now, rotation owed; nothing owed after a step that was not lazy",
     lazy=True)


def defer(name, why, expect, env=None, **kw):
    _add("eig_defer", "eig_warm", f"defer.{name} J96 r8", [r"eig\.projector m=0 strict=0 fused_scale=1 fused_tail=1 "
         r"wide=0 lazy=1 defer_now=1 ok=1", r"eig\.verify " + ("accepted" if expect == 0 else
                                                              "discarded" if kw.get("discard") else "rejected")],
         why, J=96, rank=8, spec="geo", expect=expect, once=True, env=env or {"PPALS_EIG_DEFER": "1"}, **kw)


defer("accept", "eig_deferred, then eig_verify accepts", 0)
defer("own_gram", "the Gram in the slot's own buffer (eig_gram)", 0, own_gram=True)
defer("fail", "the deferred check reports failure: the next call takes the checked route", 1,
      env={"PPALS_EIG_DEFER_FAIL": "1"}, hip_only=True)  # (the stand-in's failing step hands out a wrong basis)
defer("discard", "eig_verify(slot, true) drops the step", 1, discard=True)
defer("events", "the event hand-over", 0, env={"PPALS_EIG_DEFER": "2"})

# ---- orthonormalize
for r in (1, 5, 64, 65, 100, 130):
    for rows in sorted({r, r + 1, 300}):
        cond = (1.0, 1e3, 1e6)[(r + rows) % 3] if r > 1 else 1.0
        _add("orthonormalize", "orthonormalize", f"r{r} rows{rows} cond{cond:g}", [f"orthonormalize nblk={(r + 63) // 64}(?!\\d)"],
             "block Gram-Schmidt over 64-column blocks of CholeskyQR2", rows=rows, r=r, cond=cond)
for r in (64, 65, 130):
    for cond in (1.0, 1e3, 1e6):
        _add("orthonormalize", "orthonormalize", f"r{r} rows301 cond{cond:g}", [f"orthonormalize nblk={(r + 63) // 64}(?!\\d)"],
             "every block count at every condition number", rows=301, r=r, cond=cond)
_add("orthonormalize", "orthonormalize", "r0", [], "no columns: true, nothing touched", rows=10, r=0)
for kind, col, r in (("dup", 3, 40), ("zero", 3, 40), ("dup", 70, 100), ("zero", 129, 130)):
    _add("orthonormalize", "orthonormalize", f"{kind} column {col} of {r}", [f"orthonormalize nblk={(r + 63) // 64}"],
         "exactly rank deficient: false", rows=300, r=r, cond=10.0, bad=(kind, col))

# ---- the small ops
for r in (1, 4, 5, 9):
    for rows in (1, 63, 64, 65, 300):
        _add("sign_align", "small_ops", f"sign_align rows{rows} r{r}", [], "(r + 3) / 4 blocks, a wave per column",
             rows=rows, r=r, zero=r - 1, nan=(0 if r > 1 else None))
for K in (1, 16, 87):
    for form, Cc in (("plain", 5), ("D", K), ("Dalias", 7), ("inplace", K), ("inplace", 3), ("inplace", K + 2 if K < 80 else K - 3)):
        _add("rows_times_small", "small_ops", f"rows_times_small {form} K{K} C{Cc}",
             [f"rows_times_small copy={int(form == 'inplace')}"], "D null / distinct / aliasing out; out == A",
             rows=301, K=K, C=Cc, form=form)
_add("rows_times_small", "small_ops", "rows_times_small refused K87 C89", [], "K C 8 > 60 KiB is refused",
     rows=10, K=87, C=89, form="plain", refused=True)
for dt in ("f32", "f64"):
    for n, R, r in ((1, 1, 1), (255, 7, 3), (257, 40, 16), (5000, 7, 16), (257, 1, 3), (255, 40, 1)):
        _add("lowrank", "small_ops", f"lowrank_accumulate {dt} n{n} R{R} r{r}", [], "a rank-r update of the cached tensor",
             dt=dt, n=n, R=R, r=r)
for n in (1, 255, 256, 257, 70000):
    _add("add_inplace", "small_ops", f"add_inplace n{n}", [], "one rounding per element", n=n)
for dt in ("f32", "f64", "bf16"):
    for rows, cols, batch in ((1, 1, 1), (31, 33, 3), (32, 32, 1), (33, 31, 3), (100, 1, 3), (1, 100, 1), (100, 33, 3)):
        _add("transpose", "small_ops", f"transpose {dt} {rows}x{cols}x{batch}", [], "exact, 64 x 64 tiles", dt=dt, rows=rows,
             cols=cols, batch=batch)
    _add("transpose", "small_ops", f"transpose2d {dt} 33x100", [], "the unbatched entry", dt=dt, rows=33, cols=100, batch=1,
         batched=False)

FAMILIES = sorted({c["family"] for c in CASES})

# Every tag family these launchers can log. eig.full.* also appear under eig.warm.direct / bootstrap,
# chol_qr2.blocks and orthonormalize under the projector route's wide bases.
EXPECTED_TAGS = sorted(
    ["unfold_gram.sym", "unfold_gram.syrk", "unfold_gram.mfma.f32", "unfold_gram.mfma.f64", "unfold_gram.valu.f32",
     "unfold_gram.valu.f64", "eig.full.lds_jacobi", "eig.full.onesided_jacobi", "eig.full.dsyevd", "eig.small",
     "eig.warm.direct", "eig.warm.frob_retry", "eig.warm.bootstrap", "eig.projector", "eig.cold.ritz",
     "eig.cold.subspace", "eig.cold.bisect", "eig.verify", "orthonormalize", "chol_qr2.blocks", "rows_times_small"])


def tag_family(tag):
    return tag.split(" ")[0]
