"""Op-level cases of the multi-start, constraint and diagnostic ops and their one checker
(tests/test_gpu_multistart_ops.py on the HIP kernels, tests/test_multistart_ops_hostsim.py on the host stand-in,
both through tests/opshim): cp_mode_update_ragged, gram_ragged, the three non-negative (HALS) updates, cp_hold_rows,
cp_pinv_ragged, core_score, factor_congruence, row_dots and fold_slice_sums. The buffers, the image checker and the
route check are those of tests/contraction_cases.py; St, within, sumsq_check, make_grams, check_system, check_gram and
check_solve those of tests/update_cases.py, whose case fields are used here too.

Per case: inputs from the case's seed ("pos" = uniform[0.5, 1), "mix" = uniform[-1, 1)), every input followed by
4 KiB of NaN, every output between two 4 KiB NaN guards with NaN in every leading-dimension gap; after the calls every
byte outside the results is unchanged. Every case runs TWICE on fresh buffers and the two sets of output images must be
equal bit for bit (fixed summation orders, no atomics). A case with `poison` = b runs a third time with start b's M, W
and Grams replaced by NaN: every byte that is not start b's must equal the clean run's.

References are numpy in long double; u = 2^-53. Every check feeds the reference with what the device itself wrote
upstream, so conditioning never enters unless stated. The bars:
* ragged update: S, S^-1, grad, W, gradsq and the Gram by update_cases.check_system / check_solve / check_gram, start by
  start with the start's own rank;
* HALS, one step at a time from the device's own output: for row x and column r, with the S the device wrote and w'
  the device's NEW row for q < r and the OLD row for q >= r,
      v_ref = w_old[x, r] + (M[x, r] - sum_q w'[q] S[q, r]) / S[r, r],   w_ref = max(1e-16, v_ref)
      bar   = (R + 3) u (|M| + sum_q |w'[q]| |S[q, r]|) / S[r, r] + 2u (|w_old[x, r]| + |v_ref|)
  (R products and sums, one subtraction, one division, one addition; the clamp is 1-Lipschitz). A column whose S[r, r]
  is not a positive finite number keeps its bits, a NaN v lands on the floor. grad against the pre-update row:
  (R + 3) u (|W_old| |S_dev| + |M|); S against the Hadamard product: N u (|H| + |lambda|). With S == nullptr the same
  check runs against the S of a second run of the same inputs that did ask for it, and W, grad, gradsq and the Gram of
  the two runs must be equal bit for bit (the kernel fills LDS and S_out from one register; measured equal on both
  back ends, profiles/multistart_ops_bars.md, so no ulp allowance is made);
* same bits: gram_ragged, cp_hold_rows and the non-negative finish kernels against Ops::gram of the same columns; the
  three non-negative forms against each other on W, grad, gradsq, S and the Gram for one start;
* cp_hold_rows: moves and zeros exact, gradsq n u relative over the kept entries, a start whose bit is clear untouched;
* cp_pinv_ragged: the start with W = [I; 0] shows the device's G^-1 itself: symmetric bit for bit,
  ||Ginv G - I||_F / ||I||_F < 1e-10 cond; its twin (same Grams) P against W Ginv_dev with (R + 1) u |W| |Ginv_dev|;
  every good block ||P G - W||_F <= 1e-10 cond ||W||_F; a bad block exactly zero and its flag 1;
* core_score: 100 (n + 2) u s_ref / R + u |cc_ref|, n = R^N; the superdiagonal core gives exactly 100;
* factor_congruence: Phi absolute fms_ref.bar_phi, the weights 8 N (s_max + 8) u relative (fms_ref.bar_fms);
* row_dots (R + 1) u sum |P||W|; fold_slice_sums count u sum |src|.
"""
import os
import re

import numpy as np

import contraction_cases as CC
import fms_ref
import opshim_util
import update_cases as UC
from contraction_cases import check_image, check_route
from update_cases import (LD, U, St, check_gram, check_solve, check_system, colmajor, gall_flat, make_grams, mat, midx,
                          sumsq_check, vals, within)

G = CC.GUARD
WORST = UC.WORST  # family -> largest err / bar seen (within() keeps it there)
FLOOR = 1e-16
F64 = np.dtype(np.float64)


# ------------------------------------------------------------------------------------------ helpers
def table(ranks):
    """(nstarts, col, sq) of a StartTable"""
    col = np.concatenate([[0], np.cumsum(ranks)])
    sq = np.concatenate([[0], np.cumsum(np.square(ranks))])
    return len(ranks), [int(x) for x in col], [int(x) for x in sq]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


class MSt(St):
    """St with typed outputs, outputs that may hold NaN / inf results, and the owner (start) of every element"""

    def __init__(self, sh, c, hip, log):
        St.__init__(self, sh, c, hip, log)
        self.types, self.nan_ok, self.owner = {}, set(), {}

    def inp_t(self, arr):
        b = CC._In(self.sh, np.ascontiguousarray(arr))
        self.keep.append(b)
        return b

    def out(self, name, n, res=None, idx=None, init=None, raw=False, t=np.float64, nan_ok=False, owner=None):
        with np.errstate(invalid="ignore"):  # (an integer output is initialised in full: no NaN is cast)
            o = CC._Out(self.sh, n, t, idx, init)
        self.keep.append(o)
        self.outs[name] = (o, np.arange(n) if res is None else np.asarray(res, dtype=np.int64), raw)
        self.types[name] = np.dtype(t)
        if nan_ok:
            self.nan_ok.add(name)
        if owner is not None:
            self.owner[name] = np.asarray(owner)
        return o

    def got(self, name):
        o, res, raw = self.outs[name]
        if raw:
            return St.got(self, name)
        what, t = f"{self.c['name']} {name}", self.types[name]
        if name not in self.nan_ok:
            return check_image(what, o.img, self.posts[name], t, res)
        pre, post = o.img, self.posts[name]
        a, b = pre[G:-G].view(t).copy(), post[G:-G].view(t).copy()
        got = b[res].copy()
        a[res] = 0
        b[res] = 0
        assert np.array_equal(pre[:G], post[:G]) and np.array_equal(pre[-G:], post[-G:]), f"{what}: a guard was written"
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{what}: a gap between result elements was written"
        return got


def within_nf(st, what, got, ref, bar):
    """within() where the reference may hold inf / NaN: there the result must be the same inf, or a NaN"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=LD)
    bar = np.broadcast_to(np.asarray(bar, dtype=LD), ref.shape)
    ok = np.isfinite(ref) & np.isfinite(bar)
    g, r = got[~ok], ref[~ok].astype(np.float64)
    same = (np.isnan(g) & np.isnan(r)) | (g == r)
    assert np.all(same), f"{st.c['name']} {what}: {int(np.sum(~same))} non-finite results differ from the reference"
    within(st, what, np.where(ok, got, 0.0), np.where(ok, ref, LD(0)), np.where(ok, bar, LD(1)))


def sumsq_nf(st, what, got, terms):
    t = np.asarray(terms, dtype=np.float64)
    if np.all(np.isfinite(t)):
        return sumsq_check(st, what, got, t)
    if np.any(np.isnan(t)):
        assert np.isnan(got), f"{st.c['name']} {what}: {got} where a term is NaN"
    else:
        assert got == np.inf, f"{st.c['name']} {what}: {got} where a term is inf"


def owners(n, blocks):
    """blocks: (start, indices) pairs -> the owner of every element of an output of n elements, -1 for nobody's"""
    own = np.full(n, -1, np.int64)
    for b, idx in blocks:
        own[np.asarray(idx, dtype=np.int64)] = b
    return own


def col_owner(rows, ld, col, extra=0):
    """the owner of every element of a rows x col[-1] matrix with leading dimension ld (+ extra columns behind it)"""
    C = col[-1]
    own = np.full(ld * (C + extra), -1, np.int64)
    for b in range(len(col) - 1):
        own[midx(rows, col[b + 1] - col[b], ld, col[b])] = b
    return own


def _hadamard(Gs, mode, lam):
    R = Gs[0].shape[0]
    H = np.ones((R, R), dtype=LD)
    with np.errstate(all="ignore"):
        for j, Gj in enumerate(Gs):
            if j != mode:
                H = H * Gj.astype(LD)
        return H + LD(lam) * np.eye(R, dtype=LD), np.abs(H)


def _systems(rng, c, ranks):
    """one system per start from make_grams; an indefinite start sets the launch's one lambda (-2), the others'
    first Gram is shifted so that they stay positive definite with cond <= 1e3 (update_cases._shift)"""
    N, mode, indef = c["N"], c["mode"], c.get("indef", ())
    sysb = [make_grams(rng, N, mode, R, c.get("lam", 0.0), b in indef) for b, R in enumerate(ranks)]
    lam = c.get("lam", 0.0)
    if indef:
        lam = -2.0
        sysb = [s if b in indef else UC._shift(s, lam) for b, s in enumerate(sysb)]
    return sysb, lam


def _gall(sysb, poison):
    blocks = []
    for b, s in enumerate(sysb):
        g = gall_flat(s[0])
        blocks.append(np.full(g.size, np.nan) if b == poison else g)
    return np.concatenate(blocks)


def _poison_cols(A, col, poison):
    if poison is not None:
        A = A.copy()
        A[:, col[poison]:col[poison + 1]] = np.nan
    return A


def _gram_blocks(N, mode, ranks, sq):
    return [(b, N * sq[b] + mode * R * R + np.arange(R * R)) for b, R in enumerate(ranks)]


# ------------------------------------------------------------------------------------------ cp_mode_update_ragged
def ragged_route(rows, ranks):
    """the launcher's one decision per launch, made with the largest rank (hip_ops.hip)"""
    R = max(ranks)
    if R > 64:
        return "loop"
    if UC.staged(rows, R):
        return "staged"
    return "loop" if rows * R > 6144 else "unstaged"


def op_ragged(st, poison=None):
    c, sh, rng = st.c, st.sh, st.rng
    N, mode, ranks, rows, null = c["N"], c["mode"], c["ranks"], c["rows"], c.get("null", False)
    K, col, sq = table(ranks)
    C, SQ = col[K], sq[K]
    ldm, ldw, ldg = rows + c.get("xm", 0), rows + c.get("xw", 0), rows + c.get("xg", 0)
    sysb, lam = _systems(rng, c, ranks)
    M, W0 = vals(rng, c["cls"], (rows, C)), vals(rng, c["cls"], (rows, C))
    gflat = _gall(sysb, poison)
    Mp, Wp = _poison_cols(M, col, poison), _poison_cols(W0, col, poison)
    keepi = np.flatnonzero(~np.isnan(gflat))
    gb = _gram_blocks(N, mode, ranks, sq)
    g = st.out("G", N * SQ + 7, res=np.concatenate([i for _, i in gb]), idx=keepi, init=gflat[keepi],
               owner=owners(N * SQ + 7, [(b, N * sq[b] + np.arange(N * R * R)) for b, R in enumerate(ranks)]))
    m = st.inp(colmajor(Mp, ldm))
    iw = midx(rows, C, ldw)
    w = st.out("W", ldw * (C + 1), res=iw, idx=iw, init=Wp.reshape(-1, order="F"), nan_ok=poison is not None,
               owner=col_owner(rows, ldw, col, 1))
    gr = st.out("grad", ldg * (C + 1), res=midx(rows, C, ldg), owner=col_owner(rows, ldg, col, 1))
    gq = st.out("gradsq", K + 1, res=np.arange(K), owner=owners(K + 1, [(b, [b]) for b in range(K)]))
    S = Si = 0
    if not null:
        so = owners(SQ + 5, [(b, sq[b] + np.arange(R * R)) for b, R in enumerate(ranks)])
        S = st.out("S", SQ + 5, res=np.arange(SQ), owner=so).ptr
        Si = st.out("Sinv", SQ + 5, res=np.arange(SQ), owner=so).ptr
    sh.cp_mode_update_ragged(g.ptr, N, mode, (K, col, sq), lam, m.ptr, ldm, w.ptr, ldw, gr.ptr, ldg, rows, gq.ptr, S, Si)
    st.finish()

    def verify():
        gpost = st.posts["G"][G:-G].view(np.float64)
        st.got("G")
        Wd, gd, gqd = mat(st.got("W"), rows, C), mat(st.got("grad"), rows, C), st.got("gradsq")
        for b, R in enumerate(ranks):
            _, _, S_ref, absH, cond = sysb[b]
            cs, what = slice(col[b], col[b + 1]), f"[{b}] "
            if null:
                check_solve(st, what, c, M[:, cs], W0[:, cs], S_ref, None, gd[:, cs], None, None, None, gqd[b], True,
                            extra=N)
                want = M[:, cs] @ np.linalg.inv(S_ref.astype(np.float64))
                fro = np.linalg.norm(Wd[:, cs] - want) / np.linalg.norm(want)
                assert fro < 1e-10 * cond, f"{c['name']} {what}W: {fro:.3e} over 1e-10 * cond {cond:.3g}"
            else:
                Sd = mat(st.got("S")[sq[b]:sq[b + 1]], R, R)
                Sid = mat(st.got("Sinv")[sq[b]:sq[b + 1]], R, R)
                check_system(st, what, Sd, Sid, S_ref, absH, lam, N, cond)
                check_solve(st, what, c, M[:, cs], W0[:, cs], Sd, Sid, gd[:, cs], Wd[:, cs], None, None, gqd[b], False)
            check_gram(st, what + "G", mat(gpost[gb[b][1]], R, R), Wd[:, cs], rows)
    st.verify = verify


# ------------------------------------------------------------------------------------------ the HALS updates
def _nn_systems(rng, c, ranks):
    """make_grams systems; `zero_diag` / `inf_diag` = (start, r0): that entry of one OTHER mode's Gram becomes 0 / inf,
    so S[r0, r0] is 0 (lambda 0) / inf"""
    N, mode, lam = c["N"], c["mode"], c.get("lam", 0.0)
    out = []
    for b, R in enumerate(ranks):
        Gs, _, S_ref, absH, _ = make_grams(rng, N, mode, R, lam, False)
        for key, v in (("zero_diag", 0.0), ("inf_diag", np.inf)):
            if key in c and c[key][0] == b:
                r0 = c[key][1]
                Gs[next(j for j in range(N) if j != mode)][r0, r0] = v
                S_ref, absH = _hadamard(Gs, mode, lam)
        out.append((Gs, lam, S_ref, absH, None))
    return out, lam


def check_hals(st, what, M, Wold, Wnew, Sd):
    """the one-step reference of the module docstring, column by column, from the device's own row"""
    R = Sd.shape[0]
    Ml, absS = M.astype(LD), np.abs(Sd).astype(LD)
    gots, refs, bars = [], [], []
    with np.errstate(all="ignore"):
        for r in range(R):
            d = Sd[r, r]
            if not (d > 0.0 and np.isfinite(d)):
                assert same_bits(Wnew[:, r], Wold[:, r]), f"{st.c['name']} {what}: column {r} (S[r,r] = {d}) was changed"
                continue
            wp = np.concatenate([Wnew[:, :r], Wold[:, r:]], axis=1).astype(LD)
            v = Wold[:, r].astype(LD) + (Ml[:, r] - wp @ Sd[:, r].astype(LD)) / LD(d)
            bar = (R + 3) * U * (np.abs(Ml[:, r]) + np.abs(wp) @ absS[:, r]) / LD(d) + \
                2 * U * (np.abs(Wold[:, r]) + np.abs(v))
            nanv = np.isnan(v)
            assert np.all(Wnew[nanv, r] == FLOOR), f"{st.c['name']} {what}: a NaN step of column {r} is not on the floor"
            gots.append(Wnew[~nanv, r])
            refs.append(np.where(v > FLOOR, v, LD(FLOOR))[~nanv])
            bars.append(bar[~nanv])
    if gots:
        within(st, what + "W", np.concatenate(gots), np.concatenate(refs), np.concatenate(bars))


def nn_route(c):
    form, rows, ranks = c["form"], c["rows"], c["ranks"]
    if rows == 0:
        return []
    tiles = (rows + 63) // 64
    one = [rf"update_nn R={ranks[0]} tiles={tiles}"]
    bat = [rf"update_nn_batched R={ranks[0]} tiles={tiles} starts={len(ranks)}"]
    rag = [rf"update_nn_ragged rmax={max(ranks)} tiles={tiles} starts={len(ranks)}"]
    return {"single": one, "batched": bat, "ragged": rag, "forms": one + bat + rag}[form]


def op_nn(st, poison=None):
    c, sh, rng = st.c, st.sh, st.rng
    form, N, mode, ranks, rows = c["form"], c["N"], c["mode"], c["ranks"], c["rows"]
    K, col, sq = table(ranks)
    C, SQ = col[K], sq[K]
    ldm, ldw, ldg = rows + c.get("xm", 0), rows + c.get("xw", 0), rows + c.get("xg", 0)
    sysb, lam = _nn_systems(rng, c, ranks)
    M, W0 = vals(rng, c["cls"], (rows, C)), vals(rng, "pos", (rows, C))
    if "nan_row" in c:
        M[c["nan_row"], :] = np.nan
    odd = any(k in c for k in ("nan_row", "inf_diag")) or poison is not None
    gflat = _gall(sysb, poison)
    Mp, Wp = _poison_cols(M, col, poison), _poison_cols(W0, col, poison)
    keepi = np.flatnonzero(~np.isnan(gflat))
    gb = _gram_blocks(N, mode, ranks, sq)
    iw = midx(rows, C, ldw)

    def launch(tag, frm, with_S):
        o = {}
        o["G"] = st.out(tag + "G", N * SQ + 7, res=np.concatenate([i for _, i in gb]), idx=keepi, init=gflat[keepi],
                        owner=owners(N * SQ + 7, [(b, N * sq[b] + np.arange(N * R * R)) for b, R in enumerate(ranks)]))
        m = st.inp(colmajor(Mp, ldm))
        o["W"] = st.out(tag + "W", ldw * (C + 1), res=iw, idx=iw, init=Wp.reshape(-1, order="F"), nan_ok=odd,
                        owner=col_owner(rows, ldw, col, 1))
        o["grad"] = st.out(tag + "grad", ldg * (C + 1), res=midx(rows, C, ldg), nan_ok=odd,
                           owner=col_owner(rows, ldg, col, 1))
        o["gradsq"] = st.out(tag + "gradsq", K + 1, res=np.arange(K), nan_ok=odd,
                             owner=owners(K + 1, [(b, [b]) for b in range(K)]))
        S = 0
        if with_S:
            o["S"] = st.out(tag + "S", SQ + 5, res=np.arange(SQ), nan_ok=odd,
                            owner=owners(SQ + 5, [(b, sq[b] + np.arange(R * R)) for b, R in enumerate(ranks)]))
            S = o["S"].ptr
        args = (lam, m.ptr, ldm, o["W"].ptr, ldw, o["grad"].ptr, ldg, rows, o["gradsq"].ptr, S)
        if frm == "single":
            sh.cp_mode_update_nn(o["G"].ptr, N, mode, ranks[0], *args)
        elif frm == "batched":
            sh.cp_mode_update_nn_batched(o["G"].ptr, N, mode, ranks[0], K, *args)
        else:
            sh.cp_mode_update_nn_ragged(o["G"].ptr, N, mode, (K, col, sq), *args)
        # Ops::gram of the columns the update left: the finish kernels promise its bits
        o["Gop"] = st.out(tag + "Gop", SQ + 5, res=np.arange(SQ), nan_ok=odd,
                          owner=owners(SQ + 5, [(b, sq[b] + np.arange(R * R)) for b, R in enumerate(ranks)]))
        for b, R in enumerate(ranks):
            sh.gram(o["W"].ptr + 8 * col[b] * ldw, rows, ldw, R, o["Gop"].ptr + 8 * sq[b])
        return o

    assert form in ("single", "batched", "ragged", "forms") and (form in ("ragged",) or len(set(ranks)) == 1)
    assert form not in ("single", "forms") or K == 1
    has_S = rows > 0  # (an update of no rows returns before S is formed: the op then gets S == nullptr)
    tags = {"single": [("", "single")], "batched": [("", "batched")], "ragged": [("", "ragged")],
            "forms": [("", "single"), ("batched.", "batched"), ("ragged.", "ragged")]}[form]
    for tag, frm in tags:
        launch(tag, frm, has_S)
    if c.get("null"):
        launch("null.", tags[0][1], False)
    st.finish()

    def verify():
        gpost = st.posts["G"][G:-G].view(np.float64)
        Wd, gd, gqd = mat(st.got("W"), rows, C), mat(st.got("grad"), rows, C), st.got("gradsq")
        Gop = st.got("Gop")
        Sall = st.got("S") if has_S else None
        for b, R in enumerate(ranks):
            _, _, S_ref, absH, _ = sysb[b]
            cs, what = slice(col[b], col[b + 1]), f"[{b}] "
            Gm = mat(gpost[gb[b][1]], R, R)
            if rows == 0:
                assert gqd[b] == 0.0 and not np.any(Gm), f"{c['name']} {what}: no rows, but gradsq {gqd[b]}"
                assert same_bits(Gm, mat(Gop[sq[b]:sq[b + 1]], R, R)), f"{c['name']} {what}G: not the bits of Ops::gram"
                continue
            Sd = mat(Sall[sq[b]:sq[b + 1]], R, R)
            within_nf(st, what + "S", Sd, S_ref, N * U * (absH + abs(lam) * np.eye(R)))
            with np.errstate(all="ignore"):
                gref = W0[:, cs].astype(LD) @ Sd.astype(LD) - M[:, cs].astype(LD)
                gbar = (R + 3) * U * (np.abs(W0[:, cs]).astype(LD) @ np.abs(Sd).astype(LD) + np.abs(M[:, cs]))
            within_nf(st, what + "grad", gd[:, cs], gref, gbar)
            sumsq_nf(st, what + "gradsq", gqd[b], gd[:, cs])
            check_hals(st, what, M[:, cs], W0[:, cs], Wd[:, cs], Sd)
            if c.get("expect_floor"):
                assert np.any(Wd[:, cs] == FLOOR), f"{c['name']} {what}: no entry on the floor"
            if "nan_row" in c:
                assert np.all(Wd[c["nan_row"], cs] == FLOOR), f"{c['name']} {what}: the NaN row is not on the floor"
            check_gram(st, what + "G", Gm, Wd[:, cs], rows)
            assert same_bits(Gm, mat(Gop[sq[b]:sq[b + 1]], R, R)), f"{c['name']} {what}G: not the bits of Ops::gram"
        others = [t for t, _ in tags[1:]] + (["null."] if c.get("null") else [])
        for t in others:  # the same bits from every form, and with S == nullptr
            for k in ("W", "grad", "gradsq", "G", "Gop") + (("S",) if t != "null." and has_S else ()):
                assert np.array_equal(st.posts[k], st.posts[t + k]), f"{c['name']}: {t}{k} differs from {k} in bits"
    st.verify = verify


# ------------------------------------------------------------------------------------------ gram_ragged
def op_gram_ragged(st, poison=None):
    c, sh, rng = st.c, st.sh, st.rng
    N, mode, ranks, rows = c["N"], c["mode"], c["ranks"], c["rows"]
    K, col, sq = table(ranks)
    C, SQ, ld = col[K], sq[K], rows + c.get("xld", 0)
    W = vals(rng, c["cls"], (rows, C))
    w = st.inp(colmajor(_poison_cols(W, col, poison), ld))
    gb = _gram_blocks(N, mode, ranks, sq)
    odd = poison is not None
    g = st.out("G", N * SQ + 7, res=np.concatenate([i for _, i in gb]), owner=owners(N * SQ + 7, gb), nan_ok=odd)
    sh.gram_ragged(w.ptr, rows, ld, (K, col, sq), N, mode, g.ptr)
    gop = st.out("Gop", SQ + 5, res=np.arange(SQ), nan_ok=odd,
                 owner=owners(SQ + 5, [(b, sq[b] + np.arange(R * R)) for b, R in enumerate(ranks)]))
    for b, R in enumerate(ranks):
        sh.gram(w.ptr + 8 * col[b] * ld, rows, ld, R, gop.ptr + 8 * sq[b])
    st.finish()

    def verify():
        st.got("G")
        gpost, Gop = st.posts["G"][G:-G].view(np.float64), st.got("Gop")
        for b, R in enumerate(ranks):
            Gm = mat(gpost[gb[b][1]], R, R)
            check_gram(st, f"[{b}] G", Gm, W[:, col[b]:col[b + 1]], rows)
            assert same_bits(Gm, mat(Gop[sq[b]:sq[b + 1]], R, R)), f"{c['name']} [{b}]: not the bits of Ops::gram"
    st.verify = verify


# ------------------------------------------------------------------------------------------ cp_hold_rows
def keep_table(rng, kind, rows):
    k = np.ones(rows, np.uint8)
    if kind == "none":
        k[:] = 0
    elif kind == "edges":
        k[[x for x in (0, 63, 64, rows - 1) if 0 <= x < rows]] = 0
    elif kind == "random":
        k[rng.random(rows) < 0.3] = 0
    else:
        assert kind == "all", kind
    return k


def hold_mask(K, holds):
    return holds & ((1 << K) - 1) if K < 32 else holds & 0xFFFFFFFF


def op_hold(st, poison=None):
    c, sh, rng = st.c, st.sh, st.rng
    N, mode, ranks, rows, holds = c["N"], c["mode"], c["ranks"], c["rows"], c["holds"]
    K, col, sq = table(ranks)
    C, SQ = col[K], sq[K]
    ldw, ldg, lds = rows + c.get("xw", 0), rows + c.get("xg", 0), rows + c.get("xs", 0)
    kinds = c["keep"] if isinstance(c["keep"], list) else [c["keep"]] * K
    keep = np.stack([keep_table(rng, kinds[b % len(kinds)], rows) for b in range(K)])
    W0, g0, s0 = vals(rng, c["cls"], (rows, C)), vals(rng, c["cls"], (rows, C)), vals(rng, "mix", (rows, C))
    G0, q0 = vals(rng, "mix", N * SQ + 7), vals(rng, "mix", K + 1)
    on = [b for b in range(K) if (hold_mask(K, holds) >> b) & 1]
    odd = poison is not None
    if odd:
        W0, g0 = _poison_cols(W0, col, poison), _poison_cols(g0, col, poison)

    def colres(ld):
        return np.concatenate([midx(rows, ranks[b], ld, col[b]) for b in on]) if on else []

    def io(name, A, ld):
        i = midx(rows, C, ld)
        return st.out(name, ld * (C + 1), res=colres(ld), idx=i, init=A.reshape(-1, order="F"), nan_ok=odd,
                      owner=col_owner(rows, ld, col, 1))

    w, gr, sc = io("W", W0, ldw), io("grad", g0, ldg), io("scores", s0, lds)
    gb = _gram_blocks(N, mode, ranks, sq)
    g = st.out("G", N * SQ + 7, res=np.concatenate([gb[b][1] for b in on]) if on else [], idx=np.arange(N * SQ + 7),
               init=G0, nan_ok=odd, owner=owners(N * SQ + 7, gb))
    gq = st.out("gradsq", K + 1, res=on, idx=np.arange(K + 1), init=q0, nan_ok=odd,
                owner=owners(K + 1, [(b, [b]) for b in range(K)]))
    kp = st.inp_t(keep.reshape(-1))
    sh.cp_hold_rows(w.ptr, ldw, gr.ptr, ldg, sc.ptr, lds, rows, (K, col, sq), kp.ptr, holds, g.ptr, N, mode, gq.ptr)
    gop = st.out("Gop", SQ + 5, res=np.concatenate([sq[b] + np.arange(ranks[b] ** 2) for b in on]) if on else [],
                 nan_ok=odd, owner=owners(SQ + 5, [(b, sq[b] + np.arange(R * R)) for b, R in enumerate(ranks)]))
    for b in on:
        sh.gram(w.ptr + 8 * col[b] * ldw, rows, ldw, ranks[b], gop.ptr + 8 * sq[b])
    st.finish()

    def verify():
        for k in ("W", "grad", "scores", "G", "gradsq", "Gop"):
            st.got(k)  # guards, gaps and every start whose bit is clear: untouched
        body = {k: st.posts[k][G:-G].view(np.float64) for k in ("W", "grad", "scores", "G", "gradsq", "Gop")}
        for b in on:
            R, kb = ranks[b], keep[b].astype(bool)[:, None]
            cs, what = slice(col[b], col[b + 1]), f"{c['name']} [{b}]"
            Wn = mat(body["W"][midx(rows, R, ldw, col[b])], rows, R)
            gn = mat(body["grad"][midx(rows, R, ldg, col[b])], rows, R)
            sn = mat(body["scores"][midx(rows, R, lds, col[b])], rows, R)
            assert same_bits(Wn, np.where(kb, W0[:, cs], 0.0)), f"{what}: W is not the kept rows and exact zeros"
            assert same_bits(gn, np.where(kb, g0[:, cs], 0.0)), f"{what}: grad is not the kept rows and exact zeros"
            assert same_bits(sn, np.where(kb, 0.0, W0[:, cs])), f"{what}: scores are not the held-out rows of W"
            kept = g0[:, cs][keep[b].astype(bool)]
            if kept.size:
                sumsq_check(st, f"[{b}] gradsq", body["gradsq"][b], kept)
            else:
                assert body["gradsq"][b] == 0.0, f"{what}: gradsq {body['gradsq'][b]} with every row held out"
            Gm = mat(body["G"][gb[b][1]], R, R)
            check_gram(st, f"[{b}] G", Gm, Wn, rows)
            assert kept.size or not np.any(Gm), f"{what}: a Gram of zeros is not zero"
            assert same_bits(Gm, mat(body["Gop"][sq[b]:sq[b + 1]], R, R)), f"{what}: not the bits of Ops::gram"
    st.verify = verify


# ------------------------------------------------------------------------------------------ cp_pinv_ragged
def _spd(rng, R):
    Q, _ = np.linalg.qr(rng.standard_normal((R, R)))
    A = (Q * (np.logspace(0.0, 2.0, R) if R > 1 else np.array([1.5]))) @ Q.T
    A = 0.5 * (A + A.T)
    assert np.linalg.cond(A) <= 1e3
    return A


def _bad_gram(A, kind):
    R = A.shape[0]
    A = A.copy()
    if kind == "zero":  # a zero first pivot
        A[0, 0] = 0.0
    elif kind == "ones2":  # the second pivot is an exact 0 after one sweep
        assert R == 2
        A[:] = 1.0
    elif kind == "neg2":  # a negative second pivot
        assert R == 2
        A[:] = [[1.0, 2.0], [2.0, 1.0]]
    elif kind == "nan":  # (the last pivot)
        A[R - 1, R - 1] = np.nan
    else:
        assert kind == "inf", kind
        A[0, 0] = np.inf
    return A


def op_pinv(st, poison=None):
    c, sh, rng = st.c, st.sh, st.rng
    rows, ranks = c["rows"], c["ranks"]
    N = len(rows)
    K, col, sq = table(ranks)
    C, SQ = col[K], sq[K]
    twin, bad, preset = c.get("twin"), c.get("bad", {}), c.get("preset", {})
    Gs = [[_spd(rng, R) for _ in range(N)] for R in ranks]
    Ws = [vals(rng, c["cls"], (rows[i], C)) for i in range(N)]
    if twin:
        ia, ib = twin
        assert ranks[ia] == ranks[ib] and ia not in bad and ib not in bad
        Gs[ib] = [A.copy() for A in Gs[ia]]
        for i in range(N):
            if rows[i] >= ranks[ia]:
                Ws[i][:, col[ia]:col[ia + 1]] = np.eye(rows[i], ranks[ia])
    is_bad = np.zeros((K, N), bool)
    for b, (kind, modes) in bad.items():
        for i in (range(N) if modes is None else modes):
            Gs[b][i] = _bad_gram(Gs[b][i], kind)
            is_bad[b, i] = True
    gflat = np.concatenate([np.full(N * R * R, np.nan) if b == poison else np.concatenate([A.reshape(-1, order="F") for A in Gs[b]])
                            for b, R in enumerate(ranks)])
    g = st.inp(gflat)
    win = [st.inp(_poison_cols(Ws[i], col, poison).reshape(-1, order="F")) for i in range(N)]
    pout = [st.out(f"P{i}", rows[i] * C, owner=col_owner(rows[i], rows[i], col)) for i in range(N)]
    flags0 = np.zeros(K + 1, np.int32)
    for b, v in preset.items():
        flags0[b] = v
    fl = st.out("bad", K + 1, res=np.arange(K), idx=np.arange(K + 1), init=flags0, t=np.int32,
                owner=owners(K + 1, [(b, [b]) for b in range(K)]))
    sh.cp_pinv_ragged(g.ptr, N, (K, col, sq), [x.ptr for x in win], rows, [x.ptr for x in pout], fl.ptr)
    st.finish()

    def verify():
        flags = st.got("bad")
        want = [1 if (is_bad[b].any() or preset.get(b)) else 0 for b in range(K)]
        assert list(flags.astype(int)) == want, f"{c['name']}: flags {list(flags.astype(int))}, expected {want}"
        worst = [0.0, 0.0]  # the two normwise residuals in units of cond (the bar: 1e-10)
        for i in range(N):
            P = mat(st.got(f"P{i}"), rows[i], C)
            ginv = None
            for b in ([twin[0]] if twin else []) + [b for b in range(K) if not twin or b != twin[0]]:
                R, cs, what = ranks[b], slice(col[b], col[b + 1]), f"{c['name']} [{b}] mode {i}"
                Pb, Wb, A = P[:, cs], Ws[i][:, cs], Gs[b][i]
                if is_bad[b, i]:
                    assert not np.any(bits(Pb)), f"{what}: the block of a bad start is not exactly zero"
                    continue
                cond = np.linalg.cond(A)
                res = np.linalg.norm(Pb @ A - Wb)
                assert res <= 1e-10 * cond * np.linalg.norm(Wb), f"{what}: ||P G - W|| {res:.3e}, cond {cond:.3g}"
                worst[0] = max(worst[0], res / (cond * np.linalg.norm(Wb)))
                if not twin or rows[i] < R or b not in twin:
                    continue
                if b == twin[0]:
                    ginv = Pb[:R]
                    assert not np.any(bits(Pb[R:])), f"{what}: rows of zeros times G^-1 are not exactly zero"
                    assert same_bits(ginv, ginv.T), f"{what}: G^-1 is not symmetric bit for bit"
                    r = np.linalg.norm(ginv @ A - np.eye(R)) / np.sqrt(R)
                    assert r < 1e-10 * cond, f"{what}: ||Ginv G - I|| / ||I|| {r:.3e} over 1e-10 cond {cond:.3g}"
                    worst[1] = max(worst[1], r / cond)
                else:
                    within(st, f"[{b}] P{i}", Pb, Wb.astype(LD) @ ginv.astype(LD),
                           (R + 1) * U * (np.abs(Wb).astype(LD) @ np.abs(ginv).astype(LD)))
        if st.log is not None:
            st.log.append(f"{c['name']} normwise: ||P G - W|| / (cond ||W||) {worst[0]:.3g}, "
                          f"||Ginv G - I|| / (cond ||I||) {worst[1]:.3g}, bar 1e-10")
    st.verify = verify


def pinv_route(rows, ranks):
    return rf"pinv_ragged starts={len(ranks)} rmax={max(ranks)} tiles={min((max(rows) + 255) // 256, 1024)}"


# ------------------------------------------------------------------------------------------ core_score
def op_core(st, poison=None):
    c, sh, rng = st.c, st.sh, st.rng
    R, N, kind = c["R"], c["N"], c["kind"]
    n, dstride = R ** N, sum(R ** i for i in range(N))
    T = np.zeros(n)
    T[::dstride] = 1.0
    assert T.sum() == R
    if kind in ("random", "bad"):
        core = vals(rng, c["cls"], n)
    else:
        core = T.copy()
        if kind == "diag+1":
            assert n > 1 and 1 % dstride
            core[1] = 1.0
    isbad = kind == "bad"
    co = st.out("core", n, res=np.arange(n) if isbad else [], idx=np.arange(n), init=core, nan_ok=True)
    flag = st.inp_t(np.array([3 if isbad else 0], np.int32))
    cc = st.out("cc", 1, nan_ok=True)
    sh.core_score(co.ptr, R, N, flag.ptr, cc.ptr)
    st.finish()

    def verify():
        got, after = st.got("cc")[0], st.got("core")
        if isbad:
            assert np.isnan(got) and np.all(np.isnan(after)), f"{c['name']}: a bad start's core and score are not NaN"
        elif kind == "diag":
            assert got == 100.0, got
        elif kind == "diag+1":
            assert got == 100.0 * (1.0 - 1.0 / R), got
        else:
            s = np.sum((core.astype(LD) - T) ** 2)
            ref = 100 * (1 - s / R)
            within(st, "cc", np.array([got]), np.array([ref]), np.array([100 * (n + 2) * U * s / R + U * abs(ref)]))
    st.verify = verify


# ------------------------------------------------------------------------------------------ factor_congruence
def fms_slabs(rows_a, rows_b):
    """the workgroups of k_fms_cross: chunks of 32 rows, at most 32 slabs a mode (hip_ops.hip: fms_args)"""
    at = 0
    for ra, rb in zip(rows_a, rows_b):
        chunks = (max(ra, rb) + 31) // 32
        cps = (chunks + 31) // 32
        at += (chunks + cps - 1) // cps
    return at


def fms_reference(A, B, mask):
    """(Phi, wa, wb, bad_a, bad_b) in long double"""
    Ca, Cb = A[0].shape[1], B[0].shape[1]
    phi, wa, wb = np.ones((Ca, Cb), dtype=LD), np.ones(Ca, dtype=LD), np.ones(Cb, dtype=LD)
    bad_a, bad_b = np.zeros(Ca, bool), np.zeros(Cb, bool)
    with np.errstate(all="ignore"):
        for i in range(len(A)):
            a, b = A[i].astype(LD), B[i].astype(LD)
            na, nb = np.sqrt(np.sum(a * a, axis=0)), np.sqrt(np.sum(b * b, axis=0))
            wa, wb = wa * na, wb * nb
            if not (mask >> i) & 1:
                continue
            bad_a |= ~((na > 0) & np.isfinite(na))
            bad_b |= ~((nb > 0) & np.isfinite(nb))
            phi = phi * ((a.T @ b) / na[:, None] / nb[None, :])
    phi[bad_a, :] = 0
    phi[:, bad_b] = 0
    return phi, wa, wb, bad_a, bad_b


def op_fms(st, poison=None):
    c, sh, rng = st.c, st.sh, st.rng
    ra, rb, Ca, Cb, mask = c["rows_a"], c["rows_b"], c["Ca"], c["Cb"], c["mask"]
    N = len(ra)
    lda, ldb = [r + c.get("xa", 0) for r in ra], [r + c.get("xb", 0) for r in rb]
    A = [vals(rng, c["cls"], (ra[i], Ca)) for i in range(N)]
    B = [vals(rng, c["cls"], (rb[i], Cb)) for i in range(N)]
    pair, special = c.get("pair"), c.get("special")
    if pair:
        assert Ca == Cb and ra == rb
        B = [a.copy() for a in A]
        ldb = lda
    i0 = next(i for i in range(N) if (mask >> i) & 1)
    As, Bs = [a.copy() for a in A], [b.copy() for b in B]
    for side, cc_, kind in special or []:
        X = (As if side == "a" else Bs)[i0]
        if kind == "zero":
            X[:, cc_] = 0.0
        else:
            X[X.shape[0] // 2, cc_] = np.inf if kind == "inf" else np.nan

    def launch(tag, Af, Bf, shared):
        a = [st.inp(colmajor(Af[i], lda[i])) for i in range(N)]
        b = a if shared else [st.inp(colmajor(Bf[i], ldb[i])) for i in range(N)]
        sa, sb = ([x.ptr for x in a], lda, ra, Ca), ([x.ptr for x in b], ldb, rb, Cb)
        nbytes = sh.factor_congruence_work(N, sa, sb)
        work = st.out(tag + "work", (nbytes + 7) // 8, raw=True).ptr if nbytes else 0
        phi = st.out(tag + "Phi", Ca * Cb)
        wa, wb = st.out(tag + "wa", Ca, nan_ok=True), st.out(tag + "wb", Cb, nan_ok=True)
        sh.factor_congruence(N, sa, sb, mask, work, phi.ptr, wa.ptr, wb.ptr)

    if special:
        launch("clean.", A, B, False)
    launch("", As, Bs, pair is not None)
    if pair:
        launch("apart.", As, Bs, False)
    st.finish()

    def verify():
        phi, wa, wb = mat(st.got("Phi"), Ca, Cb), st.got("wa"), st.got("wb")
        ref, wa_ref, wb_ref, bad_a, bad_b = fms_reference(As, Bs, mask)
        lens = [max(ra[i], rb[i]) for i in range(N) if (mask >> i) & 1]
        assert not np.any(bits(phi[bad_a, :])) and not np.any(bits(phi[:, bad_b])), \
            f"{c['name']}: Phi of a column without a norm is not exactly zero"
        within(st, "Phi", phi, ref, np.full(ref.shape, fms_ref.bar_phi(lens)))
        with np.errstate(all="ignore"):
            within_nf(st, "wa", wa, wa_ref, 8.0 * N * (max(ra) + 8.0) * U * np.abs(wa_ref))
            within_nf(st, "wb", wb, wb_ref, 8.0 * N * (max(rb) + 8.0) * U * np.abs(wb_ref))
        if special:  # nothing else changes: every other entry has the clean run's bits
            pc, ac, bc = mat(st.got("clean.Phi"), Ca, Cb), st.got("clean.wa"), st.got("clean.wb")
            ka, kb = np.ones(Ca, bool), np.ones(Cb, bool)
            for side, cc_, _ in special:
                (ka if side == "a" else kb)[cc_] = False
            assert same_bits(phi[ka][:, kb], pc[ka][:, kb]) and same_bits(wa[ka], ac[ka]) and \
                same_bits(wb[kb], bc[kb]), f"{c['name']}: a special column changed entries of other columns"
        if pair:
            for k in ("Phi", "wa", "wb"):
                assert np.array_equal(st.posts[k], st.posts["apart." + k]), \
                    f"{c['name']} {k}: one side given twice and two equal buffers differ in bits"
    st.verify = verify


def fms_route(c):
    pats = []
    n = fms_slabs(c["rows_a"], c["rows_b"])
    if c.get("special") or c.get("pair"):
        pats.append(rf"fms\.cross slabs={n} ca={c['Ca']} cb={c['Cb']} same=0")
    if not c.get("special"):
        pats.append(rf"fms\.cross slabs={n} ca={c['Ca']} cb={c['Cb']} same={1 if c.get('pair') else 0}")
    return pats


# ------------------------------------------------------------------------------------------ row_dots, fold_slice_sums
def op_row_dots(st, poison=None):
    c, sh, rng = st.c, st.sh, st.rng
    rows, R, ld = c["rows"], c["R"], c["rows"] + c.get("xld", 0)
    P, W = vals(rng, c["cls"], (rows, R)), vals(rng, c["cls"], (rows, R))
    p, w, o = st.inp(colmajor(P, ld)), st.inp(colmajor(W, ld)), st.out("out", rows)
    sh.row_dots(p.ptr, w.ptr, rows, R, ld, o.ptr)
    st.finish()
    st.verify = lambda: within(st, "out", st.got("out"), np.sum(P.astype(LD) * W, axis=1),
                               (R + 1) * U * np.sum(np.abs(P) * np.abs(W), axis=1))


def op_fold(st, poison=None):
    c, sh, rng = st.c, st.sh, st.rng
    lens = list(c["lens"])
    total = int(np.prod(lens))
    src = vals(rng, c["cls"], total)
    s, o = st.inp(src), st.out("out", sum(lens))
    sh.fold_slice_sums(s.ptr, lens, o.ptr)
    st.finish()

    def verify():
        X = src.reshape(lens, order="F").astype(LD)  # (the first listed mode fastest)
        ref, bar = [], []
        for j in range(len(lens)):
            ax = tuple(k for k in range(len(lens)) if k != j)
            ref.append(np.sum(X, axis=ax))
            bar.append((total // lens[j]) * U * np.sum(np.abs(X), axis=ax))
        within(st, "out", st.got("out"), np.concatenate(ref), np.concatenate(bar))
    st.verify = verify


# ------------------------------------------------------------------------------------------ refusals
def op_refuse(st, poison=None):
    """a call the launcher must refuse: the ShimError named by `raises`, every buffer untouched, and the Shim usable
    afterwards (a row_dots). On the host stand-in only the refusals of the shared defaults in ops.h are made
    (`host`): the others are checks of the HIP launchers, and the stand-in would walk the malformed arguments."""
    c, sh, rng = st.c, st.sh, st.rng
    what, t = c["what"], c.get("table")

    def d(name, n=256):
        return st.out(name, n, res=[], idx=np.arange(n), init=vals(rng, "mix", n)).ptr

    def side(n, cols, rows, ld, N=2):
        return ([d(f"{n}{i}") for i in range(N)], [ld] * N, [rows] * N, cols)

    calls = {
        "ragged": lambda: sh.cp_mode_update_ragged(d("G"), 3, 0, t, 0.0, d("M"), 4, d("W"), 4, d("g"), 4, 4, d("q"),
                                                   d("S"), d("Si")),
        "gram_ragged": lambda: sh.gram_ragged(d("W"), 4, 4, t, 3, 0, d("G")),
        "nn_ragged": lambda: sh.cp_mode_update_nn_ragged(d("G", 3 * 65 * 65), 3, 0, t, 0.0, d("M", 520), 4, d("W", 520),
                                                         4, d("g", 520), 4, 4, d("q"), d("S", 65 * 65)),
        "nn_single": lambda: sh.cp_mode_update_nn(d("G", 3 * 65 * 65), 3, 0, 65, 0.0, d("M", 520), 4, d("W", 520), 4,
                                                  d("g", 520), 4, 4, d("q"), d("S", 65 * 65)),
        "nn_batched": lambda: sh.cp_mode_update_nn_batched(d("G", 3 * 65 * 65), 3, 0, 65, 1, 0.0, d("M", 520), 4,
                                                           d("W", 520), 4, d("g", 520), 4, 4, d("q"), d("S", 65 * 65)),
        "hold": lambda: sh.cp_hold_rows(d("W"), c.get("ldw", 4), d("g"), 4, d("s"), 4, 4, t, 0 if c.get("nokeep") else d("k"),
                                        1, d("G"), 3, c.get("mode", 0), d("q")),
        "pinv": lambda: sh.cp_pinv_ragged(d("G", 65 * 65), 1, t, [d("W", 260)], [4], [d("P", 260)], d("bad")),
        "fms": lambda: sh.factor_congruence(2, side("a", c.get("Ca", 3), c.get("ra", 4), c.get("lda", 4)),
                                            side("b", c.get("Cb", 3), 4, 4), 0b11, 0 if c.get("nowork") else d("work", 4096),
                                            d("Phi", 129 * 129), d("wa"), d("wb")),
        "fold": lambda: sh.fold_slice_sums(d("src"), [2] * c.get("n", 0), d("out")),
    }
    if what == "armed":
        G_, S_, Si_ = d("G"), d("S"), d("Si")
        calls["armed"] = lambda: (sh.arm_gram_system(G_, 3, 0, 4, 0.0, S_, Si_),
                                  sh.cp_mode_update_nn(G_, 3, 0, 4, 0.0, d("M"), 4, d("W"), 4, d("g"), 4, 4, d("q"), S_))
    if st.hip or c.get("host"):
        try:
            calls[what]()
            refused = None
        except opshim_util.ShimError as e:
            refused = str(e)
        assert refused is not None, f"{c['name']}: the call was not refused"
        assert c["raises"] in refused, f"{c['name']}: refused with {refused!r}"
    P, W = vals(rng, "mix", (5, 3)), vals(rng, "mix", (5, 3))
    o = st.out("after", 5)
    sh.row_dots(st.inp(P.reshape(-1, order="F")).ptr, st.inp(W.reshape(-1, order="F")).ptr, 5, 3, 5, o.ptr)
    st.finish()
    st.verify = lambda: within(st, "after", st.got("after"), np.sum(P.astype(LD) * W, axis=1),
                               4 * U * np.sum(np.abs(P * W), axis=1))


OPS = {"ragged": op_ragged, "nn": op_nn, "gram_ragged": op_gram_ragged, "hold": op_hold, "pinv": op_pinv,
       "core": op_core, "fms": op_fms, "row_dots": op_row_dots, "fold": op_fold, "refuse": op_refuse}


# ------------------------------------------------------------------------------------------ running a case
def _independent(c, clean, pois, b):
    """every byte that is not start b's is that of the clean run"""
    for name, (o, _, raw) in clean.outs.items():
        if raw:
            continue
        t, own = clean.types[name], clean.owner.get(name)
        p0, p1 = clean.posts[name], pois.posts[name]
        x, y = p0[G:-G].view(t).copy(), p1[G:-G].view(t).copy()
        if own is not None:
            x[own == b] = 0
            y[own == b] = 0
        assert np.array_equal(p0[:G], p1[:G]) and np.array_equal(p0[-G:], p1[-G:]) and \
            np.array_equal(x.view(np.uint8), y.view(np.uint8)), \
            f"{c['name']} {name}: NaN in start {b} changed bytes of another start"


def run_case(sh, c, hip, log=None, perturb=None):
    """Runs a case twice on the shim `sh`, compares the two runs bit for bit and checks the second; with `poison` a
    third run checks the independence of the starts. perturb(st): the self-test's hook on the outcome before it is
    verified. Returns the route tags of one clean run."""
    first = None
    for rep in (0, 1):
        st = MSt(sh, c, hip, log if rep else None)
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
            if c.get("poison") is not None and not perturb:
                sp = MSt(sh, c, hip, None)
                try:
                    OPS[c["op"]](sp, c["poison"])
                    _independent(c, st, sp, c["poison"])
                finally:
                    sp.free()
                    sh.route_take()
            return st.tags
        finally:
            st.free()


def run_own_shim(kind, c, hip, log=None, perturb=None):
    """a case with `env`: it gets a Shim of its own (the switches are read when an Ops is made, and the state a
    refused armed call leaves behind goes with it)"""
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
        return run_case(sh, c, hip, log, perturb)
    finally:
        sh.close()


# ------------------------------------------------------------------------------------------ the table
CASES = []
_seed = [9000]


def _add(op, family, name, route, why, **kw):
    _seed[0] += 1
    kw.setdefault("cls", "pos" if _seed[0] % 2 else "mix")
    c = dict(op=op, family=family, name=f"{family}:{name}", route=route if isinstance(route, list) else [route],
             why=why, seed=_seed[0], **kw)
    CASES.append(c)
    return c


# ---- cp_mode_update_ragged
def rag(name, why, expect, **kw):
    rows, ranks = kw["rows"], kw["ranks"]
    rt = ragged_route(rows, ranks)
    assert rt == expect, (name, rt)
    pats = [r"update_ragged\." + rt]
    if rt == "loop":  # start by start through cp_mode_update: its tags too
        for R in ranks:
            pats.append(r"update\." + UC.update_route(rows, R).replace("staged", "staged presolved=0"))
    return _add("ragged", "ragged_update", name, pats, why, **kw)


rag("staged", "small ranks in LDS", "staged", rows=26, ranks=[1, 10, 3], N=3, mode=0, lam=0.125, poison=1)
rag("staged R_max=64 tile edges", "matrix-core tile edges", "staged", rows=20, ranks=[1, 64, 15, 16, 17], N=4, mode=1,
    poison=2)
rag("unstaged beside small starts", "rank-sweep shape", "unstaged", rows=104, ranks=[2, 48, 5], N=3, mode=1, lam=0.125,
    poison=0)
rag("unstaged R=64", "largest rank first", "unstaged", rows=21, ranks=[64, 1, 33], N=3, mode=2, poison=2)
rag("loop rows", "start by start", "loop", rows=933, ranks=[10, 4], N=4, mode=2, lam=0.125, poison=1)
rag("loop rank", "start by start", "loop", rows=17, ranks=[65, 3], N=4, mode=3, poison=1)
rag("32 starts", "table full", "staged", rows=9, ranks=[1 + b % 4 for b in range(32)], N=3, mode=0, lam=0.125, poison=31)
rag("equal ranks", "table engine never builds", "staged", rows=26, ranks=[5, 5, 5], N=4, mode=0, poison=0)
rag("staged indefinite start", "Jacobi in one start only", "staged", rows=26, ranks=[3, 10, 4], N=3, mode=1, indef=(1,))
rag("unstaged indefinite start", "Jacobi in one start only", "unstaged", rows=21, ranks=[64, 2], N=3, mode=0, indef=(0,))
rag("staged null S", "S, Sinv not returned", "staged", rows=26, ranks=[1, 10, 3], N=3, mode=2, null=True, lam=0.125)
rag("unstaged null S", "S, Sinv not returned", "unstaged", rows=104, ranks=[2, 48, 5], N=4, mode=3, null=True)
for k, x in enumerate(({"xm": 3}, {"xw": 2}, {"xg": 5}, {"xm": 1, "xw": 2, "xg": 3})):
    rag(f"staged ld {x}", "wide leading dimensions", "staged", rows=27, ranks=[1, 10, 3], N=3, mode=k % 3,
        lam=0.125 * (k % 2), poison=k % 3, **x)
rag("unstaged ld", "wide leading dimensions", "unstaged", rows=21, ranks=[64, 1, 33], N=3, mode=1, xm=2, xw=3, xg=1)


# ---- the HALS updates
def nn(family, name, why, **kw):
    return _add("nn", family, name, nn_route(kw), why, **kw)


NM = [(3, 0), (3, 1), (3, 2), (4, 0), (4, 1), (4, 2), (4, 3)]
_k = 0
for R in (1, 2, 17, 64):
    for rows in (1, 63, 64, 65, 129):
        N_, mode_ = NM[_k % len(NM)]
        nn("nn_single", f"tiles R={R} rows={rows}", "tile edges by rank", form="single", ranks=[R], rows=rows, N=N_,
           mode=mode_, lam=0.125 * (_k % 2), xm=1 + _k % 3, xw=2, xg=3 - _k % 3)
        _k += 1
nn("nn_single", "no rows", "empty factor", form="single", ranks=[17], rows=0, N=3, mode=1, xm=1, xw=2, xg=3)
nn("nn_single", "floor", "entries onto the floor", form="single", ranks=[17], rows=65, N=3, mode=0, cls="mix", xm=1, xw=1,
   xg=1, expect_floor=True)
nn("nn_single", "S[r,r] == 0", "column keeps its bits", form="single", ranks=[17], rows=65, N=3, mode=2, zero_diag=(0, 5),
   xm=2, xw=1, xg=3)
nn("nn_single", "S[r,r] == inf", "column keeps its bits", form="single", ranks=[2], rows=64, N=3, mode=0, inf_diag=(0, 0),
   xm=2, xw=1, xg=3)
nn("nn_single", "NaN row of M", "row onto the floor", form="single", ranks=[17], rows=129, N=4, mode=1, nan_row=70,
   lam=0.125, xm=2, xw=1, xg=3)
nn("nn_single", "null S", "S not returned", form="single", ranks=[64], rows=65, N=3, mode=1, null=True, lam=0.125, xm=1,
   xw=2, xg=3)
for K, R, rows in ((1, 17, 65), (3, 64, 65), (32, 2, 129), (3, 1, 63), (3, 17, 64), (3, 2, 1)):
    nn("nn_batched", f"K={K} R={R} rows={rows}", "tile sums per start", form="batched", ranks=[R] * K, rows=rows,
       N=3 + K % 2, mode=K % 3, lam=0.125 * (R % 2), xm=1, xw=2, xg=3, poison=K - 1 if K > 1 else None)
nn("nn_batched", "no rows", "empty factor", form="batched", ranks=[17] * 3, rows=0, N=3, mode=1, xm=1, xw=2, xg=3)
nn("nn_batched", "null S", "S not returned", form="batched", ranks=[17] * 3, rows=65, N=3, mode=0, null=True, xm=1, xw=2,
   xg=3)
nn("nn_batched", "S[r,r] == 0 in one start", "column keeps its bits", form="batched", ranks=[17] * 3, rows=65, N=4, mode=3,
   zero_diag=(1, 16), xm=1, xw=2, xg=3)
nn("nn_batched", "NaN row of M", "row onto the floor", form="batched", ranks=[2] * 3, rows=65, N=3, mode=2, nan_row=64,
   lam=0.125, xm=1, xw=2, xg=3)
for rows in (1, 63, 64, 65, 129):
    nn("nn_ragged", f"ranks 1,64,17 rows={rows}", "front of the LDS", form="ragged", ranks=[1, 64, 17], rows=rows,
       N=3 + rows % 2, mode=rows % 3, lam=0.125 * (rows % 2), xm=3, xw=1, xg=2, poison=rows % 3)
nn("nn_ragged", "32 starts", "table full", form="ragged", ranks=[1 + b % 4 for b in range(32)], rows=65, N=3, mode=0,
   lam=0.125, xm=3, xw=1, xg=2, poison=31)
nn("nn_ragged", "table of one", "one start", form="ragged", ranks=[2], rows=129, N=4, mode=2, xm=3, xw=1, xg=2)
nn("nn_ragged", "no rows", "empty factor", form="ragged", ranks=[1, 64, 17], rows=0, N=3, mode=1, xm=1, xw=2, xg=3)
nn("nn_ragged", "null S", "S not returned", form="ragged", ranks=[1, 64, 17], rows=65, N=3, mode=2, null=True, lam=0.125,
   xm=1, xw=2, xg=3)
nn("nn_ragged", "S[r,r] == 0 in one start", "column keeps its bits", form="ragged", ranks=[2, 17], rows=65, N=3, mode=1,
   zero_diag=(1, 0), xm=1, xw=2, xg=3)
nn("nn_ragged", "S[r,r] == inf in one start", "column keeps its bits", form="ragged", ranks=[2, 17], rows=63, N=3, mode=1,
   inf_diag=(0, 1), xm=1, xw=2, xg=3)
nn("nn_ragged", "NaN row of M", "row onto the floor", form="ragged", ranks=[17, 2], rows=65, N=4, mode=0, nan_row=0,
   xm=1, xw=2, xg=3)
for R, rows in ((1, 65), (17, 129), (64, 65), (2, 1)):
    nn("nn_forms", f"R={R} rows={rows}", "three forms, same bits", form="forms", ranks=[R], rows=rows, N=3, mode=R % 3,
       lam=0.125 * (rows % 2), xm=1, xw=2, xg=3)

# ---- gram_ragged: the four-chain loop and its tail, 2080 pairs over 16 waves
for k, rows in enumerate((1, 64, 255, 256, 257, 449)):
    N_ = (3, 8)[k % 2]
    _add("gram_ragged", "gram_ragged", f"rows={rows} N={N_}", [], "row loop edges", rows=rows, ranks=[1, 6, 64], N=N_,
         mode=(0, N_ - 1)[(k // 2) % 2], xld=1 + k, poison=k % 3)

# ---- cp_hold_rows
RH = [1, 17, 33, 3]
for k, rows in enumerate((1, 63, 64, 65, 257)):
    hm = 0b1011
    _add("hold", "hold_rows", f"rows={rows} edges", rf"hold_rows starts=4 holds={hm:#x}", "wave-edge rows held out", rows=rows,
         ranks=RH, N=3 + k % 2, mode=k % 3, holds=hm, keep=["edges", "random"], xw=1, xg=2, xs=3, poison=(0, 1, 3)[k % 3])
_add("hold", "hold_rows", "all kept", r"hold_rows starts=4 holds=0xf", "scores zeroed", rows=65, ranks=RH, N=3, mode=2,
     holds=0xF, keep="all", xw=3, xg=1, xs=2)
_add("hold", "hold_rows", "all held out", r"hold_rows starts=4 holds=0xf", "Gram, gradsq exactly zero", rows=65, ranks=RH, N=3,
     mode=0, holds=0xF, keep="none", xw=2, xg=3, xs=1)
_add("hold", "hold_rows", "clear bit between", r"hold_rows starts=4 holds=0x5", "one start untouched", rows=64, ranks=RH, N=4,
     mode=3, holds=0b0101, keep="random", xw=1, xg=2, xs=3, poison=0)
_add("hold", "hold_rows", "bits above nstarts", r"hold_rows starts=4 holds=0x5", "high bits masked", rows=63, ranks=RH, N=3,
     mode=1, holds=0xFFFFFFF5, keep="random", xw=1, xg=2, xs=3)
_add("hold", "hold_rows", "32 starts bit 31", r"hold_rows starts=32 holds=0x80000005", "unshifted mask", rows=65,
     ranks=[1 + b % 4 for b in range(32)], N=3, mode=0, holds=0x80000005, keep=["random", "edges"], xw=1, xg=2, xs=3,
     poison=31)
_add("hold", "hold_rows", "holds 0", [], "no launch, nothing written", rows=65, ranks=RH, N=3, mode=0, holds=0,
     keep="random", xw=1, xg=2, xs=3, not_route=[r"hold_rows"])
_add("hold", "hold_rows", "only high bits", [], "masked to nothing", rows=65, ranks=RH, N=3, mode=0, holds=0xF0,
     keep="random", xw=1, xg=2, xs=3, not_route=[r"hold_rows"])


# ---- cp_pinv_ragged
def pinv(name, why, **kw):
    return _add("pinv", "pinv_ragged", name, pinv_route(kw["rows"], kw["ranks"]), why, **kw)


pinv("N=1", "one mode", rows=[257], ranks=[1, 64, 17, 17], twin=(2, 3), poison=1)
pinv("N=3 idle tiles", "longest mode drives tiles", rows=[1, 255, 600], ranks=[1, 64, 17, 64], twin=(1, 3), poison=2)
pinv("N=8", "every mode", rows=[1, 255, 256, 257, 2, 17, 64, 65], ranks=[17, 1, 17], twin=(0, 2), poison=1)
pinv("tile cap", "strided row loop", rows=[262144 + 300], ranks=[1, 2, 2], twin=(1, 2))
pinv("bad pivots", "flag and zero block", rows=[5, 70, 3], ranks=[1, 2, 2, 2, 1, 3, 3],
     bad={0: ("zero", None), 1: ("ones2", None), 2: ("neg2", None), 3: ("nan", None), 4: ("inf", None)}, twin=(5, 6))
pinv("bad in one mode", "other modes still served", rows=[5, 300, 3], ranks=[3, 17, 3], bad={1: ("zero", [1])},
     twin=(0, 2))
pinv("bad later pivot", "NaN in the last pivot", rows=[40, 9], ranks=[17, 17, 64], bad={2: ("nan", [0])}, twin=(0, 1),
     poison=0)
pinv("flag preset", "a flag stays 1", rows=[9, 70], ranks=[2, 3, 3], preset={0: 1}, twin=(1, 2))

# ---- core_score: n below, at and above the 1024 threads
for R, N_ in ((1, 1), (1, 3), (2, 2), (7, 4), (32, 2), (33, 2), (64, 3), (2, 8)):
    _add("core", "core_score", f"R={R} N={N_}", [], "sum over the core", R=R, N=N_, kind="random")
for R, N_ in ((1, 3), (2, 2), (7, 4), (33, 2), (64, 3), (2, 8)):
    _add("core", "core_score", f"R={R} N={N_} superdiagonal", [], "exactly 100", R=R, N=N_, kind="diag")
    if R > 1:
        _add("core", "core_score", f"R={R} N={N_} superdiagonal + 1", [], "exactly 100 (1 - 1/R)", R=R, N=N_, kind="diag+1")
for R, N_ in ((2, 2), (33, 2)):
    _add("core", "core_score", f"R={R} N={N_} bad", [], "core and score NaN", R=R, N=N_, kind="bad")


# ---- factor_congruence
def fms(name, why, **kw):
    kw.setdefault("rows_b", kw["rows_a"])
    kw.setdefault("mask", (1 << len(kw["rows_a"])) - 1)
    return _add("fms", "congruence", name, fms_route(kw), why, **kw)


_FR = (1, 31, 32, 33, 1024, 1025)
for k, (Ca, Cb) in enumerate(((1, 1), (15, 17), (16, 16), (17, 128), (128, 1), (128, 128))):
    fms(f"cols {Ca}x{Cb} N=1 rows={_FR[k]}", "column tiles", rows_a=[_FR[k]], Ca=Ca, Cb=Cb, xa=1 + k % 2, xb=2)
    fms(f"cols {Ca}x{Cb} N=3", "column tiles", rows_a=[_FR[(k + 1) % 6], _FR[(k + 3) % 6], _FR[(k + 5) % 6]], Ca=Ca,
        Cb=Cb, xa=3, xb=1 + k % 2)
fms("N=8", "every mode", rows_a=[1, 31, 32, 33, 65, 2, 7, 64], Ca=15, Cb=17, xa=1, xb=2)
fms("skipped mode rows_a > rows_b", "mask, unequal extents", rows_a=[33, 70, 5], rows_b=[33, 40, 5], mask=0b101, Ca=17,
    Cb=15, xa=1, xb=2)
fms("skipped mode rows_a < rows_b", "mask, unequal extents", rows_a=[33, 5, 1025], rows_b=[33, 64, 1025], mask=0b101,
    Ca=16, Cb=16, xa=2, xb=1)
for kind in ("zero", "inf", "nan"):
    fms(f"{kind} column each side", "row and column of zeros", rows_a=[33, 65, 5], mask=0b110, Ca=17, Cb=33, xa=1, xb=2,
        special=[("a", 16, kind), ("b", 0, kind)])
fms("one side twice", "same and separate staging", rows_a=[1025, 33, 5], Ca=17, Cb=17, xa=2, pair=True)
fms("one side twice 128 cols", "same and separate staging", rows_a=[65, 31], Ca=128, Cb=128, xa=1, pair=True)

# ---- row_dots, fold_slice_sums
for k, rows in enumerate((1, 255, 256, 257, 70000)):
    _add("row_dots", "row_dots", f"rows={rows}", [], "grid edges", rows=rows, R=(1, 17, 64)[k % 3], xld=1 + k)
_add("row_dots", "row_dots", "rows=257 R=64", [], "grid edges", rows=257, R=64, xld=3)
for lens in ((1,), (5,), (3, 4), (7, 1, 5), (2, 3, 4, 5), (300, 7), (2, 1, 3, 2, 1, 2, 3, 2)):
    _add("fold", "fold_slice_sums", f"lens={lens}", rf"fold_slice_sums:n{len(lens)}", "terms per entry", lens=lens)


# ---- refusals
def ref(name, what, raises, host=False, **kw):
    return _add("refuse", "refusals", name, [], "refused, nothing written", what=what, raises=raises, host=host, **kw)


TABLE = "malformed table of starts"
_BAD_TABLES = {"nstarts 0": (0, [0], [0]), "nstarts 33": (33, list(range(33)), list(range(33))),
               "rank 0": (2, [0, 2, 2], [0, 4, 4]), "sq": (2, [0, 2, 5], [0, 4, 12])}
for tn, t in _BAD_TABLES.items():
    for what in ("ragged", "gram_ragged", "nn_ragged", "hold", "pinv"):
        ref(f"{what} table {tn}", what, TABLE, table=t)
ref("nn single R=65", "nn_single", "supports R <= 64", host=True)
ref("nn batched R=65", "nn_batched", "supports R <= 64", host=True)
ref("nn ragged R=65", "nn_ragged", "supports R <= 64", host=True, table=table([65]))
ref("pinv R=65", "pinv", "support ranks <= 64", host=True, table=table([65]))
ref("hold ld < rows", "hold", "cp_hold_rows arguments out of range", table=table([2]), ldw=3)
ref("hold mode >= N", "hold", "cp_hold_rows arguments out of range", table=table([2]), mode=3)
ref("hold null keep", "hold", "cp_hold_rows arguments out of range", table=table([2]), nokeep=True)
ref("fms 0 columns", "fms", "supports 1 .. 128 columns", host=True, Ca=0)
ref("fms 129 columns", "fms", "supports 1 .. 128 columns", host=True, Cb=129)
ref("fms ld < rows", "fms", "rows / leading dimension out of range", lda=3)
ref("fms rows differ", "fms", "extents differ in a compared mode", ra=3, lda=3)
ref("fms null work", "fms", "without its work buffer", nowork=True)
ref("fold n=0", "fold", "fold_slice_sums order out of range", n=0)
ref("fold n=9", "fold", "fold_slice_sums order out of range", n=9)
ref("armed system before nn", "armed", "armed S / Normalize in front of a non-negative mode update", env={})

FAMILIES = sorted({c["family"] for c in CASES})

# Every tag family these launchers can log. update_ragged.loop goes start by start through cp_mode_update and logs
# the tags of the launchers behind it as well (the unfused update: gram_system and cp_update).
EXPECTED_TAGS = sorted(
    ["update_ragged.staged", "update_ragged.unstaged", "update_ragged.loop", "update.staged", "update.unfused",
     "gram_system.wave", "gram_system.mfma", "cp_update.rows", "cp_update.gemm", "update_nn", "update_nn_batched",
     "update_nn_ragged", "hold_rows", "pinv_ragged", "fms.cross", "fold_slice_sums"])


def tag_family(tag):
    return re.split(r"[ :]", tag)[0]


def run(kind, sh, c, hip, log=None, perturb=None):
    return run_own_shim(kind, c, hip, log, perturb) if "env" in c else run_case(sh, c, hip, log, perturb)
