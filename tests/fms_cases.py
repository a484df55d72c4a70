"""The cases of the factor congruence and the factor match score shared by tests/test_fms_hostsim.py (the
engine's control flow and the C ABI's checks on the host stand-in) and tests/test_gpu_fms.py (the HIP
kernels k_fms_cross / k_fms_finish): each takes the binding `pp` it runs on. Reference and bars:
tests/fms_ref.py. The tensors are tiny and never read unless a case sweeps."""
import ctypes as C

import numpy as np

import bf16_util
import fms_ref as R

F32, F64 = 0, 1

# (lens, ranks of a multi-start session): what each shape reaches is said in the suites' docstrings
MULTI = [([13, 6, 5], [1, 5, 2]), ([4100, 3, 2], [7, 7, 7]), ([33, 17, 9, 5], [32] * 4), ([20, 18, 17], [17] * 4)]
CHUNKED = MULTI[1]


def ident(v):
    if isinstance(v, (list, tuple)):
        return "x".join(map(str, v))
    return str(v)


def tensor(pp, ctx, lens, dtype=F64):
    return pp.Tensor(ctx, lens, dtype).fill_uniform(1)


def cp(pp, ctx, t, Ws, schedule=None, nonneg=False):
    s = pp.CP(ctx, t, Ws[0].shape[1])
    if schedule:
        s.set_schedule(schedule)
    if nonneg:
        s.set_nonneg(True)
    s.set_factors(Ws)
    return s


def multi(pp, ctx, t, starts, schedule=None, nonneg=False):
    m = pp.CPMulti.with_ranks(ctx, t, [W[0].shape[1] for W in starts])
    if schedule:
        m.set_schedule(schedule)
    if nonneg:
        m.set_nonneg(True)
    m.set_factors(-1, starts)
    return m


def starts_of(lens, ranks, seed):
    return [R.factors(lens, r, seed + 7 * b) for b, r in enumerate(ranks)]


def close(*hs):
    for h in hs:
        h.close()


def check_phi(what, got, A, B, lens, skip_mode=None):
    ref, _, _ = R.congruence(A, B, skip_mode)
    err, bar = np.max(np.abs(got - ref)), R.bar_phi(lens)
    print(f"[fms] {what}: |Phi - numpy| {err:.3e} bar {bar:.3e}")
    assert got.shape == ref.shape and not np.any(np.isnan(got))
    assert err <= bar, (what, err, bar)
    return ref


# ---- 1. Phi against numpy
def multi_phi(pp, ctx, lens, ranks, seed=3):
    """congruence of a multi-start session with itself and with a second session"""
    t = tensor(pp, ctx, lens)
    Sa, Sb = starts_of(lens, ranks, seed), starts_of(lens, ranks[::-1], seed + 100)
    a, b = multi(pp, ctx, t, Sa), multi(pp, ctx, t, Sb)
    A, B = R.hstack(Sa), R.hstack(Sb)
    bar = R.bar_phi(lens)
    own = a.congruence()
    check_phi(f"multi {ident(lens)} ranks {ident(ranks)} (itself)", own, A, A, lens)
    print(f"[fms]   |diag - 1| {np.max(np.abs(np.diag(own) - 1)):.3e} |Phi - Phi^T| {np.max(np.abs(own - own.T)):.3e}")
    assert np.max(np.abs(np.diag(own) - 1.0)) <= bar and np.max(np.abs(own - own.T)) <= bar
    check_phi(f"multi {ident(lens)} ranks {ident(ranks)} (other)", a.congruence(b), A, B, lens)
    close(a, b, t)


def ordinary_phi(pp, ctx, lens, ra, rb, seed=5):
    """two ordinary sessions, both ways round"""
    t = tensor(pp, ctx, lens)
    A, B = R.factors(lens, ra, seed), R.factors(lens, rb, seed + 1)
    a, b = cp(pp, ctx, t, A), cp(pp, ctx, t, B)
    check_phi(f"ordinary {ident(lens)} R={ra} against R={rb}", a.congruence(b), A, B, lens)
    check_phi(f"ordinary {ident(lens)} R={rb} against R={ra}", b.congruence(a), B, A, lens)
    close(a, b, t)


def skipped_mode_phi(pp, ctx, seed=9):
    """[13, 6, 5] against [9, 6, 5] with skip_mode = 0: ordinary sessions and multi_congruence(s, other)"""
    la, lb = [13, 6, 5], [9, 6, 5]
    ta, tb = tensor(pp, ctx, la), tensor(pp, ctx, lb)
    A, B = R.factors(la, 4, seed), R.factors(lb, 3, seed + 1)
    a, b = cp(pp, ctx, ta, A), cp(pp, ctx, tb, B)
    check_phi("skip_mode 0, ordinary", a.congruence(b, skip_mode=0), A, B, la, 0)
    f, perm = a.fms(b, skip_mode=0, weights=True, return_perm=True)
    want, _ = R.fms(A, B, 0, True)   # (the norms of the skipped mode are in w)
    assert abs(f - want) <= R.bar_fms(la, True), (f, want)
    Sa, Sb = starts_of(la, [2, 3], seed + 2), starts_of(lb, [3, 1, 2], seed + 3)
    ma, mb = multi(pp, ctx, ta, Sa), multi(pp, ctx, tb, Sb)
    check_phi("skip_mode 0, multi against another", ma.congruence(mb, skip_mode=0), R.hstack(Sa), R.hstack(Sb), la, 0)
    close(a, b, ma, mb, ta, tb)


# ---- 2. invariance
def invariance(pp, ctx, seed=13):
    lens, rank = [13, 6, 5], 4
    rng = np.random.default_rng(seed)
    t = tensor(pp, ctx, lens)
    A = R.factors(lens, rank, seed)
    pi = rng.permutation(rank)                     # column p of a is column pi[p] of b
    scale = rng.uniform(0.9, 1.1, (len(lens), rank))
    sign = np.ones((len(lens), rank))
    sign[0, [0, 2]] = -1.0                         # two modes of some columns
    sign[2, [0, 2]] = -1.0
    B = [np.zeros_like(W) for W in A]
    for i in range(len(lens)):
        B[i][:, pi] = A[i] * (scale[i] * sign[i])[None, :]
    a, b = cp(pp, ctx, t, A), cp(pp, ctx, t, B)
    f, perm = a.fms(b, return_perm=True)
    print(f"[fms] invariance: |fms - 1| {abs(f - 1):.3e} bar {R.bar_fms(lens):.3e}")
    assert abs(f - 1.0) <= R.bar_fms(lens) and list(perm) == list(pi)
    c = np.prod(scale, axis=0)                     # w_b[pi[p]] = c[p] w_a[p]
    closed = np.mean(1.0 - np.abs(1.0 - c) / np.maximum(1.0, c))
    fw, permw = a.fms(b, weights=True, return_perm=True)
    print(f"[fms] invariance, weights: |fms - closed form| {abs(fw - closed):.3e} bar {R.bar_fms(lens, True):.3e}")
    assert abs(fw - closed) <= R.bar_fms(lens, True) and list(permw) == list(pi)
    assert abs(R.fms(A, B, None, True)[0] - closed) <= R.bar_fms(lens, True)   # (the planted matching is the optimum)
    B[1][:, pi[1]] *= -1.0                         # ONE mode of one column
    b.set_factors(B)
    phi = a.congruence(b)
    assert abs(phi[1, pi[1]] + 1.0) <= R.bar_phi(lens), phi[1, pi[1]]
    close(a, b, t)


# ---- 3. fms against brute force
def ordinary_fms(pp, ctx, lens, ra, rb, seed=17):
    t = tensor(pp, ctx, lens)
    A, B = R.factors(lens, ra, seed), R.factors(lens, rb, seed + 1)
    a, b = cp(pp, ctx, t, A), cp(pp, ctx, t, B)
    for x, y, X, Y in ((a, b, A, B), (b, a, B, A)):
        for weights in (False, True):
            f, perm = x.fms(y, weights=weights, return_perm=True)
            want, _ = R.fms(X, Y, None, weights)
            bar = R.bar_fms(lens, weights)
            print(f"[fms] ordinary {ident(lens)} R={X[0].shape[1]} against R={Y[0].shape[1]} weights={weights}: "
                  f"|fms - brute force| {abs(f - want):.3e} bar {bar:.3e}")
            assert abs(f - want) <= bar
            assert x.fms(y, weights=weights) == f
            # the matching handed out is injective, of min(ra, rb) pairs, and attains the score
            m = min(X[0].shape[1], Y[0].shape[1])
            hit = perm[perm >= 0]
            assert len(hit) == m and len(set(hit)) == m and np.all(hit < Y[0].shape[1])
            sc = R.score(*R.congruence(X, Y), weights)
            assert abs(sum(sc[p, q] for p, q in enumerate(perm) if q >= 0) / m - want) <= bar
    close(a, b, t)


def multi_fms(pp, ctx, seed=19):
    """K x K of a rank sweep, fms_between, and fms[a, b] against ordinary sessions filled by take"""
    lens, ranks = [13, 6, 5], [1, 5, 2]
    t = tensor(pp, ctx, lens)
    Sa, Sb = starts_of(lens, ranks, seed), starts_of(lens, [2, 4, 5], seed + 50)
    ma, mb = multi(pp, ctx, t, Sa), multi(pp, ctx, t, Sb)
    K = len(ranks)
    for weights in (False, True):
        bar = R.bar_fms(lens, weights)
        F = ma.fms(weights=weights)
        assert F.shape == (K, K)
        for x in range(K):
            for y in range(K):
                want, _ = R.fms(Sa[x], Sa[y], None, weights)
                assert abs(F[x, y] - want) <= bar, (x, y, F[x, y], want)
        assert np.max(np.abs(F - F.T)) <= bar and np.max(np.abs(np.diag(F) - 1.0)) <= bar
        between = ma.fms_between(mb, weights=weights)
        assert between.shape == (K,)
        for k in range(K):
            assert abs(between[k] - R.fms(Sa[k], Sb[k], None, weights)[0]) <= bar
        singles = [ma.take(k, pp.CP(ctx, t, ranks[k])) for k in range(K)]
        for x in range(K):
            for y in range(K):
                assert abs(singles[x].fms(singles[y], weights=weights) - F[x, y]) <= bar
        close(*singles)
    close(ma, mb, t)


# ---- 4. queued work is seen
def queued_work(pp, ctx, dtype, seed=23):
    lens, ranks = [13, 6, 5], [1, 5, 2]
    t = pp.Tensor(ctx, lens, dtype).fill_uniform(seed, -1.0, 1.0)
    m = multi(pp, ctx, t, starts_of(lens, ranks, seed))
    m.sweeps(2)
    phi = m.congruence()      # no sync in between
    F = m.fms()
    S = m.get_factors(-1)
    check_phi("after sweeps(2), no sync", phi, R.hstack(S), R.hstack(S), lens)
    for x in range(len(ranks)):
        for y in range(len(ranks)):
            assert abs(F[x, y] - R.fms(S[x], S[y])[0]) <= R.bar_fms(lens)
    close(m, t)


# ---- 5. read-only
def _same(a, b):
    return len(a) == len(b) and all(bf16_util.same_values(x, y) for x, y in zip(a, b))


def read_only(pp, ctx, dtype, kind, schedule, seed=29):
    """two identical sessions, 1 + 1 sweeps each, one with the calls in between: bit-equal factors and
    gradients. kind: "ordinary", "multi" or "nonneg" (a non-negative multi-start session)"""
    lens, ranks = [12, 11, 10, 9], [2, 5, 3]
    nonneg = kind == "nonneg"
    t = pp.Tensor(ctx, lens, dtype).fill_uniform(seed, 0.1 if nonneg else -1.0, 1.0)
    fac = (lambda r, s: [np.abs(W) + 0.01 for W in R.factors(lens, r, s)]) if nonneg else (lambda r, s: R.factors(lens, r, s))
    out = []
    for call in (True, False):
        if kind == "ordinary":
            s = cp(pp, ctx, t, fac(4, seed), schedule=schedule)
            o = cp(pp, ctx, t, fac(3, seed + 1), schedule=schedule)
            step = lambda: s.sweeps_dt(1)
            diag = lambda: [s.congruence(o), s.congruence(s, skip_mode=1), np.atleast_1d(s.fms(o, weights=True))]
            read = lambda: s.get_factors(with_grad=True)
        else:
            s = multi(pp, ctx, t, [fac(r, seed + 7 * b) for b, r in enumerate(ranks)], schedule=schedule, nonneg=nonneg)
            o = None
            step = lambda: s.sweeps(1)
            diag = lambda: [s.congruence(), s.fms(weights=True), s.fms_between(s, skip_mode=0)]
            read = lambda: s.get_factors(-1, with_grad=True)
        step()
        if call:
            first = diag()
            assert _same(first, diag())   # the kept buffers, and the same bits
        step()
        W, G = read()
        if kind != "ordinary":
            W, G = [w for Ws in W for w in Ws], [g for Gs in G for g in Gs]
        out.append((W, G))
        close(s, *([o] if o is not None else []))
    assert _same(out[0][0], out[1][0]), "the factors differ after a congruence / fms call"
    assert _same(out[0][1], out[1][1]), "the gradients differ after a congruence / fms call"
    t.close()


# ---- 6. the same bits twice
def same_bits_twice(pp, ctx, seed=31):
    lens, ranks = CHUNKED
    t = tensor(pp, ctx, lens)
    m = multi(pp, ctx, t, starts_of(lens, ranks, seed))
    assert bf16_util.same_values(m.congruence(), m.congruence())
    assert bf16_util.same_values(m.fms(weights=True), m.fms(weights=True))
    close(m, t)


# ---- 7. the zero rule
def zero_rule(pp, ctx, seed=37):
    lens, ranks, badb, badc, badmode = [13, 6, 5], [2, 3, 2], 1, 1, 2
    t = tensor(pp, ctx, lens)
    S = starts_of(lens, ranks, seed)
    S[badb][badmode][:, badc] = 0.0
    m = multi(pp, ctx, t, S)
    A = R.hstack(S)
    C_ = sum(ranks)
    phi = np.full((C_, C_), np.nan, order="F")
    n = C.c_int64(0)
    assert pp.lib().ppals_cp_multi_congruence(m._h, None, -1, pp._dp(phi), C.byref(n)) == 0   # PPALS_OK
    assert n.value == C_ * C_ and not np.any(np.isnan(phi))
    z = ranks[0] + badc
    assert np.all(phi[z, :] == 0.0) and np.all(phi[:, z] == 0.0)
    ref = check_phi("zero rule", phi, A, A, lens)
    assert np.all(ref[z, :] == 0.0) and np.count_nonzero(ref == 0.0) == 2 * C_ - 1   # the others are not touched
    F = m.fms()
    for x in range(len(ranks)):
        for y in range(len(ranks)):
            assert abs(F[x, y] - R.fms(S[x], S[y])[0]) <= R.bar_fms(lens)
    # the zero column lies in the skipped mode: Phi does not see it, w does
    phi2 = m.congruence(skip_mode=badmode)
    check_phi("zero column in the skipped mode", phi2, A, A, lens, badmode)
    assert np.all(phi2[z, :] != 0.0)
    Fw = m.fms(skip_mode=badmode, weights=True)
    assert not np.any(np.isnan(Fw))
    for x in range(len(ranks)):
        for y in range(len(ranks)):
            assert abs(Fw[x, y] - R.fms(S[x], S[y], badmode, True)[0]) <= R.bar_fms(lens, True)
    assert abs(Fw[badb, badb] - (ranks[badb] - 1) / ranks[badb]) <= R.bar_fms(lens, True)   # that pair scores 0
    close(m, t)
