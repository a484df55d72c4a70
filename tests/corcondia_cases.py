"""The cases of the core consistency diagnostic shared by tests/test_corcondia_hostsim.py (the engine's
control flow on the host stand-in) and tests/test_gpu_corcondia.py (the HIP kernels): each takes the binding
`pp` it runs on. Reference and bars: tests/corcondia_ref.py."""
import ctypes as C

import numpy as np

import bf16_util
import corcondia_ref as R

F32, F64, BF16 = R.F32, R.F64, R.BF16

# (lens, rank): order 3 and 4, extents that are no multiples of 4 or 8, the bf16 row fall-back ([13, 6, 5])
SINGLE = [([12, 11, 10, 9], 2), ([12, 11, 10, 9], 4), ([12, 11, 10, 9], 5), ([9, 8, 7], 3), ([13, 6, 5], 5)]
SWEEP_LENS, SWEEP_RANKS = [12, 11, 10, 9], [2, 5, 3, 4]
WIDE_LENS, WIDE_RANK, WIDE_STARTS = [20, 18, 17], 17, 4   # 68 columns in the shared scan


def ident(v):
    if isinstance(v, (list, tuple)):
        return "x".join(map(str, v))
    return {F32: "F32", F64: "F64", BF16: "BF16"}.get(v, str(v)) if isinstance(v, int) else str(v)


def session(pp, ctx, t, Ws, nonneg=False, schedule=None):
    s = pp.CP(ctx, t, Ws[0].shape[1])
    if schedule:
        s.set_schedule(schedule)
    if nonneg:
        s.set_nonneg(True)
    s.set_factors(Ws)
    return s


def closed_form(pp, ctx, lens, rank, dtype, seed=11):
    """V = H x_i W_i with H = T + 0.3 U(-1, 1): the core is H, cc = 100 (1 - ||H - T||^2 / R)"""
    N = len(lens)
    rng = np.random.default_rng(seed)
    Ws = R.factors(lens, rank, seed + 1)
    H = R.superdiagonal(rank, N) + 0.3 * rng.uniform(-1.0, 1.0, (rank,) * N)
    V = R.tucker_tensor(H, Ws)
    Vs = R.stored(V, dtype)
    t = pp.Tensor(ctx, lens, dtype).upload(V)
    s = session(pp, ctx, t, Ws)
    cc, core = s.core_consistency(return_core=True)
    what = f"closed form {ident(lens)} R={rank} {ident(dtype)}"
    G_ref, cc_ref, e, cc_bar = R.check(what, Vs, Ws, dtype, cc, core)
    # numpy on V as stored against the closed form: apart by what the storage rounding of V does to the core,
    # and by numpy's own fp64 chain (inverse included), held to the fp64 bar
    slack = (np.prod([np.linalg.norm(R.pinv_t(W), 2) for W in Ws]) * np.linalg.norm(Vs - V)
             + R.bars(Vs, Ws, R.U_OF[F64], G_ref)[0])
    assert np.linalg.norm(G_ref - H) <= slack, (np.linalg.norm(G_ref - H), slack)
    if dtype == F64:  # nothing is rounded on the way in: the library against the closed form itself
        cc_H = 100.0 * (1.0 - np.sum((H - R.superdiagonal(rank, N)) ** 2) / rank)
        print(f"[corcondia] {what}: against H: core {np.linalg.norm(core - H):.3e} bar {e:.3e}, "
              f"cc {abs(cc - cc_H):.3e} bar {cc_bar:.3e}")
        assert np.linalg.norm(core - H) <= e and abs(cc - cc_H) <= cc_bar
    assert s.core_consistency() == cc  # the same state gives the same bits, with and without the core
    s.close()
    t.close()


def exact_cp(pp, ctx, lens, rank, dtype, seed=23):
    """V = [[W]]: cc = 100"""
    Ws = R.factors(lens, rank, seed)
    V = R.cp_tensor(Ws)
    t = pp.Tensor(ctx, lens, dtype).upload(V)
    s = session(pp, ctx, t, Ws)
    cc = s.core_consistency()
    what = f"exact CP {ident(lens)} R={rank} {ident(dtype)}"
    _, cc_ref, _, cc_bar = R.check(what, R.stored(V, dtype), Ws, dtype, cc)
    if dtype == F64:
        assert abs(cc_ref - 100.0) < 1e-8 and abs(cc - 100.0) <= cc_bar
    s.close()
    t.close()


def noisy_tensor(lens, rank, seed):
    """a rank-`rank` CP tensor plus 10 % noise: something for two sweeps to fit at every rank"""
    rng = np.random.default_rng(seed)
    V = R.cp_tensor(R.factors(lens, rank, seed + 1))
    E = rng.uniform(-1.0, 1.0, lens)
    return V + 0.1 * np.linalg.norm(V) / np.linalg.norm(E) * E


def multi_equals_ordinary(pp, ctx, dtype, lens, ranks, equal, sweeps=2, nonneg=False, seed=31):
    """every start of a multi-start session against numpy and against an ordinary session of the start's
    rank holding the same factors; equal: the session of ppals_cp_multi_create"""
    V = noisy_tensor(lens, 3, seed)
    if nonneg:
        V = np.abs(V)
    Vs = R.stored(V, dtype)
    t = pp.Tensor(ctx, lens, dtype).upload(V)
    m = pp.CPMulti(ctx, t, ranks[0], len(ranks)) if equal else pp.CPMulti.with_ranks(ctx, t, ranks)
    W0 = [R.factors(lens, r, seed + 7 * b) for b, r in enumerate(ranks)]
    if nonneg:
        W0 = [[np.abs(W) for W in Ws] for Ws in W0]
        m.set_nonneg(True)
    m.set_factors(-1, W0)
    m.sweeps(sweeps)
    ccs = m.core_consistencies()
    assert ccs.shape == (len(ranks),)
    for b, r in enumerate(ranks):
        Wb = m.get_factors(b)
        core = m.core(b)
        what = f"multi {ident(lens)} ranks {ident(ranks)} start {b} {ident(dtype)}" + (" nonneg" if nonneg else "")
        _, _, e, cc_bar = R.check(what, Vs, Wb, dtype, ccs[b], core)
        s = session(pp, ctx, t, Wb)   # (unconstrained, whatever the multi session is)
        cc_o, core_o = s.core_consistency(return_core=True)
        R.check(what + " (ordinary)", Vs, Wb, dtype, cc_o, core_o)
        print(f"[corcondia] {what}: multi - ordinary: cc {abs(ccs[b] - cc_o):.3e} bar {cc_bar:.3e}, "
              f"core {np.linalg.norm(core - core_o):.3e} bar {e:.3e}")
        assert abs(ccs[b] - cc_o) <= cc_bar and np.linalg.norm(core - core_o) <= e
        s.close()
        if nonneg:  # a non-negative ordinary session holding the same factors: the same figure
            sn = session(pp, ctx, t, Wb, nonneg=True)
            cc_n = sn.core_consistency()
            assert abs(cc_n - cc_o) <= cc_bar, (cc_n, cc_o, cc_bar)
            sn.close()
    m.close()
    t.close()


def _same(a, b):
    return all(bf16_util.same_values(x, y) for x, y in zip(a, b))


def read_only(pp, ctx, dtype, multi, schedule, seed=41):
    """two identical sessions, 1 + 1 sweeps each, one with the diagnostic in between: bit-equal factors and
    gradients"""
    lens, ranks = SWEEP_LENS, SWEEP_RANKS
    t = pp.Tensor(ctx, lens, dtype).upload(noisy_tensor(lens, 3, seed))
    out = []
    for call in (True, False):
        if multi:
            s = pp.CPMulti.with_ranks(ctx, t, ranks)
            s.set_schedule(schedule)
            s.set_factors(-1, [R.factors(lens, r, seed + 7 * b) for b, r in enumerate(ranks)])
            step = lambda: s.sweeps(1)
            diag = lambda: (s.core_consistencies(), s.core(1))
            read = lambda: s.get_factors(-1, with_grad=True)
        else:
            s = session(pp, ctx, t, R.factors(lens, 4, seed), schedule=schedule)
            step = lambda: s.sweeps_dt(1)
            diag = lambda: s.core_consistency(return_core=True)
            read = lambda: s.get_factors(with_grad=True)
        step()
        if call:
            first = diag()
            again = diag()  # the kept buffers, and the same bits
            assert _same([np.atleast_1d(first[0]), first[1]], [np.atleast_1d(again[0]), again[1]])
        step()
        W, G = read()
        if multi:
            W, G = [w for Ws in W for w in Ws], [g for Gs in G for g in Gs]
        out.append((W, G))
        s.close()
    assert _same(out[0][0], out[1][0]), "the factors differ after a core consistency call"
    assert _same(out[0][1], out[1][1]), "the gradients differ after a core consistency call"
    t.close()


def nan_rule(pp, ctx, dtype, seed=53):
    """a start with an exactly zero column: NaN for that start alone, PPALS_OK all the same"""
    lens, ranks, badb = SWEEP_LENS, SWEEP_RANKS, 1
    V = noisy_tensor(lens, 3, seed)
    Vs = R.stored(V, dtype)
    t = pp.Tensor(ctx, lens, dtype).upload(V)
    W0 = [R.factors(lens, r, seed + 7 * b) for b, r in enumerate(ranks)]
    W0[badb][2][:, 3] = 0.0
    m = pp.CPMulti.with_ranks(ctx, t, ranks)
    m.set_factors(-1, W0)
    ccs = np.full(len(ranks), -1.0)
    assert pp.lib().ppals_cp_multi_core_consistency(m._h, pp._dp(ccs)) == 0   # PPALS_OK
    assert np.isnan(ccs[badb]), ccs
    for b in range(len(ranks)):
        if b != badb:
            R.check(f"NaN rule, start {b} beside a bad one {ident(dtype)}", Vs, W0[b], dtype, ccs[b], m.core(b))
    core = m.core(badb)
    assert core.shape == (ranks[badb],) * len(lens) and np.all(np.isnan(core))
    s = session(pp, ctx, t, W0[badb])
    cc = C.c_double(-1.0)
    n = C.c_int64(0)
    core = np.zeros(ranks[badb] ** len(lens))
    assert pp.lib().ppals_cp_core_consistency(s._h, C.byref(cc), pp._dp(core), C.byref(n)) == 0
    assert np.isnan(cc.value) and n.value == core.size and np.all(np.isnan(core))
    for h in (s, m, t):
        h.close()
