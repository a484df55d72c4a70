"""The core consistency diagnostic (Bro & Kiers 2003) in numpy, fp64, on V as stored — the reference of
tests/test_corcondia_hostsim.py and tests/test_gpu_corcondia.py — and the bars those tests hold the
library to, computed from each test's own inputs.

    P_i = W_i (W_i^T W_i)^-1,   G = V x_0 P_0^T ... x_{N-1} P_{N-1}^T,   cc = 100 (1 - ||G - T||_F^2 / R)

Bars. u = KTOL of tests/contraction_cases.py, the project's Frobenius bar of ONE contraction (2e-6 where the
tensor is stored as fp32 or bf16, 1e-10 for fp64). The core is a chain of N contractions, each within u of
its own result norm and each amplifying what it is given by at most ||P_i||_2, so norm-wise
    ||G - G_ref||_F <= e = N u prod_i ||P_i||_2 ||V||_F,
and with d = G - G_ref:  | ||G - T||^2 - ||G_ref - T||^2 | <= 2 ||G_ref - T|| ||d|| + ||d||^2, hence
    |cc - cc_ref| <= 100 (2 ||G_ref - T||_F e + e^2) / R."""
import numpy as np

import bf16_util
import contraction_cases as CC

F32, F64, BF16 = 0, 1, 3
U_OF = {F32: CC.KTOL[CC.U24], BF16: CC.KTOL[CC.U24], F64: CC.KTOL[CC.U53]}


def stored(V, dtype):
    """V as a tensor of that storage type holds it, in fp64"""
    V = np.asarray(V, dtype=np.float64)
    if dtype == F32:
        return V.astype(np.float32).astype(np.float64)
    if dtype == BF16:
        return bf16_util.bf16_round(V)
    return V


def factors(lens, R, seed):
    """U(-1, 1): zero mean, so the columns are far from collinear"""
    rng = np.random.default_rng(seed)
    return [np.asfortranarray(rng.uniform(-1.0, 1.0, (s, R))) for s in lens]


def pinv_t(W):
    return W @ np.linalg.inv(W.T @ W)


def mode_products(X, Ms):
    """X x_0 M_0^T x_1 M_1^T ...: index i_k of X contracted with the rows of M_k"""
    for M in Ms:
        X = np.tensordot(X, M, axes=(0, 0))  # the new index goes last: after N steps the order is natural
    return X


def superdiagonal(R, N):
    T = np.zeros((R,) * N)
    T[tuple([np.arange(R)] * N)] = 1.0
    return T


def cp_tensor(Ws):
    return mode_products(superdiagonal(Ws[0].shape[1], len(Ws)), [W.T for W in Ws])


def tucker_tensor(H, Ws):
    return mode_products(H, [W.T for W in Ws])


def score(G):
    R, N = G.shape[0], G.ndim
    return 100.0 * (1.0 - np.sum((G - superdiagonal(R, N)) ** 2) / R)


def reference(V, Ws):
    """(core, cc) of the factors Ws on V"""
    G = mode_products(V, [pinv_t(W) for W in Ws])
    return G, score(G)


def bars(V, Ws, u, G_ref):
    """(e, cc_bar) of the module docstring"""
    N, R = V.ndim, Ws[0].shape[1]
    e = N * u * np.prod([np.linalg.norm(pinv_t(W), 2) for W in Ws]) * np.linalg.norm(V)
    gt = np.linalg.norm(G_ref - superdiagonal(R, N))
    return e, 100.0 * (2.0 * gt * e + e * e) / R


def check(what, V, Ws, dtype, cc, core=None):
    """cc (and the core) of the library against numpy on V as stored, each figure printed beside its bar;
    returns (G_ref, cc_ref, e, cc_bar)"""
    G_ref, cc_ref = reference(V, Ws)
    e, cc_bar = bars(V, Ws, U_OF[dtype], G_ref)
    cc_err = abs(cc - cc_ref)
    line = f"[corcondia] {what}: cc {cc:.9g} ref {cc_ref:.9g} |diff| {cc_err:.3e} bar {cc_bar:.3e}"
    if core is not None:
        assert core.shape == G_ref.shape, (core.shape, G_ref.shape)
        g_err = np.linalg.norm(core - G_ref)
        line += f"; core error {g_err:.3e} bar {e:.3e}"
    print(line)
    assert np.isfinite(cc) and cc_err <= cc_bar, line
    if core is not None:
        assert np.all(np.isfinite(core)) and g_err <= e, line
    return G_ref, cc_ref, e, cc_bar
