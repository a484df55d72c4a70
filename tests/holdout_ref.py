"""Plain numpy fp64 CP-ALS with hold-out rows in one mode (the reference of the hold-out suites): cyclic mode
updates 0..N-1 without Normalize, as ppals_cpd_als / PPALS_OPT_SIMPLE runs them, on the FULL tensor, with the
held-out rows of W[mode] and of its gradient put back to zero behind every update of `mode` — and what the
update computed for them kept as the predicted scores."""
import numpy as np


def mttkrp(V, W, i):
    """M[x, r] = sum over the other indices of V[.., x, ..] * prod_{j != i} W_j[i_j, r]"""
    others = [j for j in range(V.ndim) if j != i]
    out = np.einsum("x...j,jr->x...r", np.moveaxis(V, i, 0), W[others[-1]])   # the last axis first: r joins
    for j in others[-2::-1]:
        out = np.einsum("x...jr,jr->x...r", out, W[j])
    return out


def system(W, i, lam):
    S = np.ones((W[0].shape[1],) * 2)
    for j in range(len(W)):
        if j != i:
            S = S * (W[j].T @ W[j])
    return S + lam * np.eye(S.shape[0])


def als_holdout(V, W0, G0, mode, keep, sweeps, lam=0.0):
    """(W, grad, scores) after `sweeps` sweeps from W0 (gradients G0): W[mode] and grad[mode] have zero rows where
    keep is False, scores (s_mode, R) holds those rows as last computed (before any sweep: W0's) and 0 elsewhere"""
    keep = np.asarray(keep, dtype=bool)
    W = [np.array(w, dtype=np.float64) for w in W0]
    G = [np.array(g, dtype=np.float64) for g in G0]
    scores = np.where(keep[:, None], 0.0, W[mode])
    W[mode][~keep] = 0.0
    G[mode][~keep] = 0.0
    for _ in range(sweeps):
        for i in range(V.ndim):
            M, S = mttkrp(V, W, i), system(W, i, lam)
            G[i] = -M + W[i] @ S
            W[i] = np.linalg.solve(S, M.T).T
            if i == mode:
                scores = np.where(keep[:, None], 0.0, W[i])
                W[i][~keep] = 0.0
                G[i][~keep] = 0.0
    return W, G, scores
