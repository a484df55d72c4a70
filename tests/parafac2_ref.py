"""PARAFAC2 by direct fitting (Kiers, ten Berge & Bro 1999) in numpy fp64: the reference of
tests/parafac2_cases.py and tests/test_parafac2_ref_cpu.py.

X is I x J x K, X_k = X[:, :, k] ~ P_k B diag(C[k]) A^T with P_k^T P_k = I. P is kept as K x I x R."""
import numpy as np

U = 2.0 ** -52
# the shapes (I, J, K, R) of the GPU cases (tests/parafac2_cases.py) and the driver's
SHAPES = ((23, 17, 5, 3), (70, 9, 6, 2), (16, 130, 4, 5), (9, 7, 33, 4), (40, 33, 5, 17))
DRIVER = (30, 20, 12, 3)
KAPPA_CAP = 1e5
# the larger ranks (planted_wide / step_case_wide): the binding-level shapes, and the op-level table of
# tests/parafac2_op_cases.py — the rank sweep at (130, 70, 2) and the edges
SHAPES_WIDE = ((65, 96, 2, 33), (130, 70, 3, 49), (64, 64, 2, 64))
OP_SWEEP_RANKS = (2, 15, 16, 17, 32, 33, 48, 49, 63, 64)
OP_SWEEP = tuple((130, 70, 2, R) for R in OP_SWEEP_RANKS)
OP_EDGES = ((64, 64, 1, 64), (65, 64, 2, 64), (64, 65, 2, 64), (128, 96, 2, 64), (33, 33, 3, 33), (64, 130, 2, 33),
            (49, 64, 3, 49), (70, 49, 2, 49))
KAPPA_WIDE_CAP = 1e3          # a condition on the inputs of these cases: p_bound is at most 1.4e-8 under it


def identity_projections(I, K, R):
    P = np.zeros((K, I, R))
    P[:, np.arange(R), np.arange(R)] = 1.0
    return P


def q_slices(X, B, A, C):
    """Q_k = X_k A diag(C[k]) B^T as K x I x R"""
    return np.einsum("ijk,jr,kr,sr->kis", X, A, C, B)


def kappas(X, B, A, C):
    """the 2-norm condition number of every Q_k (inf for a slice without full column rank)"""
    out = []
    for Q in q_slices(X, B, A, C):
        s = np.linalg.svd(Q, compute_uv=False)
        out.append(np.inf if s[-1] == 0 else s[0] / s[-1])
    return np.array(out)


def polar(Q):
    """the orthonormal polar factor U V^T of a full-rank Q"""
    u, _, vt = np.linalg.svd(Q, full_matrices=False)
    return u @ vt


def step(X, B, A, C, P_prev=None):
    """one projection step: (P, Y, lost_sq, failed); P K x I x R, Y R x J x K. A slice whose Q_k has no full
    column rank keeps P_prev[k] (the first R identity columns without P_prev) and counts in failed."""
    I, J, K = X.shape
    R = A.shape[1]
    P = identity_projections(I, K, R) if P_prev is None else np.array(P_prev, dtype=np.float64)
    failed = 0
    for k, Q in enumerate(q_slices(X, B, A, C)):
        s = np.linalg.svd(Q, compute_uv=False)
        if not np.all(np.isfinite(s)) or s[-1] <= s[0] * 2.0 ** -20:   # theta_min <= theta_max 2^-40
            failed += 1
        else:
            P[k] = polar(Q)
    Y = np.einsum("kir,ijk->rjk", P, X)
    return P, Y, float(np.sum(X * X) - np.sum(Y * Y)), failed


def cp_model(B, A, C):
    return np.einsum("ir,jr,kr->ijk", B, A, C)


def model(P, B, A, C):
    """the I x J x K model: slice k is P_k B diag(C[k]) A^T"""
    return np.einsum("kis,sr,kr,jr->ijk", P, B, C, A)


def loss(X, P, B, A, C):
    return float(np.sum((X - model(P, B, A, C)) ** 2))


def khatri_rao(U1, U2):
    """column-wise Kronecker product, the rows of U2 fastest"""
    return np.einsum("ir,jr->ijr", U1, U2).reshape(-1, U1.shape[1])


def als_sweep(Y, B, A, C):
    """one unconstrained ALS sweep on Y (R x J x K) over the modes 0 (B), 1 (A), 2 (C), no normalisation"""
    R = A.shape[1]
    Y0 = Y.reshape(Y.shape[0], -1, order="F")                      # columns (j, k), j fastest
    B = np.linalg.solve((A.T @ A) * (C.T @ C), (Y0 @ khatri_rao(C, A)).T).T
    Y1 = np.transpose(Y, (1, 0, 2)).reshape(Y.shape[1], -1, order="F")
    A = np.linalg.solve((B.T @ B) * (C.T @ C), (Y1 @ khatri_rao(C, B)).T).T
    Y2 = np.transpose(Y, (2, 0, 1)).reshape(Y.shape[2], -1, order="F")
    C = np.linalg.solve((B.T @ B) * (A.T @ A), (Y2 @ khatri_rao(A, B)).T).T
    assert B.shape == (R, R)
    return B, A, C


def fit(X, B, A, C, n_iter, inner_sweeps=1):
    """n_iter iterations of { step; inner_sweeps sweeps }, then one last step: (P, B, A, C, losses), losses[t] the
    loss after the step of iteration t (n_iter + 1 entries), each lost_sq + ||Y - [[B, A, C]]||^2"""
    P, losses = None, []
    for _ in range(n_iter):
        P, Y, lost, _ = step(X, B, A, C, P)
        losses.append(lost + float(np.sum((Y - cp_model(B, A, C)) ** 2)))
        for _ in range(inner_sweeps):
            B, A, C = als_sweep(Y, B, A, C)
    P, Y, lost, _ = step(X, B, A, C, P)
    losses.append(lost + float(np.sum((Y - cp_model(B, A, C)) ** 2)))
    return P, B, A, C, losses


def planted(I, J, K, R, seed, noise=0.0):
    """a planted model: random orthonormal P_k, A in U(0.1, 1), C in U(0.5, 1.5), B = I + 0.3 U(-1, 1); noise is
    relative to ||X||. Returns (X, P, B, A, C), X first index fastest."""
    rng = np.random.default_rng(seed)
    P = np.stack([np.linalg.qr(rng.standard_normal((I, R)))[0] for _ in range(K)])
    A = rng.uniform(0.1, 1.0, (J, R))
    C = rng.uniform(0.5, 1.5, (K, R))
    B = np.eye(R) + 0.3 * rng.uniform(-1.0, 1.0, (R, R))
    X = model(P, B, A, C)
    if noise:
        E = rng.standard_normal(X.shape)
        X = X + noise * np.linalg.norm(X) / np.linalg.norm(E) * E
    return np.asfortranarray(X), P, B, A, C


def start_factors(J, K, R, seed):
    """the drivers' start: B = I, C = 1, A uniform"""
    return np.eye(R), np.random.default_rng(seed).uniform(0.0, 1.0, (J, R)), np.ones((K, R))


def step_case(shape, seed):
    """the inputs of a step-values case: noisy planted data and factors near, not at, the planted ones"""
    I, J, K, R = shape
    X, _, B, A, C = planted(I, J, K, R, seed, noise=0.05)
    rng = np.random.default_rng(seed + 1000)
    B = B + 0.05 * rng.standard_normal(B.shape)
    A = A + 0.05 * rng.uniform(0.0, 1.0, A.shape)
    C = C + 0.05 * rng.uniform(0.0, 1.0, C.shape)
    return X, B, A, C


def planted_wide(I, J, K, R, seed, noise=0.0):
    """a planted model whose Q_k stay well conditioned up to R = 64 (J >= R): random orthonormal P_k, A with
    orthogonal columns of lengths in U(0.5, 1.5), C in U(0.5, 1.5), B = I + 0.3 / sqrt(R) U(-1, 1); noise is
    relative to ||X||. Returns (X, P, B, A, C), X first index fastest."""
    rng = np.random.default_rng(seed)
    P = np.stack([np.linalg.qr(rng.standard_normal((I, R)))[0] for _ in range(K)])
    A = np.linalg.qr(rng.standard_normal((J, R)))[0] * rng.uniform(0.5, 1.5, R)
    C = rng.uniform(0.5, 1.5, (K, R))
    B = np.eye(R) + 0.3 / np.sqrt(R) * rng.uniform(-1.0, 1.0, (R, R))
    X = model(P, B, A, C)
    if noise:
        E = rng.standard_normal(X.shape)
        X = X + noise * np.linalg.norm(X) / np.linalg.norm(E) * E
    return np.asfortranarray(X), P, B, A, C


def step_case_wide(shape, seed):
    """step_case for the larger ranks: noisy planted_wide data, the factors moved off the planted ones by
    0.05 / sqrt(R) (B), 0.05 / sqrt(J) (A) and 0.05 U(0, 1) (C)"""
    I, J, K, R = shape
    X, _, B, A, C = planted_wide(I, J, K, R, seed, noise=0.05)
    rng = np.random.default_rng(seed + 1000)
    B = B + 0.05 / np.sqrt(R) * rng.standard_normal(B.shape)
    A = A + 0.05 / np.sqrt(J) * rng.standard_normal(A.shape)
    C = C + 0.05 * rng.uniform(0.0, 1.0, C.shape)
    return X, B, A, C


def p_bound(kappa):
    """the Gram route's error model for P_k: 64 kappa^2 2^-52"""
    return 64.0 * kappa ** 2 * U
