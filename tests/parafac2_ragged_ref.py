"""PARAFAC2 on slices of unequal length in numpy fp64: the reference of tests/parafac2_ragged_cases.py and
tests/test_parafac2_ragged_cpu.py, on top of tests/parafac2_ref.py.

The data is a list of K matrices X_k (rows[k] x J), X_k ~ P_k B diag(C[k]) A^T with P_k^T P_k = I; P is a list of
K arrays rows[k] x R, Y is R x J x K as in the equal-length reference."""
import numpy as np

import parafac2_ref as ref

# the step-values tables of the GPU cases: (rows, J, R)
TABLES = (((3, 64, 65, 17, 130), 17, 3), ((5, 5), 5, 5), ((40,), 9, 2), ((33, 96, 64), 70, 33),
          ((17, 129, 20), 130, 17), ((64, 200, 65), 64, 64))
EQUAL = (((23,) * 5, 17, 3), ((65, 65), 96, 33))      # equal rows: the bits of the equal-length path
FAILED = ((9, 12, 7), 8, 3)                           # a zero slice and a rank-deficient slice
DRIVER = ((30, 22, 41, 30, 18, 35), 20, 3)
LAYOUTS = ("packed", "stacked", "padded")
MIN_RATIO = 2.0 ** -20                                # the singular-value rule of parafac2_ref.step


def cap(R):
    """the condition the inputs of a case are held to"""
    return ref.KAPPA_CAP if R <= 16 else ref.KAPPA_WIDE_CAP


def identity_projections(rows, R):
    out = []
    for n in rows:
        P = np.zeros((n, R))
        P[np.arange(R), np.arange(R)] = 1.0
        out.append(P)
    return out


def q_slices(slices, B, A, C):
    """Q_k = X_k A diag(C[k]) B^T, a list of rows[k] x R arrays"""
    return [X @ (A * C[k]) @ B.T for k, X in enumerate(slices)]


def kappas(slices, B, A, C):
    """the 2-norm condition number of every Q_k (inf for a slice the step's rule refuses)"""
    out = []
    for Q in q_slices(slices, B, A, C):
        s = np.linalg.svd(Q, compute_uv=False)
        out.append(np.inf if not np.all(np.isfinite(s)) or s[-1] <= s[0] * MIN_RATIO else s[0] / s[-1])
    return np.array(out)


def step_ragged(slices, B, A, C, P_prev=None):
    """one projection step: (P, Y, lost_sq, failed). A slice whose Q_k fails the rule of parafac2_ref.step keeps
    P_prev[k] (the first R identity columns without P_prev) and counts in failed."""
    R = A.shape[1]
    P = identity_projections([X.shape[0] for X in slices], R) if P_prev is None else [np.array(p, dtype=np.float64)
                                                                                      for p in P_prev]
    failed = 0
    for k, Q in enumerate(q_slices(slices, B, A, C)):
        s = np.linalg.svd(Q, compute_uv=False)
        if not np.all(np.isfinite(s)) or s[-1] <= s[0] * MIN_RATIO:
            failed += 1
        else:
            P[k] = ref.polar(Q)
    Y = np.stack([P[k].T @ X for k, X in enumerate(slices)], axis=2)
    xx = float(sum(np.sum(X * X) for X in slices))
    return P, Y, xx - float(np.sum(Y * Y)), failed


def model(P, B, A, C):
    """the list of model slices P_k B diag(C[k]) A^T"""
    return [P[k] @ (B * C[k]) @ A.T for k in range(len(P))]


def loss(slices, P, B, A, C):
    return float(sum(np.sum((X - M) ** 2) for X, M in zip(slices, model(P, B, A, C))))


def fit(slices, B, A, C, n_iter, inner_sweeps=1):
    """parafac2_ref.fit on a list of slices: (P, B, A, C, losses)"""
    P, losses = None, []
    for _ in range(n_iter):
        P, Y, lost, _ = step_ragged(slices, B, A, C, P)
        losses.append(lost + float(np.sum((Y - ref.cp_model(B, A, C)) ** 2)))
        for _ in range(inner_sweeps):
            B, A, C = ref.als_sweep(Y, B, A, C)
    P, Y, lost, _ = step_ragged(slices, B, A, C, P)
    losses.append(lost + float(np.sum((Y - ref.cp_model(B, A, C)) ** 2)))
    return P, B, A, C, losses


def planted_ragged(rows, J, R, seed, noise=0.0):
    """a planted model on slices of rows[k] rows: random orthonormal P_k; A, C, B as parafac2_ref.planted draws
    them for R <= 16 and as parafac2_ref.planted_wide for larger ranks (J >= R there). noise is relative to the
    norm over all slices. Returns (slices, P, B, A, C)."""
    rng = np.random.default_rng(seed)
    K = len(rows)
    P = [np.linalg.qr(rng.standard_normal((n, R)))[0] for n in rows]
    if R <= 16:
        A = rng.uniform(0.1, 1.0, (J, R))
        C = rng.uniform(0.5, 1.5, (K, R))
        B = np.eye(R) + 0.3 * rng.uniform(-1.0, 1.0, (R, R))
    else:
        A = np.linalg.qr(rng.standard_normal((J, R)))[0] * rng.uniform(0.5, 1.5, R)
        C = rng.uniform(0.5, 1.5, (K, R))
        B = np.eye(R) + 0.3 / np.sqrt(R) * rng.uniform(-1.0, 1.0, (R, R))
    slices = model(P, B, A, C)
    if noise:
        E = [rng.standard_normal(X.shape) for X in slices]
        f = noise * np.sqrt(sum(np.sum(X * X) for X in slices) / sum(np.sum(e * e) for e in E))
        slices = [X + f * e for X, e in zip(slices, E)]
    return slices, P, B, A, C


def step_case_ragged(rows, J, R, seed):
    """noisy planted data and factors near, not at, the planted ones (parafac2_ref.step_case / step_case_wide)"""
    slices, _, B, A, C = planted_ragged(rows, J, R, seed, noise=0.05)
    rng = np.random.default_rng(seed + 1000)
    if R <= 16:
        B = B + 0.05 * rng.standard_normal(B.shape)
        A = A + 0.05 * rng.uniform(0.0, 1.0, A.shape)
    else:
        B = B + 0.05 / np.sqrt(R) * rng.standard_normal(B.shape)
        A = A + 0.05 / np.sqrt(J) * rng.standard_normal(A.shape)
    C = C + 0.05 * rng.uniform(0.0, 1.0, C.shape)
    return slices, B, A, C


# the seeds of the cases; test_parafac2_ragged_cpu.py shows that every input stays under cap(R)
def values_inputs(t):
    rows, J, R = TABLES[t]
    return step_case_ragged(rows, J, R, 500 + t)


def truth_inputs(t):
    rows, J, R = TABLES[t]
    return planted_ragged(rows, J, R, 540 + t)


def equal_inputs(t):
    rows, J, R = EQUAL[t]
    return step_case_ragged(rows, J, R, 560 + t)


def failed_inputs():
    """slice 0 all zero, slice 2 of exact rank R - 1 (entries exact in fp32, as failed_slice_inputs of
    parafac2_cases_inputs.py builds them)"""
    rows, J, R = FAILED
    slices, B, A, C = step_case_ragged(rows, J, R, 580)
    slices[0] = np.zeros_like(slices[0])
    rng = np.random.default_rng(581)
    L = rng.integers(-1, 2, (rows[2], R - 1)).astype(np.float64)
    M = np.round(rng.uniform(-1.0, 1.0, (R - 1, J)) * 256.0) / 256.0
    slices[2] = 0.125 * (L @ M)
    return slices, B, A, C


def driver_inputs():
    rows, J, R = DRIVER
    slices = planted_ragged(rows, J, R, 590, noise=0.05)[0]
    return (slices,) + ref.start_factors(J, len(rows), R, 591)


def zero_pad(slices):
    """the slices zero-padded to the longest, as an I_max x J x K array, first index fastest"""
    I = max(X.shape[0] for X in slices)
    out = np.zeros((I, slices[0].shape[1], len(slices)), order="F")
    for k, X in enumerate(slices):
        out[:X.shape[0], :, k] = X
    return out


def pack(slices, layout, dtype=np.float64):
    """the slices in one flat buffer: (buffer, offsets, col_strides) in elements, X_k[i, j] at
    offsets[k] + i + col_strides[k] j.
      packed   each slice column-major, one after another (what NULL offsets and strides mean)
      stacked  the N x J column-major matrix of the slices stacked on top of each other
      padded   column strides of rows[k] + 3, five elements between slices and two in front, NaN in every element
               no slice owns"""
    rows = [X.shape[0] for X in slices]
    J, N = slices[0].shape[1], sum(rows)
    if layout == "packed":
        cs = list(rows)
        off = [J * o for o in np.cumsum([0] + rows[:-1])]
        size = N * J
    elif layout == "stacked":
        cs = [N] * len(rows)
        off = [int(o) for o in np.cumsum([0] + rows[:-1])]
        size = N * J
    elif layout == "padded":
        cs = [n + 3 for n in rows]
        off, o = [], 2
        for c in cs:
            off.append(o)
            o += c * J + 5
        size = o
    else:
        raise ValueError(layout)
    buf = np.full(size, np.nan, dtype=dtype)
    for X, o, c in zip(slices, off, cs):
        n = X.shape[0]
        idx = o + np.arange(n)[:, None] + c * np.arange(J)[None, :]
        buf[idx] = X
    return buf, [int(o) for o in off], [int(c) for c in cs]


def unpack(buf, offsets, col_strides, rows, J):
    """the slices a flat buffer holds, as fp64"""
    return [np.asarray(buf[o + np.arange(n)[:, None] + c * np.arange(J)[None, :]], dtype=np.float64)
            for o, c, n in zip(offsets, col_strides, rows)]
