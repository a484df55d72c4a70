"""N-PLS as the paper states it (Bro, J. Chemometrics 10 (1996) 47-61; `npls` of the N-way toolbox), numpy fp64:
the DEFLATING algorithm. It copies X, subtracts t o W after every component, and goes through the (deflated) tensor in
every round of the loop u -> Z -> w -> t -> q -> u. Deliberately the other formulation than the engine's, which never
deflates: the two agree to rounding, and that is what the tests assert.

Shared with the engine are only the conventions of include/ppals.h: q starts at the column of Y_res with the largest
sum of squares; the rank-one step is numpy.linalg.svd for a matrix Z and alternating power iterations, started from
the fibres through the entry of largest magnitude (first in memory order, first index fastest), otherwise; every weight
vector has unit norm, the entry of largest magnitude of all but the last is positive and the last makes <Z, W>
positive; B[:f+1, f] = (T^T T)^-1 T^T u_f."""
import numpy as np


def outer(ws):
    W = ws[0]
    for w in ws[1:]:
        W = np.multiply.outer(W, w)
    return W


def mode_product(Z, ws, k):
    """Z contracted with ws over every mode but k"""
    v = Z
    for j in reversed(range(Z.ndim)):
        if j != k:
            v = np.tensordot(v, ws[j], axes=(j, 0))
    return v


def fix_signs(Z, ws):
    ws = [w.copy() for w in ws]
    for k in range(len(ws) - 1):
        if ws[k][np.argmax(np.abs(ws[k]))] < 0:
            ws[k] = -ws[k]
    if len(ws) > 1 and float(np.tensordot(Z, outer(ws), axes=Z.ndim)) < 0:
        ws[-1] = -ws[-1]
    return ws


def rank_one(Z, hopm_tol=1e-12, hopm_max=500, svd=True):
    """(unit vectors or None for a zero / non-finite Z, rounds, capped)"""
    if not np.all(np.isfinite(Z)) or not np.any(Z):
        return None, 0, False
    if Z.ndim == 1:
        return [Z / np.linalg.norm(Z)], 0, False
    if Z.ndim == 2 and svd:
        u, _, vt = np.linalg.svd(Z)
        return fix_signs(Z, [u[:, 0], vt[0]]), 0, False
    p = np.unravel_index(np.argmax(np.abs(Z).ravel(order="F")), Z.shape, order="F")
    ws = []
    for k in range(Z.ndim):
        idx = list(p)
        idx[k] = slice(None)
        v = Z[tuple(idx)]
        ws.append(v / np.linalg.norm(v))
    rounds, settled = 0, False
    while rounds < hopm_max and not settled:
        moved = 0.0
        for k in range(Z.ndim):
            v = mode_product(Z, ws, k)
            v = v / np.linalg.norm(v)
            moved = max(moved, float(np.max(np.abs(v - ws[k]))))
            ws[k] = v
        rounds += 1
        settled = moved <= hopm_tol
    return fix_signs(Z, ws), rounds, not settled


def fit(X, Y, F, mode=0, hopm_tol=1e-12, hopm_max=500, inner_tol=1e-12, inner_max=200, svd=True):
    """dict: T, U (I x F), W (a list of lens x F), Q (M x F), B (F x F), ssx, ssy, status, hopm_rounds, inner_rounds"""
    X = np.asarray(X, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64).reshape(X.shape[mode], -1)
    Xres = np.array(np.moveaxis(X, mode, 0))  # the copy that is deflated
    I, ext, M = Xres.shape[0], Xres.shape[1:], Y.shape[1]
    K = len(ext)
    Yres = Y.copy()
    T, U, Q, B = np.zeros((I, F)), np.zeros((I, F)), np.zeros((M, F)), np.zeros((F, F))
    W = [np.zeros((n, F)) for n in ext]
    ssx, ssy, status, hr, ir = [], [], [], 0, 0
    nx, ny = np.sum(X * X), np.sum(Y * Y)
    f = 0
    while f < F:
        best = int(np.argmax(np.sum(Yres * Yres, axis=0)))
        q = np.zeros(M)
        q[best] = 1.0
        u = Yres[:, best].copy()
        st, ws, rounds = 0, None, 0
        while True:
            Z = np.tensordot(u, Xres, axes=(0, 0))
            ws, r, capped = rank_one(Z, hopm_tol, hopm_max, svd)
            if ws is None:
                break
            hr = max(hr, r)
            st = (st & ~1) | int(capped)
            Wf = outer(ws)
            t = np.tensordot(Xres, Wf, axes=(list(range(1, K + 1)), list(range(K))))
            qn = Yres.T @ t
            nq = np.linalg.norm(qn)
            if not nq > 0:
                ws = None
                break
            qn = qn / nq
            moved = float(np.max(np.abs(qn - q)))
            q = qn
            rounds += 1
            if M == 1 or moved <= inner_tol:
                break
            if rounds >= inner_max:
                st |= 2
                break
            u = Yres @ q
        if ws is None:
            break
        ir = max(ir, rounds)
        T[:, f], Q[:, f] = t, q
        U[:, f] = Yres @ q
        for k in range(K):
            W[k][:, f] = ws[k]
        Tf = T[:, :f + 1]
        B[:f + 1, f] = np.linalg.solve(Tf.T @ Tf, Tf.T @ U[:, f])
        Xres -= np.multiply.outer(t, Wf)
        Yres = Y - Tf @ B[:f + 1, :f + 1] @ Q[:, :f + 1].T
        ssx.append(1.0 - np.sum(Xres * Xres) / nx)
        ssy.append(1.0 - np.sum(Yres * Yres) / ny)
        status.append(st)
        f += 1
    return dict(T=T[:, :f], U=U[:, :f], W=[w[:, :f] for w in W], Q=Q[:, :f], B=B[:f, :f], ssx=np.array(ssx),
                ssy=np.array(ssy), status=np.array(status, dtype=np.int64), hopm_rounds=hr, inner_rounds=ir, mode=mode,
                Yres=Yres)


def predict(model, Xnew, ncomp=None):
    """(Yhat, T_new) by deflating the new samples component after component"""
    k = model["T"].shape[1] if ncomp is None else ncomp
    Xr = np.array(np.moveaxis(np.asarray(Xnew, dtype=np.float64), model["mode"], 0))
    K = Xr.ndim - 1
    T = np.zeros((Xr.shape[0], k))
    for f in range(k):
        Wf = outer([w[:, f] for w in model["W"]])
        T[:, f] = np.tensordot(Xr, Wf, axes=(list(range(1, K + 1)), list(range(K))))
        Xr -= np.multiply.outer(T[:, f], Wf)
    return T @ model["B"][:k, :k] @ model["Q"][:, :k].T, T
