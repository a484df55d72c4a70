"""numpy fp64 reference of CP with element weights (ppals_cp_wls_device / ppals_cp_wls, include/ppals.h):
Kiers' majorization step, the weighted loss, and the MM-ALS loop built on them."""
import numpy as np

LET = "abcdefgh"


def cp_model(W):
    N = len(W)
    return np.einsum(",".join(f"{LET[i]}z" for i in range(N)) + "->" + LET[:N], *W, optimize=True)


def step(x, h, m):
    """the per-element rule: (z, loss). h >= 1: z = x, (x - m)^2; h <= 0 or NaN: z = m, 0 (x is not looked
    at and may be NaN or Inf); else z = m + h (x - m), h (x - m)^2"""
    x, h, m = (np.asarray(v, dtype=np.float64) for v in (x, h, m))
    x, h, m = np.broadcast_arrays(x, h, m)
    off = ~(h > 0)                  # h <= 0 or NaN
    full = h >= 1
    xs = np.where(off, m, x)        # never look at x where the weight is off
    d = xs - m
    z = np.where(off, m, np.where(full, xs, m + np.where(off | full, 0.0, h) * d))
    w = np.where(off, 0.0, np.where(full, 1.0, h))
    return z, float(np.sum(w * d * d))


def loss(x, h, m):
    return step(x, h, m)[1]


def majorizer(x, h, m0, m):
    """sum (z - m)^2 + sum h (1 - h) (x - m0)^2 with z = step(x, h, m0), h clipped to [0, 1]: >= loss(x, h, m)
    for every m, with equality at m = m0"""
    z, _ = step(x, h, m0)
    hc = np.where(h > 0, np.minimum(h, 1.0), 0.0)
    d0 = np.where(hc > 0, x, m0) - m0
    return float(np.sum((z - m) ** 2) + np.sum(hc * (1 - hc) * d0 * d0))


def unfold(T, n):
    return np.moveaxis(T, n, 0).reshape(T.shape[n], -1)


def khatri_rao_rest(W, n):
    """rows ordered like unfold(., n): the remaining modes in order, the last fastest"""
    out = None
    for i, w in enumerate(W):
        if i == n:
            continue
        out = w if out is None else (out[:, None, :] * w[None, :, :]).reshape(-1, w.shape[1])
    return out


def als_sweep(T, W):
    """one exact ALS sweep on T, in place on the list W (no normalisation: the model is what matters)"""
    for n in range(len(W)):
        G = np.ones((W[0].shape[1],) * 2)
        for i, w in enumerate(W):
            if i != n:
                G = G * (w.T @ w)
        W[n] = np.linalg.solve(G, (unfold(T, n) @ khatri_rao_rest(W, n)).T).T
    return W


def mm_als(x, h, W0, iters, inner_sweeps=1, store=None, look=None):
    """iters iterations of { Z = step(x, h, model); inner_sweeps ALS sweeps on Z } from the factors W0.
    store: a function rounding Z to a storage type (None: fp64). look(k, loss): called with the weighted loss
    of the factors iteration k starts from. Returns (factors, final loss)."""
    W = [np.array(w, dtype=np.float64) for w in W0]
    for k in range(iters):
        z, l = step(x, h, cp_model(W))
        if look:
            look(k, l)
        if store:
            z = store(z)
        for _ in range(inner_sweeps):
            als_sweep(z, W)
    return W, loss(x, h, cp_model(W))
