"""numpy fp64 reference of robust CP (ppals_cp_huber_device / ppals_cp_robust / ppals_cp_abs_residual_quantile,
include/ppals.h): Huber's function, the majorization step with its loss and clipped count, the majorizer, the
MM-ALS loop built on them, and the quantile of the absolute residuals, implemented literally."""
import math

import numpy as np

from wls_ref import als_sweep, cp_model  # noqa: F401  (cp_model is part of this module's surface)


def rho(r, c):
    """Huber's function scaled so that its quadratic part is r^2: r^2 for |r| <= c, c (2 |r| - c) otherwise"""
    a = np.abs(np.asarray(r, dtype=np.float64))
    if not np.isfinite(c):
        return a * a
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(a > c, c * (2.0 * a - c), a * a)


def step(x, h, m, c):
    """the per-element rule: (z, loss, clipped). h=None: weight 1 everywhere. !(h > 0): z = m, loss 0, x is not
    looked at; !(|x - m| > c): the weighted rule (z = x where h >= 1, else m + h (x - m), loss min(h, 1) (x - m)^2);
    otherwise z = m + min(h, 1) copysign(c, x - m), loss min(h, 1) c (2 |x - m| - c), counted as clipped"""
    x, m = np.asarray(x, dtype=np.float64), np.asarray(m, dtype=np.float64)
    h = np.ones_like(m) if h is None else np.asarray(h, dtype=np.float64)
    x, h, m = np.broadcast_arrays(x, h, m)
    off = ~(h > 0)                  # h <= 0 or NaN
    full = h >= 1
    w = np.where(off, 0.0, np.where(full, 1.0, h))
    xs = np.where(off, m, x)        # never look at x where the weight is off
    d = xs - m
    clip = np.abs(d) > c            # (never where off: d = 0 there; never for a NaN)
    dq = np.where(clip, 0.0, d)     # the quadratic branch's residual
    z = np.where(off, m, np.where(full, xs, m + np.where(off | full, 0.0, h) * dq))
    per = w * dq * dq
    if clip.any():
        cc = float(c)               # (finite: something exceeds it)
        z = np.where(clip, m + w * np.copysign(cc, d), z)
        with np.errstate(invalid="ignore"):
            per = np.where(clip, w * (cc * (2.0 * np.where(clip, np.abs(d), cc) - cc)), per)
    return z, float(np.sum(per)), int(np.count_nonzero(clip))


def loss(x, h, m, c):
    return step(x, h, m, c)[1]


def majorizer(x, h, m0, m, c):
    """sum (z - m)^2 + const(m0), z = step(x, h, m0, c): >= loss(x, h, m, c) for every m, equality at m = m0.
    const(m0) = loss(m0) - sum (z - m0)^2"""
    z, l0, _ = step(x, h, m0, c)
    return float(np.sum((z - m) ** 2) + (l0 - np.sum((z - m0) ** 2)))


def mm_als(x, h, W0, iters, c, inner_sweeps=1, store=None, look=None):
    """iters iterations of { Z = step(x, h, model, c); inner_sweeps ALS sweeps on Z } from the factors W0.
    store: a function rounding Z to a storage type (None: fp64). look(k, loss, clipped): called with the Huber
    loss of the factors iteration k starts from. Returns (factors, final loss)."""
    W = [np.array(w, dtype=np.float64) for w in W0]
    for k in range(iters):
        z, l, n = step(x, h, cp_model(W), c)
        if look:
            look(k, l, n)
        if store:
            z = store(z)
        for _ in range(inner_sweeps):
            als_sweep(z, W)
    return W, loss(x, h, cp_model(W), c)


def quantile(x, h, m, p):
    """(value, count): over the elements with h > 0 (all with h=None), a = float32(|x - m|), NaN sorted last;
    count = n, k = min(n - 1, max(0, ceil(p n) - 1)), value = the k-th smallest a as a Python float; (nan, 0)
    for n = 0"""
    x, m = np.asarray(x, dtype=np.float64), np.asarray(m, dtype=np.float64)
    x, m = np.broadcast_arrays(x, m)
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.abs(x - m).astype(np.float32)
    if h is not None:
        a = a[np.broadcast_to(np.asarray(h, dtype=np.float64), a.shape) > 0]
    a = np.sort(a.ravel())          # (numpy sorts NaN to the end)
    n = a.size
    if n == 0:
        return float("nan"), 0
    k = min(n - 1, max(0, math.ceil(p * n) - 1))
    return float(a[k]), n
