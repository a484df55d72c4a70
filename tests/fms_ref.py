"""The factor congruence and the factor match score (include/ppals.h) in numpy, fp64 — the reference of
tests/test_fms_hostsim.py, tests/test_gpu_fms.py and tests/test_fms_cpu.py — and the bars those tests hold
the library to.

    Phi[p,q] = prod over compared modes i of (a_i[:,p] . b_i[:,q]) / (|a_i[:,p]| |b_i[:,q]|)
    w_a[p]   = prod over ALL modes of |a_i[:,p]|
    fms      = (1/m) max over injective matchings of m = min(ra, rb) pairs of sum score[p, pi(p)]

Bars (derived, not measured; u = 2^-53). A dot product of length s in any summation order errs by at most
gamma_s |x||y|, a cosine therefore by at most about (2s + 4) u, a product of at most N cosines of modulus
<= 1 by at most N times that; against a numpy reference with the same error the absolute bar on Phi is
    2 N (2 s_max + 8) u.
An fms without weights is a mean of entries of Phi: the same bar. With weights, add 8 N (s_max + 8) u for
the relative error of the norm products."""
import itertools

import numpy as np

U = 2.0 ** -53


def factors(lens, R, seed):
    """U(-1, 1): entries of both signs"""
    rng = np.random.default_rng(seed)
    return [np.asfortranarray(rng.uniform(-1.0, 1.0, (s, R))) for s in lens]


def bar_phi(lens):
    return 2.0 * len(lens) * (2.0 * max(lens) + 8.0) * U


def bar_fms(lens, weights=False):
    return bar_phi(lens) + (8.0 * len(lens) * (max(lens) + 8.0) * U if weights else 0.0)


def compared(N, skip_mode):
    return [i for i in range(N) if skip_mode is None or i != skip_mode]


def congruence(A, B, skip_mode=None):
    """Phi (Ca, Cb), w_a, w_b of two lists of factor matrices"""
    N = len(A)
    Ca, Cb = A[0].shape[1], B[0].shape[1]
    phi = np.ones((Ca, Cb))
    bad_a, bad_b = np.zeros(Ca, bool), np.zeros(Cb, bool)
    wa, wb = np.ones(Ca), np.ones(Cb)
    with np.errstate(all="ignore"):
        for i in range(N):
            na, nb = np.sqrt(np.sum(A[i] * A[i], axis=0)), np.sqrt(np.sum(B[i] * B[i], axis=0))
            wa, wb = wa * na, wb * nb
            if i not in compared(N, skip_mode):
                continue
            bad_a |= ~((na > 0) & np.isfinite(na))
            bad_b |= ~((nb > 0) & np.isfinite(nb))
            phi = phi * ((A[i].T @ B[i]) / na[:, None] / nb[None, :])
    phi[bad_a, :] = 0.0
    phi[:, bad_b] = 0.0
    return phi, wa, wb


def score(phi, wa, wb, weights):
    if not weights:
        return phi
    with np.errstate(all="ignore"):
        mx = np.maximum(wa[:, None], wb[None, :])
        f = 1.0 - np.abs(wa[:, None] - wb[None, :]) / mx
    ok = (mx > 0) & np.isfinite(mx) & np.isfinite(f)
    return np.where(ok, phi * np.where(ok, f, 0.0), 0.0)


def brute_force(sc):
    """(perm, total): the best injective matching of min(ra, rb) pairs by trying them all (ranks <= 5)"""
    ra, rb = sc.shape
    assert max(ra, rb) <= 5
    best, best_perm = -np.inf, None
    if ra <= rb:
        for cols in itertools.permutations(range(rb), ra):
            t = sum(sc[p, q] for p, q in enumerate(cols))
            if t > best:
                best, best_perm = t, list(cols)
    else:
        for rows in itertools.permutations(range(ra), rb):
            t = sum(sc[p, q] for q, p in enumerate(rows))
            if t > best:
                best = t
                best_perm = [-1] * ra
                for q, p in enumerate(rows):
                    best_perm[p] = q
    return np.array(best_perm), best


def fms(A, B, skip_mode=None, weights=False):
    phi, wa, wb = congruence(A, B, skip_mode)
    perm, total = brute_force(score(phi, wa, wb, weights))
    return total / min(phi.shape), perm


def hstack(starts):
    """the factors of several starts side by side, as a multi-start session holds them"""
    return [np.hstack([W[i] for W in starts]) for i in range(len(starts[0]))]
