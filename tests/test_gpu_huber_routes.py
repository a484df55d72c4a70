"""Ops::model_wls, Ops::model_huber and Ops::model_absres_hist of the HIP back end at the op level
(tests/huber_shim: the ops on host arrays under the simplest plan, with their route logs): the Huber step is
logged as model.huber.*, without a weights view as model.huber.*.now, the histogram pass as
model.absres_hist.*, and a weighted step in the same process still as model.wls.* with the LDS it had; with
c = inf the Huber step stores the weighted step's bytes and returns its loss, and without weights it stores
the data. Reference: tests/huber_ref.py on numpy's fp64 Q P^T."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import huber_ref

pytestmark = pytest.mark.gpu

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "huber_shim")
BINS = 2048


@pytest.fixture(scope="module")
def shim():
    subprocess.check_call(["make", "-s", "-C", DIR])
    lib = C.CDLL(os.path.join(DIR, "build", "libhuber_shim.so"))
    lib.huber_shim_error.restype = C.c_char_p
    lib.huber_shim_run.restype = C.c_int
    lib.huber_shim_run.argtypes = [C.c_int64, C.c_int64, C.c_int] + [C.c_void_p] * 5 + [C.c_double] + \
        [C.c_void_p] * 3 + [C.c_char_p, C.c_int]
    yield lib
    lib.huber_shim_close()


def run(shim, A, B, K, c, seed=3):
    g = np.random.default_rng(seed)
    Q, P = np.asfortranarray(g.uniform(0, 1, (A, K))), np.asfortranarray(g.uniform(0, 1, (B, K)))
    M, absM = Q @ P.T, np.abs(Q) @ np.abs(P).T
    X = (M + g.normal(size=(A, B))).astype(np.float32)
    H = g.uniform(0.01, 0.99, (A, B)).astype(np.float32)
    u = g.uniform(size=(A, B))
    H[u < 0.1] = 0.0
    H[u > 0.8] = 1.0
    V0 = g.uniform(0.5, 1.5, (A, B)).astype(np.float32)
    f = [np.asfortranarray(v) for v in (V0, X, H)]
    out = np.zeros((3, B, A), dtype=np.float32)          # each A x B, the first index fastest
    sums, hist = np.zeros(5), np.zeros((2, BINS), dtype=np.uint64)
    route = C.create_string_buffer(2048)
    rc = shim.huber_shim_run(A, B, K, f[0].ctypes.data, f[1].ctypes.data, f[2].ctypes.data, Q.ctypes.data,
                             P.ctypes.data, c, out.ctypes.data, sums.ctypes.data, hist.ctypes.data, route, 2048)
    assert rc == 0, shim.huber_shim_error().decode()
    tags = route.value.decode().split("\n")
    print(f"[huber] op level A={A} B={B} K={K} c={c}: {tags}")
    return tags, out.transpose(0, 2, 1), sums, hist, (M, absM, X.astype(np.float64), H.astype(np.float64))


def lds_of(tag):
    return int(re.search(r"lds=(\d+)", tag).group(1))


@pytest.mark.parametrize("A,B,K", [(70, 130, 3), (128, 192, 10), (64, 64, 128)])
def test_routes_lds_values_and_histogram(shim, A, B, K):
    M0 = None
    for c in (None, float("inf")):
        if c is None:   # the median absolute residual: both branches are hit about equally
            _, _, _, _, (M0, _, X0, _) = run(shim, A, B, K, 1.0)
            c = float(np.median(np.abs(X0 - M0)))
        tags, out, sums, hist, (M, absM, X, H) = run(shim, A, B, K, c)
        assert len(tags) == 5, tags
        for tag, head in zip(tags, ("model.wls.f32.f32 K=", "model.huber.f32.f32 K=", "model.huber.f32.f32.now K=",
                                    "model.absres_hist.f32 K=", "model.absres_hist.f32.now K=")):
            assert tag.startswith(head + f"{K} flags="), (tag, head)
        base = 640 * 4 * ((K + 3) // 4) + 36352          # Q rows + the fp64 image + the offsets
        assert [lds_of(t) for t in tags] == [base, base, base, base + 4 * BINS, base + 4 * BINS], tags
        assert re.search(r"flags=(\d+)", tags[0]).group(1) == re.search(r"flags=(\d+)", tags[1]).group(1)
        on = H > 0
        mag = absM + np.abs(X)
        for i, h in ((1, H), (2, None)):
            z, loss, clipped = huber_ref.step(X, h, M, c)
            err = np.abs(out[i].astype(np.float64) - z)
            assert (err <= np.spacing(np.abs(z.astype(np.float32))).astype(np.float64) + 1e-13 * mag).all(), (i, err.max())
            sel = on if h is not None else np.ones_like(on)
            scale = float(np.sum((np.minimum(h, 1.0) if h is not None else 1.0) * sel * X * X))
            assert abs(sums[2 * i - 1] - loss) <= 1e-10 * scale, (i, sums, loss)
            a = np.abs(X - M)
            n_lo = int(np.count_nonzero(sel & (a > c + 1e-13 * mag)))
            n_hi = int(np.count_nonzero(sel & (a > c - 1e-13 * mag)))
            assert n_lo <= sums[2 * i] <= n_hi and sums[2 * i] == int(sums[2 * i]), (i, sums, n_lo, n_hi)
        if np.isinf(c):
            assert out[1].tobytes() == out[0].tobytes() and sums[1] == sums[0] and sums[2] == 0
            assert np.array_equal(out[2], X.astype(np.float32)) and sums[4] == 0
        else:
            assert 0.3 * on.sum() < sums[2] < 0.7 * on.sum()
        # the first histogram pass: every selected element once; bins as numpy's, but for the elements whose key
        # changes bin within the fp64 bar on the model
        a = np.abs(X - M)
        for i, sel in ((0, on), (1, np.ones_like(on))):
            assert int(hist[i].sum()) == int(sel.sum())
            key = lambda v: (np.maximum(v, 0.0).astype(np.float32).view(np.uint32) >> 20).astype(np.int64)
            want = np.bincount(key(a[sel]), minlength=BINS)
            unsure = int(np.count_nonzero(key((a - 1e-13 * mag)[sel]) != key((a + 1e-13 * mag)[sel])))
            assert int(np.abs(hist[i].astype(np.int64) - want).sum()) <= 2 * unsure, (i, unsure)
