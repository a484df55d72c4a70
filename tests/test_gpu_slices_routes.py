"""Ops::residual_slices of the HIP back end at the op level (tests/slices_shim: the op on host arrays, with
its route log): which kernel serves which shape — MODE 3 of k_rank_mfma with each of its instantiations,
k_slice_stream for what that does not take — and the walk in slabs, the two-level row fold of a pass of more
than 64 k-chunks included. Reference: numpy, fp64, on V as stored; bar: tests/slices_ref.py (relative 1e-9 per
entry: sums of non-negative fp64 terms, here at most 9000 a row)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bf16_util
import slices_ref as R

pytestmark = pytest.mark.gpu

F32, F64, BF16 = 0, 1, 3
DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "slices_shim")
NAMES = {F32: "F32", F64: "F64", BF16: "BF16"}


@pytest.fixture(scope="module")
def shim():
    subprocess.check_call(["make", "-s", "-C", DIR])
    lib = C.CDLL(os.path.join(DIR, "build", "libslices_shim.so"))
    lib.slices_shim_error.restype = C.c_char_p
    lib.slices_shim_run.restype = C.c_int
    lib.slices_shim_run.argtypes = [C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
    yield lib
    lib.slices_shim_close()


def _inputs(M, K, rank, dtype, seed=7):
    """(V as stored in fp64, its storage bytes, Q, P): V uniform on (0.5, 1), operands on (0, 1)"""
    rng = np.random.default_rng(seed)
    V = rng.uniform(0.5, 1.0, (M, K))
    if dtype == F32:
        raw = np.asfortranarray(V, dtype=np.float32)
        Vs = raw.astype(np.float64)
    elif dtype == BF16:
        raw = np.asfortranarray(bf16_util.bf16_bits(V))
        Vs = bf16_util.bf16_round(V)
    else:
        raw = np.asfortranarray(V)
        Vs = V
    return Vs, raw, np.asfortranarray(rng.uniform(0, 1, (M, rank))), np.asfortranarray(rng.uniform(0, 1, (K, rank)))


def run(shim, M, K, rank, dtype, cap=256 << 20, misalign=0):
    Vs, raw, Q, P = _inputs(M, K, rank, dtype)
    row, col, tot = np.zeros(M), np.zeros(K), np.zeros(1)
    route = C.create_string_buffer(1024)
    rc = shim.slices_shim_run(dtype, M, K, rank, raw.ctypes.data, Q.ctypes.data, P.ctypes.data, cap, misalign,
                              row.ctypes.data, col.ctypes.data, tot.ctypes.data, route, 1024)
    assert rc == 0, shim.slices_shim_error().decode()
    E2 = (Vs - Q @ P.T) ** 2
    tags = route.value.decode().split("\n")
    errs = [float(np.max(np.abs(row - E2.sum(1)) / E2.sum(1))), float(np.max(np.abs(col - E2.sum(0)) / E2.sum(0))),
            abs(tot[0] - E2.sum()) / E2.sum()]
    print(f"[slices] op level M={M} K={K} R={rank} {NAMES[dtype]} cap {cap}: {tags}; relative errors of rows, "
          f"columns, total {errs[0]:.2e} {errs[1]:.2e} {errs[2]:.2e} (bar {R.SS_RTOL:.0e})")
    assert max(errs) <= R.SS_RTOL
    assert abs(row.sum() - tot[0]) <= R.SUM_RTOL * tot[0] and abs(col.sum() - tot[0]) <= R.SUM_RTOL * tot[0]
    return tags, (row, col, tot)


# every instantiation of MODE 3: <MAXRB, REM> from R, as the residual chooses them
@pytest.mark.parametrize("dtype", [F32, F64], ids=NAMES.get)
@pytest.mark.parametrize("rank,rb,rem", [(3, 1, 0), (9, 2, 1), (10, 2, 2), (12, 3, 0), (13, 3, 1), (16, 4, 0),
                                         (17, 4, 1), (20, 5, 0), (32, 8, 0)])
def test_fused_route_and_its_instantiations(shim, rank, rb, rem, dtype):
    tags, _ = run(shim, 24, 84, rank, dtype)
    assert tags[0].startswith("slices_mfma:" + ("f32" if dtype == F32 else "f64")), tags
    assert f",R{rank},RB{rb},rem{rem}," in tags[0], tags


@pytest.mark.parametrize("M,K,rank,dtype,misalign", [
    (24, 84, 10, BF16, 0),    # bf16 storage
    (7, 30, 3, F32, 0),       # odd M
    (25, 30, 3, F64, 0),      # odd M
    (24, 84, 33, F32, 0),     # R above 32
    (24, 84, 70, F64, 0),     # R above 64: any-rank kernel
    (24, 84, 10, F32, 1),     # an unaligned shard
], ids=str)
def test_general_route(shim, M, K, rank, dtype, misalign):
    tags, _ = run(shim, M, K, rank, dtype, misalign=misalign)
    assert tags[0].startswith("slices_stream:"), tags


def _slabs(tags):
    m = [re.fullmatch(r"slices_slabs:(\d+)x(\d+)", t) for t in tags]
    m = [x for x in m if x]
    assert len(m) == 1, tags
    return int(m[0].group(1)), int(m[0].group(2))


@pytest.mark.parametrize("dtype", [F32, F64, BF16], ids=NAMES.get)
def test_many_chunks_fold_in_groups(shim, dtype):
    """M = 8, K = 9000: one row tile by 71 k-chunks of 8 column blocks on the fused route (groups of 2), by 282
    of 32 columns on the general one (groups of 5). Whole, and under a cap of one byte in slabs of ONE group
    each, the last a partial group: the same bits."""
    tags, free = run(shim, 8, 9000, 5, dtype)
    assert _slabs(tags) == (1, 1)
    assert tags[0].startswith("slices_stream:" if dtype == BF16 else "slices_mfma:"), tags
    chunks = int(re.search(r"chunks(\d+)", tags[0]).group(1))
    assert chunks > 64, tags
    G = (chunks + 63) // 64
    tags1, capped = run(shim, 8, 9000, 5, dtype, cap=1)
    assert _slabs(tags1) == (1, (chunks + G - 1) // G) and chunks % G != 0, (tags1, chunks, G)
    assert all(bf16_util.same_values(a, b) for a, b in zip(free, capped))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=NAMES.get)
def test_row_tiles_and_chunks_in_slabs(shim, dtype):
    """three row tiles by several chunks, one tile a slab when three do not fit: the same bits"""
    tags, free = run(shim, 528, 1200, 12, dtype)
    assert _slabs(tags) == (1, 1)
    chunks = int(re.search(r"chunks(\d+)", tags[0]).group(1))
    one_tile = 8 * (1200 + chunks * 256)
    tags1, capped = run(shim, 528, 1200, 12, dtype, cap=one_tile + 8 * 1024)
    assert _slabs(tags1) == (3, 1), tags1
    assert all(bf16_util.same_values(a, b) for a, b in zip(free, capped))
