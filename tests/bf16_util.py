"""The bf16 rounding of PPALS_BF16 storage in numpy (no torch): fp64 -> fp32 round-to-nearest-even, then
fp32 -> bf16 round-to-nearest-even — what torch's float64 -> bfloat16 cast does. Shared by the bf16
tests."""
import numpy as np


def bf16_bits(x):
    """the bf16 bit patterns (uint16) of x rounded as the tensor stores it; NaN -> quiet NaN"""
    with np.errstate(over="ignore"):
        f = np.asarray(x, dtype=np.float64).astype(np.float32)
    u = f.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = np.isnan(f)
    r[nan] = ((u[nan] >> 16) | 0x40).astype(np.uint16)
    return r


def bf16_round(x):
    """x rounded to bf16 as the tensor stores it, as float64 (exact)"""
    b = bf16_bits(x).astype(np.uint32) << 16
    return b.view(np.float32).astype(np.float64).reshape(np.shape(x))


def same_values(a, b):
    """bitwise equality of two fp64 arrays, NaNs compared as NaNs"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(
        a[~na].view(np.uint64), b[~nb].view(np.uint64))
