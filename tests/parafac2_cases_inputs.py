"""The inputs of the PARAFAC2 GPU cases (tests/parafac2_cases.py, tests/parafac2_op_cases.py), numpy only, so that
tests/test_parafac2_ref_cpu.py can show on the CPU that they stay within the caps the GPU tolerances rely on."""
import numpy as np

import parafac2_ref as ref

ALL_SHAPES = ref.SHAPES + ref.SHAPES_WIDE      # the binding-level step-values cases 0..7


def values_inputs(i):
    """step values, shape i: noisy planted data, factors near the planted ones (5..7: the wide generator)"""
    if i < len(ref.SHAPES):
        return ref.step_case(ref.SHAPES[i], 20 + i)
    return ref.step_case_wide(ALL_SHAPES[i], 20 + i)


def truth_inputs(i):
    """noise-free planted data with the planted factors: (X, B, A, C, P)"""
    I, J, K, R = ALL_SHAPES[i]
    X, P, B, A, C = (ref.planted if i < len(ref.SHAPES) else ref.planted_wide)(I, J, K, R, 40 + i)
    return X, B, A, C, P


def zero_slice_inputs():
    X, B, A, C = ref.step_case(ref.SHAPES[0], 60)
    X[:, :, 3] = 0.0
    return X, B, A, C


def driver_inputs():
    I, J, K, R = ref.DRIVER
    X = ref.planted(I, J, K, R, 70, noise=0.05)[0]
    return (X,) + ref.start_factors(J, K, R, 71)


def all_step_inputs():
    for i in range(len(ref.SHAPES)):
        yield f"values {i}", values_inputs(i)
        yield f"truth {i}", truth_inputs(i)[:4]
    yield "zero slice", zero_slice_inputs()


def op_inputs(shape):
    """the op-level case of a shape (tests/parafac2_op_cases.py): (X, B, A, C)"""
    I, J, K, R = shape
    return ref.step_case_wide(shape, 300 + 7 * I + 3 * J + K + 11 * R)


FAILED_SHAPES = ((33, 33, 3, 33), (49, 64, 3, 49))     # K = 3 at three and at four rank tiles
FAILED_KINDS = ("zero", "rank")


def failed_slice_inputs(shape, kind):
    """the op-level case with slice 1 without a polar factor: all zero, or of exact rank R - 1 — the product of an
    I x (R - 1) matrix of entries -1, 0, 1 and an (R - 1) x J matrix of multiples of 2^-8 in [-1, 1], scaled by
    2^-3: every entry is a sum of at most 63 products of at most 10 bits, exact in fp32, so an f32 view holds a
    slice of that rank too"""
    I, J, K, R = shape
    X, B, A, C = op_inputs(shape)
    if kind == "zero":
        X[:, :, 1] = 0.0
    else:
        rng = np.random.default_rng(900 + R)
        L = rng.integers(-1, 2, (I, R - 1)).astype(np.float64)
        M = np.round(rng.uniform(-1.0, 1.0, (R - 1, J)) * 256.0) / 256.0
        X[:, :, 1] = 0.125 * (L @ M)
    return X, B, A, C


def all_wide_inputs():
    """every input that is held to KAPPA_WIDE_CAP: the binding-level cases 5..7 and the op-level table (the failed
    slice of a failed-slice case excepted: see test_parafac2_ref_cpu.py)"""
    for i in range(len(ref.SHAPES), len(ALL_SHAPES)):
        yield f"values {i}", values_inputs(i)
        yield f"truth {i}", truth_inputs(i)[:4]
    for shape in ref.OP_SWEEP + ref.OP_EDGES:
        yield f"op {shape}", op_inputs(shape)
    for shape in FAILED_SHAPES:
        for kind in FAILED_KINDS:
            yield f"op failed {kind} {shape}", failed_slice_inputs(shape, kind)
