"""The inputs of the PARAFAC2 GPU cases (tests/parafac2_cases.py), numpy only, so that
tests/test_parafac2_ref_cpu.py can show on the CPU that they stay within the caps the GPU tolerances rely on."""
import parafac2_ref as ref


def values_inputs(i):
    """step values, shape i: noisy planted data, factors near the planted ones"""
    return ref.step_case(ref.SHAPES[i], 20 + i)


def truth_inputs(i):
    """noise-free planted data with the planted factors: (X, B, A, C, P)"""
    I, J, K, R = ref.SHAPES[i]
    X, P, B, A, C = ref.planted(I, J, K, R, 40 + i)
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
