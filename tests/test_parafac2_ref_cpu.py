"""Self-tests of tests/parafac2_ref.py, the numpy reference of the PARAFAC2 GPU cases: the polar factor, the
loss identity, the monotone loss, and the condition numbers of every GPU case's inputs (the caps the GPU
tolerances rely on are shown here, on the CPU)."""
import numpy as np
import pytest

import parafac2_ref as ref


def test_polar_factor_is_orthonormal_and_maximises_the_trace():
    rng = np.random.default_rng(0)
    for I, R in ((9, 4), (40, 17), (70, 2)):
        Q = rng.standard_normal((I, R)) @ rng.standard_normal((R, R))
        P = ref.polar(Q)
        assert np.abs(P.T @ P - np.eye(R)).max() < 1e-13
        H = P.T @ Q                                     # symmetric positive definite: Q = P H
        assert np.abs(H - H.T).max() < 1e-12 * np.abs(H).max() and np.linalg.eigvalsh((H + H.T) / 2).min() > 0
        G = Q.T @ Q                                     # the Gram route gives the same factor
        w, V = np.linalg.eigh(G)
        assert np.abs(Q @ (V / np.sqrt(w)) @ V.T - P).max() < 1e-10
        for _ in range(5):
            O = np.linalg.qr(rng.standard_normal((I, R)))[0]
            assert np.trace(O.T @ Q) <= np.trace(H) + 1e-12


@pytest.mark.parametrize("shape", ref.SHAPES)
def test_loss_identity(shape):
    X, B, A, C = ref.step_case(shape, 7)
    P, Y, lost, failed = ref.step(X, B, A, C)
    assert failed == 0
    inner = float(np.sum((Y - ref.cp_model(B, A, C)) ** 2))
    total = ref.loss(X, P, B, A, C)
    assert abs(lost + inner - total) <= 1e-12 * np.sum(X * X)
    assert lost >= -1e-12 * np.sum(X * X)


@pytest.mark.parametrize("shape", ref.SHAPES + (ref.DRIVER,))
def test_loss_never_rises(shape):
    I, J, K, R = shape
    X = ref.planted(I, J, K, R, 11, noise=0.05)[0]
    losses = ref.fit(X, *ref.start_factors(J, K, R, 12), 30)[4]
    xx = float(np.sum(X * X))
    assert all(b <= a + 1e-12 * xx for a, b in zip(losses, losses[1:])), losses
    assert losses[-1] < losses[0]


def test_exact_projections_at_the_truth():
    for shape in ref.SHAPES:
        I, J, K, R = shape
        X, P0, B, A, C = ref.planted(I, J, K, R, 3)
        P, _, lost, failed = ref.step(X, B, A, C)
        assert failed == 0 and np.abs(P - P0).max() < 1e-9 and abs(lost) <= 1e-12 * np.sum(X * X)


def test_a_zero_slice_keeps_its_projection():
    X, B, A, C = ref.step_case(ref.SHAPES[0], 5)
    X[:, :, 2] = 0.0
    P, Y, _, failed = ref.step(X, B, A, C)
    assert failed == 1 and np.array_equal(P[2], ref.identity_projections(23, 5, 3)[2]) and not Y[:, :, 2].any()


def test_condition_numbers_of_every_gpu_case_stay_below_the_cap():
    import parafac2_cases_inputs as inputs
    for name, (X, B, A, C) in inputs.all_step_inputs():
        kap = ref.kappas(X, B, A, C)
        finite = kap[np.isfinite(kap)]
        assert finite.size >= kap.size - 1, name          # (only the zero-slice case has a slice without rank)
        assert finite.max() <= ref.KAPPA_CAP, (name, finite.max())
    X, B, A, C = inputs.driver_inputs()
    assert ref.kappas(X, B, A, C).max() <= 500.0


def test_the_driver_case_has_something_to_do():
    """the reference's loss at the first look (a step from the start, no sweep yet) is several times its loss
    after twenty iterations, so a driver that does nothing cannot pass the GPU case that compares with it"""
    import parafac2_cases_inputs as inputs
    X, B, A, C = inputs.driver_inputs()
    losses = ref.fit(X, B, A, C, 20)[4]
    xx = float(np.sum(X * X))
    print("driver reference: loss / ||X||^2 at the first look, after 1 and after 20 iterations:",
          losses[0] / xx, losses[1] / xx, losses[20] / xx)
    assert losses[20] < 0.5 * losses[0] and losses[20] < 0.01 * xx
