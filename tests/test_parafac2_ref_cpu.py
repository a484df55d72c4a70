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


def test_condition_numbers_of_the_wide_inputs_stay_below_their_cap():
    """every op-level input (tests/parafac2_op_cases.py) and the binding-level cases 5..7, as fp64 values and
    rounded to fp32 (what an f32 view holds): KAPPA_WIDE_CAP is a condition on these inputs. A failed-slice case
    has exactly one slice outside it, slice 1, far on the other side of the status rule's threshold."""
    import parafac2_cases_inputs as inputs
    worst = 0.0
    for name, (X, B, A, C) in inputs.all_wide_inputs():
        for Xv in (X, X.astype(np.float32).astype(np.float64)):
            sv = [np.linalg.svd(((Xv[:, :, k] @ A) * C[k]) @ B.T, compute_uv=False) for k in range(Xv.shape[2])]
            with np.errstate(divide="ignore"):
                kap = np.array([s[0] / s[-1] if s[0] > 0 else np.inf for s in sv])
            if "failed" in name:
                assert not kap[1] ** -2.0 > 2.0 ** -45, (name, kap)
                kap = np.delete(kap, 1)
            assert np.all(np.isfinite(kap)) and kap.max() <= ref.KAPPA_WIDE_CAP, (name, kap)
            worst = max(worst, kap.max())
    print("the largest condition number of a wide input:", worst)
    for shape in inputs.FAILED_SHAPES:
        X1 = inputs.failed_slice_inputs(shape, "rank")[0][:, :, 1]
        assert np.array_equal(X1, X1.astype(np.float32)) and np.linalg.matrix_rank(X1) == shape[3] - 1


def test_the_wide_generator_keeps_the_loss_identity_and_the_truth():
    for shape in ref.SHAPES_WIDE:
        I, J, K, R = shape
        X, B, A, C = ref.step_case_wide(shape, 7)
        P, Y, lost, failed = ref.step(X, B, A, C)
        xx = np.sum(X * X)
        assert failed == 0 and abs(lost + np.sum((Y - ref.cp_model(B, A, C)) ** 2) - ref.loss(X, P, B, A, C)) <= 1e-12 * xx
        X, P0, B, A, C = ref.planted_wide(I, J, K, R, 3)
        P, _, lost, failed = ref.step(X, B, A, C)
        assert failed == 0 and np.abs(P - P0).max() < 1e-9 and abs(lost) <= 1e-12 * np.sum(X * X)


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
