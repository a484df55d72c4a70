"""Pins tests/npls_ref.py, the deflating N-PLS of the paper that the engine is compared with: what it computes is
checked here against facts that do not depend on it."""
import numpy as np

import npls_cases as NC
import npls_ref


def test_matrix_case_is_pls1():
    """N = 2, M = 1: the weights are the normalised X_res^T y_res of the deflated matrix, component after component,
    y_res the residual of regressing y on the scores so far"""
    X, y, _ = NC.planted([15, 9], 1, seed=11)
    m = npls_ref.fit(X, y, 3, 0)
    Xr, yr, T = X.copy(), y[:, 0].copy(), np.zeros((15, 0))
    for f in range(3):
        w = Xr.T @ yr
        w /= np.linalg.norm(w)
        np.testing.assert_allclose(m["W"][0][:, f], w, rtol=0, atol=1e-13)
        t = Xr @ w
        np.testing.assert_allclose(m["T"][:, f], t, rtol=0, atol=1e-12 * np.max(np.abs(t)))
        Xr -= np.outer(t, w)
        T = np.column_stack([T, t])
        yr = y[:, 0] - T @ np.linalg.lstsq(T, y[:, 0], rcond=None)[0]
    np.testing.assert_allclose(m["Yres"][:, 0], yr, rtol=0, atol=1e-12 * np.max(np.abs(y)))


def test_ssy_never_decreases_and_svd_equals_power_iterations():
    for case in NC.FIT_CASES:
        X, Y, _, mode = NC.fit_inputs(case)
        m = npls_ref.fit(X, Y, case[3], mode)
        assert not np.any(m["status"])
        assert np.all(np.diff(m["ssy"]) >= -1e-15) and 0 < m["ssy"][0] and m["ssy"][-1] <= 1 + 1e-15
        assert np.all(np.diff(m["ssx"]) >= -1e-15)
        assert np.allclose(np.triu(m["B"]), m["B"])
        for w in m["W"]:
            np.testing.assert_allclose(np.sum(w * w, axis=0), 1.0, rtol=0, atol=1e-14)
        if X.ndim == 3:  # the rank-one step by SVD and by power iterations
            m2 = npls_ref.fit(X, Y, case[3], mode, svd=False)
            assert m2["hopm_rounds"] > 0 and not np.any(m2["status"])
            for a, b in zip(m["W"] + [m["T"]], m2["W"] + [m2["T"]]):
                assert np.max(np.abs(a - b)) <= 1e-11 * np.max(np.abs(a))


def test_sign_rule():
    rng = np.random.default_rng(0)
    Z = rng.standard_normal((4, 5, 3))
    for svd in (True, False):
        ws, _, capped = npls_ref.rank_one(-Z, svd=svd)
        assert not capped
        for w in ws[:-1]:
            assert w[np.argmax(np.abs(w))] > 0
        assert np.tensordot(-Z, npls_ref.outer(ws), axes=3) > 0
    assert npls_ref.rank_one(np.zeros((3, 2)))[0] is None and npls_ref.rank_one(np.array([[1.0, np.nan]]))[0] is None


def test_planted_model_is_predicted_to_rounding():
    """y = X x_{!= mode} W, noise-free, W an outer product of unit vectors, and samples whose unfolding has
    orthonormal columns (so that X^T y is W itself): one component predicts y to rounding"""
    rng = np.random.default_rng(2)
    for ext, I, mode in (([4, 3], 30, 0), ([4, 3], 30, 2), ([3, 2, 2], 40, 0)):
        A = rng.standard_normal((I, int(np.prod(ext))))
        Qm, _ = np.linalg.qr(A - A.mean(axis=0, keepdims=True))
        X = np.moveaxis(Qm.reshape([I] + ext, order="F"), 0, mode)
        assert np.max(np.abs(X.mean(axis=mode))) < 1e-15
        ws = [v / np.linalg.norm(v) for v in (rng.standard_normal(n) for n in ext)]
        W = npls_ref.outer(ws)
        K = len(ext)
        y = np.tensordot(np.moveaxis(X, mode, 0), W, axes=(list(range(1, K + 1)), list(range(K))))[:, None]
        m = npls_ref.fit(X, y, 1, mode)
        yhat, _ = npls_ref.predict(m, X)
        assert np.max(np.abs(yhat - y)) <= 1e-12 * np.max(np.abs(y))
        assert abs(m["ssy"][0] - 1) <= 1e-12
        for a, b in zip(m["W"], ws):
            assert min(np.max(np.abs(a[:, 0] - b)), np.max(np.abs(a[:, 0] + b))) <= 1e-10
