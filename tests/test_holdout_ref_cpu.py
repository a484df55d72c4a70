"""tests/holdout_ref.py (numpy ALS on the FULL tensor with held-out rows put back to zero behind every update
of the sample mode) against the oracle's restatement of CPD::als with the Simple optimizer on the REDUCED
tensor (np.compress along the mode): the identity the hold-out sessions rest on, to 1e-10 relative. The
systems S at these shapes have condition numbers of about 100, so two fp64 solvers agree far inside that."""
import numpy as np
import pytest

import holdout_ref as H
import oracle_lib as O

SWEEPS, K = 4, 4


@pytest.mark.parametrize("lam", [0.0, 1e-3])
@pytest.mark.parametrize("lens,R,mode", [([12, 11, 10], 3, 0), ([12, 11, 10], 3, 1), ([12, 11, 10, 9], 3, 2),
                                         ([12, 11, 10, 9], 3, 3)])
def test_zeroed_rows_are_the_reduced_tensor(lens, R, mode, lam):
    rng = np.random.default_rng(7)
    V = np.asfortranarray(rng.random(lens))
    W0 = [np.asfortranarray(rng.random((s, R))) for s in lens]
    G0 = [np.asfortranarray(rng.random((s, R))) for s in lens]
    for g in range(K):
        keep = np.arange(lens[mode]) % K != g
        W, G, scores = H.als_holdout(V, W0, G0, mode, keep, SWEEPS, lam)
        cut = lambda Ws: [np.asfortranarray(w[keep]) if i == mode else w for i, w in enumerate(Ws)]
        Vr = np.asfortranarray(np.compress(keep, V, axis=mode))
        _, _, _, W_ref, G_ref = O.cpd_als(Vr, cut(W0), cut(G0), 0, tol=0.0, maxsweep=SWEEPS - 1, lam=lam,
                                          resprint=10 ** 9)
        for a, r in zip(cut(W), W_ref):
            assert np.linalg.norm(a - r) < 1e-10 * np.linalg.norm(r)
        for a, r in zip(cut(G), G_ref):
            assert np.linalg.norm(a - r) < 1e-10 * (1 + np.linalg.norm(r))
        assert np.all(W[mode][~keep] == 0) and np.all(G[mode][~keep] == 0) and np.all(scores[keep] == 0)
        # a held-out sample's score is its least-squares projection on the other modes' final factors
        S = H.system(W, mode, lam)
        # (the sample mode is updated before the modes behind it: project on the factors it saw)
        if mode == len(lens) - 1:
            M = H.mttkrp(V, W, mode)
            want = np.linalg.solve(S, M.T).T
            assert np.linalg.norm(scores[~keep] - want[~keep]) < 1e-10 * np.linalg.norm(want[~keep])
