"""Cases of tests/test_gpu_multistart.py that need torch, one per process:
`python multistart_cases.py <case>`. torch is imported BEFORE the binding loads libppals (one HIP runtime
for both). Exit status 0: passed."""
import os
import sys

import torch  # noqa: I001  (first: see above)
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "pairwise-perturbation_amd"))
import ppals as pp  # noqa: E402
import oracle_lib as O  # noqa: E402

FTOL = {pp.F32: 1e-5, pp.F64: 1e-8}


def relerr(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def case_take():
    """the winner of a multi-start session taken into an ordinary session: factors and gradients bit
    for bit, then the gradient norm, the model / residual export and the PP driver as after
    set_factors with the same values"""
    ctx = pp.Context(0)
    lens, R, K = [12, 11, 10, 9], 3, 4
    V = O.build_V(O.init_factors(lens, R, 1006))
    for dtype in (pp.F32, pp.F64):
        t = pp.Tensor(ctx, lens, dtype).upload(V)
        W0 = [O.init_factors(lens, R, 2000 + 31 * b) for b in range(K)]
        G0 = [O.init_factors(lens, R, 7000 + 29 * b) for b in range(K)]
        m = pp.CPMulti(ctx, t, R, K)
        m.set_factors(-1, W0, G0)
        m.sweeps(2)
        b = int(np.argmin(m.residuals()))
        W, G = m.get_factors(b, with_grad=True)
        d = pp.CP(ctx, t, R)
        d.set_factors(O.init_factors(lens, R, 1))
        d.sweeps_dt(1)             # caches alive in the destination
        m.take(b, d)
        r = pp.CP(ctx, t, R)
        r.set_factors(W, G)
        Wd, Gd = d.get_factors(with_grad=True)
        assert all(np.array_equal(a, x) for a, x in zip(Wd, W))
        assert all(np.array_equal(a, x) for a, x in zip(Gd, G))
        assert abs(d.gradnorm() - r.gradnorm()) < 1e-10 * r.gradnorm()
        tdt = torch.float64 if dtype == pp.F64 else torch.float32
        for residual in (False, True):
            a = d.model_to_torch(tdt, residual=residual)
            x = r.model_to_torch(tdt, residual=residual)
            torch.cuda.synchronize()
            assert torch.equal(a, x), residual
        kw = dict(tol=0.0, tol_init=0.5, maxiter=6, resprint=2)
        assert d.run_pp(**kw) == r.run_pp(**kw)
        for a, x in zip(d.get_factors(), r.get_factors()):
            assert relerr(a, x) < FTOL[dtype], relerr(a, x)
        for h in (d, r, m, t):
            h.close()
    ctx.close()


if __name__ == "__main__":
    name = sys.argv[1]
    {"take": case_take}[name]()
    print(f"multistart case {name}: ok")
