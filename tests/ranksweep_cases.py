"""Cases of tests/test_gpu_ranksweep.py that need torch, one per process:
`python ranksweep_cases.py <case>`. torch is imported BEFORE the binding loads libppals (one HIP runtime
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
import ranksweep_util as U  # noqa: E402

FTOL = {pp.F32: 1e-5, pp.F64: 1e-8}


def case_take():
    """start 2 (rank 3) of a ranks-[2, 5, 3, 4] session taken into an ordinary rank-3 session: factors and
    gradients bit for bit what set_factors with the same values gives, then the gradient norm, the model /
    residual export and a short PP run equal those of that twin; a rank-4 destination is refused"""
    ctx = pp.Context(0)
    lens, ranks, b = [12, 11, 10, 9], [2, 5, 3, 4], 2
    V = O.build_V(O.init_factors(lens, 3, 1006))
    for dtype in (pp.F32, pp.F64):
        t = pp.Tensor(ctx, lens, dtype).upload(V)
        W0, G0 = U.starts(O.init_factors, lens, ranks)
        m = U.sweep(pp, ctx, t, ranks, W0, G0, 2)
        W, G = m.get_factors(b, with_grad=True)
        d = pp.CP(ctx, t, ranks[b])
        d.set_factors(O.init_factors(lens, ranks[b], 1))
        d.sweeps_dt(1)             # caches alive in the destination
        m.take(b, d)
        r = pp.CP(ctx, t, ranks[b])
        r.set_factors(W, G)
        Wd, Gd = d.get_factors(with_grad=True)
        assert U.same(Wd, W) and U.same(Gd, G)
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
            assert U.relerr(a, x) < FTOL[dtype], U.relerr(a, x)
        d4 = pp.CP(ctx, t, 4)
        try:
            m.take(b, d4)
        except pp.PpalsError as e:
            assert "ppals error -3:" in str(e) and "rank 4" in str(e) and "rank 3" in str(e), str(e)
        else:
            raise AssertionError("a rank-4 destination took a rank-3 start")
        for h in (d, d4, r, m, t):
            h.close()
    ctx.close()


if __name__ == "__main__":
    name = sys.argv[1]
    {"take": case_take}[name]()
    print(f"ranksweep case {name}: ok")
