"""P ranks of a bf16-stored CP run on ONE GPU, as threads of one process (TEST INFRASTRUCTURE; launched by
tests/test_gpu_bf16.py): the product's engine + HIP kernels over tests/hipsim's staged communicator, the
tensor block-partitioned along its leading mode. Exact sweeps under both schedules and the PP driver
against the unsharded fp64 oracle on the bf16-rounded tensor.

    python bf16_sharded_rank.py P"""
import os
import sys
import threading
import traceback

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hipsim_util  # noqa: E402
import oracle_lib as O  # noqa: E402
from bf16_util import bf16_round  # noqa: E402
from hipsim_rank import ThreadRanks  # noqa: E402

BF16 = 3
SHAPES = [([17, 12, 10, 9], 4), ([20, 16, 24], 5), ([9, 8, 7, 6, 5], 3)]


def relerr(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def cases(pp, ctx, w, rank):
    for no, (lens, R) in enumerate(SHAPES):
        def problem():
            V = bf16_round(O.build_V(O.init_factors(lens, R, 1234)))
            W = O.init_factors(lens, R, 4321)
            G = O.init_factors(lens, R, 99)
            _, _, W_ref, _ = O.als_cp_dt(V, W, G, tol=0.0, maxiter=2, resprint=1000)
            Vn = np.linalg.norm(V)
            kw = dict(tol=1e-6 * Vn, tol_init=0.1, maxiter=24, resprint=1000)
            return dict(V=V, W=W, G=G, W_ref=W_ref, kw=kw, pp_ref=O.als_cp_pp(V, W, G, **kw)[1:3],
                        M_ref=[O.mttkrp(V, W, m, 0) for m in range(len(lens))])

        pr = w.once(rank, ("bf16", no), problem)
        t = pp.Tensor(ctx, lens, BF16).upload(pr["V"])
        assert abs(t.norm() - np.linalg.norm(pr["V"])) < 1e-12 * np.linalg.norm(pr["V"])
        s = pp.CP(ctx, t, R)
        s.set_factors(pr["W"])
        for m in range(len(lens)):
            assert relerr(s.mttkrp(m), pr["M_ref"][m]) < 2e-6, (lens, m)
        for schedule in ("msdt", "dt"):
            s.set_schedule(schedule)
            s.set_factors(pr["W"], pr["G"])
            s.sweeps_dt(3)
            for a, b in zip(s.get_factors(), pr["W_ref"]):
                assert relerr(a, b) < 1e-5, (lens, schedule, relerr(a, b))
        s.set_factors(pr["W"], pr["G"])
        _, it = s.run_pp(**pr["kw"])
        it_ref, W_pp = pr["pp_ref"]
        assert it == it_ref, (lens, it, it_ref)
        for a, b in zip(s.get_factors(), W_pp):
            assert relerr(a, b) < 1e-4, (lens, "pp", relerr(a, b))
        s.close()
        t.close()


def main():
    P = int(sys.argv[1])
    pp = hipsim_util.load(make=False)
    pp.preload_eigensolver()
    w = ThreadRanks(P)
    errors = []

    def body(rank):
        try:
            ctx = pp.Context(0)
            uid, keep = w.comm_uid(rank)
            ctx.init_comm(rank, P, uid)
            try:
                cases(pp, ctx, w, rank)
                w.barrier()
            finally:
                ctx.close()
            del keep
        except BaseException:
            errors.append((rank, traceback.format_exc()))
            w.abort()

    ths = [threading.Thread(target=body, args=(r,)) for r in range(P)]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    real = [e for e in errors if "BrokenBarrierError" not in e[1]] or errors
    if real or w.failed:
        for r, tb in real[:2]:
            print(f"rank {r} FAILED:\n{tb}")
        sys.exit(1)
    print(f"all {P} ranks: OK")


if __name__ == "__main__":
    main()
