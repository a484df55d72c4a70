"""Cost of ppals_cp_impute_device (the missing entries of a CP session's tensor overwritten with its model,
under a mask) at the headline extents: order 4, s = 200, R = 10, F32 storage, 30 % missing, a dense
torch.bool mask (C order).

torch is imported first (one HIP runtime for both). Every figure is wall time around a device
synchronisation of both the caller's stream and the engine's. One JSON line per case:
  impute / impute_with_residual   the fused call, and the bytes its traffic floor counts
                                  (1 + 4 f B per element; 5 + 4 f with the observed residual)
  three_call                      export_model_torch, torch.where, import_torch into preallocated tensors,
                                  V held in torch beside the engine's copy (no observed residual comes out)
  em_iteration                    impute, then one sweep; the sweep that follows an impute pays the rebuild of
                                  the second resident layout, so it is set against a first sweep after
                                  set_factors (caches equally cold, nothing rebuilt) and a steady sweep

    python tools/impute_bench.py [--s 200] [--R 10] [--missing 0.3] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import torch  # noqa: I001  (before ppals: one HIP runtime)
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pairwise-perturbation_amd"))
import ppals as pp  # noqa: E402

DEV = torch.device("cuda:0")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--s", type=int, default=200)
    ap.add_argument("--R", type=int, default=10)
    ap.add_argument("--missing", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    s, R, f = a.s, a.R, a.missing
    shape = (s,) * 4
    n = s ** 4
    ctx = pp.Context(0)

    def sync():
        torch.cuda.synchronize()
        ctx.sync()

    def timed(fn, before=None):
        ts = []
        for i in range(a.reps + 1):   # the first one warms up (workspaces, offset tables)
            if before:
                before()
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            ts.append(time.perf_counter() - t0)
        return min(ts[1:]), float(np.median(ts[1:]))

    def emit(case, best, med, **kw):
        print(json.dumps(dict(case=case, shape=list(shape), R=R, missing=f, storage="F32",
                              best_ms=round(best * 1e3, 3), median_ms=round(med * 1e3, 3), **kw)), flush=True)
        return best

    t = pp.Tensor(ctx, list(shape), pp.F32).fill_uniform(5)
    cp = pp.CP(ctx, t, R)
    W, G = pp.init_factors(shape, R, 1), pp.init_factors(shape, R, 2)
    cp.set_factors(W, G)
    mask = torch.rand(shape, device=DEV) >= f
    fm = 1.0 - float(mask.float().mean())

    floor = n * (1 + 4 * fm)
    best, med = timed(lambda: cp.impute_torch(mask))
    t_imp = emit("impute", best, med, missing_measured=round(fm, 4), floor_bytes=int(floor),
                 GBps_of_floor=round(floor / best / 1e9, 1))
    floor_r = n * (5 + 4 * fm)
    best, med = timed(lambda: cp.impute_torch(mask, want_residual=True))
    t_impr = emit("impute_with_residual", best, med, floor_bytes=int(floor_r),
                  GBps_of_floor=round(floor_r / best / 1e9, 1))

    v = t.to_torch()
    model, new = torch.empty_like(v), torch.empty_like(v)

    def three_call():
        cp.export_model_torch(model)
        torch.where(mask, v, model, out=new)
        t.import_torch(new)
    best, med = timed(three_call)
    t3 = emit("three_call", best, med, bytes_moved=25 * n, GBps=round(25 * n / best / 1e9, 1))
    print(json.dumps({"case": "fused_vs_three_call", "impute_speedup": round(t3 / t_imp, 2),
                      "impute_with_residual_speedup": round(t3 / t_impr, 2)}), flush=True)
    del v, model, new
    torch.cuda.empty_cache()

    cp.sweeps_dt(3)   # layouts built, placement under way
    best, med = timed(lambda: cp.sweeps_dt(1))
    t_steady = emit("sweep_steady", best, med)
    best, med = timed(lambda: cp.sweeps_dt(1), before=lambda: cp.set_factors(W, G))
    t_cold = emit("sweep_first_after_set_factors", best, med)
    best, med = timed(lambda: cp.sweeps_dt(1), before=lambda: (cp.set_factors(W, G), cp.impute_torch(mask)))
    t_after = emit("sweep_first_after_impute", best, med)
    rebuild = max(t_after - t_cold, 0.0)
    total = t_imp + t_after
    print(json.dumps({"case": "em_iteration", "inner_sweeps": 1, "total_ms": round(total * 1e3, 3),
                      "impute_ms": round(t_imp * 1e3, 3), "layout_rebuild_ms": round(rebuild * 1e3, 3),
                      "sweep_ms": round(t_cold * 1e3, 3), "impute_share": round(t_imp / total, 3),
                      "layout_rebuild_share": round(rebuild / total, 3),
                      "steady_sweep_ms": round(t_steady * 1e3, 3)}), flush=True)
    cp.close()
    t.close()
    ctx.close()


if __name__ == "__main__":
    main()
