"""Cost of ppals_tucker_impute_device (the missing entries of a Tucker session's tensor overwritten with its
model, under a mask) at BASELINE configs[4]: order 3, s = 400, core 20^3, F32 storage, 30 % missing.

torch is imported first (one HIP runtime for both). Every figure is wall time around a device
synchronisation of both the caller's stream and the engine's, best of --reps after a warm-up call. One JSON
line per case:
  impute / impute_with_residual   the fused call under a first-index-fastest mask (ff) and a C-order mask (c),
                                  and the bytes its traffic floor counts (1 + 4 f B per element; 5 + 4 f with
                                  the observed residual)
  three_call                      export_model_torch, torch.where, import_torch into preallocated tensors,
                                  V held in torch beside the engine's copy (no observed residual comes out)
  cp_impute_same_K                a CP session's impute at R = r_0 on the same box and C-order mask: the same
                                  Q P^T product shape through the MAXRB = 16 instantiation of k_model_view,
                                  the route the Tucker imputation would take without k_model_impute_wide
  em_iteration                    impute, then one HOOI sweep; the sweep that follows an impute pays the
                                  rebuild of the other resident layouts, so it is set against a first sweep
                                  after set_factors (nothing rebuilt) and a steady sweep

    python tools/tucker_impute_bench.py [--s 400] [--r 20] [--missing 0.3] [--reps 5]
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
    ap.add_argument("--s", type=int, default=400)
    ap.add_argument("--r", type=int, default=20)
    ap.add_argument("--missing", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    s, r, f = a.s, a.r, a.missing
    shape, ranks = (s,) * 3, (r,) * 3
    n = s ** 3
    pp.preload_eigensolver()
    ctx = pp.Context(0)

    def sync():
        torch.cuda.synchronize()
        ctx.sync()

    def timed(fn, before=None):
        ts = []
        for i in range(a.reps + 1):   # the first one warms up (workspaces, offset tables, chain buffers)
            if before:
                before()
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            ts.append(time.perf_counter() - t0)
        return min(ts[1:]), float(np.median(ts[1:]))

    def emit(case, best, med, **kw):
        print(json.dumps(dict(case=case, shape=list(shape), ranks=list(ranks), missing=f, storage="F32",
                              best_ms=round(best * 1e3, 3), median_ms=round(med * 1e3, 3), **kw)), flush=True)
        return best

    t = pp.Tensor(ctx, list(shape), pp.F32).fill_uniform(7)
    k = pp.Tucker(ctx, t, list(ranks))
    k.hosvd()
    k.sweeps_dt(2)
    W, core = k.get_factors()
    base = torch.rand(shape, device=DEV) >= f
    fm = 1.0 - float(base.float().mean())
    ff = torch.empty_strided(shape, [1, s, s * s], dtype=torch.bool, device=DEV)
    ff.copy_(base)
    floor, floor_r = n * (1 + 4 * fm), n * (5 + 4 * fm)
    best_of = {}
    for name, mask in (("ff", ff), ("c", base)):
        best, med = timed(lambda: k.impute_torch(mask))
        best_of[name] = emit("impute", best, med, mask=name, missing_measured=round(fm, 4),
                             floor_bytes=int(floor), GBps_of_floor=round(floor / best / 1e9, 1))
        best, med = timed(lambda: k.impute_torch(mask, want_residual=True))
        best_of[name + "_r"] = emit("impute_with_residual", best, med, mask=name, floor_bytes=int(floor_r),
                                    GBps_of_floor=round(floor_r / best / 1e9, 1))

    v = t.to_torch()
    model, new = torch.empty_like(v), torch.empty_like(v)

    def three_call():
        k.export_model_torch(model)
        torch.where(base, v, model, out=new)
        t.import_torch(new)
    best, med = timed(three_call)
    t3 = emit("three_call", best, med, mask="c", bytes_moved=25 * n, GBps=round(25 * n / best / 1e9, 1))
    print(json.dumps({"case": "fused_vs_three_call", "mask": "c",
                      "impute_speedup": round(t3 / best_of["c"], 2),
                      "impute_with_residual_speedup": round(t3 / best_of["c_r"], 2)}), flush=True)
    del v, model, new
    torch.cuda.empty_cache()

    # the route the new kernel replaces: a CP impute at R = r_0 on the same tensor and mask
    cp = pp.CP(ctx, t, r)
    cp.set_factors(pp.init_factors(shape, r, 1), pp.init_factors(shape, r, 2))
    for name, mask in (("ff", ff), ("c", base)):
        best, med = timed(lambda: cp.impute_torch(mask))
        tc = emit("cp_impute_same_K", best, med, mask=name, R=r)
        best, med = timed(lambda: cp.impute_torch(mask, want_residual=True))
        tcr = emit("cp_impute_same_K_with_residual", best, med, mask=name, R=r)
        print(json.dumps({"case": "tucker_vs_cp_same_K", "mask": name,
                          "cp_over_tucker": round(tc / best_of[name], 2),
                          "cp_over_tucker_with_residual": round(tcr / best_of[name + "_r"], 2)}), flush=True)
    cp.close()

    best, med = timed(lambda: k.sweeps_dt(1))
    t_steady = emit("sweep_steady", best, med)

    def reset():
        k.set_factors(W)
        k.set_core(core)
    best, med = timed(lambda: k.sweeps_dt(1), before=reset)
    t_cold = emit("sweep_first_after_set_factors", best, med)
    best, med = timed(lambda: k.sweeps_dt(1), before=lambda: (reset(), k.impute_torch(base)))
    t_after = emit("sweep_first_after_impute", best, med)
    t_imp = best_of["c"]
    rebuild = max(t_after - t_cold, 0.0)
    total = t_imp + t_after
    print(json.dumps({"case": "em_iteration", "inner_sweeps": 1, "total_ms": round(total * 1e3, 3),
                      "impute_ms": round(t_imp * 1e3, 3), "layout_rebuild_ms": round(rebuild * 1e3, 3),
                      "sweep_ms": round(t_cold * 1e3, 3), "impute_share": round(t_imp / total, 3),
                      "layout_rebuild_share": round(rebuild / total, 3),
                      "steady_sweep_ms": round(t_steady * 1e3, 3)}), flush=True)
    k.close()
    t.close()
    ctx.close()


if __name__ == "__main__":
    main()
