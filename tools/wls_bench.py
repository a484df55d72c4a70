"""Cost of ppals_cp_wls_device (the majorization step of weighted CP: the resident tensor rewritten with
m + h (x - m) from a data view and a weights view) at the headline extents: order 4, s = 200, R = 10, F32
storage, fp32 views.

torch is imported first (one HIP runtime for both). Every figure is wall time around a device
synchronisation of both the caller's stream and the engine's. One JSON line per case:
  wls_<data>_<weights>[_loss]   the fused step, without and with the loss; layouts c (C order, read with the
                                lane index along b through LDS), ff (first index fastest, read along a with
                                16-byte loads) and vec (a per-variable vector along the last mode, stride 0
                                elsewhere). Traffic floor: 12 B per element with dense fp32 weights (x, h and
                                the store), 8 B with a broadcast vector.
  torch_route                   export_model_torch, torch.lerp, import_torch into preallocated tensors (no loss
                                comes out)
  impute_with_residual          ppals_cp_impute_device under a dense C-order mask, for comparison
  wls_iteration                 step, then one sweep; the sweep that follows a step pays the rebuild of the
                                second resident layout, so it is set against a first sweep after set_factors
                                (caches equally cold, nothing rebuilt) and a steady sweep

    python tools/wls_bench.py [--s 200] [--R 10] [--reps 5]
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
PEAK = 8e12   # HBM bytes per second


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--s", type=int, default=200)
    ap.add_argument("--R", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    s, R = a.s, a.R
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
        print(json.dumps(dict(case=case, shape=list(shape), R=R, storage="F32", views="f32",
                              best_ms=round(best * 1e3, 3), median_ms=round(med * 1e3, 3), **kw)), flush=True)
        return best

    def with_floor(case, best, med, per_elem):
        floor = n * per_elem
        return emit(case, best, med, floor_bytes=int(floor), TBps_of_floor=round(floor / best / 1e12, 3),
                    floor_ms_at_peak=round(floor / PEAK * 1e3, 3), fraction_of_peak=round(floor / best / PEAK, 3))

    t = pp.Tensor(ctx, list(shape), pp.F32).fill_uniform(5)
    cp = pp.CP(ctx, t, R)
    W, G = pp.init_factors(shape, R, 1), pp.init_factors(shape, R, 2)
    cp.set_factors(W, G)
    fstr = [s ** i for i in range(4)]
    x_c = torch.rand(shape, device=DEV)
    h_c = torch.rand(shape, device=DEV)
    times = {}
    for loss in (False, True):
        tag = "_loss" if loss else ""
        best, med = timed(lambda: cp.wls_torch(x_c, h_c, want_loss=loss))
        times["c_c" + tag] = with_floor("wls_c_c" + tag, best, med, 12)
    h_vec = torch.rand((1, 1, 1, s), device=DEV)
    for loss in (False, True):
        tag = "_loss" if loss else ""
        best, med = timed(lambda: cp.wls_torch(x_c, h_vec, want_loss=loss))
        times["c_vec" + tag] = with_floor("wls_c_vec" + tag, best, med, 8)
    x_f = torch.empty_strided(shape, fstr, dtype=torch.float32, device=DEV)
    x_f.copy_(x_c)
    best, med = timed(lambda: cp.wls_torch(x_f, h_c))
    times["ff_c"] = with_floor("wls_ff_c", best, med, 12)
    del h_c
    h_f = torch.rand(shape, device=DEV).permute(3, 2, 1, 0)   # first index fastest
    best, med = timed(lambda: cp.wls_torch(x_f, h_f))
    times["ff_ff"] = with_floor("wls_ff_ff", best, med, 12)
    del x_f
    h_c = h_f.contiguous()
    del h_f

    model, new = torch.empty_like(x_c), torch.empty_like(x_c)

    def torch_route():
        cp.export_model_torch(model)
        torch.lerp(model, x_c, h_c, out=new)
        t.import_torch(new)
    best, med = timed(torch_route)
    t3 = emit("torch_route", best, med, bytes_moved=24 * n, TBps=round(24 * n / best / 1e12, 3))
    print(json.dumps({"case": "fused_vs_torch_route", "wls_c_c_speedup": round(t3 / times["c_c"], 2),
                      "wls_c_c_loss_speedup": round(t3 / times["c_c_loss"], 2)}), flush=True)
    del model, new
    mask = h_c >= 0.3
    torch.cuda.empty_cache()
    best, med = timed(lambda: cp.impute_torch(mask, want_residual=True))
    emit("impute_with_residual", best, med, missing=0.3)
    del mask

    t_step = times["c_c"]
    cp.sweeps_dt(3)   # layouts built, placement under way
    best, med = timed(lambda: cp.sweeps_dt(1))
    t_steady = emit("sweep_steady", best, med)
    best, med = timed(lambda: cp.sweeps_dt(1), before=lambda: cp.set_factors(W, G))
    t_cold = emit("sweep_first_after_set_factors", best, med)
    best, med = timed(lambda: cp.sweeps_dt(1), before=lambda: (cp.set_factors(W, G), cp.wls_torch(x_c, h_c)))
    t_after = emit("sweep_first_after_step", best, med)
    rebuild = max(t_after - t_cold, 0.0)
    total = t_step + t_after
    print(json.dumps({"case": "wls_iteration", "inner_sweeps": 1, "total_ms": round(total * 1e3, 3),
                      "step_ms": round(t_step * 1e3, 3), "layout_rebuild_ms": round(rebuild * 1e3, 3),
                      "sweep_ms": round(t_cold * 1e3, 3), "step_share": round(t_step / total, 3),
                      "layout_rebuild_share": round(rebuild / total, 3),
                      "steady_sweep_ms": round(t_steady * 1e3, 3)}), flush=True)
    cp.close()
    t.close()
    ctx.close()


if __name__ == "__main__":
    main()
