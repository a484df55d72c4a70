"""Time of the in-place preprocessing calls (Tensor.center for every mode, Tensor.scale, Tensor.slice_sumsq) against
the torch route they replace (to_torch -> x - x.mean(dim, keepdim=True) -> import_torch), in one process.

torch is imported first (one HIP runtime for both). Every call is timed with torch.cuda.Event pairs on torch's current
stream around a call that ends in the engine's work being waited for (center with offsets=None is asynchronous: the
pair brackets the call and a ctx.sync()). One JSON line per case. `of_peak` is the share of the 8 TB/s HBM peak
reached on 2 x bytes (one read and one write of the tensor; slice_sumsq: one read). The torch route's peak extra
memory is torch.cuda.max_memory_allocated over the route.

    python tools/preprocess_bench.py [--s 200] [--reps 5] [--coil]
"""
import argparse
import json
import os
import sys

import torch  # noqa: I001  (before ppals: one HIP runtime)
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pairwise-perturbation_amd"))
import ppals as pp  # noqa: E402

DEV = torch.device("cuda:0")
PEAK = 8.0e12  # MI355X HBM3E, bytes/s


def timed(fn, reps):
    fn()  # warm-up
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / 1e3)
    return min(ts), float(np.median(ts))


def report(name, lens, best, med, nbytes, passes, **kw):
    rec = {"case": name, "shape": list(lens), "best_ms": round(best * 1e3, 3), "median_ms": round(med * 1e3, 3),
           "GBps": round(passes * nbytes / best / 1e9, 1), "of_peak": round(passes * nbytes / best / PEAK, 3), **kw}
    print(json.dumps(rec), flush=True)
    return rec


def bench(ctx, name, lens, reps):
    n = int(np.prod(lens))
    nbytes = 4 * n
    t = pp.Tensor(ctx, list(lens), pp.F32).fill_uniform(1)
    ctx.sync()

    def synced(fn):
        def run():
            fn()
            ctx.sync()
        return run

    for mode in range(len(lens)):
        L, J, T = t._prep_shape(mode)[:3]
        best, med = timed(synced(lambda: t.center(mode)), reps)
        report(f"{name} center mode {mode}", lens, best, med, nbytes, 2, L=L, J=J, T=T)
    for mode in (0, len(lens) - 1):
        best, med = timed(lambda: t.slice_sumsq(mode), reps)
        report(f"{name} slice_sumsq mode {mode}", lens, best, med, nbytes, 1)
        t.fill_uniform(1)
        best, med = timed(lambda: t.scale(mode), reps)
        report(f"{name} scale mode {mode} (sumsq + rescale: 2 reads, 1 write)", lens, best, med, nbytes, 3)
    # the torch route: export, mean, subtract, import (the session's layout rebuild comes on top of both routes)
    for mode in range(len(lens)):
        def route():
            x = t.to_torch()
            x = x - x.mean(dim=mode, keepdim=True)
            t.import_torch(x)
            ctx.sync()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        best, med = timed(route, reps)
        extra = torch.cuda.max_memory_allocated() - base
        torch.cuda.empty_cache()
        report(f"{name} torch route mode {mode}", lens, best, med, nbytes, 2, peak_extra_bytes=int(extra),
               peak_extra_over_tensor=round(extra / nbytes, 2))
    t.close()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--s", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--coil", action="store_true", help="also the coil-100 extents 3 x 128 x 128 x 7200")
    a = ap.parse_args()
    ctx = pp.Context(0)
    bench(ctx, "headline", (a.s,) * 4, a.reps)
    if a.coil:
        bench(ctx, "coil100", (3, 128, 128, 7200), a.reps)
    ctx.close()


if __name__ == "__main__":
    main()
