#!/usr/bin/env python3
"""The influence plot against the plain residual and against the hand-made way (profiles/slice_residuals_bench.md).

One process per shape creates the tensor (fill_uniform) and an ordinary session of rank --rank on factors
from the counter generator, warms every row up (buffers, code objects), then times --reps rounds in which the
rows ALTERNATE, each call on the host clock between two device synchronisations:
  a  ppals_cp_residual                       one pass over the tensor, one scalar
  b  ppals_cp_slice_residuals                the same pass keeping its row and column sums, folded onto the modes
  c  ppals_cp_leverages                      no tensor read
  d  by hand (--by-hand, where memory allows three tensors): export_model_torch(residual=True) into an fp32
     tensor, square it, N sums in torch
Median, minimum and maximum per row, b / a, and the largest relative difference between b and d. Prints one
JSON line per shape. The measuring process runs under its own `timeout`.

  python tools/slice_residuals_bench.py --shapes headline:f32,headline:bf16,coil100:f32,timelapse:f32
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = {"f32": 0, "f64": 1, "bf16": 3}
SHAPES = {"headline": [200, 200, 200, 200], "coil100": [3, 128, 128, 7200], "timelapse": [33, 1344, 1024, 9]}


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", type=str, default="headline:f32,headline:bf16,coil100:f32,timelapse:f32",
                    help="comma-separated name:dtype, name one of %s or extents joined by x" % sorted(SHAPES))
    ap.add_argument("--rank", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--by-hand", action="store_true", help="row d (needs torch and room for three tensors)")
    ap.add_argument("--timeout", type=int, default=420, help="seconds the measuring process of a shape may take")
    ap.add_argument("--worker", type=str, default="", help=argparse.SUPPRESS)
    return ap.parse_args(argv)


def worker(a):
    name, dt = a.worker.split(":")
    lens = SHAPES[name] if name in SHAPES else [int(x) for x in name.split("x")]
    if a.by_hand:
        import torch  # (before libppals is loaded: one HIP runtime for both)
    sys.path.insert(0, os.path.join(ROOT, "pairwise-perturbation_amd"))
    import numpy as np
    import ppals as pp
    ctx = pp.Context(0)
    t = pp.Tensor(ctx, lens, DTYPES[dt]).fill_uniform(1)
    s = pp.CP(ctx, t, a.rank)
    s.set_factors(pp.init_factors(lens, a.rank, 1000))

    def by_hand():
        e = s.model_to_torch(residual=True)
        e.square_()
        n = len(lens)
        out = [e.sum(dim=[d for d in range(n) if d != i], dtype=torch.float64) for i in range(n)]
        return [o.cpu().numpy() for o in out]   # (the download synchronises, as call b does)

    rows = {"a": s.residual, "b": s.slice_residuals, "c": s.leverages}
    if a.by_hand:
        rows["d"] = by_hand
    first = {k: fn() for k, fn in rows.items()}   # warm-up, and the values
    times = {k: [] for k in rows}
    for _ in range(a.reps):
        for k, fn in rows.items():
            ctx.sync()
            t0 = time.perf_counter()
            fn()
            ctx.sync()
            times[k].append(time.perf_counter() - t0)
    ss, total = s.slice_residuals(return_total=True)
    out = {"tool": "slice_residuals_bench", "shape": name, "lens": lens, "dtype": dt, "rank": a.rank, "reps": a.reps,
           "total_vs_residual_sq": abs(total - first["a"] ** 2) / first["a"] ** 2}
    for k, v in times.items():
        out[k + "_ms"] = {"median": 1e3 * statistics.median(v), "min": 1e3 * min(v), "max": 1e3 * max(v)}
    out["b_over_a"] = out["b_ms"]["median"] / out["a_ms"]["median"]
    if a.by_hand:
        out["b_vs_d_max_relative"] = float(max(np.max(np.abs(x - y) / x) for x, y in zip(ss, first["d"])))
    print(json.dumps(out), flush=True)
    s.close()
    t.close()
    ctx.close()


def main():
    a = parse()
    if a.worker:
        worker(a)
        return 0
    rc = 0
    for shape in a.shapes.split(","):   # a process per shape; a failure ends the run
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--worker", shape,
               "--rank", str(a.rank), "--reps", str(a.reps)] + (["--by-hand"] if a.by_hand else [])
        rc = subprocess.call(cmd)
        if rc:
            break
    return rc


if __name__ == "__main__":
    sys.exit(main())
