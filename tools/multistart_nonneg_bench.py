#!/usr/bin/env python3
"""Non-negative multi-start CP against the same starts run one after another (profiles/multistart_nonneg_bench.md).

One process creates the headline-shaped workload once (s = 200, order 4, R = 10, fp32 storage, K = 4 by
default; a non-negative tensor, non-negative starts) and times, alternating, `--reps` windows of `--sweeps`
sweeps each:
  nn_multi    ONE K-start session with ppals_cp_multi_set_nonneg on (ppals_cp_multi_sweeps): shared tensor
              scans, one batched HALS update per mode
  sequential  the same K starts as K ordinary non-negative sessions, one after another, with
              ppals_cpd_als / PPALS_OPT_SIMPLE (no Normalize, as in a multi-start session)
  multi       an unconstrained K-start session: the same scans, the batched solve in place of HALS
Every session is warmed up first (`--warmup` sweeps: code objects, workspaces, the online placement choice
of the ordinary sessions settles) and gets its starting factors back before every timed window; a window
ends in a device synchronise. Prints one JSON line: the median times, starts*sweeps/s of each side and the
ratios. The measuring process runs under its own `timeout`.

  python tools/multistart_nonneg_bench.py --size 200 --order 4 --rank 10 --starts 4 --dtype f32
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


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--size", type=int, default=200, help="extent of every mode")
    ap.add_argument("--order", type=int, default=4)
    ap.add_argument("--lens", type=str, default="", help="comma-separated extents (overrides --size/--order)")
    ap.add_argument("--rank", type=int, default=10)
    ap.add_argument("--starts", type=int, default=4)
    ap.add_argument("--dtype", choices=sorted(DTYPES), default="f32")
    ap.add_argument("--schedule", choices=["msdt", "dt"], default="msdt")
    ap.add_argument("--sweeps", type=int, default=30, help="sweeps per timed window")
    ap.add_argument("--warmup", type=int, default=80, help="warm-up sweeps of every session")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=480, help="seconds the measuring process may take")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    return ap.parse_args(argv)


def worker(a):
    sys.path.insert(0, os.path.join(ROOT, "pairwise-perturbation_amd"))
    import numpy as np
    import ppals as pp
    lens = [int(x) for x in a.lens.split(",")] if a.lens else [a.size] * a.order
    R, K, n = a.rank, a.starts, a.sweeps
    ctx = pp.Context(0)
    # init_factors draws from [0, 1): a non-negative tensor and non-negative starting factors
    t = pp.Tensor(ctx, lens, DTYPES[a.dtype]).fill_cp(pp.init_factors(lens, R, 1000))
    W0 = [pp.init_factors(lens, R, 2000 + 31 * b) for b in range(K)]
    multis = {}
    for name in ("nn_multi", "multi"):
        m = pp.CPMulti(ctx, t, R, K)
        m.set_schedule(a.schedule)
        m.set_nonneg(name == "nn_multi")
        multis[name] = m
    solos = []
    for b in range(K):
        s = pp.CP(ctx, t, R)
        s.set_schedule(a.schedule)
        s.set_nonneg(True)
        solos.append(s)
    kw = dict(tol=0.0, resprint=10 ** 9)

    def reset():
        for m in multis.values():
            m.set_factors(-1, W0)
        for b, s in enumerate(solos):
            s.set_factors(W0[b])
        ctx.sync()

    def timed(fn):
        reset()
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        return time.perf_counter() - t0

    def sequential():
        for s in solos:
            s.cpd_als(0, maxiter=n - 1, **kw)   # maxsweep + 1 = n sweeps

    reset()
    for m in multis.values():
        m.sweeps(a.warmup)
    for s in solos:
        s.cpd_als(0, maxiter=a.warmup - 1, **kw)
    ctx.sync()
    times = {"nn_multi": [], "sequential": [], "multi": []}
    for _ in range(a.reps):
        times["nn_multi"].append(timed(lambda: multis["nn_multi"].sweeps(n)))
        times["sequential"].append(timed(sequential))
        times["multi"].append(timed(lambda: multis["multi"].sweeps(n)))
    # the two non-negative sides computed the same thing: start 0 after three sweeps
    reset()
    multis["nn_multi"].sweeps(3)
    solos[0].cpd_als(0, maxiter=2, **kw)
    err = max(float(np.linalg.norm(x - y) / np.linalg.norm(y))
              for x, y in zip(multis["nn_multi"].get_factors(0), solos[0].get_factors()))
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {
        "tool": "multistart_nonneg_bench", "lens": lens, "R": R, "starts": K, "dtype": a.dtype,
        "schedule": a.schedule, "sweeps": n, "warmup": a.warmup, "reps": a.reps,
        "nn_multi_s": med["nn_multi"], "sequential_s": med["sequential"], "multi_s": med["multi"],
        "nn_multi_all_s": times["nn_multi"], "sequential_all_s": times["sequential"], "multi_all_s": times["multi"],
        "nn_multi_starts_sweeps_per_s": K * n / med["nn_multi"],
        "sequential_starts_sweeps_per_s": K * n / med["sequential"],
        "multi_starts_sweeps_per_s": K * n / med["multi"],
        "ratio_sequential_over_nn_multi": med["sequential"] / med["nn_multi"],
        "ratio_nn_multi_over_multi": med["nn_multi"] / med["multi"],
        "ms_per_sweep_nn_multi": 1e3 * med["nn_multi"] / n, "ms_per_sweep_multi": 1e3 * med["multi"] / n,
        "ms_per_sweep_one_session": 1e3 * med["sequential"] / (n * K),
        "start0_factor_relerr_vs_session": err,
        "min_factor_entry_nn_multi": min(float(np.min(w)) for W in multis["nn_multi"].get_factors(-1) for w in W),
    }
    print(json.dumps(out), flush=True)
    for h in solos + list(multis.values()) + [t]:
        h.close()
    ctx.close()


def main():
    a = parse()
    if a.worker:
        worker(a)
        return 0
    if a.rank * a.starts > 128 or not 1 <= a.starts <= 32 or a.rank > 64:
        sys.exit("starts must be in [1, 32], rank <= 64 and rank * starts <= 128")
    cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--worker"]
    cmd += sys.argv[1:]
    return subprocess.call(cmd)


if __name__ == "__main__":
    sys.exit(main())
