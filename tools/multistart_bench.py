#!/usr/bin/env python3
"""Multi-start CP-ALS against the same starts run one after another (profiles/multistart_bench.md).

One process creates the workload once and times, alternating, `--reps` times each:
  multi       n sweeps of ONE K-start session (ppals_cp_multi_sweeps), and the same through its driver
              (ppals_cp_multi_run: a gradient-norm / residual look per start before and after, as cpd_als has)
  sequential  the same K starts as K ordinary sessions, one after another, n sweeps each with
              ppals_cpd_als / PPALS_OPT_SIMPLE — code this feature does not touch
Every session is warmed up first (`--warmup` sweeps: code objects, workspaces, the online placement
choice of the ordinary sessions settles) and gets its starting factors back before every timed window;
a window ends in a device synchronise. Prints one JSON line: the median times, starts*sweeps/s of each
side and the ratios. The measuring process runs under its own `timeout`.

  python tools/multistart_bench.py --size 200 --order 4 --rank 10 --starts 4 --dtype f32 --schedule msdt
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
    import ppals as pp
    lens = [int(x) for x in a.lens.split(",")] if a.lens else [a.size] * a.order
    R, K, n = a.rank, a.starts, a.sweeps
    ctx = pp.Context(0)
    t = pp.Tensor(ctx, lens, DTYPES[a.dtype]).fill_cp(pp.init_factors(lens, R, 1000))
    W0 = [pp.init_factors(lens, R, 2000 + 31 * b) for b in range(K)]
    G0 = [pp.init_factors(lens, R, 7000 + 29 * b) for b in range(K)]
    multi = pp.CPMulti(ctx, t, R, K)
    multi.set_schedule(a.schedule)
    solos = []
    for b in range(K):
        s = pp.CP(ctx, t, R)
        s.set_schedule(a.schedule)
        solos.append(s)
    kw = dict(tol=0.0, resprint=10 ** 9)

    def reset():
        multi.set_factors(-1, W0, G0)
        for b, s in enumerate(solos):
            s.set_factors(W0[b], G0[b])
        ctx.sync()

    def timed(fn):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        return time.perf_counter() - t0

    def sequential():
        for s in solos:
            s.cpd_als(0, maxiter=n - 1, **kw)   # maxsweep + 1 = n sweeps

    reset()
    multi.sweeps(a.warmup)
    for s in solos:
        s.cpd_als(0, maxiter=a.warmup - 1, **kw)
    ctx.sync()
    tm, tr, ts = [], [], []
    for _ in range(a.reps):
        reset()
        tm.append(timed(lambda: multi.sweeps(n)))
        reset()
        ts.append(timed(sequential))
        reset()
        tr.append(timed(lambda: multi.run(maxiter=n, **kw)))
    # the two sides computed the same thing: start 0 after the last window
    reset()
    multi.sweeps(3)
    solos[0].cpd_als(0, maxiter=2, **kw)
    import numpy as np
    err = max(float(np.linalg.norm(x - y) / np.linalg.norm(y))
              for x, y in zip(multi.get_factors(0), solos[0].get_factors()))
    med = statistics.median
    out = {
        "tool": "multistart_bench", "lens": lens, "R": R, "starts": K, "dtype": a.dtype,
        "schedule": a.schedule, "sweeps": n, "warmup": a.warmup, "reps": a.reps,
        "multi_sweeps_s": med(tm), "multi_run_s": med(tr), "sequential_s": med(ts),
        "multi_sweeps_all_s": tm, "multi_run_all_s": tr, "sequential_all_s": ts,
        "multi_starts_sweeps_per_s": K * n / med(tm),
        "multi_run_starts_sweeps_per_s": K * n / med(tr),
        "sequential_starts_sweeps_per_s": K * n / med(ts),
        "ratio": med(ts) / med(tm),            # ppals_cp_multi_sweeps against the K cpd_als calls
        "ratio_run": med(ts) / med(tr),        # driver against driver (both look before and after)
        "ms_per_sweep_multi": 1e3 * med(tm) / n, "ms_per_sweep_one_session": 1e3 * med(ts) / (n * K),
        "start0_factor_relerr_vs_session": err,
    }
    print(json.dumps(out), flush=True)
    for h in solos + [multi, t]:
        h.close()
    ctx.close()


def main():
    a = parse()
    if a.worker:
        worker(a)
        return 0
    if a.rank * a.starts > 128 or not 1 <= a.starts <= 32:
        sys.exit("starts must be in [1, 32] and rank * starts <= 128")
    cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--worker"]
    cmd += sys.argv[1:]
    return subprocess.call(cmd)


if __name__ == "__main__":
    sys.exit(main())
