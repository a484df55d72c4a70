#!/usr/bin/env python3
"""A rank sweep in ONE session against the same models as ordinary sessions (profiles/ranksweep_bench.md).

One process creates the workload once and times, alternating, `--reps` times each:
  sweep       n sweeps of ONE session whose starts have the ranks --ranks (ppals_cp_multi_create_ranks:
              2..10 are 54 columns of every tensor scan)
  sequential  the same models as ordinary sessions of those ranks, one after another, n sweeps each with
              ppals_cpd_als / PPALS_OPT_SIMPLE — code this feature does not touch
Every session is warmed up first (`--warmup` sweeps: code objects, workspaces, the online placement
choice of the ordinary sessions settles) and gets its starting factors back before every timed window;
a window ends in a device synchronise. After the timed windows one profiled window of each side reads the
launch profile's two counters: seconds inside tensor scans and inside the other bracketed kernels. Prints
one JSON line: the median times, ms per sweep of all models on both sides, the ratio, the counters and
start 0's factor error against its ordinary session. The measuring process runs under its own `timeout`.

  python tools/ranksweep_bench.py --size 200 --order 4 --ranks 2,3,4,5,6,7,8,9,10 --dtype f32 --schedule msdt
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
    ap.add_argument("--ranks", type=str, default="2,3,4,5,6,7,8,9,10", help="comma-separated ranks, one per start")
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
    ranks = [int(x) for x in a.ranks.split(",")]
    n = a.sweeps
    ctx = pp.Context(0)
    t = pp.Tensor(ctx, lens, DTYPES[a.dtype]).fill_cp(pp.init_factors(lens, max(ranks), 1000))
    W0 = [pp.init_factors(lens, r, 2000 + 31 * b) for b, r in enumerate(ranks)]
    G0 = [pp.init_factors(lens, r, 7000 + 29 * b) for b, r in enumerate(ranks)]
    multi = pp.CPMulti.with_ranks(ctx, t, ranks)
    multi.set_schedule(a.schedule)
    solos = []
    for r in ranks:
        s = pp.CP(ctx, t, r)
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

    def counters(fn):
        """(scan launches, scan seconds, other bracketed launches, other seconds) of one window"""
        reset()
        ctx.profile_enable(2)
        ctx.profile_reset()
        fn()
        ctx.sync()
        scan, other = ctx.profile_read(0), ctx.profile_read(1)
        ctx.profile_enable(0)
        return {"scan_launches": scan[0], "scan_s": scan[1], "other_launches": other[0], "other_s": other[1]}

    reset()
    multi.sweeps(a.warmup)
    for s in solos:
        s.cpd_als(0, maxiter=a.warmup - 1, **kw)
    ctx.sync()
    tm, ts = [], []
    for _ in range(a.reps):
        reset()
        tm.append(timed(lambda: multi.sweeps(n)))
        reset()
        ts.append(timed(sequential))
    prof_m = counters(lambda: multi.sweeps(n))
    prof_s = counters(sequential)
    # the two sides computed the same thing: start 0 after three sweeps
    reset()
    multi.sweeps(3)
    solos[0].cpd_als(0, maxiter=2, **kw)
    err = max(float(np.linalg.norm(x - y) / np.linalg.norm(y))
              for x, y in zip(multi.get_factors(0), solos[0].get_factors()))
    med = statistics.median
    out = {
        "tool": "ranksweep_bench", "lens": lens, "ranks": ranks, "columns": sum(ranks), "dtype": a.dtype,
        "schedule": a.schedule, "sweeps": n, "warmup": a.warmup, "reps": a.reps,
        "sweep_s": med(tm), "sequential_s": med(ts), "sweep_all_s": tm, "sequential_all_s": ts,
        "ms_per_sweep_of_all_one_session": 1e3 * med(tm) / n,
        "ms_per_sweep_of_all_sequential": 1e3 * med(ts) / n,
        "ratio": med(ts) / med(tm),
        "profile_one_session": prof_m, "profile_sequential": prof_s,
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
    ranks = [int(x) for x in a.ranks.split(",")]
    if not 1 <= len(ranks) <= 32 or min(ranks) < 1 or sum(ranks) > 128:
        sys.exit("ranks: 1 to 32 of them, each >= 1, at most 128 in total")
    cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--worker"]
    cmd += sys.argv[1:]
    return subprocess.call(cmd)


if __name__ == "__main__":
    sys.exit(main())
