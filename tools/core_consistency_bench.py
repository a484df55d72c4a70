#!/usr/bin/env python3
"""The core consistency of a rank sweep in ONE call against one call per rank (profiles/core_consistency_bench.md).

One process creates the workload once — a rank-sweep session of the ranks --ranks and one ordinary session
per rank, all holding the same factors after --sweeps sweeps of the rank-sweep session — and, after one
warm-up call of every session (buffers, code objects), times `--reps` repetitions each of
  multi       one ppals_cp_multi_core_consistency: ONE tensor scan on all the ranks' columns
  sequential  ppals_cp_core_consistency on the ordinary sessions, one after another: one scan per rank
  sweep       one sweep of the rank-sweep session, for scale
Every timed call ends with its scores on the host (the calls synchronise themselves; the sweep is followed
by a device synchronise). Then one more call of each side under the launch profile's two counters: seconds
inside the tensor scan and inside the other bracketed kernels (pseudo-inverse factors, chain, score).
Prints one JSON line. The measuring process runs under its own `timeout`.
`--trace-calls K`: set-up, one warm-up call, K multi calls and nothing else — for a run under
`rocprofv3 --kernel-trace --stats`, whose per-kernel totals split scan, chain and score.

  python tools/core_consistency_bench.py --size 200 --order 4 --ranks 2,3,4,5,6,7,8,9,10 --dtype f32
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
    ap.add_argument("--sweeps", type=int, default=3, help="sweeps of the rank-sweep session before the calls")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trace-calls", type=int, default=0)
    ap.add_argument("--timeout", type=int, default=480, help="seconds the measuring process may take")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    return ap.parse_args(argv)


def worker(a):
    sys.path.insert(0, os.path.join(ROOT, "pairwise-perturbation_amd"))
    import numpy as np
    import ppals as pp
    lens = [int(x) for x in a.lens.split(",")] if a.lens else [a.size] * a.order
    ranks = [int(x) for x in a.ranks.split(",")]
    ctx = pp.Context(0)
    t = pp.Tensor(ctx, lens, DTYPES[a.dtype]).fill_cp(pp.init_factors(lens, max(ranks), 1000))
    multi = pp.CPMulti.with_ranks(ctx, t, ranks)
    multi.set_factors(-1, [pp.init_factors(lens, r, 2000 + 31 * b) for b, r in enumerate(ranks)])
    multi.sweeps(a.sweeps)
    warm = multi.core_consistencies()
    if a.trace_calls:
        for _ in range(a.trace_calls):
            multi.core_consistencies()
        print(json.dumps({"tool": "core_consistency_bench", "trace_calls": a.trace_calls, "cc": list(warm)}),
              flush=True)
        multi.close()
        t.close()
        ctx.close()
        return
    solos = []
    for b, r in enumerate(ranks):
        s = pp.CP(ctx, t, r)
        multi.take(b, s)
        solos.append(s)
    seq = lambda: [s.core_consistency() for s in solos]
    warm_seq = seq()

    def timed(fn):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        return time.perf_counter() - t0

    def counters(fn):
        ctx.sync()
        ctx.profile_enable(2)
        ctx.profile_reset()
        fn()
        ctx.sync()
        scan, other = ctx.profile_read(0), ctx.profile_read(1)
        ctx.profile_enable(0)
        return {"scan_launches": scan[0], "scan_s": scan[1], "scan_bytes": scan[2],
                "other_launches": other[0], "other_s": other[1]}

    tm, ts, tw = [], [], []
    for _ in range(a.reps):
        tm.append(timed(multi.core_consistencies))
        ts.append(timed(seq))
    prof_m = counters(multi.core_consistencies)
    prof_s = counters(seq)
    for _ in range(a.reps):   # (last: the sweeps move the session's factors on)
        tw.append(timed(lambda: multi.sweeps(1)))
    med = statistics.median
    out = {
        "tool": "core_consistency_bench", "lens": lens, "ranks": ranks, "columns": sum(ranks), "dtype": a.dtype,
        "reps": a.reps, "multi_ms": 1e3 * med(tm), "sequential_ms": 1e3 * med(ts), "sweep_ms": 1e3 * med(tw),
        "multi_all_ms": [1e3 * x for x in tm], "sequential_all_ms": [1e3 * x for x in ts],
        "sweep_all_ms": [1e3 * x for x in tw], "ratio": med(ts) / med(tm),
        "profile_multi": prof_m, "profile_sequential": prof_s,
        "cc_multi": [float(x) for x in warm], "cc_sequential": [float(x) for x in warm_seq],
        "max_cc_difference": float(np.max(np.abs(np.asarray(warm) - np.asarray(warm_seq)))),
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
    cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--worker"]
    cmd += sys.argv[1:]
    return subprocess.call(cmd)


if __name__ == "__main__":
    sys.exit(main())
