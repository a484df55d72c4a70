#!/usr/bin/env python3
"""What the non-negative (HALS) mode update costs a sweep (profiles/nonneg_bench.md).

One process creates the headline-shaped workload once (s = 200, order 4, R = 10, fp32 storage by default)
and two sessions on it, one ordinary and one with ppals_cp_set_nonneg on, and times, alternating, `--reps`
windows of `--sweeps` exact sweeps each (ppals_cp_sweeps_dt). The tensor scans and cached contractions
are the same in both; what differs is the update at the end of a mode: the ordinary session's one fused
launch (S, solve, Gram, the sweep's Normalize in its last update) against the HALS kernel, the sum of its
partials, the Gram and a Normalize launch of its own. Every session is warmed up first (`--warmup` sweeps:
code objects, workspaces, the online placement choice settles) and gets its starting factors back before
every window; a window ends in a device synchronise. Prints one JSON line with the median times and their
ratio. The measuring process runs under its own `timeout`.

  python tools/nonneg_bench.py --size 200 --order 4 --rank 10 --dtype f32 --schedule msdt
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
    ap.add_argument("--dtype", choices=sorted(DTYPES), default="f32")
    ap.add_argument("--schedule", choices=["msdt", "dt"], default="msdt")
    ap.add_argument("--sweeps", type=int, default=30, help="sweeps per timed window")
    ap.add_argument("--warmup", type=int, default=80, help="warm-up sweeps of every session")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--timeout", type=int, default=300, help="seconds the measuring process may take")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    return ap.parse_args(argv)


def worker(a):
    sys.path.insert(0, os.path.join(ROOT, "pairwise-perturbation_amd"))
    import numpy as np
    import ppals as pp
    lens = [int(x) for x in a.lens.split(",")] if a.lens else [a.size] * a.order
    R, n = a.rank, a.sweeps
    ctx = pp.Context(0)
    # init_factors draws from [0, 1): a non-negative tensor and non-negative starting factors
    t = pp.Tensor(ctx, lens, DTYPES[a.dtype]).fill_cp(pp.init_factors(lens, R, 1000))
    W0 = pp.init_factors(lens, R, 2000)
    assert min(float(w.min()) for w in W0) >= 0.0
    sess = {}
    for name in ("off", "on"):
        s = pp.CP(ctx, t, R)
        s.set_schedule(a.schedule)
        s.set_nonneg(name == "on")
        sess[name] = s

    def timed(s):
        s.set_factors(W0)
        ctx.sync()
        t0 = time.perf_counter()
        s.sweeps_dt(n)
        ctx.sync()
        return time.perf_counter() - t0

    for s in sess.values():
        s.set_factors(W0)
        s.sweeps_dt(a.warmup)
    ctx.sync()
    times = {"off": [], "on": []}
    for _ in range(a.reps):
        for name in ("off", "on"):
            times[name].append(timed(sess[name]))
    med = statistics.median
    out = {
        "tool": "nonneg_bench", "lens": lens, "R": R, "dtype": a.dtype, "schedule": a.schedule,
        "sweeps": n, "warmup": a.warmup, "reps": a.reps,
        "off_s": med(times["off"]), "on_s": med(times["on"]), "off_all_s": times["off"], "on_all_s": times["on"],
        "ms_per_sweep_off": 1e3 * med(times["off"]) / n, "ms_per_sweep_on": 1e3 * med(times["on"]) / n,
        "ratio_on_over_off": med(times["on"]) / med(times["off"]),
        "residual_off": sess["off"].residual(), "residual_on": sess["on"].residual(),
        "min_factor_entry_on": min(float(np.min(w)) for w in sess["on"].get_factors()),
    }
    print(json.dumps(out), flush=True)
    for h in list(sess.values()) + [t]:
        h.close()
    ctx.close()


def main():
    a = parse()
    if a.worker:
        worker(a)
        return 0
    if a.rank > 64:
        sys.exit("a non-negative session supports rank <= 64")
    cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--worker"]
    cmd += sys.argv[1:]
    return subprocess.call(cmd)


if __name__ == "__main__":
    sys.exit(main())
