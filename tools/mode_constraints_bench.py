#!/usr/bin/env python3
"""What the per-mode constraints cost (profiles/mode_constraints_bench.md).

Part 1, one mode update by kind, from the context's HIP-event profile (ppals_profile_read, slot 1: the bracketed
launches that are not tensor scans). A session whose modes are all FIXED but mode 0 does, per sweep, exactly
the leaf contraction of mode 0 and its update; the leaf is the same launch for every kind, so the rows differ
by the update alone: the fused solve (FREE), the HALS kernel and its finishing launches (NONNEG), the three
launches of kernels_polar.hip.h (ORTHO). Shapes: 200 rows at R = 10, 7200 rows at R = 10, 200 rows at R = 64;
one start (an ordinary session, sweeps_dt: no Normalize beside a FIXED mode; its FREE and NONNEG update
launches carry no bracket, so those rows show the leaf alone) and 12 starts (a multi-start session: at most
128 columns, so 2 starts at R = 64). Median of `--reps` sweeps after `--warmup`. Beside it the stopwatch: the
wall time of a sweep (the leaf and the update of every kind, launch gaps included) in windows of 20 sweeps
between device synchronisations, profile off — the figure that compares the one-start updates.

Part 2, a sweep of the headline tensor (s = 200, order 4, R = 10, fp32 storage) with kinds
[ortho, free, free, free] and [fixed, free, free, free] against all FREE: wall time of windows of `--sweeps`
sweeps between device synchronisations, median of `--reps`, and the tensor scans each booked.

Prints markdown tables. The measuring process runs under its own `timeout`.

  python tools/mode_constraints_bench.py
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--sweeps", type=int, default=10, help="sweeps per timed window of part 2")
    ap.add_argument("--size", type=int, default=200, help="extent of every mode of the part 2 tensor")
    ap.add_argument("--timeout", type=int, default=400, help="seconds the measuring process may take")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    return ap.parse_args(argv)


def worker(a):
    sys.path.insert(0, os.path.join(ROOT, "pairwise-perturbation_amd"))
    import numpy as np
    import ppals as pp
    ctx = pp.Context(0)
    med = statistics.median
    print("| rows | R | starts | kind | launches | ms per update (+ leaf) | wall ms per sweep |")
    print("|---|---|---|---|---|---|---|")
    for lens, R in (((200, 20, 20), 10), ((7200, 8, 8), 10), ((200, 20, 20), 64)):
        t = pp.Tensor(ctx, list(lens), pp.F32).fill_cp(pp.init_factors(list(lens), min(R, 8), 1000))
        for K in (1, min(12, 128 // R)):   # (a multi-start session holds at most 128 columns)
            W0 = [pp.init_factors(list(lens), R, 2000 + b) for b in range(K)]   # uniform on [0, 1): non-negative
            for kind in ("free", "nonneg", "ortho"):
                kinds = [kind] + ["fixed"] * (len(lens) - 1)
                if K == 1:
                    s = pp.CP(ctx, t, R)
                    s.set_factors(W0[0])
                    step = lambda: s.sweeps_dt(1)
                else:
                    s = pp.CPMulti(ctx, t, R, K)
                    s.set_factors(-1, W0)
                    step = lambda: s.sweeps(1)
                s.set_mode_constraints(kinds)
                for _ in range(a.warmup):
                    step()
                ctx.sync()
                ctx.profile_enable(2)
                ms, n = [], 0
                for _ in range(a.reps):
                    ctx.profile_reset()
                    step()
                    ctx.sync()
                    n, x, _ = ctx.profile_read(1)
                    ms.append(x)
                ctx.profile_enable(0)
                wall = []   # the stopwatch, profile off: 20 sweeps between two synchronisations
                for _ in range(a.reps):
                    ctx.sync()
                    t0 = time.perf_counter()
                    for _ in range(20):
                        step()
                    ctx.sync()
                    wall.append((time.perf_counter() - t0) / 20)
                print(f"| {lens[0]} | {R} | {K} | {kind} | {n} | {med(ms):.4f} | {1e3 * med(wall):.4f} |", flush=True)
                s.close()
        t.close()
    lens, R, n = [a.size] * 4, 10, a.sweeps
    t = pp.Tensor(ctx, lens, pp.F32).fill_cp(pp.init_factors(lens, R, 1000))
    W0 = pp.init_factors(lens, R, 2000)
    print()
    print("| kinds | ms per sweep | ratio to all FREE | scans per window |")
    print("|---|---|---|---|")
    base = None
    for kinds in (["free"] * 4, ["ortho", "free", "free", "free"], ["fixed", "free", "free", "free"]):
        s = pp.CP(ctx, t, R)
        s.set_factors(W0)
        s.set_mode_constraints(kinds)
        s.sweeps_dt(8 * a.warmup)   # (the online placement choice settles)
        ctx.sync()
        times = []
        for _ in range(a.reps):
            ctx.sync()
            t0 = time.perf_counter()
            s.sweeps_dt(n)
            ctx.sync()
            times.append(time.perf_counter() - t0)
        ctx.profile_enable(1)
        ctx.profile_reset()
        s.sweeps_dt(n)
        ctx.sync()
        scans = ctx.profile_read(0)[0]
        ctx.profile_enable(0)
        per = 1e3 * med(times) / n
        base = base or per
        print(f"| {' '.join(kinds)} | {per:.4f} | {per / base:.3f} | {scans} |", flush=True)
        assert np.isfinite(s.residual())
        s.close()
    t.close()
    ctx.close()


def main():
    a = parse()
    if a.worker:
        worker(a)
        return 0
    cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--worker"]
    return subprocess.call(cmd + sys.argv[1:])


if __name__ == "__main__":
    sys.exit(main())
