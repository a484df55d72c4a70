#!/usr/bin/env python3
"""What a shape on a non-negative mode costs (profiles/mode_shapes_bench.md).

Part 1, one mode update, shaped against the plain HALS pass, from the context's HIP-event profile
(ppals_profile_read, slot 1: the bracketed launches that are not tensor scans). A multi-start session whose modes
are all FIXED but mode 0 does, per sweep, exactly the leaf contraction of mode 0 and its update; the leaf is the
same launch for every shape, so the rows differ by the update alone: the batched HALS kernel and its finishing
launch (none), the three launches of kernels_shape.hip.h (unimodal, increasing). The tensor is rows x 8 x 8 — the
update does not see the other extents — at the rows and ranks of the sessions of part 2: 200 and 128 and 7200 rows
at R = 10, 1344 rows at R = 64; 1 start and 12 starts (a multi-start session holds at most 128 columns: 2 starts
at R = 64). Median of `--reps` sweeps after `--warmup`; beside it the wall time of a sweep in windows of 20
sweeps between device synchronisations, profile off.

Part 2, whole sweeps at full extents, all modes NONNEG, one of them unimodal against none: the headline tensor
(s = 200, order 4, R = 10), the coil-100 extents (3 x 128 x 128 x 7200, R = 10) with the 7200-row mode and with a
128-row mode, the time-lapse extents (33 x 1344 x 1024 x 9, R = 64) with the 1344-row mode; fp32 storage, one
start and 12 (2 at R = 64). The configurations of a tensor are measured in alternation, window by window (`--sweeps`
sweeps between device synchronisations, `--reps` windows each), medians; the tensor scans a window booked and
their summed time come from the profile, so the table says whether the update costs more than the scans.

Prints markdown tables. The measuring process runs under its own `timeout`.

  python tools/mode_shapes_bench.py [--part 1|2] [--only headline,coil100,timelapse]
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL = {"headline": ([200, 200, 200, 200], 10, (0,)), "coil100": ([3, 128, 128, 7200], 10, (3, 1)),
        "timelapse": ([33, 1344, 1024, 9], 64, (1,))}


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sweeps", type=int, default=5, help="sweeps per timed window of part 2")
    ap.add_argument("--part", type=int, default=0, help="1 or 2; 0: both")
    ap.add_argument("--only", type=str, default="headline,coil100,timelapse", help="the tensors of part 2")
    ap.add_argument("--timeout", type=int, default=900, help="seconds the measuring process may take")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    return ap.parse_args(argv)


def part1(a, pp, ctx):
    med = statistics.median
    print("| rows | R | starts | shape | launches | ms per update (+ leaf) | wall ms per sweep |")
    print("|---|---|---|---|---|---|---|")
    for rows, R in ((200, 10), (128, 10), (7200, 10), (1344, 64)):
        lens = [rows, 8, 8]
        t = pp.Tensor(ctx, lens, pp.F32).fill_cp(pp.init_factors(lens, min(R, 8), 1000))
        for K in (1, min(12, 128 // R)):
            W0 = [pp.init_factors(lens, R, 2000 + b) for b in range(K)]   # uniform on [0, 1): non-negative
            for shape in ("none", "unimodal", "increasing"):
                s = pp.CPMulti(ctx, t, R, K)
                s.set_factors(-1, W0)
                s.set_mode_constraints(["nonneg", "fixed", "fixed"])
                s.set_mode_shapes([shape, "none", "none"])
                for _ in range(a.warmup):
                    s.sweeps(1)
                ctx.sync()
                ctx.profile_enable(2)
                ms, n = [], 0
                for _ in range(a.reps):
                    ctx.profile_reset()
                    s.sweeps(1)
                    ctx.sync()
                    n, x, _ = ctx.profile_read(1)
                    ms.append(x)
                ctx.profile_enable(0)
                wall = []
                for _ in range(a.reps):
                    ctx.sync()
                    t0 = time.perf_counter()
                    for _ in range(20):
                        s.sweeps(1)
                    ctx.sync()
                    wall.append((time.perf_counter() - t0) / 20)
                print(f"| {rows} | {R} | {K} | {shape} | {n} | {med(ms):.4f} | {1e3 * med(wall):.4f} |", flush=True)
                s.close()
        t.close()


def part2(a, pp, ctx):
    med = statistics.median
    print("| tensor | R | starts | shaped mode (rows) | ms per sweep | sweeps/s | ratio to no shape | scans per sweep | scan ms per sweep |")
    print("|---|---|---|---|---|---|---|---|---|")
    for name in a.only.split(","):
        lens, R, modes = FULL[name]
        N = len(lens)
        t = pp.Tensor(ctx, lens, pp.F32).fill_cp(pp.init_factors(lens, 8, 1000))
        for K in (1, min(12, 128 // R)):
            W0 = [pp.init_factors(lens, R, 2000 + b) for b in range(K)]
            cfgs = []
            for mode in (None,) + tuple(modes):
                if K == 1:
                    s = pp.CP(ctx, t, R)
                    s.set_factors(W0[0])
                    step = (lambda s: lambda n: s.sweeps_dt(n))(s)
                else:
                    s = pp.CPMulti(ctx, t, R, K)
                    s.set_factors(-1, W0)
                    step = (lambda s: lambda n: s.sweeps(n))(s)
                s.set_mode_constraints(["nonneg"] * N)
                s.set_mode_shapes(["unimodal" if i == mode else "none" for i in range(N)])
                step(8 * a.warmup)   # (the online placement choice settles)
                ctx.sync()
                cfgs.append((mode, s, step, []))
            for _ in range(a.reps):   # interleaved: one window of every configuration in turn
                for _, _, step, times in cfgs:
                    ctx.sync()
                    t0 = time.perf_counter()
                    step(a.sweeps)
                    ctx.sync()
                    times.append((time.perf_counter() - t0) / a.sweeps)
            base = None
            for mode, s, step, times in cfgs:
                ctx.profile_enable(1)
                ctx.profile_reset()
                step(a.sweeps)
                ctx.sync()
                scans, scan_ms, _ = ctx.profile_read(0)
                ctx.profile_enable(0)
                per = 1e3 * med(times)
                base = base or per
                which = "none" if mode is None else f"{mode} ({lens[mode]})"
                print(f"| {name} | {R} | {K} | {which} | {per:.4f} | {1e3 / per:.1f} | {per / base:.3f} | "
                      f"{scans / a.sweeps:.1f} | {scan_ms / a.sweeps:.4f} |", flush=True)
                s.close()
        t.close()


def worker(a):
    sys.path.insert(0, os.path.join(ROOT, "pairwise-perturbation_amd"))
    import ppals as pp
    ctx = pp.Context(0)
    if a.part in (0, 1):
        part1(a, pp, ctx)
        print()
    if a.part in (0, 2):
        part2(a, pp, ctx)
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
