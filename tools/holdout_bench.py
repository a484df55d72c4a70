#!/usr/bin/env python3
"""A segmented jackknife in ONE hold-out session against the same fits on reduced tensors (profiles/holdout_bench.md).

One process creates the tensor once and measures
  (a) hold-out  n sweeps of a multi-start session of `--segments` + 1 starts of rank R whose starts hold out
                their segment of the samples of `--mode` (ppals_cp_multi_set_holdout), against
      plain     the same session with no hold-out set — alternating, `--reps` windows each. The expected
                difference is the one small launch behind the sample mode's update; the launch profile's counters
                of one more window of each say what it is.
  (b) sequential  the same segments + 1 fits as ORDINARY sessions, one after another, each on its own reduced
                tensor (the tensor without the segment's slices, filled from the same factors), n sweeps with
                ppals_cpd_als / PPALS_OPT_SIMPLE — a tensor and a session at a time, so the memory stays that of
                one fit; the time to create each reduced tensor and its session is reported beside the sweeps.
Every session is warmed up first (`--warmup` sweeps) and gets its starting factors back before every timed
window; a window ends in a device synchronise. Prints one JSON line. The measuring process runs under its own
`timeout`.

  python tools/holdout_bench.py --size 200 --order 4 --rank 10 --segments 11 --dtype f32
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
    ap.add_argument("--segments", type=int, default=11)
    ap.add_argument("--mode", type=int, default=0, help="the sample mode")
    ap.add_argument("--dtype", choices=sorted(DTYPES), default="f32")
    ap.add_argument("--schedule", choices=["msdt", "dt"], default="msdt")
    ap.add_argument("--sweeps", type=int, default=20, help="sweeps per timed window")
    ap.add_argument("--warmup", type=int, default=60, help="warm-up sweeps of every session")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-sequential", action="store_true", help="(a) only")
    ap.add_argument("--timeout", type=int, default=540, help="seconds the measuring process may take")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    return ap.parse_args(argv)


def worker(a):
    sys.path.insert(0, os.path.join(ROOT, "pairwise-perturbation_amd"))
    import numpy as np
    import ppals as pp
    lens = [int(x) for x in a.lens.split(",")] if a.lens else [a.size] * a.order
    R, K, mode, n = a.rank, a.segments + 1, a.mode, a.sweeps
    ctx = pp.Context(0)
    Wtrue = pp.init_factors(lens, R, 1000)
    t = pp.Tensor(ctx, lens, DTYPES[a.dtype]).fill_cp(Wtrue)
    W0 = [pp.init_factors(lens, R, 2000 + 31 * b) for b in range(K)]
    G0 = [pp.init_factors(lens, R, 7000 + 29 * b) for b in range(K)]
    keep = np.vstack([np.ones((1, lens[mode]), dtype=bool), pp.holdout_segments(lens[mode], a.segments)])
    sessions = {}
    for name in ("holdout", "plain"):
        m = pp.CPMulti(ctx, t, R, K)
        m.set_schedule(a.schedule)
        if name == "holdout":
            m.set_holdout(mode, keep)
        sessions[name] = m

    def timed(fn):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        return time.perf_counter() - t0

    def reset(m):
        m.set_factors(-1, W0, G0)
        ctx.sync()

    def counters(m):
        reset(m)
        ctx.profile_enable(2)
        ctx.profile_reset()
        m.sweeps(n)
        ctx.sync()
        scan, other = ctx.profile_read(0), ctx.profile_read(1)
        ctx.profile_enable(0)
        return {"scan_launches": scan[0], "scan_ms": scan[1], "scan_bytes": scan[2], "other_launches": other[0],
                "other_ms": other[1]}

    for m in sessions.values():
        reset(m)
        m.sweeps(a.warmup)
    times = {name: [] for name in sessions}
    for _ in range(a.reps):
        for name, m in sessions.items():
            reset(m)
            times[name].append(timed(lambda: m.sweeps(n)))
    prof = {name: counters(m) for name, m in sessions.items()}
    med = statistics.median
    out = {
        "tool": "holdout_bench", "lens": lens, "rank": R, "starts": K, "columns": R * K, "mode": mode,
        "dtype": a.dtype, "schedule": a.schedule, "sweeps": n, "warmup": a.warmup, "reps": a.reps,
        "holdout_all_s": times["holdout"], "plain_all_s": times["plain"],
        "holdout_ms_per_sweep": 1e3 * med(times["holdout"]) / n, "plain_ms_per_sweep": 1e3 * med(times["plain"]) / n,
        "profile_holdout": prof["holdout"], "profile_plain": prof["plain"],
    }
    out["holdout_minus_plain_us_per_sweep"] = 1e3 * (out["holdout_ms_per_sweep"] - out["plain_ms_per_sweep"])
    out["extra_other_launches_per_sweep"] = (prof["holdout"]["other_launches"] - prof["plain"]["other_launches"]) / n
    out["extra_other_us_per_sweep"] = 1e3 * (prof["holdout"]["other_ms"] - prof["plain"]["other_ms"]) / n
    if not a.skip_sequential:
        # start 0 of the hold-out session after three sweeps, to compare with the first ordinary fit below
        reset(sessions["holdout"])
        sessions["holdout"].sweeps(3)
        last = sessions["holdout"].get_factors(K - 1)
        for m in sessions.values():
            m.close()
        sessions = {}
        kw = dict(tol=0.0, resprint=10 ** 9)
        sweep_s, setup_s, err = [], [], None
        for b in range(K):
            cut = lambda Ws: [np.asfortranarray(w[keep[b]]) if i == mode else w for i, w in enumerate(Ws)]
            t0 = time.perf_counter()
            tr = pp.Tensor(ctx, [int(keep[b].sum()) if i == mode else s for i, s in enumerate(lens)], DTYPES[a.dtype])
            tr.fill_cp(cut(Wtrue))
            s = pp.CP(ctx, tr, R)
            s.set_schedule(a.schedule)
            ctx.sync()
            setup_s.append(time.perf_counter() - t0)
            s.set_factors(cut(W0[b]), cut(G0[b]))
            s.cpd_als(0, maxiter=a.warmup - 1, **kw)
            best = []
            for _ in range(a.reps):
                s.set_factors(cut(W0[b]), cut(G0[b]))
                best.append(timed(lambda: s.cpd_als(0, maxiter=n - 1, **kw)))   # maxsweep + 1 = n sweeps
            sweep_s.append(med(best))
            if b == K - 1:
                s.set_factors(cut(W0[b]), cut(G0[b]))
                s.cpd_als(0, maxiter=2, **kw)
                err = max(float(np.linalg.norm(x - y) / np.linalg.norm(y)) for x, y in zip(cut(last), s.get_factors()))
            s.close()
            tr.close()
        out.update({
            "sequential_sweep_s_per_fit": sweep_s, "sequential_setup_s_per_fit": setup_s,
            "sequential_ms_per_sweep_of_all": 1e3 * sum(sweep_s) / n,
            "ratio_sequential_over_holdout": (1e3 * sum(sweep_s) / n) / out["holdout_ms_per_sweep"],
            "last_start_factor_relerr_vs_reduced_session": err,
        })
    print(json.dumps(out), flush=True)
    for m in sessions.values():
        m.close()
    t.close()
    ctx.close()


def main():
    a = parse()
    if a.worker:
        worker(a)
        return 0
    if not 2 <= a.segments + 1 <= 32 or a.rank < 1 or (a.segments + 1) * a.rank > 128:
        sys.exit("segments + 1 starts: at most 32, and at most 128 columns in total")
    cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--worker"]
    cmd += sys.argv[1:]
    return subprocess.call(cmd)


if __name__ == "__main__":
    sys.exit(main())
