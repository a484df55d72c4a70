"""Exact (multi-sweep) ALS sweeps/s with the tensor stored as F32 and as BF16, in one process, same seeds.

Runs: the headline (order 4, s = 200, R = 10) in F32 then BF16, under the multi-sweep schedule and under
the two-node DT schedule (whose first-level scans keep only s^2 rows: the K-split case); order 3 at
s = 800, R = 10 (a kept mode of s rows); R = 100 at s = 200 in both storages; BASELINE configs[3]
(order 4, s = 400, R = 20) in both storages. Per run: a timed
block of sweeps (wall clock around ppals_ctx_sync), then the same number of sweeps again with the scan
profiler on, which reports the scans' time and algorithmic bytes (the tensor at its storage size plus
the result written): `scan_frac` = those bytes / scan time / 8 TB/s. One JSON line per run. For one
kernel's own time per launch, run it under `rocprofv3 --kernel-trace --stats -- python ...`.

    python tools/bf16_bench.py [--steps 10] [--warmup 3] [--only headline|dt|order3|r100|cfg3]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pairwise-perturbation_amd"))
import ppals as pp  # noqa: E402

PEAK = 8.0e12  # MI355X HBM3E, bytes/s
RUNS = {
    "headline": [([200] * 4, 10, pp.F32, "msdt"), ([200] * 4, 10, pp.BF16, "msdt")],
    "dt": [([200] * 4, 10, pp.F32, "dt"), ([200] * 4, 10, pp.BF16, "dt")],
    "order3": [([800] * 3, 10, pp.F32, "msdt"), ([800] * 3, 10, pp.BF16, "msdt")],
    "r100": [([200] * 4, 100, pp.F32, "msdt"), ([200] * 4, 100, pp.BF16, "msdt")],
    "cfg3": [([400] * 4, 20, pp.F32, "msdt"), ([400] * 4, 20, pp.BF16, "msdt")],
}
ORDER = ["headline", "dt", "order3", "r100", "cfg3"]


def one(ctx, lens, R, dtype, schedule, steps, warmup):
    V = pp.Tensor(ctx, lens, dtype).fill_cp(pp.init_factors(lens, R, 1000))
    cp = pp.CP(ctx, V, R)
    cp.set_schedule(schedule)
    cp.set_factors(pp.init_factors(lens, R, 2000), pp.init_factors(lens, R, 3000))
    cp.sweeps_dt(warmup)
    ctx.sync()
    t0 = time.perf_counter()
    cp.sweeps_dt(steps)
    ctx.sync()
    dt = (time.perf_counter() - t0) / steps
    ctx.profile_reset()
    ctx.profile_enable(1)
    cp.sweeps_dt(steps)
    ctx.sync()
    ctx.profile_enable(0)
    launches, scan_ms, scan_bytes = ctx.profile_read(0)
    rec = dict(lens=lens, R=R, storage={pp.F32: "f32", pp.BF16: "bf16"}[dtype], schedule=schedule, steps=steps,
               ms_per_sweep=1e3 * dt, sweeps_per_s=1.0 / dt, scan_launches=launches,
               scan_ms_per_sweep=scan_ms / steps,
               scan_frac=(scan_bytes / (scan_ms * 1e-3) / PEAK) if scan_ms > 0 else None)
    cp.close()
    V.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=sorted(RUNS), default=None)
    a = ap.parse_args()
    ctx = pp.Context(0)
    for name in ([a.only] if a.only else ORDER):
        for lens, R, dtype, schedule in RUNS[name]:
            rec = one(ctx, lens, R, dtype, schedule, a.steps, a.warmup)
            rec["run"] = name
            print(json.dumps(rec), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
