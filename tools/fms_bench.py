#!/usr/bin/env python3
"""The factor match score of all pairs of starts in ONE call against the same matrix on the host
(profiles/fms_bench.md).

One process creates the workload once — a multi-start session of --starts starts of rank --rank after
--sweeps sweeps — and, after one warm-up of both sides (buffers, code objects), alternates `--reps`
repetitions each of
  device   one CPMulti.fms(): two launches on the factors in HBM, one download of Phi, w_a, w_b, the
           matching of every pair on the host (ppals_cp_multi_fms)
  host     get_factors of every start, the congruence in numpy (one cross-Gram per mode of the stacked
           factors), the same matching through ppals_match_columns
and then of
  sweep    one sweep of the session, for scale.
Every timed call ends with its result on the host (the sweep is followed by a device synchronise). Then one
more device call under the launch profile's counters. Prints one JSON line. The measuring process runs
under its own `timeout`.
`--trace-calls K`: set-up, one warm-up call, K device calls and nothing else — for a run under
`rocprofv3 --kernel-trace --stats`.

  python tools/fms_bench.py --lens 200,200,200,200 --starts 12 --rank 10
  python tools/fms_bench.py --lens 3,128,128,7200 --starts 12 --rank 10
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
    ap.add_argument("--lens", type=str, default="200,200,200,200", help="comma-separated extents")
    ap.add_argument("--starts", type=int, default=12)
    ap.add_argument("--rank", type=int, default=10)
    ap.add_argument("--dtype", choices=sorted(DTYPES), default="f32")
    ap.add_argument("--sweeps", type=int, default=2, help="sweeps of the session before the calls")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trace-calls", type=int, default=0)
    ap.add_argument("--timeout", type=int, default=480, help="seconds the measuring process may take")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    return ap.parse_args(argv)


def host_fms(pp, np, multi):
    """the K x K scores from the downloaded factors: numpy for the congruence, the library's matcher"""
    K, N = multi.nstarts, len(multi.lens)
    S = [multi.get_factors(b) for b in range(K)]
    phi = 1.0
    for i in range(N):
        A = np.hstack([S[b][i] for b in range(K)])
        n = np.sqrt(np.sum(A * A, axis=0))
        phi = phi * ((A.T @ A) / n[:, None] / n[None, :])
    off = np.concatenate([[0], np.cumsum(multi.ranks)])
    out = np.empty((K, K))
    for x in range(K):
        for y in range(K):
            blk = phi[off[x]:off[x + 1], off[y]:off[y + 1]]
            out[x, y] = pp.match_columns(blk)[1] / min(blk.shape)
    return out


def worker(a):
    sys.path.insert(0, os.path.join(ROOT, "pairwise-perturbation_amd"))
    import numpy as np
    import ppals as pp
    lens = [int(x) for x in a.lens.split(",")]
    ctx = pp.Context(0)
    t = pp.Tensor(ctx, lens, DTYPES[a.dtype]).fill_cp(pp.init_factors(lens, a.rank, 1000))
    multi = pp.CPMulti(ctx, t, a.rank, a.starts)
    multi.set_factors(-1, [pp.init_factors(lens, a.rank, 2000 + 31 * b) for b in range(a.starts)])
    multi.sweeps(a.sweeps)
    warm = multi.fms()
    if a.trace_calls:
        for _ in range(a.trace_calls):
            multi.fms()
        print(json.dumps({"tool": "fms_bench", "trace_calls": a.trace_calls}), flush=True)
        multi.close()
        t.close()
        ctx.close()
        return
    warm_host = host_fms(pp, np, multi)

    def timed(fn):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        return time.perf_counter() - t0

    td, th, tw = [], [], []
    for _ in range(a.reps):
        td.append(timed(multi.fms))
        th.append(timed(lambda: host_fms(pp, np, multi)))
    ctx.sync()
    ctx.profile_enable(2)
    ctx.profile_reset()
    multi.fms()
    ctx.sync()
    scan, other = ctx.profile_read(0), ctx.profile_read(1)
    ctx.profile_enable(0)
    for _ in range(a.reps):   # (last: the sweeps move the session's factors on)
        tw.append(timed(lambda: multi.sweeps(1)))
    med = statistics.median
    offdiag = warm[~np.eye(a.starts, dtype=bool)]
    out = {
        "tool": "fms_bench", "lens": lens, "starts": a.starts, "rank": a.rank, "columns": a.starts * a.rank,
        "dtype": a.dtype, "reps": a.reps,
        "device_ms": 1e3 * med(td), "host_ms": 1e3 * med(th), "sweep_ms": 1e3 * med(tw),
        "device_min_max_ms": [1e3 * min(td), 1e3 * max(td)], "host_min_max_ms": [1e3 * min(th), 1e3 * max(th)],
        "sweep_min_max_ms": [1e3 * min(tw), 1e3 * max(tw)],
        "ratio_host_over_device": med(th) / med(td), "device_over_sweep": med(td) / med(tw),
        "profile_device": {"scan_launches": scan[0], "other_launches": other[0], "other_ms": other[1],
                           "other_bytes": other[2]},
        "max_difference": float(np.max(np.abs(warm - warm_host))),
        "fms_offdiagonal_min_max": [float(offdiag.min()), float(offdiag.max())],
        "factor_bytes_downloaded_by_host_side": 8 * sum(lens) * a.starts * a.rank,
    }
    print(json.dumps(out), flush=True)
    multi.close()
    t.close()
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
