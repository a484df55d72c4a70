#!/usr/bin/env python3
"""What do the packed twins of the resident layouts (PPALS_PACK_LAYOUT) give on the headline problem?
ONE process, the cfg2 tensor resident (so every session scans the same physical buffer), sessions
created alternately with two values of PPALS_PACK_LAYOUT — `--a` against `--b`, by default 0 (never
pack) against unset (the engine's own rule: 26-bit twins where they qualify); `--a 0 --b 1` is the
plain-against-28-bit comparison, `--a 1 --b unset` 28 against 26 bits. Per session `warm` sweeps to
let the online placement choice settle, then `sweeps` settled sweeps between two synchronises. Every
session printed, medians and the pass criterion (every b session faster than every a session) at the
end; the factors of all sessions must be the same bits.
usage: tools/pack_ab.py [pairs=6] [sweeps=50] [warm=80] [--a VALUE] [--b VALUE]   (VALUE: 0, 1, 2 or unset)"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pairwise-perturbation_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401
import ppals  # noqa: E402


def set_switch(value):
    if value == "unset":
        os.environ.pop("PPALS_PACK_LAYOUT", None)
    else:
        os.environ["PPALS_PACK_LAYOUT"] = value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("pairs", nargs="?", type=int, default=6)
    ap.add_argument("sweeps", nargs="?", type=int, default=50)
    ap.add_argument("warm", nargs="?", type=int, default=80)
    ap.add_argument("--a", default="0", choices=["0", "1", "2", "unset"])
    ap.add_argument("--b", default="unset", choices=["0", "1", "2", "unset"])
    ap.add_argument("--all-escapes", action="store_true",
                    help="odd slices of every mode scaled by 2^-6 (three top bytes per mode): a block mixes slices of two "
                         "or three modes, spans 6..13 top bytes and has an escape plane (prices the escape decode at a "
                         "share of about 1; the report gives the count)")
    args = ap.parse_args()
    a, b = args.a, args.b
    lens, R = [200] * 4, 10
    ctx = ppals.Context(0)
    V = ppals.Tensor(ctx, lens, ppals.F32).fill_cp(ppals.init_factors(lens, R, 1000))
    if args.all_escapes:
        for m in range(4):
            V.rescale(m, np.where(np.arange(lens[m]) % 2 == 1, 2.0 ** -6, 1.0))
    W0, G0 = ppals.init_factors(lens, R, 2000), ppals.init_factors(lens, R, 3000)
    ms = {a: [], b: []}
    setup = {a: [], b: []}
    ref = None
    same = True
    for p in range(args.pairs):
        for env in ((a, b) if p % 2 == 0 else (b, a)):
            set_switch(env)
            ctx.sync()
            t0 = time.perf_counter()
            cp = ppals.CP(ctx, V, R)
            ctx.sync()
            t1 = time.perf_counter()
            cp.set_factors(W0, G0)
            cp.sweeps_dt(args.warm)
            ctx.sync()
            t2 = time.perf_counter()
            cp.sweeps_dt(args.sweeps)
            ctx.sync()
            t3 = time.perf_counter()
            W = np.concatenate([w.ravel() for w in cp.get_factors()]).tobytes()
            rep = cp.placement_report()["packed"]
            cp.close()
            ref = W if ref is None else ref
            same = same and W == ref
            ms[env].append(1e3 * (t3 - t2) / args.sweeps)
            setup[env].append(t1 - t0)
            twins = [r for r in rep["layouts"] if r["packed"]]
            print(f"pair {p} PACK_LAYOUT={env}: create {t1 - t0:.3f} s, settled {ms[env][-1]:.4f} ms/sweep, "
                  f"twins {len(twins)} formats {sorted({r.get('format', 28) for r in twins})} "
                  f"escape blocks {[r.get('escape_blocks', 0) for r in twins]} of "
                  f"{[(r['rows'] + 255) // 256 * r['batches'] * ((r['reduced'] + 15) // 16) for r in twins]}, "
                  f"factors {'same' if W == ref else 'DIFFER'}", flush=True)
    ma, mb = statistics.median(ms[a]), statistics.median(ms[b])
    for name, m in ((a, ma), (b, mb)):
        print(f"PACK_LAYOUT={name}: median {m:.4f} ms/sweep (min {min(ms[name]):.4f}, max {max(ms[name]):.4f}), "
              f"create median {statistics.median(setup[name]):.3f} s")
    ok = max(ms[b]) < min(ms[a])
    print(f"median gain of {b} over {a}: {100 * (ma / mb - 1):.2f} % sweeps/s; every {b} session faster than every "
          f"{a} one: {'yes' if ok else 'NO'}; factors the same bits in all sessions: {'yes' if same else 'NO'}")
    return 0 if ok and same else 1


if __name__ == "__main__":
    sys.exit(main())
