#!/usr/bin/env python3
"""What do the packed twins of the resident layouts (PPALS_PACK_LAYOUT) give on the headline problem?
ONE process, the cfg2 tensor resident (so every session scans the same physical buffer), sessions
created alternately with PPALS_PACK_LAYOUT=0 and =1: `warm` sweeps to let the online placement
choice settle, then `sweeps` settled sweeps between two synchronises. Every session printed, medians
and the pass criterion (every packed session faster than every plain one) at the end; the factors of
all sessions must be the same bits.   usage: tools/pack_ab.py [pairs=6] [sweeps=50] [warm=80]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pairwise-perturbation_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401
import ppals  # noqa: E402


def main():
    pairs = int(sys.argv[1]) if len(sys.argv) > 1 else 6
    sweeps = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    warm = int(sys.argv[3]) if len(sys.argv) > 3 else 80
    lens, R = [200] * 4, 10
    ctx = ppals.Context(0)
    V = ppals.Tensor(ctx, lens, ppals.F32).fill_cp(ppals.init_factors(lens, R, 1000))
    W0, G0 = ppals.init_factors(lens, R, 2000), ppals.init_factors(lens, R, 3000)
    ms = {"0": [], "1": []}
    setup = {"0": [], "1": []}
    ref = None
    same = True
    for p in range(pairs):
        for env in (("0", "1") if p % 2 == 0 else ("1", "0")):
            os.environ["PPALS_PACK_LAYOUT"] = env
            ctx.sync()
            t0 = time.perf_counter()
            cp = ppals.CP(ctx, V, R)
            ctx.sync()
            t1 = time.perf_counter()
            cp.set_factors(W0, G0)
            cp.sweeps_dt(warm)
            ctx.sync()
            t2 = time.perf_counter()
            cp.sweeps_dt(sweeps)
            ctx.sync()
            t3 = time.perf_counter()
            W = np.concatenate([w.ravel() for w in cp.get_factors()]).tobytes()
            rep = cp.placement_report()["packed"]
            cp.close()
            ref = W if ref is None else ref
            same = same and W == ref
            ms[env].append(1e3 * (t3 - t2) / sweeps)
            setup[env].append(t1 - t0)
            print(f"pair {p} PACK_LAYOUT={env}: create {t1 - t0:.3f} s, settled {ms[env][-1]:.4f} ms/sweep, "
                  f"twins {sum(1 for r in rep['layouts'] if r['packed'])}, factors {'same' if W == ref else 'DIFFER'}",
                  flush=True)
    m0, m1 = statistics.median(ms["0"]), statistics.median(ms["1"])
    print(f"plain : median {m0:.4f} ms/sweep (min {min(ms['0']):.4f}, max {max(ms['0']):.4f}), create median "
          f"{statistics.median(setup['0']):.3f} s")
    print(f"packed: median {m1:.4f} ms/sweep (min {min(ms['1']):.4f}, max {max(ms['1']):.4f}), create median "
          f"{statistics.median(setup['1']):.3f} s")
    ok = max(ms["1"]) < min(ms["0"])
    print(f"median gain {100 * (m0 / m1 - 1):.2f} % sweeps/s; every packed session faster than every plain one: "
          f"{'yes' if ok else 'NO'}; factors the same bits in all sessions: {'yes' if same else 'NO'}")
    return 0 if ok and same else 1


if __name__ == "__main__":
    sys.exit(main())
