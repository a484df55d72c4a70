"""Cost of ppals_parafac2_step_ragged_device (PARAFAC2 on slices of unequal length) against the route it replaces:
the same slices zero-padded to the longest and stepped with ppals_parafac2_step_device.

torch is imported first (one HIP runtime for both). Every figure is wall time around a device synchronisation of
both the caller's stream and the engine's. The cases of a configuration are INTERLEAVED: each round runs every
case once, in turn; a case's figure is the median over the rounds after the first (warm-up), its spread the range
min .. max over them. Configurations, f32 data, F32 storage, J = 2000, K = 400, R = 10:
  (a) rows drawn once from seed 1, uniform in [500, 2000]: `ragged` (the packed list) against `padded` (zero-padded
      to 2000 rows). The yardstick is bytes: the ragged step reads N / (K I_max) of what the padded one reads.
  (b) equal rows of 2000: `ragged` against `equal` (the existing route) on the same buffer.
  (c) the device memory each object of (a) takes (hipMemGetInfo around its creation).
The step's time by launch comes from one more step of each case under torch.profiler, after the timed rounds.

    python tools/parafac2_ragged_bench.py [--rounds 7] [--small] [--out-dir profiles]
"""
import argparse
import json
import os
import sys
import time

import torch  # noqa: I001  (before ppals: one HIP runtime)
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pairwise-perturbation_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ppals as pp  # noqa: E402
from parafac2_bench import by_launch  # noqa: E402

DEV = torch.device("cuda:0")


def sync(ctx):
    torch.cuda.synchronize()
    ctx.sync()


def made(ctx, make):
    """(the object, the device bytes its creation took)"""
    sync(ctx)
    free0 = torch.cuda.mem_get_info()[0]
    p = make()
    sync(ctx)
    return p, free0 - torch.cuda.mem_get_info()[0]


def timed(ctx, cases, rounds):
    ts = {name: [] for name, _ in cases}
    for rnd in range(rounds + 1):
        for name, fn in cases:
            sync(ctx)
            t0 = time.perf_counter()
            fn()
            sync(ctx)
            if rnd:
                ts[name].append(time.perf_counter() - t0)
    return {name: np.array(v) * 1e3 for name, v in ts.items()}


def config(ctx, label, rows, J, R, rounds, out):
    K, N, I = len(rows), int(sum(rows)), int(max(rows))
    flat = torch.rand(N * J, device=DEV)                              # the packed list, each slice column-major
    Xp = torch.zeros((K, J, I), device=DEV)                           # the same slices zero-padded, I x J x K
    o = 0
    for k, n in enumerate(rows):
        Xp[k, :, :n] = flat[o:o + n * J].view(J, n)
        o += n * J
    Xp = Xp.permute(2, 1, 0)
    pr, mem_r = made(ctx, lambda: pp.Parafac2.ragged(ctx, rows, J, R, pp.F32))
    pe, mem_e = made(ctx, lambda: pp.Parafac2(ctx, I, J, K, R, pp.F32))
    other = "equal" if N == K * I else "padded"
    cases = [("ragged", lambda: pr.step_torch(flat, want=False)), (other, lambda: pe.step_torch(Xp, want=False))]
    ts = timed(ctx, cases, rounds)
    same = pr.step_torch(flat) == pe.step_torch(Xp)                   # lost_sq, failed: equal rows give the same bits
    for name, _ in cases:
        v = ts[name]
        row = dict(config=label, case=name, J=J, K=K, R=R, N=N, I_max=I, rounds=rounds,
                   median_ms=round(float(np.median(v)), 3), min_ms=round(float(v.min()), 3),
                   max_ms=round(float(v.max()), 3), object_bytes=int(mem_r if name == "ragged" else mem_e))
        out.append(row)
        print(json.dumps(row), flush=True)
    med = {name: float(np.median(ts[name])) for name, _ in cases}
    row = dict(config=label, case="ratio", time_ratio_ragged_over_other=round(med["ragged"] / med[other], 4),
               byte_ratio_N_over_K_Imax=round(N / (K * I), 4), memory_ratio=round(mem_r / mem_e, 4),
               outputs_equal=bool(same))
    out.append(row)
    print(json.dumps(row), flush=True)
    for name, p, x in (("ragged", pr, flat), (other, pe, Xp)):
        def one():
            p.step_torch(x)
            sync(ctx)
        launches = by_launch(one)
        row = dict(config=label, case="by_launch_us_" + name, **{k: round(v, 1) for k, v in sorted(launches.items())})
        out.append(row)
        print(json.dumps(row), flush=True)
    pr.close()
    pe.close()
    del flat, Xp
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--small", action="store_true", help="J = 300, K = 40, rows in [100, 400]: a quick look")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    J, K, R, lo, hi = (300, 40, 10, 100, 400) if a.small else (2000, 400, 10, 500, 2000)
    rows = [int(r) for r in np.random.default_rng(1).integers(lo, hi + 1, K)]
    ctx = pp.Context(0)
    out = []
    config(ctx, "a_ragged_rows", rows, J, R, a.rounds, out)
    config(ctx, "b_equal_rows", [hi] * K, J, R, a.rounds, out)
    ctx.close()
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "parafac2_ragged_bench.jsonl"), "w") as f:
        for r in out:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
