"""Time of the N-PLS passes over the resident tensor (Tensor.contract_mode at C = 1 and 4, Tensor.slice_inner at C = 1
and 5), of a 5-component fit and of a prediction, for every sample mode, against the torch route they replace
(to_torch, then tensordot / movedim + reshape + matmul in fp32), in one process.

torch is imported first (one HIP runtime for both). The passes are timed on the device by the engine's own profile
events around the op (ppals_profile_read, slot 0): the host pointers of the C ABI make a call's wall time mostly the
copy of W or Z. `of_peak` is the share of the 8 TB/s HBM peak on the bytes a pass MUST read, the tensor once; a call
of more than NPLS_CW = 4 columns reads it once per chunk and shows that here. Fit and prediction are wall time
(they return with their results on the host); `passes_ms` is the device time of all their tensor-sized ops. The
torch calls are timed with torch.cuda.Event pairs. Best of --reps.

    python tools/npls_bench.py [--s 200] [--reps 3] [--coil] [--out profiles]

Writes <out>/npls_bench.jsonl and <out>/npls_bench.md (the tables; what follows a line `## Notes` in an existing
file is kept)."""
import argparse
import json
import os
import sys
import time

import torch  # noqa: I001  (before ppals: one HIP runtime)
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pairwise-perturbation_amd"))
import ppals as pp  # noqa: E402

PEAK = 8.0e12  # MI355X HBM3E, bytes/s
RECS = []


def rec(**kw):
    print(json.dumps(kw), flush=True)
    RECS.append(kw)


def device_ms(ctx, fn, reps):
    """best device time of the engine's profiled ops inside fn, and best wall time"""
    fn()
    dev, wall = [], []
    for _ in range(reps):
        ctx.profile_reset()
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(ctx.profile_read(0)[1])
    return min(dev), min(wall)


def torch_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return min(ts)


def bench(ctx, name, lens, reps):
    n = int(np.prod(lens))
    nbytes = 4 * n
    rng = np.random.default_rng(0)
    # 8 collinear components and 1 % noise (the `-tensor c` fill); the response is the first sample-mode factor column
    R = 8
    Wt = pp.collinear_factors(list(lens), R, seed=0)
    t = pp.Tensor(ctx, list(lens), pp.F32).fill_collinear(R, ratio_noise=0.01, seed=0)
    ctx.sync()
    ctx.profile_enable(1)
    x = t.to_torch()
    torch.cuda.synchronize()
    for mode in range(len(lens)):
        L, I, T = t._prep_shape(mode)[:3]
        LT = L * T
        base = dict(case=name, shape=list(lens), mode=mode, L=L, I=I, T=T)
        col = rng.standard_normal(LT)
        for op, C in (("contract", 1), ("contract", 4), ("slice_inner", 1), ("slice_inner", 5)):
            if op == "contract":
                A = np.asfortranarray(rng.standard_normal((I, C)))
                ms, wall = device_ms(ctx, lambda: t.contract_mode(mode, A), reps)
                Ad = torch.from_numpy(A).to(x.device, torch.float32)
                tms = torch_ms(lambda: torch.tensordot(x, Ad, dims=([mode], [0])), reps)
            else:
                A = np.empty((LT, C), order="F")
                A[:] = col[:, None]
                ms, wall = device_ms(ctx, lambda: t.slice_inner(mode, A), reps)
                Ad = torch.from_numpy(col).to(x.device, torch.float32)[:, None].repeat(1, C)
                tms = torch_ms(lambda: x.movedim(mode, 0).reshape(I, LT) @ Ad, reps)
                del A
            rec(**base, op=op, C=C, ms=round(ms, 3), call_wall_ms=round(wall, 1), GBps=round(nbytes / ms / 1e6, 1),
                of_peak=round(nbytes / (ms * 1e-3) / PEAK, 3), torch_ms=round(tms, 3))
            del Ad
            torch.cuda.empty_cache()
        F = min(5, I)
        t.center(mode)
        Y = np.array(Wt[mode][:, :1] + 0.3 * Wt[mode][:, 1:2])
        Y -= Y.mean(axis=0)
        model = []

        def fit():
            for m in model:
                m.close()
            model[:] = [pp.npls(t, Y, F, mode)]
        ms, wall = device_ms(ctx, fit, reps)
        m = model[0]
        rec(**base, op="fit", F=int(m.ncomp), M=1, wall_ms=round(wall, 2), passes_ms=round(ms, 3),
            status=[int(s) for s in m.status], ssy=round(float(m.ssy[-1]), 4) if m.ncomp else None)
        if m.ncomp:
            ms, wall = device_ms(ctx, lambda: m.predict(t), reps)
            rec(**base, op="predict", F=int(m.ncomp), wall_ms=round(wall, 2), passes_ms=round(ms, 3),
                of_peak=round(nbytes / (ms * 1e-3) / PEAK, 3))
        m.close()
        t.fill_collinear(R, ratio_noise=0.01, seed=0)
    ctx.profile_enable(0)
    del x
    t.close()
    torch.cuda.empty_cache()


def write(out):
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "npls_bench.jsonl"), "w") as f:
        for r in RECS:
            f.write(json.dumps(r) + "\n")
    path = os.path.join(out, "npls_bench.md")
    notes = ""
    if os.path.exists(path):
        old = open(path).read()
        if "\n## Notes" in old:
            notes = old[old.index("\n## Notes"):]
    lines = ["# N-PLS passes, fit and prediction against the torch route", "",
             "`python tools/npls_bench.py --coil`, one MI355X, one process, F32 storage (`npls_bench.jsonl` holds the JSON",
             "lines). Passes: device time of the op by the engine's profile events, best run; \"of 8 TB/s\" on the bytes a",
             "pass must read, the tensor once. torch: `tensordot` / `movedim + reshape + matmul` in fp32 on the exported",
             "tensor, the export not counted. Fit (M = 1) and prediction: wall time, and the device time of their",
             "tensor-sized ops.", ""]
    for name in dict.fromkeys(r["case"] for r in RECS):
        rs = [r for r in RECS if r["case"] == name]
        lines += [f"## {name}, {' x '.join(map(str, rs[0]['shape']))}", "",
                  "| sample mode | [L, I, T] | op | ms | GB/s | of 8 TB/s | torch ms | faster |", "|---|---|---|---|---|---|---|---|"]
        for r in rs:
            ljt = f"{r['L']}, {r['I']}, {r['T']}"
            if r["op"] in ("contract", "slice_inner"):
                lines.append(f"| {r['mode']} | {ljt} | `{r['op']}` C = {r['C']} | {r['ms']} | {r['GBps']} | {r['of_peak']} | "
                             f"{r['torch_ms']} | {'**torch**' if r['torch_ms'] < r['ms'] else 'ppals'} |")
            elif r["op"] == "fit":
                lines.append(f"| {r['mode']} | {ljt} | fit, F = {r['F']} | {r['wall_ms']} wall, {r['passes_ms']} in passes | | | | |")
            else:
                lines.append(f"| {r['mode']} | {ljt} | predict, F = {r['F']} | {r['wall_ms']} wall, {r['passes_ms']} in the pass | | "
                             f"{r['of_peak']} | | |")
        lines.append("")
    with open(path, "w") as f:
        f.write("\n".join(lines) + notes + ("" if notes.endswith("\n") or not notes else "\n"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--s", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--coil", action="store_true", help="also the coil-100 extents 3 x 128 x 128 x 7200")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    ctx = pp.Context(0)
    bench(ctx, "headline", (a.s,) * 4, a.reps)
    if a.coil:
        bench(ctx, "coil100", (3, 128, 128, 7200), a.reps)
    ctx.close()
    write(a.out)


if __name__ == "__main__":
    main()
