"""Time of the wide-column N-PLS passes and of N-PLS cross-validation, for every sample mode, in one process:

* Tensor.contract_columns / slice_inner_columns at C = 8, 16 and 64 against the narrow passes (Tensor.contract_mode /
  slice_inner, chunks of NPLS_CW = 4 columns) at the same C and against torch's matmul in fp32 on the exported tensor
  (tensordot / movedim + reshape + matmul);
* a 7-segment, F = 5, M = 1 cross-validation (ppals.npls_crossval) against the route it replaces: per segment a
  reduced tensor through torch (index_select, Tensor.from_torch), Tensor.center, ppals.npls, and NPLS.predict of the
  held-out samples for 1 .. F components.

torch is imported first (one HIP runtime for both). The passes are timed on the device by the engine's own profile
events around the op (ppals_profile_read, slot 0): the host pointers of the C ABI make a call's wall time mostly the
copy of the thin operand and of the result. The torch calls are timed with torch.cuda.Event pairs; a torch call whose
first run takes more than two seconds is not repeated. The two cross-validation routes are wall time, the export of
the tensor to torch not counted. Best of --reps; the routes alternate within one process.

    python tools/npls_cv_bench.py [--s 200] [--reps 3] [--coil] [--out profiles]

Writes <out>/npls_cv_bench.jsonl and <out>/npls_cv_bench.md (the tables; what follows a line `## Notes` in an
existing file is kept)."""
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
COLUMNS = (8, 16, 64)
RECS = []


def rec(**kw):
    print(json.dumps(kw), flush=True)
    RECS.append(kw)


def device_ms(ctx, fn, reps):
    """best device time of the engine's profiled ops inside fn"""
    fn()
    dev = []
    for _ in range(reps):
        ctx.profile_reset()
        fn()
        dev.append(ctx.profile_read(0)[1])
    return min(dev)


def torch_ms(fn, reps):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    first = (time.perf_counter() - t0) * 1e3
    if first > 2000:
        return first
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


def parent_route(ctx, t, x, Y, F, mode, seg, S):
    """leave-segments-out by the calls that existed before: reduce through torch, centre, fit, predict"""
    I = Y.shape[0]
    Ycv = np.zeros((I, Y.shape[1], F))
    for s in range(S):
        tr = np.flatnonzero(seg != s)
        ho = np.flatnonzero(seg == s)
        dev = x.device
        ttr = pp.Tensor.from_torch(ctx, x.index_select(mode, torch.from_numpy(tr).to(dev)))
        off = ttr.center(mode, "torch")
        my = Y[tr].mean(axis=0, keepdims=True)
        m = pp.npls(ttr, Y[tr] - my, F, mode)
        tho = pp.Tensor.from_torch(ctx, x.index_select(mode, torch.from_numpy(ho).to(dev)))
        tho.shift(mode, off, -1.0)
        for k in range(1, m.ncomp + 1):
            Ycv[ho, :, k - 1] = m.predict(tho, ncomp=k) + my
        for k in range(m.ncomp, F):
            Ycv[ho, :, k] = Ycv[ho, :, k - 1] if k else my
        for h in (m, ttr, tho):
            h.close()
    return Ycv


def bench(ctx, name, lens, reps):
    n = int(np.prod(lens))
    nbytes = 4 * n
    rng = np.random.default_rng(0)
    R = 8
    Wt = pp.collinear_factors(list(lens), R, seed=0)
    t = pp.Tensor(ctx, list(lens), pp.F32).fill_collinear(R, ratio_noise=0.01, seed=0)
    ctx.sync()
    x = t.to_torch()
    torch.cuda.synchronize()
    for mode in range(len(lens)):
        L, I, T = t._prep_shape(mode)[:3]
        LT = L * T
        base = dict(case=name, shape=list(lens), mode=mode, L=L, I=I, T=T)
        ctx.profile_enable(1)
        for Cn in COLUMNS:
            for op in ("contract", "slice_inner"):
                A = np.asfortranarray(rng.standard_normal((I if op == "contract" else LT, Cn)))
                Ad = torch.from_numpy(A).to(x.device, torch.float32)
                if op == "contract":
                    wide = device_ms(ctx, lambda: t.contract_columns(mode, A), reps)
                    narrow = device_ms(ctx, lambda: t.contract_mode(mode, A), reps)
                    tms = torch_ms(lambda: torch.tensordot(x, Ad, dims=([mode], [0])), reps)
                else:
                    wide = device_ms(ctx, lambda: t.slice_inner_columns(mode, A), reps)
                    narrow = device_ms(ctx, lambda: t.slice_inner(mode, A), reps)
                    tms = torch_ms(lambda: x.movedim(mode, 0).reshape(I, LT) @ Ad, reps)
                rec(**base, op=op, C=Cn, wide_ms=round(wide, 3), narrow_ms=round(narrow, 3), torch_ms=round(tms, 3),
                    of_peak=round(nbytes / (wide * 1e-3) / PEAK, 3))
                del A, Ad
                torch.cuda.empty_cache()
        ctx.profile_enable(0)
        # cross-validation: 7 segments, F = 5, M = 1, centred
        S, F = min(7, I), 5
        seg = np.arange(I) % S
        F = max(1, min(F, I - int(np.max(np.bincount(seg))) - 1))
        Y = np.array(Wt[mode][:, :1] + 0.3 * Wt[mode][:, 1:2])
        new, old, r, ref = [], [], None, None
        for _ in range(reps):
            ctx.sync()
            t0 = time.perf_counter()
            r = pp.npls_crossval(t, Y, F, mode=mode, segments=seg, center=True)
            new.append((time.perf_counter() - t0) * 1e3)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ref = parent_route(ctx, t, x, Y, F, mode, seg, S)
            old.append((time.perf_counter() - t0) * 1e3)
        dev = float(np.max(np.abs(r.Ycv - ref)) / np.max(np.abs(ref)))
        rec(**base, op="crossval", S=S, F=F, M=1, crossval_ms=round(min(new), 1), per_segment_ms=round(min(old), 1),
            x_passes=r.x_passes, fitted=[int(v) for v in r.fitted], status_any=bool(np.any(r.status)),
            best_ncomp=r.best_ncomp, deviation=dev)
    del x
    t.close()
    torch.cuda.empty_cache()


def write(out):
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "npls_cv_bench.jsonl"), "w") as f:
        for r in RECS:
            f.write(json.dumps(r) + "\n")
    path = os.path.join(out, "npls_cv_bench.md")
    notes = ""
    if os.path.exists(path):
        old = open(path).read()
        if "\n## Notes" in old:
            notes = old[old.index("\n## Notes"):]
    lines = ["# Wide-column N-PLS passes and N-PLS cross-validation", "",
             "`python tools/npls_cv_bench.py --coil`, one MI355X, one process, F32 storage (`npls_cv_bench.jsonl` holds the",
             "JSON lines). Passes: device time of the op by the engine's profile events, best run; wide: the `_columns`",
             "calls, narrow: the existing calls in chunks of 4 columns; \"of 8 TB/s\" is the wide pass on the bytes it must",
             "read, the tensor once. torch: `tensordot` / `movedim + reshape + matmul` in fp32 on the exported tensor.",
             "Cross-validation: 7 segments, F = 5, M = 1, centred, wall time, against a reduced tensor per segment through",
             "torch, centred, fitted and predicted with the existing calls; `deviation` is the largest difference of the",
             "two routes' predictions relative to the largest prediction (the per-segment route rounds its centred copy",
             "to fp32).", ""]
    for name in dict.fromkeys(r["case"] for r in RECS):
        rs = [r for r in RECS if r["case"] == name]
        lines += [f"## {name}, {' x '.join(map(str, rs[0]['shape']))}", "",
                  "| sample mode | [L, I, T] | op | wide ms | of 8 TB/s | narrow ms | torch ms | fastest |", "|---|---|---|---|---|---|---|---|"]
        for r in rs:
            ljt = f"{r['L']}, {r['I']}, {r['T']}"
            if r["op"] == "crossval":
                lines.append(f"| {r['mode']} | {ljt} | cross-validation S = {r['S']}, F = {r['F']} | {r['crossval_ms']} wall, "
                             f"{r['x_passes']} passes | | per segment: {r['per_segment_ms']} wall | | deviation {r['deviation']:.1e} |")
            else:
                best = min(("wide", r["wide_ms"]), ("narrow", r["narrow_ms"]), ("**torch**", r["torch_ms"]), key=lambda p: p[1])[0]
                lines.append(f"| {r['mode']} | {ljt} | `{r['op']}` C = {r['C']} | {r['wide_ms']} | {r['of_peak']} | {r['narrow_ms']} | "
                             f"{r['torch_ms']} | {best} |")
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
