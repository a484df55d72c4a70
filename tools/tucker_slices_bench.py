"""The influence plot of a Tucker session against the route through torch and against the imputation
(profiles/tucker_slice_residuals_bench.md; raw lines in tucker_slice_residuals_bench.jsonl beside it).

torch is imported first (one HIP runtime for both). Every figure is wall time around a device synchronisation
of both torch's stream and the engine's, best and median of --reps calls after a warm-up call. Per shape:
  a  Tucker.slice_residuals()                 one pass over the tensor, sums only
  b  export_model_torch(residual=True), square_, N sums, into preallocated tensors: the route without the call
  c  impute_torch(first-index-fastest mask, want_residual=True): the same bytes plus a mask, and stores
  d  Tucker.leverages() against get_factors() and a numpy QR
and the pass kernels one call of (a) launches, counted by name in a torch.profiler trace, with the tensor's
bytes (read exactly once) over the call's best time.

    python tools/tucker_slices_bench.py [--shapes cfg4,coil100] [--reps 5]
    python tools/tucker_slices_bench.py --resources     (no GPU: the kernels' resource lines, from the compiler)
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pairwise-perturbation_amd")
OUT_MD = os.path.join(ROOT, "profiles", "tucker_slice_residuals_bench.md")
OUT_JSONL = os.path.join(ROOT, "profiles", "tucker_slice_residuals_bench.jsonl")
OUT_RES = os.path.join(ROOT, "profiles", "tucker_slices_kernel_resources.txt")
KEPT = "<!-- below this line: kept by hand, the tool does not rewrite it -->"

# BASELINE configs[4] (order 3, s = 400, core 20^3) and the coil-100 extents with the reference's Tucker ranks
SHAPES = {"cfg4": ([400, 400, 400], [20, 20, 20]), "coil100": ([3, 128, 128, 7200], [3, 10, 10, 70])}
PEAK = 8e12  # bytes / s


def resources():
    out = subprocess.run([sys.executable, os.path.join(PKG, "kernel_resources.py")], capture_output=True, text=True,
                         check=True).stdout
    keep = ("k_model_slices", "k_model_impute_wide", "k_slice_fold", "k_fold_slice_sums", "k_row_dots")
    rows = [l for l in out.splitlines() if l.replace("ppals::", "").startswith(keep)]
    with open(OUT_RES, "w") as f:
        f.write("Kernel resources of a Tucker session's influence plot (ppals_tucker_slice_residuals), gfx950, beside\n"
                "the imputation's wide kernel; pairwise-perturbation_amd/kernel_resources.py\n\n" + "\n".join(rows) + "\n")
    print("\n".join(rows))


def measure(name, reps):
    import torch  # noqa: I001  (before ppals: one HIP runtime)
    import numpy as np
    sys.path.insert(0, PKG)
    import ppals as pp
    dev = torch.device("cuda:0")
    lens, ranks = SHAPES[name]
    n, N = int(np.prod(lens)), len(lens)
    pp.preload_eigensolver()
    ctx = pp.Context(0)

    def sync():
        torch.cuda.synchronize()
        ctx.sync()

    def timed(fn):
        ts = []
        for _ in range(reps + 1):   # the first one warms up (workspaces, offset tables, chain buffers)
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            ts.append(time.perf_counter() - t0)
        return round(min(ts[1:]) * 1e3, 3), round(float(np.median(ts[1:])) * 1e3, 3)

    t = pp.Tensor(ctx, lens, pp.F32).fill_uniform(7)
    k = pp.Tucker(ctx, t, ranks)
    g = np.random.default_rng(1)   # orthonormal factors and the core that belongs to them: no eigensolver in the way
    k.set_factors([np.linalg.qr(g.standard_normal((s, r)))[0] for s, r in zip(lens, ranks)])
    k.set_core(None)
    rec = {"tool": "tucker_slices_bench", "shape": name, "lens": lens, "ranks": ranks, "storage": "F32", "reps": reps}
    rec["a_slice_residuals_ms"] = timed(k.slice_residuals)
    # the pass kernels of one call, counted by name in a torch.profiler trace (the launch profile's slot 1 also books
    # the chain that builds Z); the bytes are the tensor's, which the pass reads exactly once
    from torch.profiler import ProfilerActivity, profile
    sync()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        ss, total = k.slice_residuals(return_total=True)
        sync()
    names = [e.name for e in prof.events() if "k_model_slices" in e.name]
    launches, nbytes = len(names), 4 * n
    best = rec["a_slice_residuals_ms"][0] * 1e-3
    rec["total_against_residual_sq_relative"] = abs(total - k.residual() ** 2) / total
    rec.update(a_pass_launches=launches, a_pass_kernel="k_model_slices_wide" if any("_wide" in x for x in names)
               else "k_model_slices", a_tensor_bytes_per_element=nbytes / n,
               a_GBps=round(nbytes / best / 1e9, 1), a_share_of_8TBps=round(nbytes / best / PEAK, 4))

    res = torch.empty(lens[::-1], dtype=torch.float32, device=dev).permute(*range(N - 1, -1, -1))  # first index fastest
    sums = [torch.empty(lens[i], dtype=torch.float32, device=dev) for i in range(N)]

    def by_hand():
        k.export_model_torch(res, residual=True)
        res.square_()
        for i in range(N):
            torch.sum(res, dim=[d for d in range(N) if d != i], out=sums[i])
    rec["b_torch_route_ms"] = timed(by_hand)
    rec["b_extra_bytes"] = 4 * n
    rec["a_vs_b_largest_relative_difference"] = max(
        float(np.max(np.abs(s.double().cpu().numpy() - a) / a)) for s, a in zip(sums, ss))
    del res
    torch.cuda.empty_cache()

    rec["d_leverages_ms"] = timed(k.leverages)

    def lev_by_hand():
        W, _ = k.get_factors()
        return [np.sum(np.linalg.qr(w)[0] ** 2, axis=1) for w in W]
    rec["d_get_factors_numpy_ms"] = timed(lev_by_hand)

    base = torch.rand(lens, device=dev) >= 0.3
    ff = torch.empty_strided(lens, [int(np.prod(lens[:i])) for i in range(N)], dtype=torch.bool, device=dev)
    ff.copy_(base)
    rec["c_impute_with_residual_ff_mask_ms"] = timed(lambda: k.impute_torch(ff, want_residual=True))
    k.close()
    t.close()
    ctx.close()
    print(json.dumps(rec), flush=True)


def write_md(recs, reps, out_md):
    kept = ""
    if os.path.exists(OUT_MD):   # (the hand-kept part always comes from the committed profile)
        old = open(OUT_MD).read()
        if KEPT in old:
            kept = old.split(KEPT, 1)[1]
    L = ["# Influence plot of a Tucker session (`ppals_tucker_slice_residuals`, `ppals_tucker_leverages`)", "",
         f"`python tools/tucker_slices_bench.py --reps {reps}` on one MI355X (gfx950), a process per shape, F32 storage, a",
         "session holding random orthonormal factors and the core that belongs to them. Wall time around a device synchronisation, best (median) of the",
         f"{reps} calls after a warm-up call, in ms; raw lines: `tucker_slice_residuals_bench.jsonl`; the kernels'",
         "registers and LDS: `tucker_slices_kernel_resources.txt`.", "",
         "| shape | ranks | (a) `slice_residuals()` | (b) residual export, `square_`, N sums in torch | b / a | "
         "(c) `impute_torch(ff mask, want_residual=True)` | c / a | (d) `leverages()` | `get_factors` + numpy QR |",
         "|---|---|---|---|---|---|---|---|---|"]

    def bm(x):
        return f"{x[0]} ({x[1]})"
    for r in recs:
        a, b, c = r["a_slice_residuals_ms"], r["b_torch_route_ms"], r["c_impute_with_residual_ff_mask_ms"]
        L.append(f"| {'x'.join(map(str, r['lens']))} | {'x'.join(map(str, r['ranks']))} | {bm(a)} | {bm(b)} | "
                 f"{b[0] / a[0]:.2f} | {bm(c)} | {c[0] / a[0]:.2f} | {bm(r['d_leverages_ms'])} | "
                 f"{bm(r['d_get_factors_numpy_ms'])} |")
    L += ["", "| shape | pass launches of one call (by kernel name) | tensor bytes read per element | GB/s of those bytes at the best time | "
          "share of the 8 TB/s peak | extra memory of (b) | largest relative difference (a) against (b) |",
          "|---|---|---|---|---|---|---|"]
    for r in recs:
        L.append(f"| {'x'.join(map(str, r['lens']))} | {r['a_pass_launches']} x `{r['a_pass_kernel']}` | {r['a_tensor_bytes_per_element']:.3g} | "
                 f"{r['a_GBps']} | {100 * r['a_share_of_8TBps']:.1f} % | {r['b_extra_bytes'] / 2 ** 20:.0f} MiB | "
                 f"{r['a_vs_b_largest_relative_difference']:.1e} (b sums fp32 values in fp32) |")
    L += ["", "(a) is the whole call: the settle, the transposed factors, the chain that builds Z, the pass, the folds and the",
          "copy of the N vectors to the host; the share of peak is therefore a call's, not the pass kernel's.", "", KEPT]
    with open(out_md, "w") as f:
        f.write("\n".join(L) + (kept if kept else "\n"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="cfg4,coil100")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--worker")
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--out-dir", default=os.path.dirname(OUT_MD), help="where the .md and .jsonl go")
    a = ap.parse_args()
    if a.resources:
        return resources()
    if a.worker:
        return measure(a.worker, a.reps)
    recs = []
    for name in a.shapes.split(","):   # a process per shape: nothing of one shape's memory in the next one's way
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", name, "--reps", str(a.reps)],
                           capture_output=True, text=True, timeout=900)
        sys.stderr.write(p.stderr[-4000:])
        if p.returncode != 0:
            raise SystemExit(f"shape {name}: exit {p.returncode}\n{p.stdout[-2000:]}")
        line = [l for l in p.stdout.splitlines() if l.startswith("{")][-1]
        print(line, flush=True)
        recs.append(json.loads(line))
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, os.path.basename(OUT_JSONL)), "w") as f:
        f.write("".join(json.dumps(r) + "\n" for r in recs))
    write_md(recs, a.reps, os.path.join(a.out_dir, os.path.basename(OUT_MD)))


if __name__ == "__main__":
    main()
