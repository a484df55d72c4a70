"""Cost of ppals_parafac2_step_device (the projection step of PARAFAC2: two passes over the data view and one
small polar factor per slice) against the torch route on the same box in the same process.

torch is imported first (one HIP runtime for both). Every figure is wall time around a device synchronisation of
both the caller's stream and the engine's. The cases of a configuration are INTERLEAVED: each round runs every
case once, in turn; a case's figure is the median over the rounds after the first (warm-up), its spread the range
min .. max over them. Cases:
  step            ppals_parafac2_step_device without outputs
  step_outputs    the same with lost_sq and failed (three small launches more, and the read-back)
  torch_step      torch.bmm for Q, batched torch.linalg.svd for the polar factors, torch.bmm for Y, in the view's type
The step's time by launch comes from one more step under torch.profiler (the kernels of both libraries run in this
process), after the timed rounds. Configurations: F32 data of about 6.4 GB (2000 x 2000 x 400, R = 10), the size
class of the headline tensor, and a chromatography-sized case (400 x 300 x 60, R = 5).

    python tools/parafac2_bench.py [--rounds 5] [--small-only] [--out-dir profiles]
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
import ppals as pp  # noqa: E402

DEV = torch.device("cuda:0")
PEAK = 8e12   # HBM bytes per second


def by_launch(fn):
    """{kernel name: microseconds} of the k_p2_* / k_sum_partials launches of one call of fn, or {} when the
    profiler sees none of them"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            fn()
        out = {}
        for e in prof.key_averages():
            name = e.key
            if "k_p2_" in name or "k_sum_partials" in name:
                us = getattr(e, "device_time_total", None)
                if us is None:
                    us = getattr(e, "cuda_time_total", 0.0)
                short = name.split("ppals::")[-1].split("(")[0]
                out[short] = out.get(short, 0.0) + float(us)
        return out
    except Exception as ex:   # the profile is a convenience: the timed figures above do not depend on it
        print(f"by-launch profile unavailable: {ex!r}", flush=True)
        return {}


def config(ctx, I, J, K, R, rounds, rows):
    def sync():
        torch.cuda.synchronize()
        ctx.sync()

    X = torch.rand((K, J, I), device=DEV).permute(2, 1, 0)      # I x J x K, unit stride in mode 0
    p = pp.Parafac2(ctx, I, J, K, R, pp.F32)
    B, A, Cm = (torch.from_numpy(w).to(DEV).float() for w in p.cp.get_factors())
    Xb = X.permute(2, 0, 1)                                     # K x I x J, a view: no copy
    Yt = torch.empty((K, R, J), device=DEV)

    def torch_step():
        M = (A[None] * Cm[:, None, :]) @ B.T                    # K x J x R
        Q = torch.bmm(Xb, M)
        U, _, Vh = torch.linalg.svd(Q, full_matrices=False)
        P = torch.bmm(U, Vh)
        torch.bmm(P.transpose(1, 2), Xb, out=Yt)

    cases = [("step", lambda: p.step_torch(X, want=False)), ("step_outputs", lambda: p.step_torch(X)),
             ("torch_step", torch_step)]
    ts = {name: [] for name, _ in cases}
    for rnd in range(rounds + 1):
        for name, fn in cases:
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            if rnd:
                ts[name].append(time.perf_counter() - t0)
    nbytes = 2.0 * I * J * K * 4
    for name, _ in cases:
        v = np.array(ts[name]) * 1e3
        row = dict(case=name, I=I, J=J, K=K, R=R, data="f32", storage="F32", rounds=rounds,
                   median_ms=round(float(np.median(v)), 3), min_ms=round(float(v.min()), 3),
                   max_ms=round(float(v.max()), 3))
        if name != "torch_step":
            row["fraction_of_peak_two_reads_of_X"] = round(nbytes / (float(np.median(v)) * 1e-3) / PEAK, 3)
        rows.append(row)
        print(json.dumps(row), flush=True)

    def one():
        p.step_torch(X)
        sync()

    launches = by_launch(one)
    row = dict(case="by_launch_us", I=I, J=J, K=K, R=R, **{k: round(v, 1) for k, v in sorted(launches.items())})
    for k, v in launches.items():
        if "project" in k or "compress" in k:
            row["fraction_of_peak_" + ("project" if "project" in k else "compress")] = round(
                0.5 * nbytes / (v * 1e-6) / PEAK, 3)
    rows.append(row)
    print(json.dumps(row), flush=True)
    p.close()
    del X, Xb, Yt
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    ctx = pp.Context(0)
    rows = []
    shapes = [(400, 300, 60, 5)] + ([] if a.small_only else [(2000, 2000, 400, 10)])
    for I, J, K, R in shapes:
        config(ctx, I, J, K, R, a.rounds, rows)
    ctx.close()
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "parafac2_bench.jsonl"), "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    with open(os.path.join(a.out_dir, "parafac2_bench.md"), "w") as f:
        f.write("# The PARAFAC2 projection step\n\n"
                f"`python tools/parafac2_bench.py --rounds {a.rounds}` on {torch.cuda.get_device_name(0)}: f32 data with "
                "unit stride in mode 0, F32 storage; the cases interleaved in one process, the median over "
                f"{a.rounds} rounds after a warm-up round, the spread min .. max over them. The fraction is that of "
                "the 8 TB/s HBM peak on the two reads of X.\n\n"
                "| I x J x K, R | case | median ms | min .. max ms | fraction of 8 TB/s |\n|---|---|---|---|---|\n")
        for r in rows:
            if "median_ms" in r:
                f.write(f"| {r['I']} x {r['J']} x {r['K']}, {r['R']} | {r['case']} | {r['median_ms']} | "
                        f"{r['min_ms']} .. {r['max_ms']} | {r.get('fraction_of_peak_two_reads_of_X', '')} |\n")
        f.write("\n## By launch (one step with outputs under torch.profiler, microseconds)\n\n")
        for r in rows:
            if r["case"] == "by_launch_us":
                rest = {k: v for k, v in r.items() if k not in ("case", "I", "J", "K", "R")}
                f.write(f"- {r['I']} x {r['J']} x {r['K']}, R = {r['R']}: "
                        + ("; ".join(f"{k} {v}" for k, v in rest.items()) or "the profiler saw none of the launches")
                        + "\n")
        f.write("\n(The section 'Which limit the two passes hit' of the committed profile is written by hand from these "
                "figures: carry it over, or redo its arithmetic, when this file is regenerated.)\n")


if __name__ == "__main__":
    main()
