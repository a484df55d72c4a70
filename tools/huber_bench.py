"""Cost of ppals_cp_huber_device (the Huber step of robust CP: the resident tensor rewritten with
m + h clip(x - m, -c, c)) and of ppals_cp_abs_residual_quantile at the headline extents: order 4, s = 200,
R = 10, F32 storage, dense C-order fp32 views.

torch is imported first (one HIP runtime for both). Every figure is wall time around a device synchronisation
of both the caller's stream and the engine's. The cases are INTERLEAVED: each round runs every case once, in
turn, so drift of the box (clocks, other tenants) falls on all of them alike; a case's figure is the median
over the rounds after the first, and its spread the range min .. max over them. Cases:
  huber_now            the step without a weights view (8 B per element: x and the store)
  huber_weighted       the step with a dense weights view (12 B per element)
  wls                  ppals_cp_wls_device on the same views: the comparison figure, measured in this run
  huber_broadcast      the step fed a one-element weights view with all strides 0 (what weights == NULL would
                       be routed to if the family without weights earned nothing)
  torch_step           export_model_torch + clamp + import_torch into preallocated tensors
  quantile             the median by ppals_cp_abs_residual_quantile (three histogram passes)
  torch_quantile       export_model_torch(residual=True) + abs + kthvalue (the tensor holding x beforehand)
and, once the rounds are done, the two decisions that hang on them, written into huber_bench.md with the table.

    python tools/huber_bench.py [--s 200] [--R 10] [--rounds 7] [--out-dir profiles]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--s", type=int, default=200)
    ap.add_argument("--R", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    s, R = a.s, a.R
    shape = (s,) * 4
    n = s ** 4
    ctx = pp.Context(0)

    def sync():
        torch.cuda.synchronize()
        ctx.sync()

    t = pp.Tensor(ctx, list(shape), pp.F32).fill_uniform(5)
    cp = pp.CP(ctx, t, R)
    cp.set_factors(pp.init_factors(shape, R, 1), pp.init_factors(shape, R, 2))
    x = torch.rand(shape, device=DEV)
    h = torch.rand(shape, device=DEV)
    one = torch.ones((1, 1, 1, 1), device=DEV)
    buf, new = torch.empty_like(x), torch.empty_like(x)
    c = 1.345 * cp.robust_scale(x)
    clipped = cp.huber_torch(x, c, want_loss=True)[1] / n

    def torch_step():
        cp.export_model_torch(buf)
        torch.sub(x, buf, out=new)
        new.clamp_(-c, c).add_(buf)
        t.import_torch(new)

    kth = n // 2   # kthvalue is 1-based: the element of 0-based rank ceil(n / 2) - 1 for even n
    got = {}

    def torch_quantile():   # (the resident tensor holds x: `before` below)
        cp.export_model_torch(buf, residual=True)
        got["torch"] = float(buf.abs_().view(-1).kthvalue(kth).values)

    def quantile():
        got["ppals"] = cp.abs_residual_quantile_torch(x, 0.5)[0]

    cases = [("huber_now", lambda: cp.huber_torch(x, c), 8),
             ("huber_weighted", lambda: cp.huber_torch(x, c, weights=h), 12),
             ("wls", lambda: cp.wls_torch(x, h), 12),
             ("huber_broadcast", lambda: cp.huber_torch(x, c, weights=one), 8),
             ("huber_now_outputs", lambda: cp.huber_torch(x, c, want_loss=True), 8),
             ("torch_step", torch_step, 24),
             ("quantile", quantile, 12),
             ("torch_quantile", torch_quantile, None)]
    before = {"torch_quantile": lambda: t.import_torch(x)}   # untimed: the residual export reads the tensor
    ts = {name: [] for name, _, _ in cases}
    for rnd in range(a.rounds + 1):   # the first round warms up (workspaces, offset tables, allocator)
        for name, fn, _ in cases:
            if name in before:
                before[name]()
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            if rnd:
                ts[name].append(time.perf_counter() - t0)
    rows = []
    for name, _, per_elem in cases:
        v = np.array(ts[name]) * 1e3
        row = dict(case=name, shape=list(shape), R=R, storage="F32", views="f32", rounds=a.rounds,
                   median_ms=round(float(np.median(v)), 3), min_ms=round(float(v.min()), 3),
                   max_ms=round(float(v.max()), 3))
        if per_elem:
            row.update(bytes_per_element=per_elem,
                       fraction_of_peak=round(n * per_elem / (float(np.median(v)) * 1e-3) / PEAK, 3))
        rows.append(row)
    med = {r["case"]: r["median_ms"] for r in rows}
    spread = {r["case"]: r["max_ms"] - r["min_ms"] for r in rows}
    gain = med["huber_broadcast"] - med["huber_now"]
    noise = max(spread["huber_broadcast"], spread["huber_now"])
    extra = med["huber_weighted"] - med["wls"]
    noise2 = max(spread["huber_weighted"], spread["wls"])
    rows.append(dict(case="decision_family_without_weights", now_faster_than_broadcast_by_ms=round(gain, 3),
                     spread_ms=round(noise, 3), keep=bool(gain > noise)))
    rows.append(dict(case="decision_huber_rule_cost", weighted_slower_than_wls_by_ms=round(extra, 3),
                     spread_ms=round(noise2, 3), slower_beyond_spread=bool(extra > noise2)))
    rows.append(dict(case="context", c=c, clipped_fraction=round(clipped, 4), median_ppals=got["ppals"],
                     median_torch=got["torch"], step_vs_torch=round(med["torch_step"] / med["huber_now"], 2),
                     quantile_vs_torch=round(med["torch_quantile"] / med["quantile"], 2)))
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "huber_bench.jsonl"), "w") as f:
        for r in rows:
            print(json.dumps(r), flush=True)
            f.write(json.dumps(r) + "\n")
    with open(os.path.join(a.out_dir, "huber_bench.md"), "w") as f:
        f.write("# The Huber step and the residual quantile at the headline shape\n\n"
                f"`python tools/huber_bench.py --s {s} --R {R} --rounds {a.rounds}`: order 4, s = {s}, R = {R}, F32 "
                "storage, dense C-order fp32 views; the cases interleaved in one process, the median over "
                f"{a.rounds} rounds after a warm-up round, the spread min .. max over them. c = 1.345 x the MAD scale "
                f"of the residuals = {c:.4g}; {100 * clipped:.1f} % of the elements are clipped.\n\n"
                "| case | median ms | min .. max ms | B / element | fraction of 8 TB/s |\n|---|---|---|---|---|\n")
        for r in rows:
            if "median_ms" in r:
                f.write(f"| {r['case']} | {r['median_ms']} | {r['min_ms']} .. {r['max_ms']} | "
                        f"{r.get('bytes_per_element', '')} | {r.get('fraction_of_peak', '')} |\n")
        f.write(f"\nThe medians {'agree' if got['ppals'] == got['torch'] else 'DIFFER'}: ppals {got['ppals']!r}, torch "
                f"{got['torch']!r}.\n\n## The two decisions\n\n"
                f"- The family without a weights view against the same step fed a broadcast one-element weights view: "
                f"faster by {gain:.3f} ms, the runs' spread {noise:.3f} ms. "
                + ("It is faster by more than the spread: the family stays.\n" if gain > noise else
                   "It is NOT faster by more than the spread: by the issue's rule it is to be dropped and "
                   "weights == NULL routed to the broadcast.\n")
                + f"- The weighted Huber step against ppals_cp_wls_device on the same views: slower by {extra:.3f} ms, "
                f"the runs' spread {noise2:.3f} ms. "
                + ("The Huber rule makes the weighted kernel slower than the WLS step by more than the spread.\n"
                   if extra > noise2 else "The Huber rule costs nothing beyond the spread.\n"))
    cp.close()
    t.close()
    ctx.close()


if __name__ == "__main__":
    main()
