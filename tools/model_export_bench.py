"""Bandwidth of ppals_cp_export_model_device (a CP model, or V - model, into a torch tensor in HBM) by
destination layout and tensor storage, at the headline extents (order 4, s = 200, R = 10, fp32
destination: 6.4 GB written).

torch is imported first (one HIP runtime for both). Each export is timed with torch.cuda.Event pairs on
the caller's stream, which waits for the stores (include/ppals.h). One JSON line per case; GB/s counts
the bytes written (model) or the bytes of V read plus the bytes written (residual), against the
plain-store and copy rates of profiles/r01k_stream_bench.txt. The residual is timed in both forms
(PPALS_MODEL_RESIDUAL=fused / two_pass, include/ppals.h) and in the library's default choice.

    python tools/model_export_bench.py [--s 200] [--R 10] [--reps 5]
"""
import argparse
import json
import os
import sys

import torch  # noqa: I001  (before ppals: one HIP runtime)
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pairwise-perturbation_amd"))
import ppals as pp  # noqa: E402

DEV = torch.device("cuda:0")
STORE_TBPS, COPY_TBPS = 5.1e12, 4.9e12  # plain-store stream / copy, profiles/r01k_stream_bench.txt


def timed(fn, reps):
    fn()  # warm-up (workspaces, offset tables)
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / 1e3)
    return min(ts), float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--s", type=int, default=200)
    ap.add_argument("--R", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    s, R = a.s, a.R
    shape = (s,) * 4
    n = s ** 4
    ctx = pp.Context(0)
    W, G = pp.init_factors(shape, R, 1), pp.init_factors(shape, R, 2)
    for storage, name in ((pp.F32, "F32"), (pp.BF16, "BF16")):
        t = pp.Tensor(ctx, list(shape), storage).fill_uniform(5)
        # one session per form of the residual (PPALS_MODEL_RESIDUAL is read at session creation);
        # None = the library's own choice
        sess = {}
        for form in (None, "fused", "two_pass"):
            if form:
                os.environ["PPALS_MODEL_RESIDUAL"] = form
            sess[form] = pp.CP(ctx, t, R)
            sess[form].set_factors(W, G)
            os.environ.pop("PPALS_MODEL_RESIDUAL", None)
        cp = sess[None]
        vbytes = n * (4 if storage == pp.F32 else 2)
        for layout in ("first_index_fastest", "c_order"):
            if layout == "c_order":
                out = torch.empty(shape, device=DEV)
            else:
                out = torch.empty_strided(shape, (1, s, s * s, s ** 3), device=DEV)
            for residual, form in ((False, None), (True, None), (True, "fused"), (True, "two_pass")):
                se = sess[form]
                best, med = timed(lambda: se.export_model_torch(out, residual=residual), a.reps)
                moved = n * 4 + (vbytes if residual else 0)
                ref = COPY_TBPS if residual else STORE_TBPS
                rec = {"case": "residual" if residual else "model", "form": form or "default",
                       "dst_layout": layout, "storage": name,
                       "shape": list(shape), "R": R, "dst": "float32", "bytes_moved": moved,
                       "best_ms": round(best * 1e3, 3), "median_ms": round(med * 1e3, 3),
                       "GBps": round(moved / best / 1e9, 1),
                       "frac_of_" + ("copy" if residual else "store") + "_rate": round(moved / best / ref, 3)}
                print(json.dumps(rec), flush=True)
            del out
            torch.cuda.empty_cache()
        # the session's own streaming residual (K10, no tensor written) for comparison
        best, med = timed(lambda: cp.residual(), a.reps)
        print(json.dumps({"case": "cp_residual_scalar", "storage": name, "shape": list(shape), "R": R,
                          "best_ms": round(best * 1e3, 3), "GBps_read": round(vbytes / best / 1e9, 1)}),
              flush=True)
        for se in sess.values():
            se.close()
        t.close()
    ctx.close()


if __name__ == "__main__":
    main()
