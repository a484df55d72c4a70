"""Bandwidth of ppals_tensor_import_device (torch tensor in HBM -> resident tensor) by layout and type.

torch is imported first (one HIP runtime for both). Each import is timed with torch.cuda.Event pairs on
the caller's stream, which waits for the copy (include/ppals.h). One JSON line per case; GB/s counts
bytes read plus bytes written. Also: ppals_tensor_upload of the same s = 200 tensor from host fp64
(the path the import replaces), and the wall time of a CP session's creation on it, which builds the
second resident layout with the existing transpose (run under `rocprofv3 --kernel-trace --stats` to
read that kernel's own duration beside the import kernels').

    python tools/import_bench.py [--s 200] [--reps 5] [--quick]
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
PEAK = 8.0e12  # MI355X HBM3E, bytes/s


def timed(fn, reps):
    fn()  # warm-up
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / 1e3)
    return min(ts), float(np.median(ts))


def case(name, t, x, reps, **kw):
    moved = x.numel() * x.element_size() + t_numel(t) * (4 if t.dtype == pp.F32 else 8)
    best, med = timed(lambda: t.import_torch(x, **kw), reps)
    rec = {"case": name, "shape": list(x.shape), "src": str(x.dtype).replace("torch.", ""),
           "src_stride": list(x.stride()), "storage": "F32" if t.dtype == pp.F32 else "F64",
           "bytes_moved": moved, "best_ms": round(best * 1e3, 3), "median_ms": round(med * 1e3, 3),
           "GBps": round(moved / best / 1e9, 1), "frac_of_8TBps": round(moved / best / PEAK, 3)}
    print(json.dumps(rec), flush=True)
    return rec


def t_numel(t):
    return int(np.prod(t.lens))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--s", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="the s = 200 identity / reversed cases and the CP session only")
    a = ap.parse_args()
    s, shape = a.s, (a.s,) * 4
    ctx = pp.Context(0)
    t = pp.Tensor(ctx, list(shape), pp.F32)
    # the engine's own layout (first index fastest) and torch's (C-contiguous, the reversal)
    ident = torch.empty_strided(shape, (1, s, s * s, s ** 3), device=DEV).uniform_()
    case("identity_f32", t, ident, a.reps)
    del ident
    x = torch.rand(shape, device=DEV)
    case("reversed_f32", t, x, a.reps)
    torch.cuda.synchronize()
    if not a.quick:
        xb = x.to(torch.bfloat16)
        case("reversed_bf16", t, xb, a.reps)
        del xb
        xd = x.double()
        case("reversed_f64_to_F32", t, xd, a.reps)
        del xd
        # the s = 200 tensor from host fp64 through ppals_tensor_upload (64 MB chunks, a sync each)
        hf = x.permute(3, 2, 1, 0).contiguous().cpu().double().numpy().T  # Fortran order: no copy in upload
        t0 = time.perf_counter()
        t.upload(hf)
        dt = time.perf_counter() - t0
        print(json.dumps({"case": "upload_host_f64", "shape": list(shape), "s": round(dt, 3),
                          "GBps_host_bytes": round(t_numel(t) * 8 / dt / 1e9, 2)}), flush=True)
        del hf
    # a CP session builds the second resident layout (the existing k_transpose family): the
    # reference point of the reversed case, read from a kernel trace of the same run
    t0 = time.perf_counter()
    cp = pp.CP(ctx, t, 10)
    ctx.sync()
    print(json.dumps({"case": "cp_create_with_second_layout", "shape": list(shape),
                      "wall_ms": round((time.perf_counter() - t0) * 1e3, 2)}), flush=True)
    cp.close()
    del x
    t.close()
    torch.cuda.empty_cache()
    if not a.quick:
        for name, lens in (("coil100", (3, 128, 128, 7200)), ("timelapse", (33, 1344, 1024, 9))):
            tr = pp.Tensor(ctx, list(lens), pp.F32)
            xr = torch.rand(lens, device=DEV)
            case(f"{name}_reversed_f32", tr, xr, a.reps)
            del xr
            tr.close()
            torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
