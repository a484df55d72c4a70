"""Cases of tests/test_gpu_device_io.py, one per process: `python device_io_cases.py <case>`.

torch is imported BEFORE the ppals binding loads libppals, so that both share one HIP runtime and the
library can query torch's pointers (include/ppals.h, ppals_tensor_check_device_view). Exit status 0:
the case passed. Every view handed to an import or export is a well-formed torch view; the refusal
case only ever calls the check entry point with the bad ones."""
import itertools
import os
import sys
import threading

import torch  # noqa: I001  (first: see above)
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "pairwise-perturbation_amd"))
import ppals as pp  # noqa: E402

DEV = torch.device("cuda:0")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def host(x):
    """a torch tensor as a numpy array of the same logical shape (fp64)"""
    return x.detach().to("cpu", torch.float64).numpy()


def parity():
    """import of a C-contiguous fp64 tensor == upload of the same values, bit for bit"""
    ctx = pp.Context(0)
    g = torch.Generator(device="cpu").manual_seed(1)
    for shape in [(5, 6, 7, 4), (33, 20, 16, 9), (3, 128, 12, 40), (200, 1, 7), (1, 9, 8)]:
        xh = torch.randn(shape, generator=g, dtype=torch.float64) * 1e3
        x = xh.to(DEV)
        for dt in (pp.F32, pp.F64):
            a = pp.Tensor.from_torch(ctx, x, dtype=dt).download()
            b = pp.Tensor(ctx, list(shape), dt).upload(xh.numpy()).download()
            assert same_bits(a, b), (shape, dt)
        assert pp.Tensor.from_torch(ctx, x).dtype == pp.F64
        assert pp.Tensor.from_torch(ctx, x.float()).dtype == pp.F32
    ctx.close()


def layouts():
    """all 24 stride orderings, step slices with an offset, a broadcast mode, f16 / bf16 widening"""
    ctx = pp.Context(0)
    g = torch.Generator(device="cpu").manual_seed(2)
    base = torch.randn((3, 5, 7, 9), generator=g, dtype=torch.float64)
    for perm in itertools.permutations(range(4)):
        inv = [perm.index(i) for i in range(4)]
        x = base.permute(perm).contiguous().permute(inv).to(DEV)
        assert x.shape == base.shape and x.stride() != base.stride() or perm == (0, 1, 2, 3)
        for dt in (pp.F64, pp.F32):
            got = pp.Tensor.from_torch(ctx, x, dtype=dt).download()
            want = host(base) if dt == pp.F64 else host(base.float())
            assert same_bits(got, want), (perm, dt)
    parent = torch.randn((9, 13, 22, 20), generator=g, dtype=torch.float64).to(DEV)
    views = [parent[1::2, 2:7, ::3, 1:19:2],             # steps + storage offset
             parent[2:5].permute(3, 1, 0, 2)[::3],       # permuted and stepped
             parent[0:1, :, 3:6, :].expand(4, 13, 3, 20),  # a stride-0 mode
             parent[:, 4, :, ::2]]                       # no unit-stride mode at all
    for x in views:
        for dt in (pp.F64, pp.F32):
            got = pp.Tensor.from_torch(ctx, x, dtype=dt).download()
            want = host(x) if dt == pp.F64 else host(x.float())
            assert same_bits(got, want), (x.shape, x.stride(), dt)
    for tdt in (torch.float16, torch.bfloat16):
        x = (torch.randn((6, 10, 33), generator=g) * 100).to(tdt).to(DEV)
        for dt in (pp.F32, pp.F64):
            got = pp.Tensor.from_torch(ctx, x, dtype=dt).download()
            want = host(x.float()) if dt == pp.F32 else host(x.double())
            assert same_bits(got, want), (tdt, dt)
            got = pp.Tensor.from_torch(ctx, x.transpose(0, 2).contiguous().transpose(0, 2),
                                       dtype=dt).download()
            assert same_bits(got, want), (tdt, dt, "transposed")
    # an aligned identity-layout source long enough for the vectorised stream, with a ragged tail
    x = torch.randn(4099 * 3, generator=g, dtype=torch.float32).to(DEV)
    got = pp.Tensor(ctx, [4099, 3], pp.F32).import_device(x.data_ptr(), pp.F32, [4099, 3],
                                                         [1, 4099], stream=0).download()
    assert same_bits(got, host(x).reshape((4099, 3), order="F")), "identity"
    ctx.close()


def boxes():
    """slabs along the last mode and along mode 0 assemble the whole; outside a box nothing changes"""
    ctx = pp.Context(0)
    g = torch.Generator(device="cpu").manual_seed(3)
    x = torch.randn((6, 7, 8, 23), generator=g, dtype=torch.float64).to(DEV)
    whole = pp.Tensor.from_torch(ctx, x, dtype=pp.F32).download()
    t = pp.Tensor(ctx, list(x.shape), pp.F32)
    for a, b in zip([0, 5, 12], [5, 12, 23]):
        t.import_torch(x[..., a:b], lo=[0, 0, 0, a])
    assert same_bits(t.download(), whole)
    t = pp.Tensor(ctx, list(x.shape), pp.F32)
    for a, b in zip([0, 1, 4], [1, 4, 6]):
        t.import_torch(x[a:b], lo=[a, 0, 0, 0])
    assert same_bits(t.download(), whole)
    t.fill_uniform(5)
    before = t.download()
    y = torch.randn((2, 3, 4, 5), generator=g, dtype=torch.float64).to(DEV)
    t.import_torch(y, lo=[1, 2, 3, 4])
    after = t.download()
    want = before.copy()
    want[1:3, 2:5, 3:7, 4:9] = host(y.float())
    assert same_bits(after, want)
    ctx.close()


def export():
    """to_torch == download; permuted / stepped destinations receive the box and nothing else"""
    ctx = pp.Context(0)
    g = torch.Generator(device="cpu").manual_seed(4)
    x = torch.randn((12, 8, 3), generator=g, dtype=torch.float64).to(DEV)
    for dt in (pp.F32, pp.F64):
        t = pp.Tensor.from_torch(ctx, x, dtype=dt)
        D = t.download()
        assert same_bits(host(t.to_torch(torch.float64)), D)
        assert np.array_equal(t.to_torch(torch.float32).cpu().numpy(), D.astype(np.float32))
        assert t.to_torch().dtype == torch.float32
        for tdt, ndt in ((torch.float32, np.float32), (torch.float64, np.float64)):
            P = torch.full((5, 13, 21), -7.5, dtype=tdt, device=DEV)
            dst = P.permute(2, 1, 0)[::2, 1:7, ::2]          # (11, 6, 3), no unit stride in mode 0
            t.export_torch(dst, lo=[1, 2, 0])
            E = np.full((5, 13, 21), -7.5, dtype=ndt)
            E.transpose(2, 1, 0)[::2, 1:7, ::2] = D[1:12, 2:8, 0:3].astype(ndt)
            assert np.array_equal(P.cpu().numpy(), E), (dt, tdt)
            Q = torch.full((20, 9, 4), 3.25, dtype=tdt, device=DEV)
            t.export_torch(Q[3:15, :8, 1:4])                 # unit stride in the last mode
            F = np.full((20, 9, 4), 3.25, dtype=ndt)
            F[3:15, :8, 1:4] = D.astype(ndt)
            assert np.array_equal(Q.cpu().numpy(), F), (dt, tdt)
    ctx.close()


def sessions():
    """an import bumps the generation: a live CP / Tucker session rebuilds what it derived (its second
    resident layout, cached tree nodes). A session re-filled by an import computes bit for bit what
    the same session re-filled by an upload computes, and what a fresh session on the new values
    computes up to rounding (a session that kept the old layout would be off by O(1))."""
    ctx = pp.Context(0)
    lens, R, ranks = [20, 18, 16, 14], 4, [3, 3, 3, 3]
    g = torch.Generator(device="cpu").manual_seed(5)
    A = torch.rand(lens, generator=g, dtype=torch.float64)
    B = torch.rand(lens, generator=g, dtype=torch.float64)
    W0, G0 = pp.init_factors(lens, R, 10), pp.init_factors(lens, R, 11)
    W1, G1 = pp.init_factors(lens, R, 12), pp.init_factors(lens, R, 13)

    def relerr(a, b):
        return np.linalg.norm(a - b) / np.linalg.norm(b)

    def cp_run(dt, refill):
        t = pp.Tensor(ctx, lens, dt).upload((B if refill == "fresh" else A).numpy())
        s = pp.CP(ctx, t, R)
        if refill != "fresh":
            s.set_factors(W0, G0)
            s.sweeps_dt(3)
            if refill == "import":
                t.import_torch(B.to(DEV))
            else:
                t.upload(B.numpy())
        s.set_factors(W1, G1)
        s.sweeps_dt(3)
        out = s.get_factors()
        s.close()
        t.close()
        return out

    def tucker_run(dt, refill):
        t = pp.Tensor(ctx, lens, dt).upload((B if refill == "fresh" else A).numpy())
        k = pp.Tucker(ctx, t, ranks)
        if refill != "fresh":
            k.hosvd()
            k.sweeps_dt(2)
            if refill == "import":
                t.import_torch(B.to(DEV))
            else:
                t.upload(B.numpy())
        k.hosvd()
        k.sweeps_dt(2)
        W, core = k.get_factors()
        k.close()
        t.close()
        return W + [core]

    for dt, tol in ((pp.F32, 1e-4), (pp.F64, 1e-9)):
        for name, run in (("cp", cp_run), ("tucker", tucker_run)):
            imp, upl, fresh = run(dt, "import"), run(dt, "upload"), run(dt, "fresh")
            for a, b in zip(imp, upl):
                assert same_bits(a, b), (name, dt)
            if name == "cp":
                errs = [relerr(a, b) for a, b in zip(imp, fresh)]
            else:  # a session with a history may return another basis of the same subspaces (warm
                # eigen-steps): the projectors and the core's norm are what must agree
                errs = [relerr(a @ a.T, b @ b.T) for a, b in zip(imp[:-1], fresh[:-1])]
                errs.append(abs(np.linalg.norm(imp[-1]) / np.linalg.norm(fresh[-1]) - 1))
            assert max(errs) < tol, (name, dt, errs)
            print(f"  {name} dt={dt}: import == upload bitwise; vs a fresh session "
                  f"{'bitwise' if all(same_bits(a, b) for a, b in zip(imp, fresh)) else max(errs)}",
                  flush=True)
    ctx.close()


def stream_order():
    """the copy waits for the source's stream and that stream's later work waits for the copy"""
    ctx = pp.Context(0)
    shape = (64, 1024, 1024)   # 256 MB of fp32
    s = torch.cuda.Stream()
    gen = torch.Generator(device=DEV)
    with torch.cuda.stream(s):
        gen.manual_seed(6)
        x = torch.rand(shape, generator=gen, device=DEV)
        t = pp.Tensor(ctx, list(shape), pp.F32)
        t.import_torch(x)          # torch's current stream: s
        x.zero_()                  # no synchronisation in between
        out = torch.empty(shape, device=DEV)
        t.export_torch(out)
        ok = (out == torch.rand(shape, generator=gen.manual_seed(6), device=DEV)).all()
        x2 = torch.zeros((128,) + shape[1:], device=DEV)
        t.export_torch(x2[::2])    # stepped destination, then a reduction on the same stream
        total = x2.double().sum()
    torch.cuda.synchronize()
    assert bool(ok), "the import read the source after its zeroing, or the export was not waited for"
    want = torch.rand(shape, generator=gen.manual_seed(6), device=DEV).double().sum()
    assert abs(float(total) - float(want)) <= 1e-9 * abs(float(want))
    assert float(x.abs().sum()) == 0.0
    ctx.close()


def shards():
    """P = 2 and 3 ranks on the one GPU (hipsim library): each rank imports its own rows"""
    import hipsim_util
    hp = hipsim_util.load(make=False)
    lens, R = [29, 12, 10, 9], 4
    g = torch.Generator(device="cpu").manual_seed(7)
    Xh = torch.rand(lens, generator=g, dtype=torch.float64)
    X = Xh.to(DEV)
    torch.cuda.synchronize()
    W0, G0 = hp.init_factors(lens, R, 20), hp.init_factors(lens, R, 21)
    for P in (2, 3):
        w = hipsim_util.ThreadWorld(P, timeout=300)
        errors = []

        def rank_main(rank):
            try:
                ctx = hp.Context(0)
                uid, keep = w.comm_uid(rank)
                ctx.init_comm(rank, P, uid)
                res = {}
                for dt in (hp.F32, hp.F64):
                    ti = hp.Tensor(ctx, lens, dt).import_torch(X, stream=0)
                    tu = hp.Tensor(ctx, lens, dt).upload(Xh.numpy())
                    lo, n = ti.local_rows()
                    a, b = ti.download(), tu.download()
                    assert same_bits(a, b), (P, rank, dt)
                    assert n > 0 and not a[:lo].any() and not a[lo + n:].any()
                    for t in (ti, tu):
                        s = hp.CP(ctx, t, R)
                        s.set_factors(W0, G0)
                        s.sweeps_dt(3)
                        res.setdefault(dt, []).append(s.get_factors())
                        s.close()
                    for u, v in zip(*res[dt]):
                        assert same_bits(u, v), (P, rank, dt)
                    ti.close()
                    tu.close()
                w.barrier()
                ctx.close()
                del keep
            except BaseException as e:  # noqa: BLE001
                errors.append((rank, repr(e)))
                w.abort()

        th = [threading.Thread(target=rank_main, args=(r,)) for r in range(P)]
        for x in th:
            x.start()
        for x in th:
            x.join()
        assert not errors and not w.failed, (errors, w.failed)


def refusals():
    """bad views are refused by the check entry point; a good import works on the same context after"""
    assert os.environ.get("PYTORCH_NO_CUDA_MEMORY_CACHING") == "1"
    ctx = pp.Context(0)
    lens = [40, 30]
    t = pp.Tensor(ctx, lens, pp.F32)
    good = torch.randn(lens, device=DEV)
    ERR_ARG = -3

    def good_import():
        t.import_torch(good)
        assert np.array_equal(t.download(), host(good))

    def refused(rc, what):
        msg = pp.lib().ppals_last_error().decode()
        assert rc == ERR_ARG, (what, rc, msg)
        return msg

    cpu = torch.randn(lens)
    msg = refused(t.check_view(0, cpu.data_ptr(), pp.F32, lens, cpu.stride()), "cpu")
    assert "torch must be imported before" in msg, msg
    good_import()
    pinned = torch.randn(lens).pin_memory()
    refused(t.check_view(0, pinned.data_ptr(), pp.F32, lens, pinned.stride()), "pinned")
    good_import()
    y = torch.randn((10, 30), device=DEV)
    refused(t.check_view(0, y.data_ptr(), pp.F32, [10, 30], y.stride(), lo=[35, 0]), "box")
    good_import()
    z = torch.empty(1000, device=DEV)   # no caching allocator: the allocation is this tensor
    big = pp.Tensor(ctx, [2000, 1], pp.F32)
    assert big.check_view(0, z.data_ptr(), pp.F32, [1000, 1], [1, 1]) == 0
    assert big.check_view(0, z.data_ptr(), pp.F32, [500, 1], [2, 1]) == 0
    refused(big.check_view(0, z.data_ptr(), pp.F32, [1001, 1], [1, 1]), "span")
    refused(big.check_view(0, z.data_ptr() + 4, pp.F32, [1000, 1], [1, 1]), "offset span")
    refused(big.check_view(0, z.data_ptr(), pp.F32, [501, 1], [2, 1]), "stepped span")
    good_import()
    d = torch.empty((40, 30), device=DEV)
    refused(t.check_view(1, d.data_ptr(), pp.F32, lens, [0, 1]), "overlap")
    refused(t.check_view(1, d.data_ptr(), pp.F32, lens, [1, 20]), "aliased")
    try:
        t.import_torch(cpu)   # the binding refuses it before calling in
        raise AssertionError("a CPU tensor was accepted")
    except pp.PpalsError:
        pass
    good_import()
    ctx.close()


CASES = {f.__name__: f for f in (parity, layouts, boxes, export, sessions, stream_order, shards,
                                 refusals)}

if __name__ == "__main__":
    CASES[sys.argv[1]]()
    print(f"device_io case {sys.argv[1]}: ok", flush=True)
