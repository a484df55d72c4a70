"""Cases of tests/test_gpu_bf16.py that need torch, one per process: `python bf16_torch_cases.py <case>`.

torch is imported BEFORE the ppals binding loads libppals, so that both share one HIP runtime (as in
tests/device_io_cases.py). Exit status 0: the case passed."""
import os
import sys

import torch  # noqa: I001  (first: see above)
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "pairwise-perturbation_amd"))
import ppals as pp  # noqa: E402

DEV = torch.device("cuda:0")
LENS = [11, 9, 8, 6]


def rand(dtype, seed=1, lens=LENS):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(lens, generator=g, dtype=torch.float64) * torch.exp(
        torch.empty(lens, dtype=torch.float64).uniform_(-20, 20, generator=g))
    return x.to(dtype).to(DEV)


def bits16(x):
    return x.contiguous().view(torch.int16).cpu()


def from_torch():
    """a bf16 x stored as BF16 is x bit for bit; the default storage of a bf16 x stays F32"""
    ctx = pp.Context(0)
    x = rand(torch.bfloat16)
    t = pp.Tensor.from_torch(ctx, x, dtype=pp.BF16)
    assert t.dtype == pp.BF16
    back = t.to_torch(torch.float32)
    torch.cuda.synchronize()
    assert torch.equal(bits16(back.to(torch.bfloat16)), bits16(x))
    assert torch.equal(back, x.float())
    d = pp.Tensor.from_torch(ctx, x)
    assert d.dtype == pp.F32
    assert t.to_torch().dtype == torch.float32
    t.close()
    d.close()
    ctx.close()


def rounding():
    """f16, f32 and f64 sources are rounded exactly as x.to(torch.bfloat16)"""
    ctx = pp.Context(0)
    for dt in (torch.float16, torch.float32, torch.float64):
        x = rand(dt, seed=2)
        if dt == torch.float64:   # the double-rounding case of the contract
            x.view(-1)[:3] = torch.tensor([1 + 2.0 ** -8 + 2.0 ** -30, float("inf"), -0.0], dtype=dt)
        t = pp.Tensor.from_torch(ctx, x, dtype=pp.BF16)
        got = t.to_torch(torch.float64)
        torch.cuda.synchronize()
        want = x.to(torch.bfloat16).to(torch.float64)
        assert torch.equal(got, want), dt
        t.close()
    ctx.close()


def export():
    """to_torch / export_torch widen exactly, to f32 and f64"""
    ctx = pp.Context(0)
    x = rand(torch.bfloat16, seed=3)
    t = pp.Tensor.from_torch(ctx, x, dtype=pp.BF16)
    for dt in (torch.float32, torch.float64):
        out = torch.full(LENS, 7.0, dtype=dt, device=DEV)
        t.export_torch(out)
        torch.cuda.synchronize()
        assert torch.equal(out, x.to(dt)), dt
    t.close()
    ctx.close()


def views():
    """a strided view and a C-order (reversed strides) view import and export like dense ones"""
    ctx = pp.Context(0)
    base = rand(torch.bfloat16, seed=4, lens=[22, 9, 16, 6])
    x = base[::2, :, ::2, :]            # strided
    assert not x.is_contiguous()
    t = pp.Tensor.from_torch(ctx, x, dtype=pp.BF16)
    got = t.to_torch(torch.float32)
    torch.cuda.synchronize()
    assert torch.equal(got, x.float())
    y = rand(torch.float32, seed=5)     # C order: torch's default, the reverse of the tensor's
    t2 = pp.Tensor.from_torch(ctx, y, dtype=pp.BF16)
    got = t2.to_torch(torch.float64)
    torch.cuda.synchronize()
    assert torch.equal(got, y.to(torch.bfloat16).double())
    out = torch.zeros(LENS[::-1], dtype=torch.float32, device=DEV).permute(3, 2, 1, 0)
    t2.export_torch(out)
    torch.cuda.synchronize()
    assert torch.equal(out, y.to(torch.bfloat16).float())
    t.close()
    t2.close()
    ctx.close()


CASES = {f.__name__: f for f in (from_torch, rounding, export, views)}

if __name__ == "__main__":
    name = sys.argv[1]
    CASES[name]()
    print(f"bf16 case {name}: ok", flush=True)
