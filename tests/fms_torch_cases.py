"""Cases of tests/test_gpu_fms.py that need torch, one per process: `python fms_torch_cases.py <case>`.
torch is imported BEFORE the binding loads libppals (one HIP runtime for both). Exit status 0: passed."""
import os
import sys

import torch  # noqa: I001  (first: see above)
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "pairwise-perturbation_amd"))
import ppals as pp  # noqa: E402
import fms_ref as R  # noqa: E402


def case_split_half():
    """ppals.split_half against its documented steps done by hand with the same generator: a rank-3 tensor
    plus noise, lens [13, 8, 7], mode 0 (odd extent: the halves differ), ranks [2, 3, 4], 5 sweeps, both
    kinds of split. Which rank wins is not claimed: that depends on convergence, not on this code."""
    lens, mode, ranks, sweeps, seed = [13, 8, 7], 0, [2, 3, 4], 5, 3
    rng = np.random.default_rng(77)
    W = [rng.uniform(-1.0, 1.0, (s, 3)) for s in lens]
    V = np.einsum("ir,jr,kr->ijk", *W)
    V = V + 0.05 * np.linalg.norm(V) / np.sqrt(V.size) * rng.standard_normal(lens)
    x = torch.tensor(V, dtype=torch.float32, device="cuda:0")
    ctx = pp.Context(0)
    for split in ("interleave", "blocks"):
        fms, res0, res1 = pp.split_half(ctx, x, mode, ranks, sweeps, seed=seed, split=split)
        s = lens[mode]
        halves = (x[0::2], x[1::2]) if split == "interleave" else (x[:s // 2], x[s // 2:])
        assert halves[0].shape[0] != halves[1].shape[0] and halves[0].data_ptr() == x.data_ptr()   # views, no copy
        gen = np.random.default_rng(seed)
        ts, ms = [], []
        for h in halves:
            t = pp.Tensor.from_torch(ctx, h, pp.F32)
            m = pp.CPMulti.with_ranks(ctx, t, ranks)
            m.set_factors(-1, [[gen.random((n, r)) for n in t.lens] for r in ranks])
            m.sweeps(sweeps)
            ts.append(t)
            ms.append(m)
        want = ms[0].fms_between(ms[1], skip_mode=mode)
        # ... and the reference on the factors themselves
        ref = np.array([R.fms(ms[0].get_factors(k), ms[1].get_factors(k), mode)[0] for k in range(len(ranks))])
        bar = R.bar_fms(lens)
        print(f"split_half {split}: fms {fms} by hand {want} numpy {ref} residuals {res0} {res1}")
        assert fms.shape == (len(ranks),) and res0.shape == res1.shape == (len(ranks),)
        assert np.max(np.abs(fms - want)) <= bar and np.max(np.abs(fms - ref)) <= bar
        for got, m in ((res0, ms[0]), (res1, ms[1])):
            hand = m.residuals()
            assert np.max(np.abs(got - hand)) <= bar * max(1.0, np.max(hand)), (got, hand)
        for h in ms + ts:
            h.close()
    try:
        pp.split_half(ctx, x, mode, ranks, 1, split="thirds")
    except pp.PpalsError:
        pass
    else:
        raise AssertionError("an unknown kind of split was accepted")
    ctx.close()


if __name__ == "__main__":
    name = sys.argv[1]
    {"split_half": case_split_half}[name]()
    print(f"fms case {name}: ok")
