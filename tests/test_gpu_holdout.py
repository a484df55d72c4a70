"""Hold-out rows per start of a multi-start session (ppals_cp_multi_set_holdout) on the GPU: one launch of
k_cp_hold_rows behind the sample mode's update moves the held-out samples' rows into the scores, zeroes them in
factor and gradient and redoes the start's Gram and gradient sum. Every start must evolve as an ORDINARY session
of the same library does on the reduced tensor (np.compress along the mode, uploaded from numpy) — to the bars
the project holds a multi-start start to against an ordinary session: FTOL of tests/test_gpu_multistart.py
(1e-5 for F32 / BF16 storage, 1e-8 for F64), gradients in check_start's form (100 * tol * (1 + norm)). The
cases are tests/holdout_cases.py's, shared with the host stand-in's suite. The counted checks read the launch
profile (ppals_profile_read); nothing here uses a stopwatch."""
import numpy as np
import pytest

import holdout_cases as HC

pytestmark = pytest.mark.gpu

F32, F64, BF16 = 0, 1, 3
FTOL = {F32: 1e-5, F64: 1e-8, BF16: 1e-5}
GFAC = 100.0
LENS, R, K = [12, 11, 10, 9], 3, 4


@pytest.fixture(scope="module")
def pp():
    import ppals
    return ppals


@pytest.fixture(scope="module")
def ctx(pp):
    c = pp.Context(0)
    yield c
    c.close()


def run(pp, ctx, dtype, lens, ranks, mode, keep, **kw):
    HC.parity(pp, ctx, dtype, lens, ranks, mode, keep, FTOL[dtype], GFAC,
              against_ref=dtype == F64 and not kw.get("nonneg", False), **kw)


@pytest.mark.parametrize("dtype", [F32, F64, BF16])
@pytest.mark.parametrize("schedule", ["msdt", "dt"])
@pytest.mark.parametrize("lam", [0.0, 1e-3])
@pytest.mark.parametrize("mode", [0, 2, 3])
def test_equal_ranks_match_the_reduced_tensor(pp, ctx, mode, lam, schedule, dtype):
    run(pp, ctx, dtype, LENS, [R] * (K + 1), mode, HC.keep_table(pp, LENS[mode], K), schedule=schedule, lam=lam)


@pytest.mark.parametrize("dtype", [F32, F64, BF16])
@pytest.mark.parametrize("mode,lam", [(0, 0.0), (2, 1e-3), (3, 0.0)])
def test_ragged_ranks_match_the_reduced_tensor(pp, ctx, mode, lam, dtype):
    run(pp, ctx, dtype, LENS, [1, 3, 4, 3], mode, HC.keep_table(pp, LENS[mode], 3), lam=lam)


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("mode", [0, 3])
def test_70_columns(pp, ctx, mode, dtype):
    """R = 10, 6 segments + the full start: 70 columns, the scans' route above 64"""
    lens = [12, 10, 8, 6]
    run(pp, ctx, dtype, lens, [10] * 7, mode, HC.keep_table(pp, lens[mode], 6), lam=1e-3, n=2)


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("ranks", [[3] * 5, [1, 3, 4, 3]], ids=["equal", "ragged"])
def test_nonneg_match_the_reduced_tensor(pp, ctx, ranks, dtype):
    run(pp, ctx, dtype, LENS, ranks, 2, HC.keep_table(pp, LENS[2], len(ranks) - 1), lam=1e-3, nonneg=True)


def edge_table(n, rank, rows_out):
    """start 0 holds nothing out, start 1 the listed rows, start 2 keeps only `rank` rows, start 3 every 4th"""
    keep = np.ones((4, n), dtype=bool)
    keep[1, rows_out] = False
    keep[2] = False
    keep[2, [1, n // 2, n - 1][:rank]] = True
    keep[3, 2::4] = False
    return keep


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("lens,mode,rows_out", [
    ([130, 6, 5], 0, [0, 63, 64, 127, 128, 129]),         # the wave's edges and a last partial stride
    ([6, 300, 5], 1, list(range(0, 296, 8))),             # 37 rows of 300: the Gram's four-chain loop and its tail
    ([6, 5, 130], 2, [0, 63, 64, 127, 128, 129]),
], ids=["130-first", "300-middle", "130-last"])
def test_kernel_edges(pp, ctx, lens, mode, rows_out, dtype):
    run(pp, ctx, dtype, lens, [3] * 4, mode, edge_table(lens[mode], 3, rows_out), lam=1e-3, n=2)


@pytest.mark.parametrize("dtype", [F32, F64])
def test_a_start_that_holds_nothing_out_is_untouched(pp, ctx, dtype):
    HC.untouched_start(pp, ctx, dtype, LENS, [R] * 4, 2)
    HC.untouched_start(pp, ctx, dtype, LENS, [1, 3, 4, 3], 0)
    HC.untouched_start(pp, ctx, dtype, LENS, [R] * 4, 3, nonneg=True)


def test_the_same_state_gives_the_same_bits(pp, ctx):
    HC.same_bits_twice(pp, ctx, F32, [130, 6, 5], [3] * 4, 0, edge_table(130, 3, [0, 63, 64, 127, 128, 129]))
    HC.same_bits_twice(pp, ctx, F64, LENS, [1, 3, 4, 3], 3, HC.keep_table(pp, LENS[3], 3))


@pytest.mark.parametrize("dtype", [F32, F64, BF16])
def test_core_consistency_is_the_reduced_tensors(pp, ctx, dtype):
    HC.core_consistency(pp, ctx, dtype, [9, 8, 7, 6], 2, 1, 3)


def _profile(ctx, level, fn):
    ctx.sync()
    ctx.profile_enable(level)
    ctx.profile_reset()
    fn()
    ctx.sync()
    out = ctx.profile_read(0), ctx.profile_read(1)
    ctx.profile_enable(0)
    return out


def test_scans_unchanged_and_one_more_launch_per_sweep(pp, ctx):
    """the tensor scans of a hold-out session are those of the plain session, launch for launch and byte for
    byte; the other bracketed launches grow by at most one per sweep, whatever the number of starts"""
    lens, rank, n, mode = [20, 12, 16, 10], 10, 3, 2
    t = pp.Tensor(ctx, lens, F32).fill_uniform(6)
    extra = {}
    for nstarts in (2, 7):
        W0, G0 = HC.draw(lens, [rank] * nstarts, 70)
        keep = np.ones((nstarts, lens[mode]), dtype=bool)
        for b in range(1, nstarts):
            keep[b, b % 4::4] = False      # every start but the first leaves a quarter of the samples out
        counts = {}
        for hold in (False, True):
            m = pp.CPMulti(ctx, t, rank, nstarts)
            if hold:
                m.set_holdout(mode, keep)
            m.set_factors(-1, W0, G0)
            (sn, _, sb), (on, _, _) = _profile(ctx, 2, lambda: m.sweeps(n))
            counts[hold] = (sn, sb, on)
            m.close()
        print("starts", nstarts, "(scan launches, scan bytes, other launches): plain", counts[False], "hold-out",
              counts[True])
        assert counts[False][0] > 0 and counts[True][:2] == counts[False][:2]
        extra[nstarts] = counts[True][2] - counts[False][2]
        assert 0 < extra[nstarts] <= n
    assert extra[2] == extra[7]
    t.close()


def test_jackknife_runs_on_the_device(pp, ctx):
    """the Python driver end to end on the HIP engine (its algebra is tests/test_holdout_hostsim.py's)"""
    lens, mode, rank, seg = [10, 8, 7, 6], 0, 3, 5
    t = pp.Tensor(ctx, lens, F64).upload(HC.tensor(lens, rank, 51))
    jk = pp.jackknife(ctx, t, mode, rank, seg, 4, seed=3)
    assert jk["scores"].shape == (lens[mode], rank) and np.all(np.isfinite(jk["scores"]))
    assert np.all(jk["press"] > 0) and np.all(jk["fms"] > 0) and np.all(jk["fms"] <= 1 + 1e-12)
    for i in range(1, len(lens)):
        assert np.allclose(np.linalg.norm(jk["loadings"][i], axis=1), 1.0, rtol=0, atol=1e-12)
        assert np.all(np.isfinite(jk["se"][i]))
    t.close()
