"""The core consistency diagnostic on the GPU, through the C ABI: the batched pseudo-inverse factors
(k_cp_pinv_ragged), ONE tensor scan for all starts, the chain of mode products per start and the score
(k_core_score), for F32, F64 and BF16 storage, ordinary, equal-rank and rank-sweep sessions. Reference and
bars: tests/corcondia_ref.py (numpy, fp64, on V as stored; for BF16 the rounding of tests/bf16_util.py).
The counted check reads the launch profile (ppals_profile_read); nothing here uses a stopwatch."""
import numpy as np
import pytest

import corcondia_cases as K
import corcondia_ref as R

pytestmark = pytest.mark.gpu

F32, F64, BF16 = 0, 1, 3
ALL = [F32, F64, BF16]


@pytest.fixture(scope="module")
def pp():
    import ppals
    return ppals


@pytest.fixture(scope="module")
def ctx(pp):
    c = pp.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("dtype", ALL, ids=K.ident)
@pytest.mark.parametrize("lens,rank", K.SINGLE, ids=K.ident)
def test_closed_form(pp, ctx, lens, rank, dtype):
    K.closed_form(pp, ctx, lens, rank, dtype)


@pytest.mark.parametrize("dtype", ALL, ids=K.ident)
@pytest.mark.parametrize("lens,rank", K.SINGLE, ids=K.ident)
def test_exact_cp_tensor_scores_100(pp, ctx, lens, rank, dtype):
    K.exact_cp(pp, ctx, lens, rank, dtype)


@pytest.mark.parametrize("dtype", ALL, ids=K.ident)
@pytest.mark.parametrize("equal", [False, True], ids=["ragged", "equal"])
def test_multi_equals_ordinary(pp, ctx, equal, dtype):
    ranks = [3, 3, 3] if equal else K.SWEEP_RANKS
    K.multi_equals_ordinary(pp, ctx, dtype, K.SWEEP_LENS, ranks, equal)


@pytest.mark.parametrize("dtype", ALL, ids=K.ident)
def test_multi_order_3_with_the_bf16_row_fallback_shape(pp, ctx, dtype):
    K.multi_equals_ordinary(pp, ctx, dtype, [13, 6, 5], [1, 5, 2], False)


@pytest.mark.parametrize("dtype", [F32, F64], ids=K.ident)
def test_68_columns_in_the_shared_scan(pp, ctx, dtype):
    """4 starts of rank 17 on [20, 18, 17], the factors as drawn (no sweep)"""
    K.multi_equals_ordinary(pp, ctx, dtype, K.WIDE_LENS, [K.WIDE_RANK] * K.WIDE_STARTS, True, sweeps=0)


def _scan_profile(ctx, fn):
    ctx.sync()
    ctx.profile_enable(1)
    ctx.profile_reset()
    fn()
    ctx.sync()
    n, _, by = ctx.profile_read(0)
    ctx.profile_enable(0)
    return n, by


def test_the_tensor_is_read_once_for_all_starts(pp, ctx):
    lens, rank, nstarts = K.SWEEP_LENS, 5, 4
    t = pp.Tensor(ctx, lens, F32).fill_uniform(5)
    Ws = [R.factors(lens, rank, 60 + b) for b in range(nstarts)]
    m = pp.CPMulti(ctx, t, rank, nstarts)
    m.set_factors(-1, Ws)
    wide = pp.CP(ctx, t, rank * nstarts)
    wide.set_factors([np.hstack([Ws[b][i] for b in range(nstarts)]) for i in range(len(lens))])
    one = pp.CP(ctx, t, rank)
    one.set_factors(Ws[0])
    for s in (m.core_consistencies, wide.core_consistency, one.core_consistency):
        s()   # (the buffers exist: the counted calls allocate nothing)
    got = _scan_profile(ctx, m.core_consistencies)
    want = _scan_profile(ctx, wide.core_consistency)
    single = _scan_profile(ctx, one.core_consistency)
    print("scan launches / bytes: multi", got, "R = 20 session", want, "R = 5 session", single)
    assert got[0] > 0 and got == want
    assert got[0] < nstarts * single[0] and got[1] < nstarts * single[1]
    # one scan of the fp32 tensor contracting ONE mode on 20 columns: the tensor once, the result once
    nloc = int(np.prod(lens))
    assert got[1] in [4.0 * nloc + 4.0 * (nloc // s) * rank * nstarts for s in lens], got
    for h in (m, wide, one, t):
        h.close()


@pytest.mark.parametrize("schedule", ["msdt", "dt"])
@pytest.mark.parametrize("multi", [False, True], ids=["ordinary", "multi"])
def test_read_only(pp, ctx, multi, schedule):
    K.read_only(pp, ctx, F32, multi, schedule)


def test_nan_rule(pp, ctx):
    K.nan_rule(pp, ctx, F32)


@pytest.mark.parametrize("dtype", [F32, F64], ids=K.ident)
def test_nonneg_sessions(pp, ctx, dtype):
    K.multi_equals_ordinary(pp, ctx, dtype, K.SWEEP_LENS, K.SWEEP_RANKS, False, nonneg=True)
