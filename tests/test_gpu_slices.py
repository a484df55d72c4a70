"""The influence plot on the GPU, through the C ABI: the residual's pass keeping its row and column sums —
MODE 3 of k_rank_mfma on F32 / F64 storage with R <= 32 and M a multiple of the vector width, k_slice_stream
for BF16 storage, R > 32 and odd M — the fold of the partial sums (k_slice_fold, k_fold_slice_sums) and the
leverages (k_cp_pinv_ragged, k_row_dots). Reference and bars: tests/slices_ref.py (numpy, fp64, on V as
Tensor.download() returns it). The counted checks read the launch profile; nothing here uses a stopwatch."""
import numpy as np
import pytest

import bf16_util
import slices_cases as K

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
@pytest.mark.parametrize("lens,rank", K.SHAPES, ids=K.ident)
def test_sums_against_numpy(pp, ctx, lens, rank, dtype):
    K.reference(pp, ctx, lens, rank, dtype)


def test_planted_slices(pp, ctx):
    K.planted(pp, ctx)


@pytest.mark.parametrize("lens,rank", [([12, 10, 9, 7], 9), ([8, 6, 40, 30], 16), ([7, 6, 5], 3)], ids=K.ident)
def test_exact_fit(pp, ctx, lens, rank):
    K.exact_fit(pp, ctx, lens, rank)


@pytest.mark.parametrize("lens,rank", K.LEV_SHAPES, ids=K.ident)
def test_leverages_against_pinv(pp, ctx, lens, rank):
    K.leverages(pp, ctx, lens, rank, F32)


@pytest.mark.parametrize("dtype", ALL, ids=K.ident)
def test_leverages_after_sweeps(pp, ctx, dtype):
    K.leverages_after_sweeps(pp, ctx, dtype)


def test_leverages_nan_rule(pp, ctx):
    K.leverages_nan_rule(pp, ctx, F32)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=K.ident)
def test_rank_70(pp, ctx, dtype):
    K.rank_70(pp, ctx, dtype)


@pytest.mark.parametrize("dtype", ALL, ids=K.ident)
@pytest.mark.parametrize("schedule", ["msdt", "dt"])
def test_read_only(pp, ctx, schedule, dtype):
    K.read_only(pp, ctx, dtype, schedule)


def test_read_only_nonneg(pp, ctx):
    K.read_only(pp, ctx, F32, "msdt", nonneg=True)


def _counted(ctx, fn):
    """(launches, bytes) booked in group 1 (the other bracketed kernels) and in group 0 (the tensor scans)
    by one call of fn"""
    ctx.sync()
    ctx.profile_enable(2)
    ctx.profile_reset()
    fn()
    ctx.sync()
    n1, _, b1 = ctx.profile_read(1)
    n0, _, b0 = ctx.profile_read(0)
    ctx.profile_enable(0)
    return (n1, b1), (n0, b0)


def _counted_case(pp, ctx, lens, rank, dtype, cap=None):
    t = pp.Tensor(ctx, lens, dtype).fill_uniform(3)
    s = K.session(pp, ctx, t, pp.init_factors(lens, rank, 13), cap=cap)
    s.slice_residuals()   # (the buffers exist: the counted call allocates nothing)
    if rank <= 64:
        s.leverages()
    one, scans = _counted(ctx, s.slice_residuals)
    lev = _counted(ctx, s.leverages) if rank <= 64 else None
    s.close()
    t.close()
    size = {F32: 4, F64: 8, BF16: 2}[dtype]
    print(f"[slices] counted {K.ident(lens)} R={rank} {K.ident(dtype)} cap {cap}: group 1 {one}, group 0 {scans}, "
          f"leverages {lev}")
    assert one[1] == float(np.prod(lens) * size), (one, np.prod(lens) * size)
    assert scans == (0, 0.0)
    # (one bracketed launch, the pseudo-inverse factors of the core consistency, which carries no tensor bytes)
    assert lev is None or lev == ((1, 0.0), (0, 0.0))
    return one[0]


# one fused-route and one general-route shape per storage type (BF16 is always general)
@pytest.mark.parametrize("lens,rank,dtype", [
    ([24, 22, 5, 4], 12, F32), ([7, 6, 5], 3, F32), ([8, 6, 40, 30], 16, F64), ([12, 10, 9], 33, F64),
    ([20, 18, 17], 10, BF16), ([20, 18, 17], 70, BF16)], ids=K.ident)
def test_the_tensor_is_read_exactly_once(pp, ctx, lens, rank, dtype):
    assert _counted_case(pp, ctx, lens, rank, dtype) == 1   # one pass, one launch


@pytest.mark.parametrize("dtype", ALL, ids=K.ident)
@pytest.mark.parametrize("lens,rank", K.SLAB_SHAPES, ids=K.ident)
def test_slabs(pp, ctx, lens, rank, dtype):
    """a cap of one byte: one row tile by one k-chunk a slab — at least 3 slabs on both shapes, on both
    routes. Within the bar, the same bits twice (K.reference), the bits of the uncapped session (the fold
    runs over tiles and chunks in index order however they are cut), the same byte count."""
    free = K.reference(pp, ctx, lens, rank, dtype)
    capped = K.reference(pp, ctx, lens, rank, dtype, cap=1)
    assert all(bf16_util.same_values(a, b) for a, b in zip(free[0], capped[0])) and free[1] == capped[1]
    assert _counted_case(pp, ctx, lens, rank, dtype, cap=1) >= 3

