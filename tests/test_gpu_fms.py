"""The factor congruence and the factor match score on the GPU, through the C ABI: k_fms_cross (the cross
products of all modes on v_mfma_f64_16x16x4_f64, one launch) and k_fms_finish (the fixed-order sums, the
norms, the product over the modes, the zero rule). Reference and bars: tests/fms_ref.py. The shapes, each the
smallest that reaches a place the kernel can go wrong:
  [13, 6, 5] ranks [1, 5, 2]      one partial 16-column tile, row counts that are no multiples of 4
  [1, 3, 5] R = 5 against R = 3   an extent-1 mode, extents below one MFMA k-step, ra > rb and the call swapped
  [4100, 3, 2] 3 x rank 7         two column tiles, many row chunks (several to a workgroup) in one mode, one in the others
  [33, 17, 9, 5] 4 x rank 32      128 columns: the full 8 x 8 tiles, order 4, LDS at its largest
  [20, 18, 17] 4 x rank 17        68 columns: five tiles with a 4-column remainder
  [3, 2, 2, 2, 2, 2, 2, 2]        order 8
  [13, 6, 5] against [9, 6, 5]    skip_mode = 0: different extents in the skipped mode
The counted check reads the launch profile (ppals_profile_read); nothing here uses a stopwatch."""
import os
import subprocess
import sys

import pytest

import fms_cases as K

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

F32, F64 = 0, 1


@pytest.fixture(scope="module")
def pp():
    import ppals
    return ppals


@pytest.fixture(scope="module")
def ctx(pp):
    c = pp.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("lens,ranks", K.MULTI, ids=K.ident)
def test_multi_phi_against_numpy(pp, ctx, lens, ranks):
    K.multi_phi(pp, ctx, lens, ranks)


def test_ordinary_phi_with_an_extent_1_mode(pp, ctx):
    K.ordinary_phi(pp, ctx, [1, 3, 5], 5, 3)


def test_ordinary_phi_order_8(pp, ctx):
    K.ordinary_phi(pp, ctx, [3, 2, 2, 2, 2, 2, 2, 2], 2, 2)


def test_skipped_mode_with_different_extents(pp, ctx):
    K.skipped_mode_phi(pp, ctx)


def test_invariance(pp, ctx):
    K.invariance(pp, ctx)


def test_ordinary_fms_against_brute_force(pp, ctx):
    K.ordinary_fms(pp, ctx, [1, 3, 5], 5, 3)
    K.ordinary_fms(pp, ctx, [13, 6, 5], 4, 5)


def test_multi_fms_between_and_take(pp, ctx):
    K.multi_fms(pp, ctx)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["F32", "F64"])
def test_queued_work_is_seen(pp, ctx, dtype):
    K.queued_work(pp, ctx, dtype)


@pytest.mark.parametrize("schedule", ["msdt", "dt"])
@pytest.mark.parametrize("kind", ["ordinary", "multi", "nonneg"])
def test_read_only(pp, ctx, kind, schedule):
    K.read_only(pp, ctx, F32, kind, schedule)


def test_same_bits_twice(pp, ctx):
    K.same_bits_twice(pp, ctx)


def test_zero_rule(pp, ctx):
    K.zero_rule(pp, ctx)


def _profile(ctx, fn):
    ctx.sync()
    ctx.profile_enable(2)
    ctx.profile_reset()
    fn()
    ctx.sync()
    scans, others = ctx.profile_read(0)[0], ctx.profile_read(1)[0]
    ctx.profile_enable(0)
    return scans, others


def test_launch_count_does_not_depend_on_starts_order_or_extents(pp, ctx):
    cases = [([20, 18, 17], [5] * 2), ([20, 18, 17], [5] * 12), ([12, 11, 10, 9], [5] * 3), K.CHUNKED]
    counts = []
    for lens, ranks in cases:
        t = K.tensor(pp, ctx, lens)
        m = K.multi(pp, ctx, t, K.starts_of(lens, ranks, 41))
        m.congruence()   # (the buffers exist: the counted call allocates nothing)
        counts.append(_profile(ctx, m.congruence))
        K.close(m, t)
    print("launches (tensor scans, others):", counts)
    assert all(c[0] == 0 for c in counts), counts
    assert counts[0][1] > 0 and all(c == counts[0] for c in counts), counts


def test_split_half():
    """ppals.split_half against its steps by hand. The halves go through torch, which must be imported
    before the library is loaded: a child process (tests/fms_torch_cases.py)"""
    e = dict(os.environ, PYTHONNOUSERSITE="1")
    p = subprocess.run([sys.executable, os.path.join(HERE, "fms_torch_cases.py"), "split_half"],
                       cwd=os.path.dirname(HERE), env=e, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, f"exit {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-6000:]}"
    assert "fms case split_half: ok" in p.stdout
