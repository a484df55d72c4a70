"""Ops::parafac2_step and Ops::parafac2_init of the HIP back end at the op level (tests/parafac2_shim: the op on
host arrays, with its route log): project, polar, apply, compress and the sums of kernels_parafac2.hip.h, each
against a long-double reference formed from the downloaded output of the stage before it, at every rank tile count
(R = 2 .. 64 at (130, 70, 2), and the edge shapes), f32 and f64 views, F32 and F64 storage, contiguous and padded
slices, guards around every output. Cases, references and bars: tests/parafac2_op_cases.py; the checker's own test:
tests/test_parafac2_op_cpu.py."""
import pytest

import parafac2_cases_inputs as inputs
import parafac2_op_cases as OC
import parafac2_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def shim():
    lib = OC.load()
    yield lib
    lib.parafac2_shim_close()


@pytest.fixture
def step(shim):
    return lambda c, dt, want_out=True: OC.run(shim, c, dt, want_out)


def values(step, shape, inp, **kw):
    worst, tags = OC.case_values(step, shape, inp, **kw)
    print(f"  {shape}: error / bar " + ", ".join(f"{s} {v:.3g}" for s, v in worst.items()))
    for t in sorted(set(tags)):
        print("   ", t)
    return tags


@pytest.mark.parametrize("R", ref.OP_SWEEP_RANKS)
def test_rank_sweep(step, R):
    shape = (130, 70, 2, R)
    tags = values(step, shape, inputs.op_inputs(shape))
    assert all(f" R={R} nt={(R + 15) // 16} tiles=3x2 " in t for t in tags), tags
    if R == 64:
        assert all("lds=73728,37000" in t for t in tags), tags


@pytest.mark.parametrize("shape", ref.OP_EDGES, ids=lambda s: "x".join(map(str, s)))
def test_edges(step, shape):
    values(step, shape, inputs.op_inputs(shape))


@pytest.mark.parametrize("shape", [(130, 70, 2, R) for R in OC.FULL_RANKS] + [ref.OP_EDGES[0]],
                         ids=lambda s: "x".join(map(str, s)))
def test_exact_relations(step, shape):
    OC.case_exact(step, shape, inputs.op_inputs(shape))


@pytest.mark.parametrize("kind", inputs.FAILED_KINDS)
@pytest.mark.parametrize("shape", inputs.FAILED_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_failed_slice(step, shape, kind):
    """slice 1 all zero, or of exact rank R - 1: status [1, 0, 1], out[2] == 1, P_1 and T_1 keep their prefilled
    bytes, Y_1 is the prefilled P_1's, slices 0 and 2 pass every check, nothing is NaN (all inside check())"""
    values(step, shape, inputs.failed_slice_inputs(shape, kind), want_status=[1, 0, 1])


def test_init(shim):
    """the first R identity columns in every slice at (65, ., 3, 33), the guards left alone"""
    OC.case_init(shim)
