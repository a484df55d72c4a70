"""The checker of tests/parafac2_op_cases.py without a GPU: it accepts a numpy fp64 emulation of Ops::parafac2_step
(the op's contract, Gram route included, in the shim's layout) at shapes with two, three and four rank tiles, and
rejects that emulation with one thing wrong at a time — which is what shows that tests/test_gpu_parafac2_op.py
would fail on a subtly wrong kernel."""
import numpy as np
import pytest

import parafac2_cases_inputs as inputs
import parafac2_op_cases as OC

NT2, NT3, NT4 = (130, 70, 2, 17), (33, 33, 3, 33), (130, 70, 2, 49)


def emulated(c, dt, want_out=True):
    return OC.emulate(c, dt, want_out)


@pytest.mark.parametrize("shape", (NT2, NT3, NT4))
def test_checker_accepts_the_emulation(shape):
    worst, tags = OC.case_values(emulated, shape, inputs.op_inputs(shape))
    print(shape, tags[0], {s: f"{v:.3g}" for s, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values())
    OC.case_exact(emulated, shape, inputs.op_inputs(shape))


@pytest.mark.parametrize("kind", inputs.FAILED_KINDS)
@pytest.mark.parametrize("shape", inputs.FAILED_SHAPES)
def test_checker_accepts_the_emulation_of_a_failed_slice(shape, kind):
    worst, _ = OC.case_values(emulated, shape, inputs.failed_slice_inputs(shape, kind), want_status=[1, 0, 1])
    assert all(v <= 1.0 for v in worst.values())


def rejected(c, o, **kw):
    try:
        OC.check(c, o, **kw)
    except AssertionError as e:
        return str(e)[:200]
    return None


def test_checker_rejects_one_thing_wrong_at_a_time():
    shape = NT4
    I, J, K, R = shape
    X, B, A, Cm = inputs.op_inputs(shape)
    c = OC.make_call(shape, X, B, A, Cm, OC.F64, True)
    OC.check(c, OC.emulate(c, OC.F64))

    def q_moved(o):                 # one Q element moved by 1e-9 relative
        Q = OC.inner(o, c, "Q")
        k, i, s = np.unravel_index(np.argmax(np.abs(Q)), Q.shape)
        Q[k, i, s] *= 1 + 1e-9

    def last_row_unwritten(o):      # the last row of the last row tile left at its sentinel
        OC.inner(o, c, "Q")[K - 1, I - 1, :] = OC.inner(OC.prefilled(c, OC.F64), c, "Q")[K - 1, I - 1, :]

    def chunk_remainder_dropped(o):  # j = 64..69, the remainder of the chunks of 32, left out of Q
        j = J - J % 32
        for k in range(K):
            OC.inner(o, c, "Q")[k] = (c["Xh"][:, :j, k] @ c["A"][:j]) @ (c["C"][k][:, None] * c["B"].T)

    def y_through_f32(o):           # Y rounded to f32 and back in an F64-storage run
        Y = OC.inner(o, c, "Y")
        Y[...] = Y.astype(np.float32)

    def padding_in_the_sum(o):      # out[0] with one (NaN) padding element of the view in it
        assert np.isnan(c["buf"][I])
        o["out"][0] += c["buf"][I] ** 2

    def padding_of_ones_in_the_sum(o):   # ... and what a finite padding element would do
        o["out"][0] += 1.0

    def guard_written(o):
        o["T"][-1] = 0.0

    def front_guard_written(o):
        o["status"][GUARD_LAST] = 1

    def failed_off_by_one(o):
        o["out"][2] += 1.0

    GUARD_LAST = OC.GUARD - 1
    for f in (q_moved, last_row_unwritten, chunk_remainder_dropped, y_through_f32, padding_in_the_sum,
              padding_of_ones_in_the_sum, guard_written, front_guard_written, failed_off_by_one):
        o = OC.emulate(c, OC.F64)
        f(o)
        why = rejected(c, o)
        assert why is not None, f"the checker accepted: {f.__name__}"
        print(f"{f.__name__}: {why}")


def test_checker_rejects_a_rewritten_failed_slice():
    shape = NT3
    I, J, K, R = shape
    X, B, A, Cm = inputs.failed_slice_inputs(shape, "zero")
    c = OC.make_call(shape, X, B, A, Cm, OC.F32, False)
    o = OC.emulate(c, OC.F64)
    OC.check(c, o, want_status=[1, 0, 1])
    OC.inner(o, c, "P")[1] = np.eye(I, R)          # reset to the identity columns instead of kept
    OC.inner(o, c, "Y")[:, :, 1] = 0.0             # (with the Y that goes with it)
    assert rejected(c, o, want_status=[1, 0, 1]) is not None
    o = OC.emulate(c, OC.F64)
    OC.inner(o, c, "T")[1, 0, 0] = 0.0
    assert rejected(c, o, want_status=[1, 0, 1]) is not None
    o = OC.emulate(c, OC.F64)                      # a status that says 1 for the zero slice
    o["status"][OC.GUARD + 1] = 1
    o["out"][2] = 0.0
    assert rejected(c, o) is not None


def test_route_tag_formulas_pin_the_tile_counts_and_the_lds_sizes():
    tag = lambda shape, vdt, dt: OC.route_tag(dict(shape=shape, vdt=vdt), dt)
    assert tag((130, 70, 2, 64), OC.F32, OC.F64) == "parafac2.step.f64.f32 R=64 nt=4 tiles=3x2 lds=73728,37000"
    assert " R=49 nt=4 " in tag((49, 64, 3, 49), OC.F64, OC.F32) and "lds=60168," in tag((49, 64, 3, 49), OC.F64, OC.F32)
    assert " R=48 nt=3 " in tag((130, 70, 2, 48), OC.F64, OC.F32)
    assert tag((33, 33, 3, 33), OC.F64, OC.F32) == "parafac2.step.f32.f64 R=33 nt=3 tiles=1x1 lds=49672,32392"
