"""Hold-out rows per start of a multi-start session (ppals_cp_multi_set_holdout) on the host stand-in: start b
of a session whose starts hold out their own rows of one mode must evolve exactly as an ordinary session on
the tensor without those slices does, with the held-out samples' predicted scores beside it. Host logic only —
where Ops::cp_hold_rows runs (behind each of the four multi updates, in set_factors, when the hold-out is
set), its host default, the scores, take_predicted, the stop rule, every refusal and the jackknife's algebra;
the HIP kernel is tests/test_gpu_holdout.py's."""
import ctypes as C

import numpy as np
import pytest

import corcondia_ref as CR
import holdout_cases as HC
import holdout_ref as H
import hostsim_util

F64 = 1
FTOL = 1e-8   # the fp64 bar of the hostsim suites (tests/test_multistart_hostsim.py)
LENS, R, K = [12, 11, 10, 9], 3, 4


@pytest.fixture(scope="module")
def pp():
    return hostsim_util.load()


@pytest.fixture(scope="module")
def ctx(pp):
    c = pp.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("schedule", ["msdt", "dt"])
@pytest.mark.parametrize("lam", [0.0, 1e-3])
@pytest.mark.parametrize("mode", [0, 2, 3])
def test_equal_ranks_match_the_reduced_tensor(pp, ctx, mode, lam, schedule):
    HC.parity(pp, ctx, F64, LENS, [R] * (K + 1), mode, HC.keep_table(pp, LENS[mode], K), FTOL, 1.0, schedule, lam,
              against_ref=True, residual_tol=FTOL)


@pytest.mark.parametrize("schedule", ["msdt", "dt"])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_order_3(pp, ctx, mode, schedule):
    lens = [9, 8, 7]
    HC.parity(pp, ctx, F64, lens, [2] * 4, mode, HC.keep_table(pp, lens[mode], 3), FTOL, 1.0, schedule, 1e-3,
              against_ref=True, residual_tol=FTOL)


@pytest.mark.parametrize("lam", [0.0, 1e-3])
@pytest.mark.parametrize("mode", [0, 2, 3])
def test_ragged_ranks_match_the_reduced_tensor(pp, ctx, mode, lam):
    ranks = [1, 3, 4, 3]
    HC.parity(pp, ctx, F64, LENS, ranks, mode, HC.keep_table(pp, LENS[mode], 3), FTOL, 1.0, "msdt", lam,
              against_ref=True, residual_tol=FTOL)


@pytest.mark.parametrize("ranks", [[3] * 5, [1, 3, 4, 3]], ids=["equal", "ragged"])
@pytest.mark.parametrize("mode", [0, 3])
def test_nonneg_match_the_reduced_tensor(pp, ctx, mode, ranks):
    HC.parity(pp, ctx, F64, LENS, ranks, mode, HC.keep_table(pp, LENS[mode], len(ranks) - 1), FTOL, 1.0, "msdt",
              1e-3, nonneg=True, residual_tol=FTOL)


def test_a_start_that_holds_nothing_out_is_untouched(pp, ctx):
    HC.untouched_start(pp, ctx, F64, LENS, [R] * 4, 2)
    HC.untouched_start(pp, ctx, F64, LENS, [1, 3, 4, 3], 0)
    HC.same_bits_twice(pp, ctx, F64, LENS, [R] * 3, 1, HC.keep_table(pp, LENS[1], 2))


def test_core_consistency_is_the_reduced_tensors(pp, ctx):
    HC.core_consistency(pp, ctx, F64, [9, 8, 7, 6], 2, 1, 3)


def test_set_clear_and_set_again(pp, ctx):
    """set -> sweeps -> clear -> one more sweep is an ordinary sweep from the zero rows; set again on another
    mode and set_factors behind it: the reduced tensor of the NEW table"""
    lens, mode, n = [8, 7, 6, 5], 1, 2
    V = HC.tensor(lens, R, 31)
    t = pp.Tensor(ctx, lens, F64).upload(V)
    keep = HC.keep_table(pp, lens[mode], 2)
    W0, G0 = HC.draw(lens, [R] * 3, 32)
    m = pp.CPMulti(ctx, t, R, 3)
    assert m.holdout is None
    m.set_factors(-1, W0, G0)
    m.set_holdout(mode, keep)          # behind set_factors: the rows move now
    for b in range(3):
        assert np.array_equal(m.heldout_scores(b)[~keep[b]], W0[b][mode][~keep[b]])
        assert np.all(m.get_factors(b)[mode][~keep[b]] == 0.0)
        tr, s = HC.reduced(pp, ctx, V, F64, mode, keep[b], R, W0[b], G0[b], 0, 0.0, "msdt", False)
        assert abs(m.gradnorms()[b] - s.gradnorm()) < 1e-12 * s.gradnorm()
        s.close()
        tr.close()
    m.sweeps(n)
    Wh = [m.get_factors(b, with_grad=True) for b in range(3)]
    m.set_holdout(None, None)
    assert m.holdout is None
    for b in range(3):                 # clearing moves nothing: the zero rows stay until the next update
        assert all(np.array_equal(a, x) for a, x in zip(m.get_factors(b), Wh[b][0]))
    with pytest.raises(pp.PpalsError, match="error -3.*ppals_cp_multi_heldout_scores.*no hold-out"):
        m.heldout_scores(1)
    m.sweeps(1)
    for b in range(3):                 # ... an ordinary session from those factors, on the full tensor
        s = pp.CP(ctx, t, R)
        s.set_factors(*Wh[b])
        s.cpd_als(0, tol=0.0, maxiter=0, resprint=10 ** 9)
        for a, x in zip(m.get_factors(b), s.get_factors()):
            assert HC.relerr(a, x) < FTOL
        s.close()
    mode2 = 3
    keep2 = HC.keep_table(pp, lens[mode2], 2)[::-1].copy()   # start 2 keeps everything now
    m.set_holdout(mode2, keep2)
    m.set_factors(-1, W0, G0)
    m.sweeps(n)
    for b in range(3):
        tr, s = HC.reduced(pp, ctx, V, F64, mode2, keep2[b], R, W0[b], G0[b], n, 0.0, "msdt", False)
        HC.check_against(m, b, s, mode2, keep2[b], FTOL, 1.0, "set again")
        s.close()
        tr.close()
    # one start's factors replaced: the other starts' scores stay as they are
    before = [m.heldout_scores(b) for b in range(3)]
    m.set_factors(0, W0[0], G0[0])
    assert np.array_equal(m.heldout_scores(1), before[1]) and np.array_equal(m.heldout_scores(2), before[2])
    assert np.array_equal(m.heldout_scores(0)[~keep2[0]], W0[0][mode2][~keep2[0]])
    m.set_factors(1, W0[1])            # without gradients: as without a hold-out, norm 0
    assert m.gradnorms()[1] == 0.0
    m.close()
    t.close()


def test_run_stops_on_the_largest_gradient_norm(pp, ctx):
    lens, mode = [8, 7, 6, 5], 0
    t = pp.Tensor(ctx, lens, F64).upload(HC.tensor(lens, 2, 41))
    W0, G0 = HC.draw(lens, [2] * 3, 42)
    m = pp.CPMulti(ctx, t, 2, 3)
    m.set_factors(-1, W0, G0)
    m.sweeps(3)
    gn, best = m.gradnorms(), int(np.argmin(m.residuals()))
    assert m.run(tol=1.0001 * gn[best], maxiter=50, resprint=1)[:2] == (1, 0)    # no hold-out: the best start's norm decides
    m.set_holdout(mode, pp.holdout_segments(lens[mode], 3))       # every start leaves a third of the samples out
    m.set_factors(-1, W0, G0)
    m.sweeps(3)
    gn, best = m.gradnorms(), int(np.argmin(m.residuals()))
    assert gn[best] < gn.max()
    rc, sweeps, best2 = m.run(tol=0.5 * (gn[best] + gn.max()), maxiter=0, resprint=1)
    assert (rc, sweeps, best2) == (0, 0, best)                       # the best start is below, the largest is not
    rc, sweeps, _ = m.run(tol=2.0 * gn.max(), maxiter=50, resprint=1)
    assert (rc, sweeps) == (1, 0)
    m.close()
    t.close()


def test_refusals(pp, ctx):
    lens = [6, 5, 4]
    t = pp.Tensor(ctx, lens, F64).fill_uniform(1)
    m = pp.CPMulti(ctx, t, 2, 2)
    m.set_factors(-1, HC.draw(lens, [2, 2], 5)[0])
    L, u8 = pp.lib(), C.POINTER(C.c_uint8)
    err = lambda: L.ppals_last_error().decode()
    good = np.ones((2, 5), dtype=np.uint8)
    good[1, 2] = 0
    ptr = lambda a: a.ctypes.data_as(u8)
    fn = "ppals_cp_multi_set_holdout"
    assert L.ppals_cp_multi_set_holdout(None, 1, ptr(good)) == -3 and err().startswith(fn)
    for mode in (-1, 3, 7):
        assert L.ppals_cp_multi_set_holdout(m._h, mode, ptr(good)) == -3 and err().startswith(fn + ": mode")
    none_kept = good.copy()
    none_kept[1] = 0
    assert L.ppals_cp_multi_set_holdout(m._h, 1, ptr(none_kept)) == -3 and err().startswith(fn) and "keep" in err()
    assert m.holdout is None                       # nothing of a refused call stays
    with pytest.raises(pp.PpalsError, match="shape"):
        m.set_holdout(1, np.ones((2, 4), dtype=bool))
    mode = C.c_int(5)
    fn = "ppals_cp_multi_get_holdout"
    assert L.ppals_cp_multi_get_holdout(None, C.byref(mode), None) == -3 and err().startswith(fn)
    assert L.ppals_cp_multi_get_holdout(m._h, None, None) == -3 and err().startswith(fn)
    assert L.ppals_cp_multi_get_holdout(m._h, C.byref(mode), None) == 0 and mode.value == -1
    d, d3 = pp.CP(ctx, t, 2), pp.CP(ctx, t, 3)
    out = np.empty(5 * 2)
    for fn, call in (("ppals_cp_multi_heldout_scores", lambda: L.ppals_cp_multi_heldout_scores(m._h, 0, pp._dp(out))),
                     ("ppals_cp_multi_take_predicted", lambda: L.ppals_cp_multi_take_predicted(m._h, 0, d._h))):
        assert call() == -3 and err().startswith(fn) and "no hold-out" in err()
    m.set_holdout(1, good)
    fn = "ppals_cp_multi_heldout_scores"
    assert L.ppals_cp_multi_heldout_scores(None, 0, pp._dp(out)) == -3 and err().startswith(fn)
    for start in (-1, 2, 9):
        assert L.ppals_cp_multi_heldout_scores(m._h, start, pp._dp(out)) == -3 and err().startswith(fn + ": start")
    assert L.ppals_cp_multi_heldout_scores(m._h, 0, None) == -3 and err().startswith(fn)
    fn = "ppals_cp_multi_take_predicted"
    assert L.ppals_cp_multi_take_predicted(None, 0, d._h) == -3 and err().startswith(fn)
    for start in (-1, 2):
        assert L.ppals_cp_multi_take_predicted(m._h, start, d._h) == -3 and err().startswith(fn + ": start")
    assert L.ppals_cp_multi_take_predicted(m._h, 0, None) == -3 and err().startswith(fn)
    assert L.ppals_cp_multi_take_predicted(m._h, 0, d3._h) == -3 and err().startswith(fn) and "rank" in err()
    tb = pp.Tensor(ctx, lens, F64).fill_uniform(1)
    db = pp.CP(ctx, tb, 2)
    assert L.ppals_cp_multi_take_predicted(m._h, 0, db._h) == -3 and err().startswith(fn) and "tensor" in err()
    other = pp.Context(0)
    t2 = pp.Tensor(other, lens, F64).fill_uniform(1)
    do = pp.CP(other, t2, 2)
    assert L.ppals_cp_multi_take_predicted(m._h, 0, do._h) == -3 and err().startswith(fn) and "context" in err()
    dn = pp.CP(ctx, t, 2)
    dn.set_factors(HC.draw(lens, [2], 6)[0][0])
    dn.set_nonneg(True)
    assert L.ppals_cp_multi_take_predicted(m._h, 0, dn._h) == -5 and err().startswith(fn)
    with pytest.raises(pp.PpalsError, match="error -5"):
        m.take(0, dn)                  # ... exactly what take refuses
    m.take_predicted(1, d)             # and the good calls go through
    assert m.heldout_scores(1).shape == (5, 2)
    with pytest.raises(pp.PpalsError, match="at least 2|exceed"):
        pp.jackknife(ctx, t, 0, 2, 1, 1)
    for seg, rank in ((32, 2), (12, 10)):
        with pytest.raises(pp.PpalsError, match="exceed"):
            pp.jackknife(ctx, t, 0, rank, seg, 1)
    other.close()
    for h in (d, d3, db, dn, m, tb, t):
        h.close()


def test_holdout_segments(pp):
    for split in ("interleave", "blocks"):
        k = pp.holdout_segments(11, 4, split)
        assert k.shape == (4, 11) and k.dtype == bool
        assert np.array_equal((~k).sum(axis=0), np.ones(11))      # every sample left out exactly once
        assert (~k).sum(axis=1).min() >= 2
    assert np.array_equal(~pp.holdout_segments(6, 3)[1], np.arange(6) % 3 == 1)
    assert np.array_equal(~pp.holdout_segments(6, 3, "blocks")[1], [False, False, True, True, False, False])
    with pytest.raises(pp.PpalsError):
        pp.holdout_segments(5, 6)
    with pytest.raises(pp.PpalsError):
        pp.holdout_segments(5, 2, "random")


def _model(Ws):
    return CR.cp_tensor(Ws)


def test_jackknife_algebra(pp, ctx):
    lens, mode, rank, seg, n = [10, 8, 7, 6], 0, 3, 5, 4
    V = HC.tensor(lens, rank, 51)
    t = pp.Tensor(ctx, lens, F64).upload(V)
    rng = np.random.default_rng(52)
    W0 = [rng.random((s, rank)) for s in lens]
    jk = pp.jackknife(ctx, t, mode, rank, seg, n, W0=W0)
    keep = HC.keep_table(pp, lens[mode], seg)
    assert [a.shape for a in jk["loadings"]] == [(seg, s, rank) for s in lens]
    assert jk["scores"].shape == (lens[mode], rank) and jk["fms"].shape == (seg,) and jk["press"].shape == (lens[mode],)
    assert jk["se"][mode] is None
    # the same session by hand
    m = pp.CPMulti(ctx, t, rank, seg + 1)
    m.set_holdout(mode, keep)
    m.set_factors(-1, [W0] * (seg + 1))
    m.sweeps(n)
    d = pp.CP(ctx, t, rank)
    for g in range(1, seg + 1):
        A = [a[g - 1] for a in jk["loadings"]]
        for i in range(len(lens)):
            if i != mode:
                assert np.allclose(np.linalg.norm(A[i], axis=0), 1.0, rtol=0, atol=1e-12)
                assert np.all(np.sum(A[i] * jk["reference"][i], axis=0) >= 0)
        raw = m.get_factors(g)
        assert HC.relerr(_model(A), _model(raw)) < 1e-12
        # scores[x] is the aligned held-out row of the start that left x out: with it in place of the zero
        # row the model is that of take_predicted
        out = ~keep[g]
        A_pred = [a.copy() for a in A]
        A_pred[mode][out] = jk["scores"][out]
        raw_pred = [w.copy() for w in raw]
        raw_pred[mode] = raw[mode] + m.heldout_scores(g)
        assert HC.relerr(_model(A_pred), _model(raw_pred)) < 1e-12
        assert np.allclose(jk["press"][out], m.sample_residuals(g, d)[out], rtol=1e-12, atol=0)
    assert np.allclose(jk["fms"], m.fms(skip_mode=mode)[0, 1:], rtol=0, atol=1e-12)   # (no sign flips in this run)
    for i in range(len(lens)):
        if i != mode:
            a = jk["loadings"][i]
            want = np.sqrt((seg - 1) / seg * np.sum((a - a.mean(axis=0)) ** 2, axis=0))
            assert np.allclose(jk["se"][i], want, rtol=1e-14, atol=0)
    # permuting the columns and flipping a sign pair of one start's initial factors changes nothing
    perm = [2, 0, 1]
    Wp = [w[:, perm].copy() for w in W0]
    Wp[mode][:, 1] *= -1.0            # a pair that involves the sample mode ...
    Wp[2][:, 1] *= -1.0
    Wp[1][:, 0] *= -1.0               # ... and one that does not
    Wp[3][:, 0] *= -1.0
    jk2 = pp.jackknife(ctx, t, mode, rank, seg, n, W0=[W0, W0, Wp] + [W0] * (seg - 2))
    for key in ("scores", "fms", "press"):
        assert HC.relerr(jk2[key], jk[key]) < FTOL, key
    for i in range(len(lens)):
        assert HC.relerr(jk2["loadings"][i], jk["loadings"][i]) < FTOL, i
        if i != mode:
            assert np.linalg.norm(jk2["se"][i] - jk["se"][i]) < FTOL * (1 + np.linalg.norm(jk["se"][i]))
    for h in (d, m, t):
        h.close()


def test_jackknife_default_start_and_blocks(pp, ctx):
    lens = [8, 6, 5]
    t = pp.Tensor(ctx, lens, F64).upload(HC.tensor(lens, 2, 61))
    a = pp.jackknife(ctx, t, 1, 2, 3, 3, seed=4, split="blocks")
    rng = np.random.default_rng(4)
    b = pp.jackknife(ctx, t, 1, 2, 3, 3, W0=[rng.random((s, 2)) for s in lens], split="blocks")
    assert all(np.array_equal(x, y) for x, y in zip(a["loadings"], b["loadings"]))
    assert np.array_equal(a["scores"], b["scores"]) and np.all(a["press"] > 0)
    t.close()
