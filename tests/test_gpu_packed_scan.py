"""Packed (28-bit) twins of the resident fp32 layouts and the scan kernel that reads them
(kernels_pack.hip.h, k_scan_suffix_pk, CpEngine::packed_for): a session created with
PPALS_PACK_LAYOUT=1 computes, BIT FOR BIT, what a session created with PPALS_PACK_LAYOUT=0 computes
on the same tensor — first-level tree nodes, factors, gradients and the gradient norm after three
sweeps under both schedules — whether its scans read the packed twins or, where a twin is refused
or a launch is not eligible, the plain layouts. Every comparison is of the raw bytes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pp():
    import ppals
    return ppals


@pytest.fixture(scope="module")
def ctx(pp):
    c = pp.Context(0)
    yield c
    c.close()


def model_tensor(lens, seed, lo=0.1, hi=1.0, rank=4):
    """a CP model with factors ~ U(lo, hi): positive, magnitudes over about 4 decades (several
    top bytes of the fp32 word, so the codes are not all zero)"""
    rng = np.random.default_rng(seed)
    V = np.zeros(lens, order="F")
    for _ in range(rank):
        t = np.ones((), dtype=np.float64)
        for n in lens:
            t = np.multiply.outer(t, rng.uniform(lo, hi, n))
        V += t
    return np.asfortranarray(V)


_TENSORS = {}


def shared_tensor(lens):
    key = tuple(lens)
    if key not in _TENSORS:
        V = model_tensor(lens, 7 + sum(lens))
        V.setflags(write=False)
        _TENSORS[key] = V
    return _TENSORS[key]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def run_session(pp, ctx, monkeypatch, V, R, pack, schedule="msdt", dtype=0, sweeps=3, nodes=True, env=None):
    """what a session with PPALS_PACK_LAYOUT=pack computes: first-level nodes at the initial factors,
    then factors, gradients, gradient norm after `sweeps` sweeps, and the report"""
    lens = list(V.shape)
    monkeypatch.setenv("PPALS_PACK_LAYOUT", str(pack))
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    t = pp.Tensor(ctx, lens, dtype).upload(V)
    s = pp.CP(ctx, t, R)
    s.set_schedule(schedule)
    s.set_factors(pp.init_factors(lens, R, 5), pp.init_factors(lens, R, 99))
    before = s.placement_report()["packed"]["packed_scans"]
    out = {}
    if nodes and len(lens) == 4:
        out["ab"], out["cd"] = s.tree_node("ab").copy(), s.tree_node("cd").copy()
    s.sweeps_dt(sweeps)
    W, G = s.get_factors(with_grad=True)
    out["W"], out["G"], out["gradnorm"] = np.concatenate([w.ravel() for w in W]), \
        np.concatenate([g.ravel() for g in G]), np.float64(s.gradnorm())
    rep = s.placement_report()["packed"]
    out["packed_scans"] = rep["packed_scans"] - before
    s.close()
    t.close()
    for k in (env or {}):
        monkeypatch.delenv(k)
    return out, rep


def assert_same(plain, packed, what):
    for k in plain:
        if k != "packed_scans":
            assert same_bits(plain[k], packed[k]), (what, k)


SHAPES = [
    [16, 16, 16, 16],  # row tiles and k-blocks exact
    [20, 12, 9, 17],   # row tails, k tails of 1, 9 and 12, batches of 240 rows (no multiple of 256)
    [8, 8, 8, 40],     # 2.5 k-blocks: the half-empty last block of the headline's K = 200
    [4, 4, 4, 200],    # K = 200 itself: 12.5 k-blocks, a single partly filled row tile
]


@pytest.mark.parametrize("schedule", ["dt", "msdt"])
@pytest.mark.parametrize("R", [3, 10, 16])
@pytest.mark.parametrize("lens", SHAPES)
def test_packed_session_equals_plain(pp, ctx, monkeypatch, lens, R, schedule):
    V = shared_tensor(lens)
    plain, rep0 = run_session(pp, ctx, monkeypatch, V, R, 0, schedule)
    packed, rep1 = run_session(pp, ctx, monkeypatch, V, R, 1, schedule)
    assert rep0["mode"] == "off" and rep0["refused"] == "PPALS_PACK_LAYOUT=0" and plain["packed_scans"] == 0
    assert rep1["mode"] == "on" and rep1["refused"] == "", rep1
    rows = [r for r in rep1["layouts"] if r["packed"]]
    assert rows and packed["packed_scans"] > 0, rep1   # the packed kernel really ran
    for r in rows:
        assert r["reason"] == "" and r["bytes_per_element"] > 0
        if r["rows"] % 256 == 0 and r["reduced"] % 16 == 0:   # whole blocks only: 3.5 B + the base word
            assert abs(r["bytes_per_element"] - (3.5 + 4.0 / 4096)) < 2e-4, r
    assert_same(plain, packed, (lens, R, schedule))


def test_more_than_16_columns_not_eligible(pp, ctx, monkeypatch):
    V = shared_tensor([16, 16, 16, 16])
    plain, _ = run_session(pp, ctx, monkeypatch, V, 17, 0)
    packed, rep = run_session(pp, ctx, monkeypatch, V, 17, 1)
    assert "not eligible" in rep["refused"] and "16 result columns" in rep["refused"], rep
    assert packed["packed_scans"] == 0 and not rep["layouts"]
    assert_same(plain, packed, "R=17")


def refusal_tensor(kind, lens):
    V = np.array(shared_tensor(lens))
    if kind == "mixed_sign":
        V.ravel(order="F")[::3] *= -1.0
    elif kind == "wide_range":   # 1e-30 beside 1: far more than 16 top bytes apart
        V.ravel(order="F")[5::7] *= 1e-30
    elif kind == "zeros":
        V.ravel(order="F")[11::13] = 0.0
    return np.asfortranarray(V)


@pytest.mark.parametrize("kind", ["mixed_sign", "wide_range", "zeros"])
def test_values_that_do_not_fit_are_refused(pp, ctx, monkeypatch, kind):
    lens = [16, 16, 16, 16]
    V = refusal_tensor(kind, lens)
    plain, _ = run_session(pp, ctx, monkeypatch, V, 10, 0)
    packed, rep = run_session(pp, ctx, monkeypatch, V, 10, 1)
    assert rep["refused"] == "" and rep["layouts"], rep
    for r in rep["layouts"]:                            # all or nothing per twin: none was kept
        assert not r["packed"] and r["reason"].startswith("top bytes of a block span"), r
        assert r["bytes_per_element"] == 4.0
    assert packed["packed_scans"] == 0
    assert_same(plain, packed, kind)


def test_padded_layout_is_not_packed(pp, ctx, monkeypatch):
    lens = [20, 12, 9, 17]
    V = shared_tensor(lens)
    pad = {"PPALS_PAD_LAYOUT": "1"}
    plain, _ = run_session(pp, ctx, monkeypatch, V, 10, 0, env=pad)
    packed, rep = run_session(pp, ctx, monkeypatch, V, 10, 1, env=pad)
    refused = [r for r in rep["layouts"] if r["reason"] == "padded layout"]
    assert refused and all(not r["packed"] for r in refused), rep
    assert_same(plain, packed, "padded")


def test_fp64_tensor_is_not_packed(pp, ctx, monkeypatch):
    V = shared_tensor([16, 16, 16, 16])
    plain, _ = run_session(pp, ctx, monkeypatch, V, 10, 0, dtype=1)
    packed, rep = run_session(pp, ctx, monkeypatch, V, 10, 1, dtype=1)
    assert "not eligible" in rep["refused"] and "fp32" in rep["refused"], rep
    assert packed["packed_scans"] == 0
    assert_same(plain, packed, "fp64")


def test_k_split_shape_reads_the_plain_layout(pp, ctx, monkeypatch):
    """few row tiles and a long reduction: the launcher splits K, and a k-split launch reads the
    plain layout (the packed kernel has no k-split form) — same bits"""
    lens = [4, 4, 4, 4096]
    V = shared_tensor(lens)
    plain, _ = run_session(pp, ctx, monkeypatch, V, 10, 0, sweeps=2)
    packed, _ = run_session(pp, ctx, monkeypatch, V, 10, 1, sweeps=2)
    assert_same(plain, packed, "k-split")


def test_tensor_refilled_while_the_session_lives(pp, ctx, monkeypatch):
    """new contents that still qualify are packed again, contents that do not drop the twins; the next
    sweeps are those of a fresh plain session on the same contents"""
    lens, R = [16, 16, 16, 16], 10
    V1, V2 = shared_tensor(lens), model_tensor(lens, 1234)
    V3 = refusal_tensor("mixed_sign", lens)
    W0, G0 = pp.init_factors(lens, R, 5), pp.init_factors(lens, R, 99)
    monkeypatch.setenv("PPALS_PACK_LAYOUT", "1")
    t = pp.Tensor(ctx, lens, 0).upload(V1)
    s = pp.CP(ctx, t, R)
    s.set_factors(W0, G0)
    s.sweeps_dt(2)
    for V, fits in ((V2, True), (V3, False)):
        t.upload(V)
        s.set_factors(W0, G0)
        n0 = s.placement_report()["packed"]["packed_scans"]
        s.sweeps_dt(2)
        W, G = s.get_factors(with_grad=True)
        rep = s.placement_report()["packed"]
        got = {"W": np.concatenate([w.ravel() for w in W]), "G": np.concatenate([g.ravel() for g in G]),
               "gradnorm": np.float64(s.gradnorm())}
        if fits:
            assert rep["packed_scans"] > n0 and any(r["packed"] for r in rep["layouts"]), rep
        else:
            assert rep["packed_scans"] == n0 and not any(r["packed"] for r in rep["layouts"]), rep
            assert any(r["reason"].startswith("top bytes") for r in rep["layouts"]), rep
        fresh, _ = run_session(pp, ctx, monkeypatch, V, R, 0, sweeps=2, nodes=False)
        monkeypatch.setenv("PPALS_PACK_LAYOUT", "1")
        assert_same(got, fresh, ("refill", fits))
    s.close()
    t.close()
