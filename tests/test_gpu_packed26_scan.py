"""26-bit packed twins (kernels_pack.hip.h FORMAT 26, k_scan_suffix_pk2): a session created with
PPALS_PACK_LAYOUT=2 computes, BIT FOR BIT, what a session created with PPALS_PACK_LAYOUT=0 computes
on the same tensor — first-level tree nodes, factors, gradients and the gradient norm after three
sweeps under both schedules — with no escape block, with escape blocks at chosen places, and with
every block an escape block; the pre-pass counts the escape blocks a numpy walk of the format counts
(tests/pack26_ref.py). Every comparison is of the raw bytes."""
import numpy as np
import pytest

import pack26_ref as ref
from test_gpu_packed_scan import SHAPES, assert_same, model_tensor, refusal_tensor, run_session, shared_tensor

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


_PLAIN = {}


def plain_session(pp, ctx, monkeypatch, key, V, R, schedule, **kw):
    """the PPALS_PACK_LAYOUT=0 session on V, computed once per (key, R, schedule) and left unchanged"""
    k = (key, R, schedule)
    if k not in _PLAIN:
        out, rep = run_session(pp, ctx, monkeypatch, V, R, 0, schedule, **kw)
        assert rep["mode"] == "off" and out["packed_scans"] == 0
        for v in out.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _PLAIN[k] = out
    return _PLAIN[k]


def packed_rows(rep):
    return [r for r in rep["layouts"] if r["packed"]]


def blocks_of(r):
    return (r["rows"] + 255) // 256 * r["batches"] * ((r["reduced"] + 15) // 16)


def check_rows_against_reference(V, rep, fmt=26):
    """every packed row: the format, the escape count of the numpy walk, the bytes of the layout"""
    rows = packed_rows(rep)
    assert rows, rep
    for r in rows:
        L, J, T = r["rows"], r["reduced"], r["batches"]
        want = ref.escape_blocks(ref.layout_elements(V, r["layout"]), L, J, T)
        assert want is not None and r["reason"] == "", r
        assert r["format"] == fmt and r["escape_blocks"] == want, (r, want)
        tiles = (L + 255) // 256 * T
        nbytes = tiles * ref.tile_bytes(fmt, J) + 4 * blocks_of(r) + (ref.ESC_PLANE * want if fmt == 26 else 0)
        assert abs(r["bytes_per_element"] - nbytes / (L * J * T)) < 1e-4, (r, nbytes)
    return rows


@pytest.mark.parametrize("schedule", ["dt", "msdt"])
@pytest.mark.parametrize("R", [3, 10, 16])
@pytest.mark.parametrize("lens", SHAPES)
def test_packed26_session_equals_plain(pp, ctx, monkeypatch, lens, R, schedule):
    V = shared_tensor(lens)
    plain = plain_session(pp, ctx, monkeypatch, ("model", tuple(lens)), V, R, schedule)
    packed, rep = run_session(pp, ctx, monkeypatch, V, R, 2, schedule)
    assert rep["mode"] == "on" and rep["refused"] == "", rep
    assert packed["packed_scans"] > 0, rep   # the packed kernel really ran
    for r in check_rows_against_reference(V, rep):
        assert r["escape_blocks"] == 0, r    # this tensor has no block beyond two code bits
        if r["rows"] % 256 == 0 and r["reduced"] % 16 == 0:   # whole blocks only: 3.25 B + the side word
            assert abs(r["bytes_per_element"] - (3.25 + 4.0 / 4096)) < 2e-4, r
    assert_same(plain, packed, (lens, R, schedule))


def test_switch_at_1_is_still_the_28_bit_format(pp, ctx, monkeypatch):
    lens = [16, 16, 16, 16]
    V = shared_tensor(lens)
    plain = plain_session(pp, ctx, monkeypatch, ("model", tuple(lens)), V, 10, "msdt")
    packed, rep = run_session(pp, ctx, monkeypatch, V, 10, 1)
    assert packed["packed_scans"] > 0
    for r in check_rows_against_reference_28(rep):
        if r["rows"] % 256 == 0 and r["reduced"] % 16 == 0:
            assert abs(r["bytes_per_element"] - (3.5 + 4.0 / 4096)) < 2e-4, r
    assert_same(plain, packed, "=1")


def check_rows_against_reference_28(rep):
    rows = packed_rows(rep)
    assert rows and all(r["format"] == 28 for r in rows), rep
    return rows


def natural_index(lens, layout):
    """storage position -> position in the tensor's own (first mode fastest) order"""
    idx = np.arange(int(np.prod(lens)), dtype=np.int64).reshape(lens, order="F")
    if layout == "tensor":
        return idx.ravel(order="F")
    return idx.transpose(ref.SECOND_COPY_ORDER[len(lens)]).ravel(order="F")


def chosen_blocks(L, J, T):
    """(row tile, k-block, batch): the first block of a tile, the (short) last k-block, a block of
    the (partly filled) last row tile, two consecutive blocks, a block of the last batch"""
    n_mtiles, nkb = (L + 255) // 256, (J + 15) // 16
    picks = {(0, 0, 0), (0, nkb - 1, 0), (n_mtiles - 1, nkb // 2, 0), (n_mtiles - 1, nkb - 1, T - 1),
             (0, 0, T - 1), (0, min(1, nkb - 1), T // 2), (0, min(2, nkb - 1), T // 2)}
    if nkb == 1 and n_mtiles * T > 1:   # one block per tile: consecutive blocks are consecutive tiles
        picks |= {(1 % n_mtiles, 0, 1 // n_mtiles)}
    return sorted(picks)


def escape_tensor(V, rows):
    """V with the smallest element of each chosen block of every scan shape in `rows` scaled by
    2^-10 (five top bytes down): those blocks then span 5..8 values"""
    lens = list(V.shape)
    flat = np.array(V).ravel(order="F")
    hit = set()
    for r in rows:
        L, J, T = r["rows"], r["reduced"], r["batches"]
        nat = natural_index(lens, r["layout"])
        stored = np.abs(np.float32(flat[nat]))
        for mt, kb, b in chosen_blocks(L, J, T):
            members = ref.block_members(L, J, T, mt, kb, b)
            hit.add(int(nat[members[np.argmin(stored[members])]]))
    out = flat.copy()
    out[sorted(hit)] *= 2.0 ** -10
    return np.asfortranarray(out.reshape(lens, order="F"))


_ROWS = {}


def scan_rows(pp, ctx, monkeypatch, lens, schedule):
    """the scan shapes a session of this schedule asks twins for"""
    k = (tuple(lens), schedule)
    if k not in _ROWS:
        _, rep = run_session(pp, ctx, monkeypatch, shared_tensor(lens), 10, 2, schedule)
        _ROWS[k] = packed_rows(rep)
    return _ROWS[k]


@pytest.mark.parametrize("schedule", ["dt", "msdt"])
@pytest.mark.parametrize("lens", SHAPES)
def test_escape_blocks_at_chosen_places(pp, ctx, monkeypatch, lens, schedule):
    R = 10
    V = escape_tensor(shared_tensor(lens), scan_rows(pp, ctx, monkeypatch, lens, schedule))
    plain = plain_session(pp, ctx, monkeypatch, ("escapes", tuple(lens), schedule), V, R, schedule)
    packed, rep = run_session(pp, ctx, monkeypatch, V, R, 2, schedule)
    assert rep["refused"] == "" and packed["packed_scans"] > 0, rep
    rows = check_rows_against_reference(V, rep)   # pins the pre-pass: count == the numpy walk's
    for r in rows:                                # ... and the chosen blocks of this shape are among them
        assert r["escape_blocks"] >= len(chosen_blocks(r["rows"], r["reduced"], r["batches"])), r
    assert_same(plain, packed, ("escapes", lens, schedule))


@pytest.mark.parametrize("schedule", ["dt", "msdt"])
@pytest.mark.parametrize("R", [3, 10, 16])
@pytest.mark.parametrize("lens", SHAPES)
def test_every_block_an_escape_block(pp, ctx, monkeypatch, lens, R, schedule):
    """a checkerboard of elements scaled by 2^-14 (seven top bytes): four consecutive rows of any
    block hold both colours, so every block spans 4..10 values"""
    V = np.array(shared_tensor(lens))
    odd = np.indices(lens).sum(axis=0) % 2 == 1
    V[odd] *= 2.0 ** -14
    V = np.asfortranarray(V)
    plain = plain_session(pp, ctx, monkeypatch, ("all", tuple(lens)), V, R, schedule)
    packed, rep = run_session(pp, ctx, monkeypatch, V, R, 2, schedule)
    assert rep["refused"] == "" and packed["packed_scans"] > 0, rep
    for r in check_rows_against_reference(V, rep):
        assert r["escape_blocks"] == blocks_of(r), r
    assert_same(plain, packed, ("all escapes", lens, R, schedule))


def all_escape_tensor(lens):
    V = np.array(shared_tensor(lens))
    V[np.indices(lens).sum(axis=0) % 2 == 1] *= 2.0 ** -14
    return np.asfortranarray(V)


@pytest.mark.parametrize("lens", [[20, 12, 9, 17], [4, 4, 4, 200]])
def test_branched_escape_decode_same_bits(pp, ctx, monkeypatch, lens):
    """PPALS_PK2_DECODE=branch (read when a context is made): the kernel form that adds the escape bits
    under a wave-uniform branch — on a tensor where blocks with and without escape planes alternate"""
    V = all_escape_tensor(lens)
    keep = shared_tensor(lens)
    sl = (slice(None),) * 3 + (slice(0, lens[3] // 2),)
    V[sl] = keep[sl]                      # the first half of the last mode: no escape blocks
    V = np.asfortranarray(V)
    plain = plain_session(pp, ctx, monkeypatch, ("half", tuple(lens)), V, 10, "msdt")
    monkeypatch.setenv("PPALS_PK2_DECODE", "branch")
    ctx2 = pp.Context(0)
    try:
        packed, rep = run_session(pp, ctx2, monkeypatch, V, 10, 2, "msdt")
    finally:
        ctx2.close()
    assert packed["packed_scans"] > 0
    rows = check_rows_against_reference(V, rep)
    assert any(0 < r["escape_blocks"] < blocks_of(r) for r in rows), rows
    assert_same(plain, packed, ("branch", lens))


def test_switch_unset_follows_the_rule(pp, ctx, monkeypatch):
    """a tensor of 107 MB filled on the device: with the switch unset every twin is of 26 bits exactly
    when its escape blocks are at most 1/16 of its blocks, and the bits are those of a plain session"""
    lens, R = [72, 72, 72, 72], 10
    W0, G0 = pp.init_factors(lens, R, 5), pp.init_factors(lens, R, 99)
    t = pp.Tensor(ctx, lens, 0).fill_cp(pp.init_factors(lens, 4, 1000))
    got = {}
    for mode in ("0", None):
        if mode is None:
            monkeypatch.delenv("PPALS_PACK_LAYOUT", raising=False)
        else:
            monkeypatch.setenv("PPALS_PACK_LAYOUT", mode)
        s = pp.CP(ctx, t, R)
        s.set_schedule("msdt")
        s.set_factors(W0, G0)
        s.sweeps_dt(2)
        W, G = s.get_factors(with_grad=True)
        got[mode] = {"W": np.concatenate([w.ravel() for w in W]), "G": np.concatenate([g.ravel() for g in G]),
                     "gradnorm": np.float64(s.gradnorm())}
        rep = s.placement_report()["packed"]
        s.close()
    t.close()
    assert rep["mode"] == "auto" and rep["refused"] == "" and rep["packed_scans"] > 0, rep
    for r in packed_rows(rep):
        assert r["format"] == (26 if 16 * r["escape_blocks"] <= blocks_of(r) else 28), r
    assert packed_rows(rep), rep
    assert_same(got["0"], got[None], "switch unset")


@pytest.mark.parametrize("pack", [1, 2])
def test_a_block_beyond_the_window_refuses_both_formats(pp, ctx, monkeypatch, pack):
    lens = [16, 16, 16, 16]
    V = refusal_tensor("wide_range", lens)
    plain = plain_session(pp, ctx, monkeypatch, ("wide", tuple(lens)), V, 10, "msdt")
    packed, rep = run_session(pp, ctx, monkeypatch, V, 10, pack)
    assert rep["refused"] == "" and rep["layouts"], rep
    for r in rep["layouts"]:
        assert not r["packed"] and r["reason"].startswith("top bytes of a block span"), r
        assert r["reason"].endswith("values (window 16)") and r["bytes_per_element"] == 4.0, r
    assert packed["packed_scans"] == 0   # the plain layout is read
    assert_same(plain, packed, ("wide_range", pack))


def test_tensor_refilled_while_the_26_bit_session_lives(pp, ctx, monkeypatch):
    """qualifies -> more escape blocks (the planes are sized again) -> refused; the next sweeps are
    those of a fresh plain session on the same contents"""
    lens, R = [16, 16, 16, 16], 10
    V1 = shared_tensor(lens)
    V2 = escape_tensor(model_tensor(lens, 1234), scan_rows(pp, ctx, monkeypatch, lens, "msdt"))
    V3 = refusal_tensor("mixed_sign", lens)
    W0, G0 = pp.init_factors(lens, R, 5), pp.init_factors(lens, R, 99)
    monkeypatch.setenv("PPALS_PACK_LAYOUT", "2")
    t = pp.Tensor(ctx, lens, 0).upload(V1)
    s = pp.CP(ctx, t, R)
    s.set_factors(W0, G0)
    s.sweeps_dt(2)
    assert all(r["escape_blocks"] == 0 for r in check_rows_against_reference(V1, s.placement_report()["packed"]))
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
            assert rep["packed_scans"] > n0, rep
            assert any(r["escape_blocks"] > 0 for r in check_rows_against_reference(V, rep)), rep
        else:
            assert rep["packed_scans"] == n0 and not packed_rows(rep), rep
            assert any(r["reason"].startswith("top bytes") for r in rep["layouts"]), rep
        fresh, _ = run_session(pp, ctx, monkeypatch, V, R, 0, sweeps=2, nodes=False)
        monkeypatch.setenv("PPALS_PACK_LAYOUT", "2")
        assert_same(got, fresh, ("refill", fits))
    s.close()
    t.close()
