"""The case table of the tensor streams (tests/stream_cases.py) on the host stand-in, through tests/opshim: harness,
references and derived bars are proven here before anything reaches a GPU. Bars and guards apply, routes do not
(HostOps logs nothing). Then the checker's self-test — a correct result perturbed in the ways a kernel goes wrong must
be rejected — and the opposite check: a second reference in fp64 must pass every K10 and uniform_sumsq bar."""
import re

import numpy as np
import pytest

import contraction_cases as CC
import opshim_util
import stream_cases as SC

G = CC.GUARD


@pytest.fixture(scope="module")
def sh():
    s = opshim_util.Shim("host")
    yield s
    s.close()


@pytest.mark.parametrize("family", SC.FAMILIES)
def test_table_on_hostsim(sh, family):
    cases = [c for c in SC.CASES if c["family"] == family]
    assert cases
    for c in cases:
        assert SC.run_case(sh, c, False) == [], c["name"]  # the stand-in logs nothing


def test_table_is_well_formed():
    names = [c["name"] for c in SC.CASES]
    assert len(names) == len(set(names))
    for c in SC.CASES:
        assert len(c["why"].split()) <= 6 and c["cls"] in ("pos", "mix"), c["name"]
    for fam in SC.FAMILIES:
        assert {c["cls"] for c in SC.CASES if c["family"] == fam} == {"pos", "mix"}, fam
    for fam in ("rank_mfma", "rank_split", "rank_stream"):
        res = [c for c in SC.CASES if c["family"] == fam and c["mode"] == 1]
        assert {c["vcls"] for c in res} == {"far", "at", "spike"}, fam
        assert {c["spike"] for c in res if c["vcls"] == "spike"} == {0, 1, 2, 3} or fam == "rank_split", fam
    # rank_plan as the issue states it: K = 131 is 9 column blocks in chunks of 8 and 1 on 256 CUs; the remainder goes
    # to the vector pipe for R = 5, 6, 9, 10, 13, 17 and is refused for 14, 18, 21; bf16 and a misaligned base stream
    p = SC.rank_plan(1, "f32", 260, 131, 13)
    assert (p["tiles"], p["chunks"], p["per"], p["maxrb"], p["rem"]) == (2, 2, 8, 4, 1)
    rems = {R: SC.rank_plan(1, "f64", 130, 131, R)["rem"] for R in range(1, 33)}
    assert {R for R, r in rems.items() if r} == {5, 6, 9, 10, 13, 17} and rems[6] == rems[10] == 2
    assert all(SC.rank_plan(0, "f32", 260, 131, R)["rem"] == 0 for R in range(1, 33))
    assert SC.rank_plan(1, "bf16", 512, 131, 10) is None and SC.rank_plan(1, "f32", 260, 131, 13, aligned=False) is None
    assert SC.rank_plan(1, "f32", 259, 131, 13) is None and SC.rank_plan(1, "f32", 260, 131, 33) is None
    assert [SC.split_plan(1, "f32", 68, 131, R)["maxrbw"] for R in (33, 64, 65, 128, 129, 256)] == [4, 4, 8, 8, 16, 16]
    assert SC.split_plan(1, "f32", 68, 131, 257) is None and SC.split_plan(0, "f64", 34, 131, 36)["chunks"] == 2
    assert SC.stream_plan(32 * 65535, 2)["kch"] == 32 and SC.stream_plan(32 * 65535 + 1, 2)["kch"] == 64
    # every instantiation of EXPECTED_TAGS is the route of some case, and only the multi-chunk cases are device-bound
    fams = set()
    for c in SC.K10:
        tag = re.sub(r"\\", "", c["route"][0])
        fams.add(SC.tag_family(tag))
        assert bool(c["dev"]) == ("chunks=" in tag and "chunks=1 " not in tag), c["name"]
    assert sorted(fams) == SC.EXPECTED_TAGS


K10_AND_SUMSQ = [c for c in SC.CASES if c["op"] in ("rank", "usumsq")]


def test_second_reference_passes_every_bar():
    """numpy in fp64 with its own (BLAS, pairwise) orders, no device: 100 % of the K10 and uniform_sumsq cases must
    pass the bars the devices are held to"""
    failed = []
    for c in K10_AND_SUMSQ:
        try:
            SC.second_reference(c)
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, f"{len(failed)} of {len(K10_AND_SUMSQ)} failed:\n" + "\n".join(failed)


# ------------------------------------------------------------------------------------------ the checker's self-test
def _case(pred):
    return next(c for c in SC.CASES if pred(c))


def _rejected(sh, c, p):
    SC.run_case(sh, c, False)
    with pytest.raises(AssertionError):
        SC.run_case(sh, c, False, perturb=p)


def move(name, k=4.0):
    """one result element moved by k bars (an exact result: its lowest bit flipped)"""
    def p(st):
        body, res = st.body(name)
        dt, ex = st.outs[name][2], st.expect[name]
        e = len(res) // 2
        if isinstance(ex, np.ndarray):
            body.view(np.uint8)[res[e] * body.dtype.itemsize] ^= 1
        else:
            body[res[e]] = SC.encode(np.array([ex.moved(SC.decode(body[res], dt), e, k)]), dt)[0]
    return p


def guard(name, front):
    def p(st):
        st.posts[name][G - 1 if front else -G] ^= 1
    return p


def _residual_terms(st):
    d = st.d
    e = d["Vx"] - d["Q"] @ d["P"].T
    return e * e


def without_last_element(st):
    e2 = _residual_terms(st)
    st.body("out")[0][0] = np.sum(e2) - e2[-1, -1]


def last_column_twice(st):
    e2 = _residual_terms(st)
    st.body("out")[0][0] = np.sum(e2) + np.sum(e2[:, -1])


@pytest.mark.parametrize("family", ["rank_mfma", "rank_split", "rank_stream"])
def test_checker_rejects_perturbed_k10(sh, family):
    c = _case(lambda c: c["family"] == family and c["mode"] == 1 and c["vcls"] == "far" and c["M"] > 8)
    for p in (move("out"), move("out", -4.0), without_last_element, last_column_twice, guard("out", True),
              guard("out", False)):
        _rejected(sh, c, p)
    c = _case(lambda c: c["family"] == family and c["mode"] == 1 and c["vcls"] == "at" and c["dt"] != "f64")
    for p in (without_last_element, last_column_twice):  # (sharp at the solution too: e is the storage rounding)
        _rejected(sh, c, p)
    if family != "rank_split":  # (the sum of squares never takes rank_split)
        c = _case(lambda c: c["family"] == family and c["mode"] == 2)
        _rejected(sh, c, move("out"))
    for dt in ("f32", "f64") + (("bf16",) if family == "rank_stream" else ()):
        c = _case(lambda c: c["family"] == family and c["mode"] == 0 and c["dt"] == dt)
        for p in (move("V"), guard("V", True), guard("V", False)):
            _rejected(sh, c, p)
    SC.run_case(sh, c, False, perturb=lambda st: None)  # (the hook itself does not fail a case)


def test_checker_rejects_a_write_in_front_of_a_misaligned_result(sh):
    c = _case(lambda c: c["op"] == "rank" and c["mode"] == 0 and c["voff"])

    def lead(st):
        st.body("V")[0][0] = 0

    _rejected(sh, c, lead)


def test_checker_rejects_perturbed_generators(sh):
    for op in ("uniform", "noise", "usumsq", "laplacian"):
        for dt in ("f32", "f64", "bf16") if op != "usumsq" else (None,):
            c = _case(lambda c: c["op"] == op and c.get("dt") == dt)
            name = "out" if op == "usumsq" else "V"
            for p in (move(name), guard(name, True), guard(name, False)):
                _rejected(sh, c, p)

    def wrong_shard(st):  # the values of the shard one row further down
        body, res = st.body("V")
        l0 = st.c["l0"]
        body[res[:l0 - 1]] = body[res[1:l0]].copy()

    _rejected(sh, _case(lambda c: c["op"] == "uniform" and c["dt"] == "f64"), wrong_shard)


def test_checker_rejects_perturbed_layouts_and_shards(sh):
    c = _case(lambda c: c["op"] == "pad" and c["rows"] == 70 and c["blk"] == 50)

    def pad_nonzero(st):
        body, _ = st.body("dst")
        body.view(np.uint8)[c["blk"] * body.dtype.itemsize] = 1  # element blk of the first block: padding

    for p in (pad_nonzero, move("dst"), guard("dst", True), guard("dst", False)):
        _rejected(sh, c, p)
    c = _case(lambda c: c["op"] == "unpack")
    for p in (move("full"), guard("full", False)):
        _rejected(sh, c, p)
    c = _case(lambda c: c["op"] == "krp" and len(c["fac"]) == 3)
    for p in (move("out"), guard("out", True)):
        _rejected(sh, c, p)
    c = _case(lambda c: c["op"] == "shard" and c["dt"] == "bf16")

    def other_row(st):
        st.host["host_full"][3, 0] = 0.0  # a row of another rank

    def shard_row(st):
        a = st.host["host_full"][3, c["row0"]]
        st.host["host_full"][3, c["row0"]] = np.nextafter(a, 2.0)

    for p in (move("V"), guard("V", True), other_row, shard_row):
        _rejected(sh, c, p)
