"""The contraction case table (tests/contraction_cases.py) on the host stand-in, through tests/opshim: the
harness, the numpy references and the derived bars are proven here before anything reaches a GPU. Bars and
guards apply, routes do not (HostOps logs nothing). Then the checker's self-test: a correct result perturbed in
the ways a kernel goes wrong must be rejected."""
import numpy as np
import pytest

import contraction_cases as CC
import opshim_util


@pytest.fixture(scope="module")
def sh():
    s = opshim_util.Shim("host")
    yield s
    s.close()


@pytest.mark.parametrize("family", CC.FAMILIES)
def test_table_on_hostsim(sh, family):
    cases = [c for c in CC.CASES if c["family"] == family]
    assert cases
    for c in cases:
        tags = CC.run_checked(sh, c, hip=False)
        assert tags == [], (c["name"], tags)  # the stand-in logs nothing


def test_table_is_well_formed():
    names = [c["name"] for c in CC.CASES]
    assert len(names) == len(set(names))
    for c in CC.CASES:
        assert c.get("J", 0) <= CC.MAX_J and len(c["why"].split()) <= 6, c["name"]
        assert c["route"] and c["cls"] in ("pos", "mix")
    assert {c["cls"] for c in CC.CASES} == {"pos", "mix"}


def _case(name):
    (c,) = [c for c in CC.CASES if c["name"] == name]
    return c


SELF = ["scan:f32 fast R=40", "scan:f64 buf R=17", "scan:f32 inplace gaps", "mttv:f64 jsplit acc=1 scale=-0.75",
        "mttv:f32 vec rstride", "ttm_keep:f32 L=31 J=50 Kc=17 T=1", "pp:rows=17 R=10 terms=4",
        "scan:bf16 mfma L=520 J=33 R=40", "scan:f32 prefix ksplit out32"]


@pytest.mark.parametrize("name", SELF)
def test_checker_rejects_perturbed_results(sh, name):
    """one k-term of one element dropped; one row shifted by one; one guard byte written (in front, behind, and in
    a gap where the case has one): each must fail a result that passes untouched"""
    c = _case(name)
    CC.run_case(sh, c, hip=False)
    seen = {}

    def drop_term(r):
        # the smallest |term| an element can lose: min |V| min |B| of the class ("pos": 0.25; "mix" takes the
        # element's own mean term, |V|.|B| / J)
        body = r.post[CC.GUARD:-CC.GUARD].view(r.t)
        e = len(r.idx) // 2
        term = 0.25 if c["cls"] == "pos" else float(r.absprod[e]) / r.J
        body[r.idx[e]] -= term
        seen["term/bar"] = term / float((r.J + 3) * r.u * r.absprod[e])

    def shift_row(r):
        body = r.post[CC.GUARD:-CC.GUARD].view(r.t)
        n = min(16, len(r.idx) - 1)
        body[r.idx[:n]] = body[r.idx[1:n + 1]].copy()

    def guard_front(r):
        r.post[CC.GUARD - 1] ^= 1

    def guard_back(r):
        r.post[-CC.GUARD] ^= 1

    def gap(r):
        body = r.post[CC.GUARD:-CC.GUARD].view(r.t)
        hole = np.setdiff1d(np.arange(body.size), r.idx)
        body[hole[len(hole) // 2]] = 1.0

    for p in (drop_term, shift_row, guard_front, guard_back) + ((gap,) if (c.get("rgap") or c.get("tgap")) else ()):
        with pytest.raises(AssertionError):
            CC.run_case(sh, c, hip=False, perturb=p)
    assert seen["term/bar"] > 1.0, seen  # (the bar is tight enough that one dropped term shows)
