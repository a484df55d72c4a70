"""The case table of the mode-update, Normalize and factor-side ops (tests/update_cases.py) on the host stand-in,
through tests/opshim: harness, references and derived bars are proven here before anything reaches a GPU. Bars and
guards apply, routes do not (HostOps logs nothing), the state-hazard cases check results only. Then the checker's
self-test: a correct result perturbed in the ways a kernel goes wrong must be rejected."""
import numpy as np
import pytest

import contraction_cases as CC
import opshim_util
import update_cases as UC

G = CC.GUARD


@pytest.fixture(scope="module")
def sh():
    s = opshim_util.Shim("host")
    yield s
    s.close()


def _run(sh, c, **kw):
    return UC.run_with_env("host", c, False, **kw) if c.get("env") else UC.run_case(sh, c, False, **kw)


@pytest.mark.parametrize("family", UC.FAMILIES)
def test_table_on_hostsim(sh, family):
    cases = [c for c in UC.CASES if c["family"] == family]
    assert cases
    for c in cases:
        assert _run(sh, c) == [], c["name"]  # the stand-in logs nothing


def test_table_is_well_formed():
    names = [c["name"] for c in UC.CASES]
    assert len(names) == len(set(names))
    for c in UC.CASES:
        assert len(c["why"].split()) <= 6 and c["cls"] in ("pos", "mix"), c["name"]
    for fam in UC.FAMILIES:
        assert len({c["cls"] for c in UC.CASES if c["family"] == fam}) == 2 or fam in ("sumsq",), fam
    # the staged / unstaged boundaries of the launcher's formula, as the issue states them
    assert UC.staged(932, 10) and not UC.staged(933, 10) and UC.staged(20, 64) and not UC.staged(21, 64)
    assert UC.update_route(96, 64) == "unstaged" and UC.update_route(97, 64) == "unfused why=rows"
    assert UC.update_route(101, 48) == "staged" and UC.update_route(102, 48) == "unstaged"
    assert UC.update_route(128, 48) == "unstaged" and UC.update_route(129, 48) == "unfused why=rows"
    # no R <= 32 (the most arm_gram_system arms) reaches the unstaged launch
    assert not any(UC.update_route(rows, R) == "unstaged" for R in range(1, 33) for rows in range(1, 6145 // R + 2))


def _case(name):
    (c,) = [c for c in UC.CASES if c["name"] == name]
    return c


def _body(st, name):
    return st.posts[name][G:-G].view(np.float64)


def _rejected(sh, c, p):
    with pytest.raises(AssertionError):
        _run(sh, c, perturb=p)


def test_checker_rejects_perturbed_updates(sh):
    c = _case("update_staged:ld {'xm': 1, 'xw': 2, 'xg': 3}")
    rows, R = c["rows"], c["R"]
    _run(sh, c)
    seen = {}

    def drop_term(st):
        # grad[i, j] loses the term W_old[i, 0] S[0, j]: the class is "pos" or "mix"; take the term's real size
        g, S, W = _body(st, "grad"), _body(st, "S"), st.outs["W"][0].img[G:-G].view(np.float64)
        ldg, ldw = rows + c["xg"], rows + c["xw"]
        i, j = rows // 2, R // 2
        term = W[i] * S[R * j]
        g[i + ldg * j] -= term
        bar = (R + 3) * UC.U * sum(abs(W[i + ldw * k] * S[k + R * j]) for k in range(R))
        seen["term/bar"] = abs(term) / bar

    def shift_row(st):
        w = _body(st, "W")
        ldw = rows + c["xw"]
        w[3:3 + ldw * R:ldw] = w[4:4 + ldw * R:ldw].copy()

    def gram_asym(st):
        g = _body(st, "G")
        e = c["mode"] * R * R + 1  # element (1, 0) of the refreshed Gram
        g[e] = np.nextafter(g[e], np.inf)

    def gap(st):
        _body(st, "grad")[rows] = 1.0  # the first element of the ld gap

    def guards(name, front):
        def p(st):
            st.posts[name][G - 1 if front else -G] ^= 1
        return p

    for p in (drop_term, shift_row, gram_asym, gap):
        _rejected(sh, c, p)
    for name in ("W", "grad", "gradsq", "S", "Sinv", "G"):
        for front in (True, False):
            _rejected(sh, c, guards(name, front))
    assert seen["term/bar"] > 1.0, seen  # (the bar is tight enough that one dropped term shows)


def test_checker_rejects_gradsq_short_of_a_tile(sh):
    """the row-parallel cp_update keeps one partial sum of grad^2 per 64-row tile: the second tile's (rows 64 .. 127
    of 1000) left out of gradsq"""
    c = _case("cp_update:rows R=7 rows=1000")
    rows, R, ldg = c["rows"], c["R"], c["rows"] + c["xg"]
    _run(sh, c)

    def gradsq_short(st):
        g = _body(st, "grad")
        _body(st, "gradsq")[0] -= sum(float(g[i + ldg * j]) ** 2 for i in range(64, 128) for j in range(R))

    _rejected(sh, c, gradsq_short)


def test_checker_rejects_perturbed_factor_side(sh):
    def stale_B(st):
        b = _body(st, "B1")
        b[len(b) // 2] = 0.25

    _rejected(sh, _case("diff_norms:N=8 B store=1 prev=1"), stale_B)

    def pad_row(st):
        _body(st, "blocked")[-1] = 1e-300  # the last row of the last block is padding

    _rejected(sh, _case("blocks:P=3 R=10 short"), pad_row)

    def unpack_gap(st):
        c = _case("blocks:P=3 R=10 short")
        _body(st, "nat")[c["rows"]] = 0.0

    _rejected(sh, _case("blocks:P=3 R=10 short"), unpack_gap)

    def gram_asym(st):
        g = _body(st, "G")
        g[1] = np.nextafter(g[1], np.inf)

    _rejected(sh, _case("gram:rows=257 R=10"), gram_asym)


@pytest.mark.parametrize("name", ["normalize:normalize_ms N=4 R=1 rows=3..", "normalize:normalize N=3 R=10 rows=5.."])
def test_checker_rejects_a_scale_off_by_64u(sh, name):
    """the factor (and with it the Gram) of one mode scaled by (1 + 64 u) more than the others. (At R = 64 the trace
    of 64 terms alone is allowed 32 u in the root, twice in a scale: 64 u is inside the derived bar there.)"""
    c = _case(name)
    _run(sh, c)

    def scale_off(st):
        _body(st, "W1")[:] *= 1 + 64 * UC.U
        n = c["R"] * c["R"]
        _body(st, "G")[n:2 * n] *= (1 + 64 * UC.U) ** 2

    _rejected(sh, c, scale_off)

    def scales_off(st):  # what normalize_scales() returned, on its own
        st.scales[1] *= 1 + 64 * UC.U

    _rejected(sh, c, scales_off)
    # and the bar itself stays well under that: the derived part + the measured pow allowance
    _, _, _, Ef = UC.norm_bars(len(c["rows"]), c["R"], [1.0] * len(c["rows"]))
    assert Ef < 64 * UC.U
