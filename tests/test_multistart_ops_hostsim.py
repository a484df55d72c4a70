"""The case table of the multi-start, constraint and diagnostic ops (tests/multistart_ops_cases.py) on the host
stand-in, through tests/opshim: HostOps inherits the fp64 host defaults of ops.h for all of these ops, so harness,
references and derived bars are proven here before anything reaches a GPU. Bars and guards apply, routes do not
(HostOps logs nothing) beyond the formulas asserted below. Then the checker's self-test: a correct result perturbed
in the ways a kernel goes wrong must be rejected."""
import numpy as np
import pytest

import contraction_cases as CC
import multistart_ops_cases as MC
import opshim_util
import update_cases as UC

G = CC.GUARD
U = UC.U


@pytest.fixture(scope="module")
def sh():
    s = opshim_util.Shim("host")
    yield s
    s.close()


def _run(sh, c, **kw):
    return MC.run("host", sh, c, False, **kw)


@pytest.mark.parametrize("family", MC.FAMILIES)
def test_table_on_hostsim(sh, family):
    cases = [c for c in MC.CASES if c["family"] == family]
    assert cases
    for c in cases:
        assert _run(sh, c) == [], c["name"]  # the stand-in logs nothing


def test_table_is_well_formed():
    names = [c["name"] for c in MC.CASES]
    assert len(names) == len(set(names))
    for c in MC.CASES:
        assert len(c["why"].split()) <= 6 and c["cls"] in ("pos", "mix"), c["name"]
        assert c.get("poison") is None or 0 <= c["poison"] < len(c["ranks"]), c["name"]
    for fam in MC.FAMILIES:
        assert len({c["cls"] for c in MC.CASES if c["family"] == fam}) == 2, fam
    # the one route decision of the ragged launch, made with the largest rank: the shapes the issue names
    assert MC.ragged_route(26, [1, 10, 3]) == "staged" and MC.ragged_route(20, [1, 64, 15, 16, 17]) == "staged"
    assert MC.ragged_route(21, [1, 64, 15, 16, 17]) == "unstaged"
    assert MC.ragged_route(104, [2, 48, 5]) == "unstaged" and MC.ragged_route(101, [2, 48, 5]) == "staged"
    assert MC.ragged_route(21, [64, 1, 33]) == "unstaged" and MC.ragged_route(97, [64, 1, 33]) == "loop"
    assert MC.ragged_route(932, [10, 4]) == "staged" and MC.ragged_route(933, [10, 4]) == "loop"
    assert MC.ragged_route(17, [65, 3]) == "loop" and MC.ragged_route(17, [64, 3]) == "staged"
    # the loop goes through cp_mode_update start by start: rows 933 is unfused at R = 10 and staged at R = 4
    assert UC.update_route(933, 10) == "unfused why=rows" and UC.update_route(933, 4) == "staged"
    assert UC.update_route(17, 65) == "unfused why=R" and UC.update_route(17, 3) == "staged"
    # the HALS launch at R = 64 asks for the whole 64 KB of dynamic LDS, one tile of 64 rows a workgroup
    assert 8 * (64 * 64 + 64 * 64) == 64 * 1024
    assert MC.nn_route(dict(form="single", rows=65, ranks=[17])) == ["update_nn R=17 tiles=2"]
    assert MC.nn_route(dict(form="ragged", rows=64, ranks=[1, 64, 17])) == ["update_nn_ragged rmax=64 tiles=1 starts=3"]
    # the pseudo-inverse: tiles of 256 rows of the longest mode, capped at 1024
    assert MC.pinv_route([1, 255, 256], [2]).endswith("tiles=1") and MC.pinv_route([257], [2]).endswith("tiles=2")
    assert MC.pinv_route([262144], [2]).endswith("tiles=1024") and MC.pinv_route([262144 + 300], [2]).endswith("tiles=1024")
    # the congruence: chunks of 32 rows, 1025 rows is the first extent with two chunks a slab and a short last slab
    assert MC.fms_slabs([1024], [1024]) == 32 and MC.fms_slabs([1025], [1025]) == 17 and MC.fms_slabs([33, 5], [1, 70]) == 5
    # hold-out masks
    assert MC.hold_mask(4, 0xFFFFFFF5) == 0x5 and MC.hold_mask(32, 0x80000005) == 0x80000005 and MC.hold_mask(4, 0xF0) == 0


def _case(name):
    (c,) = [c for c in MC.CASES if c["name"] == name]
    return c


def _body(st, name):
    return st.posts[name][G:-G].view(np.float64)


def _pre(st, name):
    return st.outs[name][0].img[G:-G].view(np.float64)


def _rejected(sh, c, p, match=None):
    with pytest.raises(AssertionError, match=match):
        _run(sh, c, perturb=p)


def _guards(name, front):
    def p(st):
        st.posts[name][G - 1 if front else -G] ^= 1
    return p


def test_checker_rejects_perturbed_hals(sh):
    c = _case("nn_single:tiles R=17 rows=65")
    rows, R = c["rows"], c["ranks"][0]
    ldw, ldg = rows + c["xw"], rows + c["xg"]
    r = R - 1  # the last column: nothing downstream depends on it
    _run(sh, c)
    seen = {}

    def rowsof(st):
        W, Wo, S = _body(st, "W"), _pre(st, "W"), _body(st, "S")
        new = np.array([[W[x + ldw * q] for q in range(R)] for x in range(rows)])
        old = np.array([[Wo[x + ldw * q] for q in range(R)] for x in range(rows)])
        return W, new, old, S[R * r:R * r + R], S[r + R * r]

    def drop_term(st):
        # the sum of the last column's step loses the term q = r - 1 (w' there is the NEW entry). The bar is taken
        # with |M| <= 1, its largest value in either class: term / bar > 1 there holds for the real bar too
        W, new, old, s, d = rowsof(st)
        q = r - 1
        x = max((x for x in range(rows) if new[x, r] > MC.FLOOR), key=lambda x: abs(new[x, q]))
        term = new[x, q] * s[q] / d
        W[x + ldw * r] = max(MC.FLOOR, new[x, r] + term)
        wp = np.concatenate([new[x, :r], old[x, r:]])
        bar = (R + 3) * U * (1.0 + np.sum(np.abs(wp) * np.abs(s))) / d + 2 * U * (abs(old[x, r]) + abs(new[x, r]) + abs(term))
        seen["term/bar"] = abs(term) / bar
        seen["moved"] = W[x + ldw * r] != new[x, r]

    def stale_row(st):
        # the step of the last column takes w_old[x, q] for every q < r (Jacobi instead of Gauss-Seidel)
        W, new, old, s, d = rowsof(st)
        delta = (new[:, :r] - old[:, :r]) @ s[:r] / d
        ok = [x for x in range(rows) if new[x, r] > MC.FLOOR and new[x, r] + delta[x] > MC.FLOOR]
        x = max(ok, key=lambda x: abs(delta[x]))
        W[x + ldw * r] = new[x, r] + delta[x]
        seen["stale"] = abs(delta[x])

    def gram_ulp(st):
        g = _body(st, "G")
        e = c["mode"] * R * R + 1  # element (1, 0) of the refreshed Gram
        g[e] = np.nextafter(g[e], np.inf)

    def gap(st):
        _body(st, "grad")[rows] = 1.0  # the first element of the ld gap

    for p in (drop_term, stale_row):  # (held by the one-step bar itself, in front of the Gram's)
        _rejected(sh, c, p, match=r"\[0\] W: 1 elements over the bar")
    for p in (gram_ulp, gap):
        _rejected(sh, c, p)
    assert seen["term/bar"] > 1.0 and seen["moved"] and seen["stale"] > 0.0, seen
    for name in ("W", "grad", "gradsq", "S", "G"):
        for front in (True, False):
            _rejected(sh, c, _guards(name, front))


def test_checker_rejects_gradsq_short_of_a_tile(sh):
    """the HALS row kernel keeps one partial sum of grad^2 per 64-row tile: the second tile's (rows 64 .. 127 of 129)
    left out of gradsq, for one start of a batched and of a ragged launch"""
    for name, b in (("nn_single:tiles R=17 rows=129", 0), ("nn_batched:K=32 R=2 rows=129", 7),
                    ("nn_ragged:ranks 1,64,17 rows=129", 2)):
        c = _case(name)
        rows, ldg = c["rows"], c["rows"] + c["xg"]
        _, col, _ = MC.table(c["ranks"])
        _run(sh, c)

        def gradsq_short(st):
            g = _body(st, "grad")
            _body(st, "gradsq")[b] -= sum(float(g[i + ldg * j]) ** 2 for i in range(64, 128)
                                         for j in range(col[b], col[b + 1]))

        _rejected(sh, c, gradsq_short)


def test_checker_rejects_perturbed_hold_rows(sh):
    c = _case("hold_rows:rows=65 edges")
    rows, ldw = c["rows"], c["rows"] + c["xw"]
    _run(sh, c)

    def row_left(st):  # row 0 of start 0 is held out: its entry of W left as it was
        _body(st, "W")[0] = _pre(st, "W")[0]

    def score_kept(st):  # row 1 of start 0 is kept: its score not zeroed
        _body(st, "scores")[1] = _pre(st, "scores")[1]

    def untouched_start(st):  # start 2's bit is clear
        _, col, _ = MC.table(c["ranks"])
        _body(st, "grad")[ldw * 0 + (rows + c["xg"]) * col[2]] = 0.0

    def gram_ulp(st):
        g = _body(st, "G")
        _, _, sq = MC.table(c["ranks"])
        e = c["N"] * sq[1] + c["mode"] * 17 * 17 + 1  # element (1, 0) of start 1's Gram
        g[e] = np.nextafter(g[e], np.inf)

    for p in (row_left, score_kept, untouched_start, gram_ulp, _guards("scores", True), _guards("gradsq", False)):
        _rejected(sh, c, p)


def test_checker_rejects_perturbed_ragged_and_grams(sh):
    c = _case("ragged_update:staged ld {'xm': 1, 'xw': 2, 'xg': 3}")
    rows = c["rows"]
    _run(sh, c)

    def gram_ulp(st):
        g = _body(st, "G")
        e = c["N"] * 1 + c["mode"] * 100 + 1  # element (1, 0) of start 1's Gram (ranks 1, 10, 3)
        g[e] = np.nextafter(g[e], np.inf)

    def gap(st):
        _body(st, "W")[rows] = 0.0

    def neighbour_gradsq(st):  # start 1's sum written to start 2's slot as well
        q = _body(st, "gradsq")
        q[2] = q[1]

    for p in (gram_ulp, gap, neighbour_gradsq, _guards("Sinv", True)):
        _rejected(sh, c, p)

    c = _case("gram_ragged:rows=257 N=3")

    def gram_asym(st):
        g = _body(st, "G")
        e = c["N"] * 1 + c["mode"] * 36 + 1  # element (1, 0) of start 1's Gram (ranks 1, 6, 64)
        g[e] = np.nextafter(g[e], np.inf)

    _rejected(sh, c, gram_asym)


def test_checker_rejects_perturbed_diagnostics(sh):
    c = _case("congruence:cols 15x17 N=3")
    Ca = c["Ca"]

    def padded_neighbour(st):  # entry (3, 14) read from the neighbouring column of the padded partial
        phi = _body(st, "Phi")
        phi[3 + Ca * 14] = phi[3 + Ca * 15]

    _rejected(sh, c, padded_neighbour)

    def weight_off(st):
        _body(st, "wb")[16] *= 1 + 2.0 ** -30

    _rejected(sh, c, weight_off)

    c = _case("pinv_ragged:bad pivots")

    def block_left(st):  # start 0 is bad: an entry of its block of P left non-zero
        _body(st, "P1")[3] = 1e-300

    def flag_lost(st):
        st.posts["bad"][G:-G].view(np.int32)[2] = 0

    def asym(st):  # G^-1 of the start with W = [I; 0] (start 5, rank 3, columns 8 .. 10): entry (1, 0) moved by an ulp
        p = _body(st, "P1")
        p[1 + 70 * 8] = np.nextafter(p[1 + 70 * 8], np.inf)

    for p in (block_left, flag_lost, asym, _guards("P0", False)):
        _rejected(sh, c, p)

    c = _case("core_score:R=7 N=4")

    def score_off(st):
        _body(st, "cc")[0] *= 1 + 2.0 ** -36

    _rejected(sh, c, score_off)

    c = _case("fold_slice_sums:lens=(300, 7)")

    def fold_short(st):  # the last term of the first output entry (7 terms) left out: about 1/7 of it
        _body(st, "out")[0] *= 1 - 2.0 ** -40

    _rejected(sh, c, fold_short)

    c = _case("row_dots:rows=257")

    def dots_shift(st):
        o = _body(st, "out")
        o[256] = o[255]

    _rejected(sh, c, dots_shift)
