"""The op-level cases of the Tucker eigen side (tests/tucker_ops_cases.py) on the host stand-in, and the self-test of
their checker: mutations of a correct result that it must reject. CPU only; the stand-in logs no route tags, its
top_eigvecs_warm is the full solver and its deferred hand-over sits behind PPALS_HOSTSIM_DEFER."""
import numpy as np
import pytest

import contraction_cases as CC
import opshim_util
import tucker_ops_cases as TC


@pytest.fixture(scope="module")
def sh():
    s = opshim_util.Shim("host")
    yield s
    s.close()


def _run(sh, c, perturb=None):
    if c.get("env"):
        assert perturb is None
        return TC.run_with_env("host", c, False)
    return TC.run_case(sh, c, False, perturb=perturb)


@pytest.mark.parametrize("family", TC.FAMILIES)
def test_family_on_the_stand_in(sh, family):
    failures = []
    cases = [c for c in TC.CASES if c["family"] == family and not c.get("hip_only")]
    for c in cases:
        try:
            _run(sh, c)
        except (AssertionError, opshim_util.ShimError) as e:
            failures.append(str(e))
    assert not failures, f"{len(failures)} of {len(cases)} cases failed:\n" + "\n".join(failures)


def test_numpy_stays_within_every_cap():
    """numpy eigh's own eigenvectors pass every cap with room on every matrix of the table, and the gap condition of the
    builder holds (Ref asserts it); numpy's Householder QR passes the orthogonality bound of the QR cases"""
    worst = [0.0, 0.0]
    for c in TC.CASES:
        if c["op"] in ("eig_full", "eig_warm"):
            for o, r in TC.numpy_within_caps(c):
                worst = [max(worst[0], o), max(worst[1], r)]
        elif c["op"] == "eig_defer":
            rng = np.random.default_rng(c["seed"])
            G, Q = TC.craft(rng, TC.spectrum(c["spec"], c["J"], c["rank"], rng))
            for _ in range(10):
                ref = TC.Ref(G, c["rank"], c["name"])
                _, cap_r, _ = TC.eig_caps(ref, "projector")
                assert ref.res <= cap_r / 4
                G = TC.perturbed(rng, G, 0.01)
        elif c["op"] == "orthonormalize" and c["r"] > 0 and not c.get("bad"):
            A = TC.qr_input(np.random.default_rng(c["seed"]), c["rows"], c["r"], c["cond"])
            Qh, _ = np.linalg.qr(A)
            orth = TC.qr_quantities(A, Qh)[0]
            assert orth <= 6.0 * (c["rows"] * c["r"] + c["r"] * (c["r"] + 1)) * TC.U / 4, (c["name"], orth)
    assert worst[0] <= 0.25 and worst[1] <= 0.25, worst


def test_route_formulas():
    """the launcher's decisions as restated in the table, at the shapes the issue names (256 compute units)"""
    g = lambda *a: TC.gram_route(*a, ncu=256)[0]
    assert g("f32", 1, 64, 4096) == "unfold_gram.syrk nsplit=4"
    assert g("f32", 1, 132, 4096) == "unfold_gram.syrk nsplit=4"
    assert g("f32", 1, 66, 4096).startswith("unfold_gram.mfma.f32")
    assert g("f32", 6, 64, 683).startswith("unfold_gram.mfma.f32")
    assert g("f32", 4, 68, 1024).startswith("unfold_gram.syrk")
    assert g("f64", 1, 33, 1000) == "unfold_gram.mfma.f64 nsplit=3"
    assert g("f64", 1, 64, 15).startswith("unfold_gram.mfma.f64") and g("f64", 1, 64, 4097).startswith("unfold_gram.mfma.f64")
    assert g("f64", 3, 80, 7) == "unfold_gram.sym transposed=1 lds=0"
    assert TC.gram_route("f64", 1, 100, 17, 64)[0] == "unfold_gram.sym transposed=0 lds=1"
    assert g("f32", 1, 15, 37).startswith("unfold_gram.valu.f32")
    assert [TC.full_route(J) for J in (64, 65, 128, 129)] == ["eig.full.lds_jacobi", "eig.full.onesided_jacobi",
                                                               "eig.full.onesided_jacobi", "eig.full.dsyevd"]
    assert sorted({TC.tag_family(t) for t in TC.EXPECTED_TAGS}) == TC.EXPECTED_TAGS


# ------------------------------------------------------------------------------------------ the checker's self-test
def _case(name):
    (c,) = [c for c in TC.CASES if c["name"] == name]
    return c


def _rejects(sh, c, perturb, what):
    TC.run_case(sh, c, False)  # (the unperturbed result passes)
    with pytest.raises(AssertionError, match=what):
        TC.run_case(sh, c, False, perturb=perturb)


EIG = "eig_full/onesided J96 r20 geo"


def _U(st):
    J, rank = st.c["J"], st.c["rank"]
    return st.got("U0").reshape((J, rank), order="F").copy()


def _unwanted(st, k):
    """the eigenvector number k (0-based, descending) of the case's matrix"""
    w, V = np.linalg.eigh(st.ref.G)
    return V[:, ::-1][:, k]


def test_checker_rejects_swapped_columns(sh):
    def p(st):
        Um = _U(st)
        Um[:, [3, 4]] = Um[:, [4, 3]]
        st.put("U0", Um.reshape(-1, order="F"))
    _rejects(sh, _case(EIG), p, "not descending")


def test_checker_rejects_the_wrong_eigenvector(sh):
    def p(st):
        Um = _U(st)
        Um[:, -1] = _unwanted(st, st.c["rank"])  # eigenvector rank + 1 in the place of eigenvector rank
        st.put("U0", Um.reshape(-1, order="F"))
    _rejects(sh, _case(EIG), p, "subspace sine")


def test_checker_rejects_a_scaled_column(sh):
    def p(st):
        Um = _U(st)
        Um[:, 5] *= 1 + 1e-10
        st.put("U0", Um.reshape(-1, order="F"))
    _rejects(sh, _case(EIG), p, r"U\^T U - I")


def test_checker_rejects_a_rotated_column(sh):
    def p(st):
        Um = _U(st)
        Um[:, 5] = Um[:, 5] + 1e-9 * _unwanted(st, st.c["rank"] + 7)
        st.put("U0", Um.reshape(-1, order="F"))
    _rejects(sh, _case(EIG), p, "residual|subspace sine")


GRAM = "unfold_gram/mfma f64 L1 J33 T1000 mix"


def _gram_without(sh, terms):
    """the Gram with the reduction terms `terms` (a slice of the columns of A) left out of the sum"""
    def p(st):
        A = st.A.astype(TC.LD)
        keep = np.ones(A.shape[1], bool)
        keep[terms] = False
        G = (A[:, keep] @ A[:, keep].T).astype(np.float64)
        st.put("G", G.reshape(-1, order="F"))
    return p


def test_checker_rejects_a_dropped_reduction_term(sh):
    _rejects(sh, _case(GRAM), _gram_without(sh, slice(517, 518)), "over the bar")


def test_checker_rejects_a_dropped_last_chunk(sh):
    _rejects(sh, _case(GRAM), _gram_without(sh, slice(1000 - 1000 % 32, None)), "over the bar")
    _rejects(sh, _case("unfold_gram/mfma f32 L1 J33 T1000 mean"), _gram_without(sh, slice(999, None)), "over the bar")


def test_checker_rejects_a_broken_block_seam(sh):
    c = _case("orthonormalize/r130 rows301 cond1000")

    def p(st):
        Q = st.got("U").reshape((c["rows"], c["r"]), order="F").copy()
        # column 64, the first of the second block, leaves the span of the first 65 old columns: rotated by 1e-9
        # towards column 100 (the result stays orthonormal to 1e-18)
        Q[:, 64], Q[:, 100] = Q[:, 64] + 1e-9 * Q[:, 100], Q[:, 100] - 1e-9 * Q[:, 64]
        st.put("U", Q.reshape(-1, order="F"))
    _rejects(sh, c, p, "strictly lower part")


def test_checker_rejects_a_written_guard_byte(sh):
    def front(st):
        st.posts["G"][CC.GUARD - 1] ^= 1

    def back(st):
        st.posts["U0"][-CC.GUARD] ^= 1
    _rejects(sh, _case(GRAM), front, "guard")
    _rejects(sh, _case(EIG), back, "guard")
