"""GPU parity tests (run with -m gpu on an MI355X): the HIP engine, called through the C ABI
(libppals.so via ctypes), against the fp64 CPU oracle on the same seeded inputs.

Tolerances: fp64 tensor storage -> 1e-10 relative (pure rounding-order differences); fp32 tensor
storage -> kernels 2e-6 relative, factor matrices after sweeps 1e-5 relative Frobenius (the
tolerance BASELINE.json's north_star states)."""
import os

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

KTOL = {0: 2e-6, 1: 1e-10}   # per-kernel relative Frobenius tolerance by dtype (F32, F64)
FTOL = {0: 1e-5, 1: 1e-8}    # factor matrices after several sweeps


def FTOL_R2_F32(kappa):
    """fp32 storage on the non-low-rank `r2` input, oracle on the same fp32-rounded tensor: 1e-5 plus
    the fp32 chain rounding amplified by kappa = cond(S) (measured: 0.9e-7 x kappa at kappa = 1.7e3). The
    coefficient is 3 x what the GPU run measured (profiles/r05_fp32_bars.jsonl); DESIGN.md §5."""
    return 1e-5 + 3e-7 * kappa


@pytest.fixture(scope="module")
def pp():
    import ppals
    return ppals


@pytest.fixture(scope="module")
def ctx(pp):
    c = pp.Context(0)
    yield c
    c.close()


def relerr(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def problem(lens, R, seed, kind="r2"):
    if kind == "r":
        Wt = O.init_factors(lens, R, 1000 + seed)
        V = O.build_V(Wt)
    else:
        V = O.fill_uniform(int(np.prod(lens)), 77 + seed, lo=0.5, hi=1.0).reshape(lens, order="F")
    W = O.init_factors(lens, R, 2000 + seed)
    return V, W


SHAPES = [
    ([8, 8, 8, 8], 3),        # aligned everywhere
    ([5, 6, 7, 4], 3),        # nothing aligned, tiny tails
    ([20, 12, 16, 10], 10),   # headline rank
    ([16, 8, 12, 8], 20),     # two n-tiles
    ([8, 4, 8, 4], 40),       # four n-tiles (padded to 64)
    ([24, 10, 9], 5),         # order 3 (generalised tree)
    ([6, 5, 4, 3, 4], 4),     # order 5
    ([4, 3, 4, 3, 2, 3], 2),  # order 6
    ([70, 66, 5, 3], 6),      # M spans several waves / workgroups, short K
    ([3, 5, 40, 37], 6),      # long K (split-K path), short M
]


@pytest.mark.parametrize("dtype", [0, 1])
def test_fill_and_norm(pp, ctx, dtype):
    lens = [7, 6, 5, 9]
    t = pp.Tensor(ctx, lens, dtype).fill_uniform(123, 0.5, 1.0)
    ref = O.fill_uniform(int(np.prod(lens)), 123, lo=0.5, hi=1.0)
    assert abs(t.norm() - np.linalg.norm(ref)) < (1e-6 if dtype == 0 else 1e-12) * np.linalg.norm(ref)
    Wt = O.init_factors(lens, 4, 5)
    t2 = pp.Tensor(ctx, lens, dtype).fill_cp(Wt)
    V = O.build_V(Wt)
    assert abs(t2.norm() - np.linalg.norm(V)) < (1e-6 if dtype == 0 else 1e-12) * np.linalg.norm(V)
    s = pp.CP(ctx, t2, 4)
    s.set_factors(Wt)
    assert s.residual() < (1e-6 if dtype == 0 else 1e-12) * np.linalg.norm(V)
    W2 = O.init_factors(lens, 4, 6)
    s.set_factors(W2)
    assert abs(s.residual() - O.residual(V, W2)) < (1e-6 if dtype == 0 else 1e-11) * O.residual(V, W2)


@pytest.mark.parametrize("vt", [1, 0])
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("lens,R", SHAPES)
def test_tree_nodes_and_mttkrp(pp, ctx, lens, R, dtype, vt, monkeypatch):
    """K1/K2/K3: every first-level node and every mode's MTTKRP vs the oracle. vt=1: the right
    node runs as a suffix scan of the transposed resident copy; vt=0: as the prefix scan (K2)."""
    monkeypatch.setenv("PPALS_TRANSPOSED_COPY", str(vt))
    V, W = problem(lens, R, 1)
    t = pp.Tensor(ctx, lens, dtype).upload(V)
    s = pp.CP(ctx, t, R)
    s.set_factors(W)
    tree = O.dimension_tree(len(lens))
    N = len(lens)
    for key, info in tree.items():
        if len(info["parent"]) != N or len(key) == 1:
            continue
        got = s.tree_node(key)
        want = O.tree_node(V, W, key).ravel(order="F")
        assert relerr(got, want) < KTOL[dtype], (key, relerr(got, want))
    for mode in range(N):
        got = s.mttkrp(mode)
        want = O.mttkrp(V, W, mode, 0)
        assert relerr(got, want) < KTOL[dtype], (mode, relerr(got, want))


@pytest.mark.parametrize("blocks", [2, 4, 8])
@pytest.mark.parametrize("dtype", [0, 1])
def test_update_reads_gathered_row_blocks(pp, blocks, dtype, monkeypatch):
    """The sharded mode's update on P ranks reads the all-gather's receive buffer as it lies: P row blocks
    of s / P rows, block p at p * blk * R with leading dimension blk (k_cp_mode_update's `mblk`;
    Ops::cp_mode_update_blocked). On one GPU the test hook PPALS_TEST_BLOCKED_UPDATE=P routes every
    mode update whose extent P divides through that addressing: same sweeps as the oracle."""
    monkeypatch.setenv("PPALS_TEST_BLOCKED_UPDATE", str(blocks))
    lens, R = [16, 24, 8, 32], 6
    V, W = problem(lens, R, 4, "r")
    G = O.init_factors(lens, R, 99)
    _, _, W_ref, G_ref = O.als_cp_dt(V, W, G, tol=0.0, maxiter=3, resprint=1000)
    c2 = pp.Context(0)
    t = pp.Tensor(c2, lens, dtype).upload(V)
    for schedule in ("msdt", "dt"):
        s = pp.CP(c2, t, R)
        s.set_schedule(schedule)
        s.set_factors(W, G)
        s.sweeps_dt(4)
        W_got, G_got = s.get_factors(with_grad=True)
        for a, b in zip(W_got, W_ref):
            assert relerr(a, b) < FTOL[dtype], (schedule, relerr(a, b))
        gn_ref = np.sqrt(sum(np.linalg.norm(g) ** 2 for g in G_ref))
        assert abs(s.gradnorm() - gn_ref) < 1e-3 * gn_ref + 1e-9
        s.close()
    t.close()
    c2.close()


@pytest.mark.parametrize("lens,R", [([600, 250, 12], 20), ([300, 500, 40], 20), ([520, 260, 150], 17)])
def test_scan_with_a_partial_last_round(pp, ctx, lens, R):
    """A first-level scan of a little more than one round of resident workgroups (two n-tiles, fp32:
    586 / 586 / 529 tiles of 256 rows on 512 slots) runs its last tiles in TAIL MODE
    (k_scan_suffix_fast, OPT bit 3: four workgroups per tile, the four waves of each split the k range —
    1, 3 and 10 blocks of 16 here: waves with an empty range, ragged last strip — and meet in LDS):
    node `ab` = V x_c W_c and every mode's MTTKRP against the oracle at kernel accuracy."""
    V, W = problem(lens, R, 8)
    t = pp.Tensor(ctx, lens, 0).upload(V)
    s = pp.CP(ctx, t, R)
    s.set_schedule("dt")
    s.set_factors(W)
    got = s.tree_node("ab")
    want = O.tree_node(V, W, "ab").ravel(order="F")
    assert relerr(got, want) < KTOL[0], relerr(got, want)
    for mode in range(3):
        assert relerr(s.mttkrp(mode), O.mttkrp(V, W, mode, 0)) < KTOL[0], mode
    s.close()
    t.close()


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("lens,R", [([8, 8, 8, 8], 3), ([5, 6, 7, 4], 3), ([12, 10, 9, 11], 10),
                                    ([9, 8, 7], 4), ([5, 4, 3, 4, 3], 2)])
def test_pp_operators(pp, ctx, lens, R, dtype):
    """K8: every pair operator and every full MTTKRP of the PP cache vs the oracle"""
    V, W = problem(lens, R, 2)
    t = pp.Tensor(ctx, lens, dtype).upload(V)
    s = pp.CP(ctx, t, R)
    s.set_factors(W)
    N = len(lens)
    keys = []
    for i in range(N):
        for j in range(i + 1, N):
            keys.append("".join(chr(97 + m) for m in range(N) if m not in (i, j)))
        keys.append("".join(chr(97 + m) for m in range(N) if m != i))
    for key in keys:
        got = s.pp_operator(key)
        want = O.pp_operator(V, W, key).ravel(order="F")
        assert relerr(got, want) < KTOL[dtype], (key, relerr(got, want))


@pytest.mark.parametrize("R", [3, 10, 20, 33])
def test_gram_system(pp, ctx, R):
    """K4 + the S^-1 of K6 vs the oracle's Hadamard/Gram and numpy's inverse"""
    lens = [40, 36, 50, 44]
    W = O.init_factors(lens, R, 7)
    t = pp.Tensor(ctx, [4, 4, 4, 4], 1).fill_uniform(1)
    t2 = pp.Tensor(ctx, lens, 0)
    s = pp.CP(ctx, t2, R)
    s.set_factors(W)
    for mode in range(4):
        S, Si = s.gram_system(mode, 0.125)
        want = O.gram_hadamard(W, mode, 0.125)
        assert relerr(S, want) < 1e-13
        assert relerr(Si @ want, np.eye(R)) < 1e-9 * np.linalg.cond(want)
        X = O.svd_solve(np.eye(R), want)
        assert relerr(Si, X) < 1e-9 * np.linalg.cond(want)
    del t


def test_jacobi_fallback_path(pp, tmp_path):
    """the Jacobi eigen-inverse (fallback when the pivoted-free SPD inverse meets a non-positive pivot) gives the same
    sweeps as the SPD fast path; forced through PPALS_FORCE_JACOBI on a fresh context"""
    import os
    lens, R = [12, 10, 9, 11], 4
    V, W = problem(lens, R, 3, "r")
    G = O.init_factors(lens, R, 99)
    _, _, W_ref, _ = O.als_cp_dt(V, W, G, tol=0.0, maxiter=3, resprint=1000)
    os.environ["PPALS_FORCE_JACOBI"] = "1"
    try:
        c2 = pp.Context(0)
    finally:
        del os.environ["PPALS_FORCE_JACOBI"]
    t = pp.Tensor(c2, lens, 1).upload(V)
    s = pp.CP(c2, t, R)
    s.set_factors(W, G)
    S, Si = s.gram_system(1, 0.0)
    assert relerr(Si @ S, np.eye(R)) < 1e-9 * np.linalg.cond(S)
    s.sweeps_dt(4)
    for a, b in zip(s.get_factors(), W_ref):
        assert relerr(a, b) < 1e-8
    c2.close()


@pytest.mark.parametrize("schedule", ["msdt", "dt"])
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("lens,R,kind", [([12, 10, 9, 11], 4, "r"), ([12, 10, 9, 11], 4, "r2"),
                                         ([16, 16, 16, 16], 10, "r"), ([14, 9, 11], 3, "r"),
                                         ([6, 5, 4, 5, 4, 3], 2, "r"), ([9, 7, 8, 6, 5], 2, "r")])
def test_dt_sweeps_match_oracle(pp, ctx, lens, R, kind, dtype, schedule):
    """K sweeps of the HIP engine == K sweeps of alsCP_DT in the oracle (factor matrices within
    1e-5 relative Frobenius for fp32 storage), for both sweep schedules: the multi-sweep tree
    (default: one tensor scan per N-1 mode updates) and the reference's two-node tree"""
    V, W = problem(lens, R, 3, kind)
    if dtype == 0 and kind == "r2":
        # the non-low-rank stream: the oracle runs on the tensor AS THE ENGINE HOLDS IT (fp32-rounded
        # values, as the cfg2-r2 / cfg5-r2 full-size tests do), so that the comparison sees arithmetic,
        # not storage: 2e-6 of input rounding times cond(S) would otherwise drown it
        V = np.asfortranarray(V.astype(np.float32).astype(np.float64))
    G = O.init_factors(lens, R, 99)
    K = 5
    _, _, W_ref, G_ref = O.als_cp_dt(V, W, G, tol=0.0, maxiter=K - 1, resprint=1000)
    t = pp.Tensor(ctx, lens, dtype).upload(V)
    s = pp.CP(ctx, t, R)
    s.set_schedule(schedule)
    assert s.schedule == (schedule if len(lens) >= 3 else "dt")
    s.set_factors(W, G)
    s.sweeps_dt(K)
    W_got, G_got = s.get_factors(with_grad=True)
    # `r` (exact rank) is the BASELINE problem class and carries the 1e-5 bar. A uniform random
    # tensor fitted with R = 4 is an ill-conditioned ALS problem (nearly collinear factors): what
    # the <= 64-term fp32 chains (and the fp32 first-level intermediate of the multi-sweep schedule)
    # leave in M is amplified by cond(S) = kappa, measured here and in the bar.
    kappa = max(np.linalg.cond(O.gram_hadamard(W_ref, i)) for i in range(len(lens)))
    ftol = FTOL[dtype] if (kind == "r" or dtype == 1) else FTOL_R2_F32(kappa)
    worst = max(relerr(a, b) for a, b in zip(W_got, W_ref))
    from conftest import bar_log
    bar_log("test_dt_sweeps_match_oracle", lens=str(lens), R=R, kind=kind, dtype=dtype, schedule=schedule,
            kappa=kappa, measured=worst, bar=ftol)
    for a, b in zip(W_got, W_ref):
        assert relerr(a, b) < ftol, (relerr(a, b), ftol, kappa)
    gn_ref = np.sqrt(sum(np.linalg.norm(g) ** 2 for g in G_ref))
    assert abs(s.gradnorm() - gn_ref) < 1e-3 * gn_ref + 1e-9
    # grad_W[i] = -M + W_i S (als_CP.cxx:296) element by element, against the scale that formed
    # it: -M and W_i S cancel to ~||grad|| << ||M|| near a solution, so the bar is relative to ||M||
    for i, (a, b) in enumerate(zip(G_got, G_ref)):
        scale = np.linalg.norm(W_ref[i] @ O.gram_hadamard(W_ref, i)) + np.linalg.norm(b)
        assert np.linalg.norm(a - b) < 50 * ftol * scale, (i, np.linalg.norm(a - b), scale)
    assert abs(s.residual() - O.residual(V, W_ref)) < 1e-4 * np.linalg.norm(V) * (1 if dtype == 0 else 1e-4)


def _scalar_multiple(a, b, tol):
    """a == c * b for ONE scalar c > 0 (returned)"""
    c = np.vdot(b, a) / np.vdot(b, b)
    assert c > 0 and relerr(a, c * b) < tol, (c, relerr(a, c * b))
    return c


@pytest.mark.parametrize("roots", [1, 2])
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("lens,R", [([12, 10, 9, 11], 4), ([14, 9, 11], 3), ([6, 5, 4, 5, 4, 3], 2),
                                    ([9, 7, 8, 6, 5], 2)])
def test_normalize_and_owed_scale(pp, ctx, lens, R, dtype, roots, monkeypatch):
    """K7 in isolation (Normalize, common.cxx:644-689, and the engine's bookkeeping around it).
    (1) One sweep WITH Normalize against one sweep of the class API, which has none
    (src/CP.cxx:171): every factor is ONE positive scalar times the un-normalised factor, the
    scalars multiply to 1 (the model tensor is unchanged), all ||W_i||_F come out equal, and the
    cached Grams were rescaled with them (gram_system afterwards == Hadamard of the returned
    factors' Grams). (2) The multi-sweep schedule does not rescale its cached tensors but carries
    the factor OWED to each (X_r and the tree nodes built before the Normalize) into the next
    contraction that reads it: after exactly two sweeps the gradient of every mode — whose MTTKRP
    went through an owed scalar for the modes served by the carried-over step — matches the
    oracle's element by element; a wrong or missing factor shows up as an O(1) error in exactly
    those modes."""
    N = len(lens)
    if roots > N - 2:
        pytest.skip("root set too large for this order")
    monkeypatch.setenv("PPALS_MSDT_ROOTS", str(roots))
    V, W = problem(lens, R, 5, "r")
    G = O.init_factors(lens, R, 99)
    t = pp.Tensor(ctx, lens, dtype).upload(V)
    ktol = 20 * KTOL[dtype]
    for schedule in ("msdt", "dt"):
        s = pp.CP(ctx, t, R)
        s.set_schedule(schedule)
        s.set_factors(W, G)
        s.sweeps_dt(1)
        W1 = s.get_factors()
        _, sw, _, W_nn, _ = O.cpd_als(V, W, G, 0, tol=0.0, maxsweep=0, resprint=10 ** 9)
        assert sw == 1.0
        cs = [_scalar_multiple(a, b, ktol) for a, b in zip(W1, W_nn)]
        assert abs(np.prod(cs) - 1.0) < ktol
        norms = [np.linalg.norm(a) for a in W1]
        assert max(norms) - min(norms) < 1e-12 * max(norms)
        for a, b in zip(W1, O.normalize(W_nn)):
            assert relerr(a, b) < ktol
        for i in range(N):
            S, _ = s.gram_system(i, 0.0)
            assert relerr(S, O.gram_hadamard(W1, i)) < 1e-12, (schedule, i)
        s.sweeps_dt(1)
        W2, G2 = s.get_factors(with_grad=True)
        _, _, W_ref, G_ref = O.als_cp_dt(V, W, G, tol=0.0, maxiter=1, resprint=10 ** 9)
        for i in range(N):
            assert relerr(W2[i], W_ref[i]) < 50 * ktol, (schedule, i, relerr(W2[i], W_ref[i]))
            scale = np.linalg.norm(W_ref[i] @ O.gram_hadamard(W_ref, i)) + np.linalg.norm(G_ref[i])
            assert np.linalg.norm(G2[i] - G_ref[i]) < 50 * ktol * scale, (schedule, i)
        s.close()
    t.close()


@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("lens,R", [([6, 7, 5, 8], 3), ([9, 8, 7, 6, 5], 2)])
def test_pp_operator_after_msdt_sweeps(pp, ctx, lens, R, dtype, monkeypatch):
    """ppals_pp_operator between sweeps: inside a run the PP build borrows the multi-sweep
    intermediate X_r (with the Normalize factor it is owed) as one of its level-1 operators; the
    kernel-level entry point must hand out the operator itself — V contracted with the CURRENT
    factors — whatever the sweep schedule left in its caches (Build_mttkrp_map, als_CP.cxx:352-409)"""
    monkeypatch.setenv("PPALS_MSDT_ROOTS", "1")
    V, W = problem(lens, R, 6, "r")
    G = O.init_factors(lens, R, 99)
    t = pp.Tensor(ctx, lens, dtype).upload(V)
    N = len(lens)
    for schedule in ("msdt", "dt"):
        s = pp.CP(ctx, t, R)
        s.set_schedule(schedule)
        s.set_factors(W, G)
        for nsweeps in (1, 3):
            s.sweeps_dt(nsweeps)
            Wc = s.get_factors()
            for key in [chr(97 + m) for m in range(N)] + ["ab", "".join(chr(97 + m) for m in range(1, N))]:
                got = s.pp_operator(key)
                want = O.pp_operator(V, Wc, key).ravel(order="F")
                assert relerr(got, want) < 5 * KTOL[dtype], (schedule, nsweeps, key, relerr(got, want))
        s.close()
    t.close()


@pytest.mark.parametrize("dtype", [0, 1])
def test_driver_dt_csv_matches_oracle(pp, ctx, dtype, tmp_path):
    lens, R = [10, 9, 8, 7], 3
    V, W = problem(lens, R, 4, "r")
    G = O.init_factors(lens, R, 98)
    Vn = np.linalg.norm(V)
    c_ref, c_got = str(tmp_path / "ref.csv"), str(tmp_path / "got.csv")
    rc_ref, it_ref, W_ref, _ = O.als_cp_dt(V, W, G, tol=1e-7 * Vn, maxiter=60, csv=c_ref, resprint=5)
    t = pp.Tensor(ctx, lens, dtype).upload(V)
    Wl = [w.copy(order="F") for w in W]
    Gl = [g.copy(order="F") for g in G]
    ok = pp.alsCP_DT(t, Wl, Gl, 1e-7 * Vn, 5e3, 60, 0.0, c_got, 5, False, ctx)
    h1, r1 = O.read_csv(c_ref)
    h2, r2 = O.read_csv(c_got)
    assert h1 == h2
    if dtype == 1:
        assert ok == bool(rc_ref) and len(r1) == len(r2)
    n = min(len(r1), len(r2))
    for a, b in zip(r1[:n], r2[:n]):
        assert a[0] == b[0] and a[1] == b[1] and a[4] == b[4]
        tolr = 1e-3 if dtype == 0 else 1e-5
        assert abs(a[2] - b[2]) <= tolr * abs(a[2]) + 1e-5 * Vn * (1 if dtype == 0 else 1e-6)
        assert abs(a[5] - b[5]) <= tolr * abs(a[5]) + 2e-6 * Vn * (1 if dtype == 0 else 1e-5)


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("lens,R", [([12, 11, 10, 9], 3), ([14, 12, 10], 3), ([7, 6, 6, 5, 5], 2),
                                    ([5, 4, 5, 4, 4, 3], 2)])
def test_driver_pp_matches_oracle(pp, ctx, dtype, lens, R, tmp_path):
    """alsCP_PP for orders 3 (a level-1 operator is itself a pair operator), 4, 5 and 6 (several
    levels of scaffolding between the tensor and the pair operators)"""
    V, W = problem(lens, R, 5, "r")
    G = O.init_factors(lens, R, 97)
    Vn = np.linalg.norm(V)
    c_ref, c_got = str(tmp_path / "ref.csv"), str(tmp_path / "got.csv")
    kw = dict(tol=1e-6 * Vn, tol_init=0.1, maxiter=40, resprint=1)
    rc_ref, it_ref, W_ref, _ = O.als_cp_pp(V, W, G, csv=c_ref, **kw)
    t = pp.Tensor(ctx, lens, dtype).upload(V)
    Wl = [w.copy(order="F") for w in W]
    Gl = [g.copy(order="F") for g in G]
    pp.alsCP_PP(t, Wl, Gl, kw["tol"], kw["tol_init"], 5e3, kw["maxiter"], 0.0, 1.0, c_got, 1,
                False, ctx)
    _, r1 = O.read_csv(c_ref)
    _, r2 = O.read_csv(c_got)
    assert any(r[4] == 1 for r in r2), "PP phase never entered"
    n = min(len(r1), len(r2))
    assert n >= 5
    # same DT/PP phase pattern and matching trajectories while both are far from the noise floor
    for a, b in zip(r1[:n], r2[:n]):
        if a[5] < 1e-4 * Vn:
            break
        assert a[1] == b[1] and a[4] == b[4], (a, b)
        assert abs(a[5] - b[5]) <= (2e-3 if dtype == 0 else 1e-5) * abs(a[5])
    if dtype == 1:
        for a, b in zip(Wl, W_ref):
            assert relerr(a, b) < 1e-6


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("lens,R", [([3, 10, 12, 1800], 10),     # coil-100's pattern in small: 3 x . x . x long
                                    ([7, 1700, 13, 4], 10)])     # time-lapse's: a long mode between short ones
def test_long_and_short_modes_exact_and_pp(pp, ctx, dtype, lens, R, tmp_path):
    """The reference's real-data extents in miniature (test_ALS.cxx:287-326): a mode of 1700-1800 rows
    at R = 10 is beyond the staged one-workgroup fused update (the row-parallel route of
    HipOps::cp_mode_update), and the PP operator chains contract their LONGEST mode first
    (CpEngine::pp_last_mode) instead of the reference's lowest (als_CP.cxx:385-390) — same operators,
    same iterates: exact sweeps under both schedules and the alsCP_PP driver against the oracle."""
    V, W = problem(lens, R, 21, "r")
    G = O.init_factors(lens, R, 98)
    Vn = np.linalg.norm(V)
    t = pp.Tensor(ctx, lens, dtype).upload(V)
    _, _, W_ref, _ = O.als_cp_dt(V, W, G, tol=0.0, maxiter=3, resprint=1000)
    for schedule in ("msdt", "dt"):
        s = pp.CP(ctx, t, R)
        s.set_schedule(schedule)
        s.set_factors(W, G)
        s.sweeps_dt(4)
        for a, b in zip(s.get_factors(), W_ref):
            assert relerr(a, b) < FTOL[dtype], (schedule, relerr(a, b))
        if schedule == "msdt":
            # every pair operator and full MTTKRP of the PP build against the oracle's
            Wn = s.get_factors()
            N = len(lens)
            names = "abcdefgh"
            for i in range(N):
                for j in range(i + 1, N):
                    key = "".join(names[m] for m in range(N) if m not in (i, j))
                    got = s.pp_operator(key)
                    want = O.pp_operator(V, Wn, key).ravel(order="F")
                    assert relerr(got, want) < (2e-6 if dtype == 0 else 1e-10), (key, relerr(got, want))
        s.close()
    c_ref, c_got = str(tmp_path / "ref.csv"), str(tmp_path / "got.csv")
    kw = dict(tol=1e-6 * Vn, tol_init=0.1, maxiter=25, resprint=1)
    O.als_cp_pp(V, W, G, csv=c_ref, **kw)
    Wl = [w.copy(order="F") for w in W]
    Gl = [g.copy(order="F") for g in G]
    pp.alsCP_PP(t, Wl, Gl, kw["tol"], kw["tol_init"], 5e3, kw["maxiter"], 0.0, 1.0, c_got, 1, False, ctx)
    _, r1 = O.read_csv(c_ref)
    _, r2 = O.read_csv(c_got)
    assert any(r[4] == 1 for r in r2), "PP phase never entered"
    n = min(len(r1), len(r2))
    # -pp_res_tol 0.1 on this problem overshoots now and then (the oracle's own residual jumps by 20 x and
    # recovers): from the first jump on the trajectory amplifies rounding (1e-5 in fp64 two jumps later).
    # Compared up to there.
    jumps = [k for k in range(1, n) if r1[k][5] > 1.5 * r1[k - 1][5]]
    n = jumps[0] if jumps else n
    assert any(r[4] == 1 for r in r2[:n]), "no PP row before the first overshoot"
    assert n >= 5
    for a, b in zip(r1[:n], r2[:n]):
        if a[5] < 1e-4 * Vn:
            break
        assert a[1] == b[1] and a[4] == b[4], (a, b)
        assert abs(a[5] - b[5]) <= (2e-3 if dtype == 0 else 1e-5) * abs(a[5])
    t.close()


@pytest.mark.parametrize("pct", [1.0, 0.5])
def test_driver_pp_partupdate_matches_oracle(pp, ctx, pct, tmp_path):
    """`-pp 2` (alsCP_PP_partupdate, als_CP.cxx:852-1207): same phase pattern, trajectory and final
    factors as the oracle's literal restatement (fp64 storage)"""
    lens, R = [9, 8, 7, 6], 2
    V, W = problem(lens, R, 12, "r")
    G = O.init_factors(lens, R, 56)
    Vn = np.linalg.norm(V)
    c_ref, c_got = str(tmp_path / "ref.csv"), str(tmp_path / "got.csv")
    kw = dict(tol=1e-7 * Vn, tol_init=0.1, maxiter=60, resprint=1)
    _, it_ref, W_ref, _ = O.als_cp_pp_partupdate(V, W, G, update_percentage=pct, csv=c_ref, **kw)
    t = pp.Tensor(ctx, lens, 1).upload(V)
    s = pp.CP(ctx, t, R)
    s.set_factors(W, G)
    rc, it = s.run_pp_partupdate(csv=c_got, update_percentage=pct, **kw)
    _, r1 = O.read_csv(c_ref)
    _, r2 = O.read_csv(c_got)
    assert any(r[4] == 1 for r in r2)
    n = min(len(r1), len(r2))
    assert n >= 10
    for a, b in zip(r1[:n], r2[:n]):
        if a[5] < 1e-5 * Vn:
            break
        assert a[1] == b[1] and a[4] == b[4], (a, b)
        assert abs(a[5] - b[5]) <= 1e-4 * abs(a[5])
    if it == it_ref:
        for a, b in zip(s.get_factors(), W_ref):
            assert relerr(a, b) < 1e-5


def _laplacian_numpy(N, s):
    """laplacian_tensor (common.cxx:575-642) built the way the reference does: sum over k of
    I x .. x D x .. x I with D = tridiag(-1, 2, -1); index order (a1, b1, a2, b2, ...)"""
    d = N // 2
    D = 2 * np.eye(s) - np.eye(s, k=1) - np.eye(s, k=-1)
    I = np.eye(s)
    V = np.zeros([s] * N)
    letters = "abcdefghijklmnop"
    for k in range(d):
        ops, subs = [], []
        for j in range(d):
            ops.append(D if j == k else I)
            subs.append(letters[2 * j] + letters[2 * j + 1])
        V += np.einsum(",".join(subs) + "->" + letters[:N], *ops)
    return V


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("N,s,folded", [(4, 4, False), (6, 3, False), (6, 3, True), (8, 2, True)])
def test_tensor_p_laplacian(pp, ctx, N, s, folded, dtype):
    """`-tensor p2` (order dim) and `-tensor p` (folded to order dim/2, extents size^2)"""
    Vn = _laplacian_numpy(N, s)
    if folded:
        Vn = Vn.reshape([s * s] * (N // 2), order="F")
    lens = list(Vn.shape)
    t = pp.Tensor(ctx, lens, dtype).fill_laplacian(N, s)
    assert abs(t.norm() - np.linalg.norm(Vn)) < 1e-6 * np.linalg.norm(Vn)
    R = 2
    W = O.init_factors(lens, R, 31)
    c = pp.CP(ctx, t, R)
    c.set_factors(W)
    for mode in range(len(lens)):
        assert relerr(c.mttkrp(mode), O.mttkrp(Vn, W, mode, 0)) < KTOL[dtype]


@pytest.mark.parametrize("dtype", [0, 1])
def test_tensor_c_collinear(pp, ctx, dtype):
    """`-tensor c`: factor collinearity inside [col_min, col_max], lambda weights, and the
    noise term of relative norm ratio_noise (Gen_collinearity, test_ALS.cxx:246-264)"""
    lens, R = [12, 10, 11, 9], 3
    col_min, col_max, ratio, seed = 0.5, 0.9, 0.05, 3
    W = pp.collinear_factors(lens, R, col_min, col_max, seed)
    for j, w in enumerate(W):
        wn = w / np.linalg.norm(w, axis=0)
        Cm = wn.T @ wn
        for a in range(R):
            for b in range(a):
                assert col_min <= Cm[a, b] <= col_max, (j, a, b, Cm[a, b])
    clean = O.build_V([np.asfortranarray(w) for w in W])
    noise = O.fill_uniform(clean.size, seed + 0x5EED, lo=-1.0, hi=1.0).reshape(lens, order="F")
    want = clean + ratio * np.linalg.norm(clean) / np.linalg.norm(noise) * noise
    t = pp.Tensor(ctx, lens, dtype).fill_collinear(R, col_min, col_max, ratio, seed)
    assert abs(t.norm() - np.linalg.norm(want)) < 1e-6 * np.linalg.norm(want)
    Wt = O.init_factors(lens, R, 77)
    c = pp.CP(ctx, t, R)
    c.set_factors(Wt)
    for mode in range(4):
        assert relerr(c.mttkrp(mode), O.mttkrp(want, Wt, mode, 0)) < KTOL[dtype] * 2


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("lens,R,dtype", [([8, 7, 6, 5], 3, 1), ([10, 8, 9], 4, 1),
                                          ([5, 4, 3, 4, 3], 2, 1), ([12, 10, 8, 6], 5, 0)])
def test_class_api_als_matches_oracle(pp, ctx, lens, R, dtype, kind, tmp_path):
    """CPD<double, Optimizer>::als (src/CP.cxx:100-186) for the three optimizer cadences: final
    factors / gradients, the fractional sweep counter, iteration count, return value and the CSV
    rows ([sweeps] column, print cadence) against the oracle's restatement."""
    V, W = problem(lens, R, 5, kind="r")
    G0 = O.init_factors(lens, R, 3000)
    c_ref, c_got = str(tmp_path / "r.csv"), str(tmp_path / "g.csv")
    rc_ref, sw_ref, it_ref, W_ref, G_ref = O.cpd_als(V, W, G0, kind, tol=1e-9, maxsweep=4,
                                                      csv=c_ref, resprint=2)
    t = pp.Tensor(ctx, lens, dtype).upload(V)
    s = pp.CP(ctx, t, R)
    s.set_factors(W, G0)
    rc, sw, it = s.cpd_als(kind, tol=1e-9, maxiter=4, csv=c_got, resprint=2)
    assert (rc, sw, it) == (rc_ref, sw_ref, it_ref)
    W_got, G_got = s.get_factors(with_grad=True)
    tol = 1e-8 if dtype == 1 else 2e-5
    for a, b in zip(W_got, W_ref):
        assert relerr(a, b) < tol, relerr(a, b)
    for a, b in zip(G_got, G_ref):
        assert np.linalg.norm(a - b) < 100 * tol * (1 + np.linalg.norm(b))
    h1, r1 = O.read_csv(c_ref)
    h2, r2 = O.read_csv(c_got)
    assert h1 == h2 and len(r1) == len(r2)
    for a, b in zip(r1, r2):
        assert a[0] == b[0] and a[1] == b[1] and a[4] == b[4] == 0   # dim, sweeps, pp_update
        assert abs(a[2] - b[2]) <= 1e-3 * abs(a[2]) + 1e-6            # gradnorm (6 digits in CSV)
        assert abs(a[5] - b[5]) <= 1e-3 * abs(a[5]) + 1e-5 * np.linalg.norm(V)
    s.close()
    t.close()


def test_class_api_reference_test_case(pp, ctx, tmp_path):
    """the reference's own unit test, tests/test_decomposition.cxx:38-66 (TEST_CPD): order 6,
    s = 13, R = 5, CPD<double, CPDTOptimizer<double>>, Init, als(1e-5, 1000, 30, 100, csv). It
    asserts order and rank only; here the run is also compared with the oracle."""
    from ppals import decomposition as D
    order, size, r = 6, 13, 5
    lens = [size] * order
    V = O.fill_uniform(size ** order, 7).reshape(lens, order="F")       # V->fill_random(0,1)
    W = O.init_factors(lens, r, 11)                                      # W[i].fill_random(0,1)
    t = pp.Tensor(ctx, lens, 1).upload(V)
    decom = D.CPD(order, size, r, ctx, optimizer=D.CPDTOptimizer)
    assert decom.order == 6
    assert decom.rank[0] == 5
    decom.Init(t, W)
    csv = str(tmp_path / "test.csv")
    ok = decom.als(1e-5, 1000, 30, 100, csv)
    G0 = pp.init_factors(lens, r, 3000)
    rc_ref, sw_ref, it_ref, W_ref, G_ref = O.cpd_als(V, W, G0, 1, tol=1e-5, maxsweep=30,
                                                      resprint=100)
    assert ok == bool(rc_ref) and decom.sweeps == sw_ref and decom.iters == it_ref
    for a, b in zip(decom.W, W_ref):
        assert relerr(a, b) < 1e-6, relerr(a, b)
    _, rows = O.read_csv(csv)
    assert rows[0][1] == 0 and rows[-1][1] in (sw_ref, sw_ref - 0.5)
    t.close()


EDGE_SHAPES = [([6, 5, 4], 1), ([1, 5, 4, 3], 2), ([5, 1, 4, 3], 2), ([5, 4, 3, 1], 2), ([7, 6], 3),
               ([3, 2, 3, 2, 2, 3, 2, 2], 2), ([4, 4, 4, 4], 4), ([9, 3, 3, 3], 3),
               ([64, 2, 3, 2], 2), ([2, 3, 2, 130], 3),
               ([3, 32, 32, 90], 20),    # coil-100-like aspect (test_ALS.cxx:296-299), two n-tiles
               ([33, 21, 16, 9], 32),    # time-lapse-like aspect (test_ALS.cxx:315-318), R = 32
               ([90, 85, 82], 80),       # rank above 64: unfused normal equations, two column chunks
               ([70, 9, 8, 7], 65)]      # just above 64, R above the short modes


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("lens,R", EDGE_SHAPES)
def test_edge_shapes(pp, ctx, lens, R, dtype):
    """rank 1, unit extents in every position, order 2 (a matrix) and order 8 (PPALS_MAX_ORDER),
    R = s, one long mode, the aspect ratios of the two image datasets: MTTKRP of every mode and
    three exact sweeps against the oracle"""
    if R > min(lens):  # rank above the shortest mode -> use a generic tensor
        V = O.fill_uniform(int(np.prod(lens)), 5, lo=0.5, hi=1.0).reshape(lens, order="F")
    else:
        V = O.build_V(O.init_factors(lens, R, 1))
    W, G = O.init_factors(lens, R, 2), O.init_factors(lens, R, 3)
    t = pp.Tensor(ctx, lens, dtype).upload(V)
    s = pp.CP(ctx, t, R)
    s.set_factors(W, G)
    for m in range(len(lens)):
        assert relerr(s.mttkrp(m), O.mttkrp(V, W, m, 0)) < KTOL[dtype], (lens, m)
    s.sweeps_dt(3)
    _, _, W_ref, G_ref = O.als_cp_dt(V, W, G, tol=0.0, maxiter=2, resprint=1000)
    W_got, G_got = s.get_factors(with_grad=True)
    if R > min(lens) or R > 64:
        # R exceeds a mode extent (that mode's Gram is singular) or is simply large: the Hadamard
        # product S is ill-conditioned; compare the model tensor, which both solvers agree on
        assert abs(O.residual(V, W_got) - O.residual(V, W_ref)) < 1e-3 * O.residual(V, W_ref)
        s.close()
        t.close()
        return
    # order 2 is a rank-R matrix factorisation: W_0 W_1^T is unique, the factors are not well
    # conditioned individually, so compare the model there
    if len(lens) == 2:
        assert relerr(W_got[0] @ W_got[1].T, W_ref[0] @ W_ref[1].T) < 100 * FTOL[dtype]
    else:
        for a, b in zip(W_got, W_ref):
            assert relerr(a, b) < 10 * FTOL[dtype], (lens, relerr(a, b))
    s.close()
    t.close()


def _fuzz_cases(n, seed):
    rng = np.random.default_rng(seed)
    cases = []
    for _ in range(n):
        N = int(rng.integers(2, 7))
        lens = [int(rng.integers(1, 10)) for _ in range(N)]
        lens[int(rng.integers(0, N))] = int(rng.integers(8, 40))   # one longer mode
        # rank above a mode extent makes S singular and the reference's untruncated inverse
        # undefined; its CLI resets such ranks (test_ALS.cxx:121-127)
        R = min(int(rng.integers(1, 7)), min(lens))
        cases.append((lens, R, int(rng.integers(0, 2))))
    return cases


@pytest.mark.parametrize("lens,R,dtype", _fuzz_cases(40, 20260101))
def test_random_shapes_against_oracle(pp, ctx, lens, R, dtype):
    """seeded random orders (2-6), extents (1-39), ranks (1-6) and storage types: every MTTKRP, the
    streaming residual and two exact sweeps against the oracle"""
    V = O.fill_uniform(int(np.prod(lens)), 9, lo=0.5, hi=1.0).reshape(lens, order="F")
    W, G = O.init_factors(lens, R, 21), O.init_factors(lens, R, 22)
    t = pp.Tensor(ctx, lens, dtype).upload(V)
    s = pp.CP(ctx, t, R)
    s.set_factors(W, G)
    for m in range(len(lens)):
        assert relerr(s.mttkrp(m), O.mttkrp(V, W, m, 0)) < KTOL[dtype], (lens, R, m)
    assert abs(s.residual() - O.residual(V, W)) < 1e-5 * O.residual(V, W)
    s.sweeps_dt(2)
    _, _, W_ref, _ = O.als_cp_dt(V, W, G, tol=0.0, maxiter=1, resprint=1000)
    W_got = s.get_factors()
    # generic (not low-rank) tensors can make S ill-conditioned: compare the fit of the models
    r_got, r_ref = O.residual(V, W_got), O.residual(V, W_ref)
    assert abs(r_got - r_ref) < (1e-6 if dtype == 1 else 1e-3) * max(r_ref, 1e-3 * np.linalg.norm(V))
    s.close()
    t.close()


def test_schedule_switch_mid_run(pp, ctx):
    """ppals_cp_set_schedule between sweeps: the cached contractions of the other schedule are
    dropped and the iterates continue unchanged (both schedules compute the same ALS updates)"""
    lens, R = [12, 10, 8, 6], 3
    V, W = problem(lens, R, 4, "r")
    G = O.init_factors(lens, R, 99)
    _, _, W_ref, _ = O.als_cp_dt(V, W, G, tol=0.0, maxiter=5, resprint=1000)
    t = pp.Tensor(ctx, lens, 1).upload(V)
    s = pp.CP(ctx, t, R)
    s.set_factors(W, G)
    for k, sched in enumerate(["msdt", "dt", "dt", "msdt", "msdt", "dt"]):
        s.set_schedule(sched)
        s.sweeps_dt(1)
    for a, b in zip(s.get_factors(), W_ref):
        assert relerr(a, b) < 1e-8, relerr(a, b)
    with pytest.raises(pp.PpalsError):
        s.set_schedule(7)


@pytest.mark.parametrize("roots", [1, 2, 3])
@pytest.mark.parametrize("lens,R", [([12, 10, 8, 6], 3), ([7, 6, 5, 4, 5], 2), ([5, 4, 5, 4, 3, 4], 2),
                                    ([16, 8, 12, 8], 20)])
@pytest.mark.parametrize("dtype", [0, 1])
def test_msdt_root_counts(pp, ctx, lens, R, roots, dtype, monkeypatch):
    """the multi-sweep schedule with 1, 2 or 3 modes contracted by the first-level scan (a sweep
    then needs N/(N-k) tensor scans; the engine picks k from a cost model, PPALS_MSDT_ROOTS forces
    it): root sets that wrap around the last mode, sets that are adjacent only in the second
    resident layout, both storage types — same ALS iterates as alsCP_DT"""
    if roots > len(lens) - 2:
        pytest.skip("needs at least two modes outside the root set")
    monkeypatch.setenv("PPALS_MSDT_ROOTS", str(roots))
    V, W = problem(lens, R, 7, "r")
    G = O.init_factors(lens, R, 99)
    K = 2 * len(lens) // max(1, len(lens) - roots) + 2   # several full cycles of root sets
    _, _, W_ref, G_ref = O.als_cp_dt(V, W, G, tol=0.0, maxiter=K - 1, resprint=1000)
    t = pp.Tensor(ctx, lens, dtype).upload(V)
    s = pp.CP(ctx, t, R)
    s.set_schedule("msdt")
    s.set_factors(W, G)
    s.sweeps_dt(K)
    W_got, G_got = s.get_factors(with_grad=True)
    for a, b in zip(W_got, W_ref):
        assert relerr(a, b) < FTOL[dtype], (roots, relerr(a, b))
    gn_ref = np.sqrt(sum(np.linalg.norm(g) ** 2 for g in G_ref))
    assert abs(s.gradnorm() - gn_ref) < 1e-3 * gn_ref + 1e-9
    s.close()
    t.close()


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("lens,R,never", [([3, 60, 64, 56], 4, {0}),         # coil-100's pattern: 3 x . x . x .
                                          ([60, 64, 56, 3], 4, {3}),         # time-lapse's: a short LAST mode
                                          ([3, 16, 12, 40], 10, None),       # short extents all round: pairs of modes
                                          ([3, 20, 16, 3, 12], 6, None)])    # two short modes, order 5
def test_short_modes_are_never_roots(pp, lens, R, never, dtype, tmp_path, monkeypatch):
    """The multi-sweep schedule's X_r = V x_r W_r is R / s_r times the tensor: for the reference's
    real-data extents (3 x 128 x 128 x 7200, 33 x 1344 x 1024 x 9, test_ALS.cxx:287-326) a root at
    the short mode would write and re-read MORE than the tensor. The cost model (ms_schedule_cost)
    never roots there — the root set is slid back past such modes, as past the partitioned mode of
    a sharded session — and the iterates stay alsCP_DT's."""
    trace = tmp_path / "steps.txt"
    monkeypatch.setenv("PPALS_TRACE_STEPS", str(trace))
    V, W = problem(lens, R, 5, "r")
    G = O.init_factors(lens, R, 99)
    K = 7
    _, _, W_ref, G_ref = O.als_cp_dt(V, W, G, tol=0.0, maxiter=K - 1, resprint=1000)
    c2 = pp.Context(0)
    t = pp.Tensor(c2, lens, dtype).upload(V)
    s = pp.CP(c2, t, R)
    assert s.schedule == "msdt"
    s.set_factors(W, G)
    s.sweeps_dt(K)
    W_got, _ = s.get_factors(with_grad=True)
    for a, b in zip(W_got, W_ref):
        assert relerr(a, b) < FTOL[dtype], relerr(a, b)
    roots, nscan = set(), 0
    for ln in trace.read_text().splitlines():
        kv = dict(tok.split("=") for tok in ln.split() if "=" in tok)
        rset = [(int(kv["root"]) + q) % len(lens) for q in range(int(kv["k"]))]
        roots |= set(rset)
        nscan += 1
        # whatever the cost model chose (single roots with the short mode left out, or pairs of modes):
        # no first-level intermediate as large as half the tensor
        assert R / np.prod([lens[m] for m in rset]) < 0.5, (rset, lens, R)
    assert nscan > 0
    if never is not None:   # long other modes: single roots, 3 scans per 2 sweeps, never the short mode
        assert not (roots & never), (roots, never)
        assert nscan == (3 * K + 1) // 2, (nscan, K)
    s.close()
    t.close()
    c2.close()


def _fuzz_cases_big(n, seed):
    """orders 3-5 with extents large enough for several workgroup tiles, split-K and batched
    scans, unaligned and aligned row counts, ranks on both sides of one n-tile"""
    rng = np.random.default_rng(seed)
    cases = []
    while len(cases) < n:
        N = int(rng.integers(3, 6))
        lens = [int(rng.integers(3, 70)) for _ in range(N)]
        if np.prod(lens) > 3e6 or np.prod(lens) < 2e4:
            continue
        R = min(int(rng.choice([2, 5, 10, 16, 17, 24, 33])), min(lens))
        cases.append((lens, R, int(rng.integers(0, 2))))
    return cases


@pytest.mark.parametrize("lens,R,dtype", _fuzz_cases_big(24, 20260202))
def test_random_larger_shapes_against_oracle(pp, ctx, lens, R, dtype):
    V = O.build_V(O.init_factors(lens, R, 31))
    W, G = O.init_factors(lens, R, 32), O.init_factors(lens, R, 33)
    t = pp.Tensor(ctx, lens, dtype).upload(V)
    s = pp.CP(ctx, t, R)
    s.set_factors(W, G)
    for m in range(len(lens)):
        assert relerr(s.mttkrp(m), O.mttkrp(V, W, m, 0)) < KTOL[dtype], (lens, R, m)
    s.sweeps_dt(2)
    _, _, W_ref, _ = O.als_cp_dt(V, W, G, tol=0.0, maxiter=1, resprint=1000)
    r_got, r_ref = O.residual(V, s.get_factors()), O.residual(V, W_ref)
    assert abs(r_got - r_ref) < (1e-6 if dtype == 1 else 1e-3) * max(r_ref, 1e-3 * np.linalg.norm(V))
    s.close()
    t.close()


@pytest.mark.parametrize("ratio", [0.8, 1.2])
def test_driver_pp_with_magni(pp, ctx, ratio, tmp_path):
    """-magni (ratio_step of SVD_solve_mod, common.cxx:753-756): W = W_init + ratio * (M S^-1 - W_init)
    in the PP phase"""
    lens, R = [12, 11, 10, 9], 3
    V, W = problem(lens, R, 5, "r")
    G = O.init_factors(lens, R, 97)
    Vn = np.linalg.norm(V)
    kw = dict(tol=1e-6 * Vn, tol_init=0.1, maxiter=30, resprint=1)
    c_ref, c_got = str(tmp_path / "ref.csv"), str(tmp_path / "got.csv")
    _, it_ref, W_ref, _ = O.als_cp_pp(V, W, G, ratio_step=ratio, csv=c_ref, **kw)
    t = pp.Tensor(ctx, lens, 1).upload(V)
    s = pp.CP(ctx, t, R)
    s.set_factors(W, G)
    _, it = s.run_pp(ratio_step=ratio, csv=c_got, **kw)
    assert it == it_ref
    _, r1 = O.read_csv(c_ref)
    _, r2 = O.read_csv(c_got)
    assert [r[:2] + [r[4]] for r in r1] == [r[:2] + [r[4]] for r in r2]
    assert any(r[4] == 1 for r in r2)
    for a, b in zip(s.get_factors(), W_ref):
        assert relerr(a, b) < 1e-6
    s.close()
    t.close()


@pytest.mark.parametrize("dtype", [0, 1])
def test_tensor_refill_while_session_alive(pp, ctx, dtype):
    """ppals_tensor_upload / fill_* on a tensor that live sessions were created on: the session
    notices the new generation and rebuilds what it derived from the old contents (second resident
    layout, cached contractions) — first-level nodes of BOTH halves, MTTKRPs and sweeps follow the
    new data (include/ppals.h, contract of ppals_tensor_upload)"""
    lens, R = [12, 10, 8, 6], 3
    V1, W = problem(lens, R, 4, "r")
    V2, _ = problem(lens, R, 9, "r2")
    G = O.init_factors(lens, R, 99)
    t = pp.Tensor(ctx, lens, dtype).upload(V1)
    s = pp.CP(ctx, t, R)
    s.set_factors(W, G)
    s.sweeps_dt(2)            # caches of both schedules' first step are live now
    t.upload(V2)
    s.set_factors(W, G)
    for key in ("ab", "cd"):
        assert relerr(s.tree_node(key), O.tree_node(V2, W, key).ravel(order="F")) < KTOL[dtype], key
    for m in range(4):
        assert relerr(s.mttkrp(m), O.mttkrp(V2, W, m, 0)) < KTOL[dtype], m
    t.upload(V1)              # and back, without touching the factors in between
    s.sweeps_dt(3)
    _, _, W_ref, _ = O.als_cp_dt(V1, W, G, tol=0.0, maxiter=2, resprint=1000)
    for a, b in zip(s.get_factors(), W_ref):
        assert relerr(a, b) < FTOL[dtype], relerr(a, b)
    s.close()
    t.close()


def _bench_lines(path):
    """labels of a pp_bench-format file: text before the comma of every non-empty line"""
    return [ln.split(",")[0] for ln in open(path).read().splitlines() if ln.strip()]


@pytest.mark.parametrize("maxiter,resprint", [(1, 1), (4, 2), (3, 1)])
@pytest.mark.parametrize("lens,R", [([12, 11, 10, 9], 3), ([10, 9, 8], 3)])
def test_bench_mode_matches_oracle(pp, ctx, lens, R, maxiter, resprint, tmp_path):
    """`bool bench = true` of alsCP_DT / alsCP_PP (what pp_bench.cxx:299-314 calls with maxiter 1):
    no heading, [DTtime] at every print point but iter 0 (als_CP.cxx:203-209); the PP phase without
    its restart test, with the [PPfirst]/[PPsecond] bookkeeping and iter++ on exit
    (als_CP.cxx:656-664,735-748,829-830). Factors, gradients, iteration counts, return values and
    the emitted line labels against the oracle's restatement (fp64 storage)."""
    V, W = problem(lens, R, 6, "r")
    G = O.init_factors(lens, R, 96)
    Vn = np.linalg.norm(V)
    # start where PP is a valid approximation (pp_bench itself starts from random factors, where
    # several approximate sweeps in a row are chaotic and no factor comparison means anything)
    _, _, W, G = O.als_cp_dt(V, W, G, tol=0.0, maxiter=7, resprint=1000)
    t = pp.Tensor(ctx, lens, 1).upload(V)
    s = pp.CP(ctx, t, R)
    for phase in ("dt", "pp"):
        c_ref, c_got = str(tmp_path / f"ref_{phase}.csv"), str(tmp_path / f"got_{phase}.csv")
        for c in (c_ref, c_got):
            open(c, "w").write("[timetype],[dtime]\n")   # the driver's heading; callees append
        kw = dict(tol=1e-9 * Vn, maxiter=maxiter, resprint=resprint)
        s.set_factors(W, G)
        if phase == "dt":
            rc_ref, it_ref, W_ref, G_ref = O.als_cp_dt(V, W, G, csv=c_ref, bench=1, **kw)
            rc, it = s.run_dt(csv=c_got, csv_append=1, bench=1, **kw)
        else:
            rc_ref, it_ref, W_ref, G_ref = O.als_cp_pp(V, W, G, tol_init=0.05, csv=c_ref, bench=1, **kw)
            rc, it = s.run_pp(tol_init=0.05, csv=c_got, csv_append=1, bench=1, **kw)
        assert (rc, it) == (rc_ref, it_ref), phase
        assert _bench_lines(c_got) == _bench_lines(c_ref), phase
        labels = _bench_lines(c_got)[1:]
        if phase == "dt":
            assert labels and set(labels) == {"[DTtime]"}
        else:
            assert labels == ["  [PPfirst]  ", "  [PPsecond]  "]
            assert it == maxiter + 2          # the loop's maxiter+1, then iter++ on exit
        W_got, G_got = s.get_factors(with_grad=True)
        for a, b in zip(W_got, W_ref):
            assert relerr(a, b) < 1e-8, (phase, relerr(a, b))
        for a, b in zip(G_got, G_ref):
            assert np.linalg.norm(a - b) < 1e-7 * (1 + np.linalg.norm(b)), phase
    s.close()
    t.close()


def test_bench_mode_ppfirst_starts_at_zero_in_every_pp_phase(pp, ctx, tmp_path):
    """bench-mode PP restarts after 15 sweeps (als_CP.cxx:667-697) without iter++, so alsCP_PP calls
    the PP phase again from iter 15. Its [PPfirst] bookkeeping (dtime_first, als_CP.cxx:627) starts
    at 0 in that phase too: with maxiter 15 the second phase reports at once, and [PPfirst] equals
    [PPsecond] bit for bit."""
    lens, R = [10, 10, 10, 10], 3
    V, W = problem(lens, R, 6, "r")
    G = O.init_factors(lens, R, 96)
    t = pp.Tensor(ctx, lens, 1).upload(V)
    s = pp.CP(ctx, t, R)
    s.set_factors(W, G)
    c_got, c_ref = str(tmp_path / "got.csv"), str(tmp_path / "ref.csv")
    kw = dict(tol=0.0, maxiter=15, resprint=1)
    rc, it = s.run_pp(tol_init=0.05, csv=c_got, csv_append=1, bench=1, **kw)
    rc_ref, it_ref, _, _ = O.als_cp_pp(V, W, G, tol_init=0.05, csv=c_ref, bench=1, **kw)
    assert (rc, it) == (rc_ref, it_ref)
    assert _bench_lines(c_got) == _bench_lines(c_ref) == ["  [PPfirst]  ", "  [PPsecond]  "]
    first, second = (ln.split(",")[1] for ln in open(c_got).read().splitlines() if ln.strip())
    assert first == second, (first, second)
    s.close()
    t.close()


@pytest.mark.parametrize("lens,R", [([20, 20, 20, 20], 5), ([24, 18, 16], 4)])
@pytest.mark.parametrize("dtype", [0, 1])
def test_long_run_factor_parity(pp, ctx, lens, R, dtype):
    """north_star's bar on a LONG run: 200 exact sweeps of a `-tensor r` problem (ALS on these
    collinear U(0,1) problems needs ~100-200 sweeps to converge), factor matrices within 1e-5
    relative Frobenius of the fp64 oracle for fp32 tensor storage (1e-8 for fp64 storage), checked
    along the way as well (sweeps 25, 100, 200) so that a transient drift cannot hide"""
    V, W = problem(lens, R, 11, "r")
    G = O.init_factors(lens, R, 95)
    t = pp.Tensor(ctx, lens, dtype).upload(V)
    s = pp.CP(ctx, t, R)
    s.set_factors(W, G)
    done = 0
    W_ref, G_ref = W, G
    for upto in (25, 100, 200):
        _, _, W_ref, G_ref = O.als_cp_dt(V, W_ref, G_ref, tol=0.0, maxiter=upto - done - 1, resprint=10 ** 6)
        s.sweeps_dt(upto - done)
        done = upto
        for a, b in zip(s.get_factors(), W_ref):
            assert relerr(a, b) < FTOL[dtype], (upto, relerr(a, b))
    r_ref = O.residual(V, W_ref)
    assert abs(O.residual(V, s.get_factors()) - r_ref) < (1e-5 if dtype == 0 else 1e-9) * np.linalg.norm(V)
    s.close()
    t.close()


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("lens,R", [([8, 8, 8, 8], 3), ([12, 6, 7, 5], 10), ([20, 14, 9, 11], 20),
                                    ([4, 9, 3, 7], 32), ([68, 4, 5, 3], 1), ([16, 18, 50], 7),
                                    ([6, 10, 4, 3, 5, 2], 5),
                                    # the residual's last one or two ranks on the vector pipe beside
                                    # 1..4 matrix-core steps (k_rank_mfma<.., REM>): R = 6, 9, 13, 17
                                    ([8, 7, 9], 6), ([7, 9, 8, 6], 9), ([9, 11, 10, 8], 13), ([20, 19, 18], 17),
                                    # ranks above 32: the rank-split residual (k_rank_split), with
                                    # 4 / 8 / 16 rank blocks per wave and ragged last blocks
                                    ([40, 36, 34, 33], 33), ([70, 66, 65], 64), ([120, 101, 103], 100),
                                    ([140, 9, 130, 11], 130), ([260, 257], 250)])
def test_rank_stream_on_matrix_cores(pp, ctx, lens, R, dtype):
    """K10 (build_V and the streaming residual / norm) through the fp64-MFMA kernel: row counts
    that are / are not multiples of a workgroup's 256 rows, column counts with a partial last
    16-block, ranks on both sides of a 4-wide contraction step, both storage types — tensor
    generation, ||V||, ||V - [[W]]|| far from and AT the solution against the oracle"""
    Wt = O.init_factors(lens, R, 41)
    V = O.build_V(Wt)
    Vn = np.linalg.norm(V)
    t = pp.Tensor(ctx, lens, dtype).fill_cp(Wt)
    eps = 1e-6 if dtype == 0 else 1e-13
    assert relerr(t.download(), V) < eps
    assert abs(t.norm() - Vn) < eps * Vn
    s = pp.CP(ctx, t, R)
    W = O.init_factors(lens, R, 42)
    s.set_factors(W)
    assert abs(s.residual() - O.residual(V, W)) < 10 * eps * O.residual(V, W)
    s.set_factors(Wt)    # at the solution: only the storage rounding of V is left
    assert s.residual() < (2e-7 if dtype == 0 else 1e-13) * Vn
    s.close()
    t.close()


def test_rank_above_64_non_spd_fallback(pp, monkeypatch):
    """R > 64 (the reference CLI's default is R = s/2): S^-1 by pivot-free Gauss-Jordan sweeps, and
    when a pivot is not positive the untruncated inverse through a full eigen-decomposition (the
    reference's SVD_solve, common.cxx:710-725) instead of NaNs — up to 128 columns by two conditional
    launches on the stream (one-sided Jacobi of S, Z diag(1/w) Z^T: no host synchronisation), beyond by
    the vendor solver. (1) both eigen routes, forced on an SPD problem, reproduce the sweep route; (2) a rank-deficient problem (R above three of the
    four mode extents, R = s/2 of the long one) ends without a NaN and fits as well as the oracle."""
    lens, R = [90, 85, 82], 80
    V = O.build_V(O.init_factors(lens, 12, 1))
    W, G = O.init_factors(lens, R, 2), O.init_factors(lens, R, 3)
    outs = []
    for force in ("0", "1", "2"):     # block sweeps | vendor dsyevd (host route) | the conditional device route, ungated
        monkeypatch.setenv("PPALS_FORCE_EIGINV", force)
        c2 = pp.Context(0)
        t = pp.Tensor(c2, lens, 1).upload(V)
        s = pp.CP(c2, t, R)
        s.set_factors(W, G)
        S, Si = s.gram_system(1, 0.0)
        assert np.all(np.isfinite(Si))
        assert relerr(Si @ S, np.eye(R)) < 1e-6 * np.linalg.cond(S)
        outs.append(Si)
        s.close()
        t.close()
        c2.close()
    assert relerr(outs[1], outs[0]) < 1e-7 * np.linalg.cond(S)
    assert relerr(outs[2], outs[0]) < 1e-7 * np.linalg.cond(S)
    monkeypatch.setenv("PPALS_FORCE_EIGINV", "0")
    lens, R = [140, 9, 8, 7], 70
    V = O.fill_uniform(int(np.prod(lens)), 5, lo=0.5, hi=1.0).reshape(lens, order="F")
    W, G = O.init_factors(lens, R, 2), O.init_factors(lens, R, 3)
    c2 = pp.Context(0)
    t = pp.Tensor(c2, lens, 1).upload(V)
    s = pp.CP(c2, t, R)
    s.set_factors(W, G)
    s.sweeps_dt(2)
    W_got = s.get_factors()
    assert all(np.all(np.isfinite(w)) for w in W_got)
    _, _, W_ref, _ = O.als_cp_dt(V, W, G, tol=0.0, maxiter=1, resprint=1000)
    r_got, r_ref = O.residual(V, W_got), O.residual(V, W_ref)
    assert r_got < 1.05 * r_ref + 1e-6 * np.linalg.norm(V), (r_got, r_ref)
    s.close()
    t.close()
    c2.close()


@pytest.mark.parametrize("kind", [3, 4])
@pytest.mark.parametrize("lens,R,dtype,ur", [([8, 7, 6, 5], 3, 1, 1), ([8, 7, 6, 5], 3, 1, 3),
                                             ([10, 8, 9], 4, 1, 2), ([6, 5, 4, 5, 4], 2, 1, 1),
                                             ([12, 10, 9, 11], 5, 0, 2)])
def test_class_api_low_rank_optimizers(pp, ctx, lens, R, dtype, ur, kind, tmp_path):
    _low_rank_case(pp, ctx, lens, R, dtype, ur, kind, tmp_path, 0)


@pytest.mark.parametrize("kind", [3, 4])
@pytest.mark.parametrize("lens,R,dtype,ur", [([8, 7, 6, 5], 3, 1, 1), ([8, 7, 6, 5], 3, 1, 3),
                                             ([10, 8, 9], 4, 1, 2), ([12, 10, 9, 11], 5, 0, 2)])
def test_class_api_low_rank_optimizers_randomsvd(pp, ctx, lens, R, dtype, ur, kind, tmp_path):
    """the same with -randomsvd 1: get_rankR_update_cholesky through randomized_svd(X, r, 1)
    (common.cxx:691-709, :780). The oracle follows the reference line by line on the tall matrix
    (Householder QR, one-sided Jacobi SVD of X Q); the engine works on the R x R Gram (Gram-Schmidt,
    eigenvectors of Q^T G Q) — the update U s VT they produce is the same projector X Q Q^T. Both
    draw the start matrix from the counter generator (same seed, one block per update)."""
    _low_rank_case(pp, ctx, lens, R, dtype, ur, kind, tmp_path, 1)


def _low_rank_case(pp, ctx, lens, R, dtype, ur, kind, tmp_path, randomsvd):
    """CPD<double, CPDTLROptimizer>::als / CPD<double, CPMSDTLROptimizer>::als (run.cxx -pp 2 / 3,
    -updaterank ur, -randomsvd; src/optimizer/cp_dt_lr_optimizer.cxx:170-236,
    cp_msdt_lr_optimizer.cxx:163-205, get_rankR_update_cholesky common.cxx:768-786): same CSV rows
    (fractional sweep counter, gradnorm, residual), sweep and step counts and factors as the
    oracle's restatement; with ur = R the low-rank update IS the exact one, so the run must also
    reproduce the exact optimizer it derives from (kind 1 / 2)."""
    V, W = problem(lens, R, 8, "r")
    G = O.init_factors(lens, R, 99)
    Vn = np.linalg.norm(V)
    c_ref, c_got = str(tmp_path / "r.csv"), str(tmp_path / "g.csv")
    kw = dict(tol=1e-9 * Vn, resprint=1)
    maxsweep = 12
    rc_ref, sw_ref, it_ref, W_ref, G_ref = O.cpd_als_lr(V, W, G, kind, ur, maxsweep=maxsweep,
                                                        csv=c_ref, randomsvd=randomsvd, **kw)
    t = pp.Tensor(ctx, lens, dtype).upload(V)
    s = pp.CP(ctx, t, R)
    s.set_factors(W, G)
    rc, sw, it = s.cpd_als_lr(kind, ur, randomsvd, maxiter=maxsweep, csv=c_got, **kw)
    assert (rc, it) == (rc_ref, it_ref) and abs(sw - sw_ref) < 1e-12
    ftol = FTOL[dtype] * 10
    W_got, G_got = s.get_factors(with_grad=True)
    for a, b in zip(W_got, W_ref):
        assert relerr(a, b) < ftol, relerr(a, b)
    _, r1 = O.read_csv(c_ref)
    _, r2 = O.read_csv(c_got)
    assert len(r1) == len(r2)
    for a, b in zip(r1, r2):
        assert abs(a[1] - b[1]) < 1e-5                      # [sweeps] (6 digits in the file)
        assert abs(a[2] - b[2]) < 200 * ftol * (abs(a[2]) + 1e-9 * Vn)
        assert abs(a[5] - b[5]) < 200 * ftol * Vn
    if ur == R and dtype == 1:
        s.set_factors(W, G)
        s.cpd_als(kind - 2, maxiter=maxsweep, **kw)
        for a, b in zip(s.get_factors(), W_got):
            assert relerr(a, b) < 1e-7, relerr(a, b)
    with pytest.raises(pp.PpalsError):
        s.cpd_als_lr(kind, R + 1, maxiter=2)
    with pytest.raises(pp.PpalsError):
        s.cpd_als_lr(kind, ur, 2, maxiter=2)
    s.close()
    t.close()


WIDE_SHAPES = [([64, 40, 36, 32], 100),   # the reference CLI's default rank regime (-rank s/2)
               ([68, 36, 30, 28], 65),    # rows not a multiple of the 64-row tile, 5 n-tiles (one column in the 5th)
               ([72, 44, 40, 24], 70),    # the coil-100 Tucker rank (test_ALS.cxx:366-379) as a CP rank
               ([64, 48, 32, 36], 128),   # 8 full n-tiles
               ([60, 40, 36, 32], 130),   # one wide pass + a narrow remainder of 2 columns
               ([128, 96, 80], 112),      # order 3
               ([48, 40, 36, 32], 200)]   # two wide passes (128 + 72)


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("lens,R", WIDE_SHAPES)
def test_wide_scan_one_pass(pp, lens, R, dtype, monkeypatch):
    """More than 64 result columns (common.cxx:56,83 with the reference's default -rank s/2): the
    fp32 tensor is read ONCE for up to 128 columns (k_scan_wide, tensor tile through LDS). Every
    first-level tree node (suffix form), every MTTKRP and exact sweeps under both schedules (the
    batched single-mode form) against the oracle; fp64 storage takes the 64-column chunks."""
    V, W = problem(lens, R, 3, kind="r")
    G = O.init_factors(lens, R, 3003)
    c2 = pp.Context(0)
    t = pp.Tensor(c2, lens, dtype).upload(V)
    s = pp.CP(c2, t, R)
    s.set_factors(W, G)
    N = len(lens)
    for key, info in O.dimension_tree(N).items():
        if len(info["parent"]) != N or len(key) == 1:
            continue
        e = relerr(s.tree_node(key), O.tree_node(V, W, key).ravel(order="F"))
        assert e < KTOL[dtype], (key, e)
    if dtype == 0 and N == 4:
        # alsCP_DT's sweep: two first-level nodes, ONE tensor pass per 128 columns each
        s.set_schedule("dt")
        c2.profile_enable(1)
        c2.profile_reset()
        s.sweeps_dt(1)
        c2.sync()
        n_first, _, _ = c2.profile_read(0)
        c2.profile_enable(0)
        assert n_first == 2 * -(-R // 128), n_first
        s.set_factors(W, G)
    for mode in range(N):
        e = relerr(s.mttkrp(mode), O.mttkrp(V, W, mode, 0))
        assert e < KTOL[dtype], (mode, e)
    _, _, W_ref, G_ref = O.als_cp_dt(V, W, G, tol=0.0, maxiter=1, resprint=1000)
    for schedule in ("msdt", "dt"):
        s.set_schedule(schedule)
        s.set_factors(W, G)
        s.sweeps_dt(2)
        W_got, G_got = s.get_factors(with_grad=True)
        cond = max(np.linalg.cond(np.prod([w.T @ w for j, w in enumerate(W_ref) if j != i], axis=0))
                   for i in range(N))
        bar = (1e-8 if dtype == 1 else 1e-5) + (1e-15 if dtype == 1 else 3e-8) * cond
        for a, b in zip(W_got, W_ref):
            assert relerr(a, b) < bar, (schedule, relerr(a, b), cond)
    s.close()
    t.close()
    c2.close()


def test_wide_scan_padded_layout_and_switch(pp, monkeypatch):
    """the wide scan on a padded resident layout (rows compacted as they are stored) and its A/B
    switch: PPALS_SCAN_WIDE=0 runs the 64-column chunks — both against the oracle, and against
    each other at rounding level"""
    lens, R = [50, 36, 50, 36], 80      # 50 * 4 B is no multiple of 128 B: padded leading blocks
    V, W = problem(lens, R, 5, kind="r")
    got = {}
    for wide in ("1", "0"):
        monkeypatch.setenv("PPALS_SCAN_WIDE", wide)
        monkeypatch.setenv("PPALS_PAD_LAYOUT", "1")
        c2 = pp.Context(0)
        t = pp.Tensor(c2, lens, 0).upload(V)
        s = pp.CP(c2, t, R)
        s.set_factors(W)
        got[wide] = [s.mttkrp(m) for m in range(4)] + [s.tree_node("ab"), s.tree_node("cd")]
        for m in range(4):
            assert relerr(got[wide][m], O.mttkrp(V, W, m, 0)) < KTOL[0], (wide, m)
        s.close()
        t.close()
        c2.close()
    for a, b in zip(got["1"], got["0"]):
        assert relerr(a, b) < 5e-7


@pytest.mark.parametrize("R", [65, 80, 100, 112, 128])
def test_gram_system_above_64(pp, R, monkeypatch):
    """S and S^-1 (common.cxx:710-725) for 64 < R <= 128: the block Gauss-Jordan sweeps with the
    trailing update on the fp64 matrix cores (k_gram_system_mfma) and the scalar in-LDS sweeps
    (PPALS_GJ_SCALAR=1) against the oracle's Hadamard / numpy's inverse, and against each other"""
    lens = [150, 140, 130, 135]
    W = O.init_factors(lens, R, 7)
    got = {}
    for scalar in ("0", "1"):
        monkeypatch.setenv("PPALS_GJ_SCALAR", scalar)
        c2 = pp.Context(0)
        t2 = pp.Tensor(c2, lens, 0)
        s = pp.CP(c2, t2, R)
        s.set_factors(W)
        for mode in (0, 3):
            S, Si = s.gram_system(mode, 0.125)
            want = O.gram_hadamard(W, mode, 0.125)
            cond = np.linalg.cond(want)
            assert relerr(S, want) < 1e-13
            assert relerr(Si @ want, np.eye(R)) < 1e-9 * cond, (scalar, mode, relerr(Si @ want, np.eye(R)), cond)
            assert relerr(Si, O.svd_solve(np.eye(R), want)) < 1e-9 * cond
            assert np.array_equal(Si, Si.T)       # symmetric bit for bit (both routes average the triangles)
            got[(scalar, mode)] = Si
        s.close()
        t2.close()
        c2.close()
    for mode in (0, 3):
        assert relerr(got[("0", mode)], got[("1", mode)]) < 1e-10 * cond


def _wide_cases(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        N = int(rng.integers(3, 5))
        lens = [int(rng.integers(24, 150 if N == 3 else 64)) for _ in range(N)]
        size = int(np.prod(lens))
        if size < 1.1e6 or size > 5e6:
            continue
        out.append(dict(lens=lens, R=int(rng.integers(65, 161)), sched=str(rng.choice(["dt", "msdt"])),
                        roots=int(rng.integers(0, 3)), pad=int(rng.integers(0, 2)), seed=int(rng.integers(0, 1000))))
    return out


@pytest.mark.parametrize("c", _wide_cases(int(os.environ.get("PPALS_FUZZ_CASES", "8")),
                                          int(os.environ.get("PPALS_FUZZ_SEED", "20261005"))),
                         ids=lambda c: "-".join(map(str, c["lens"])) + f"-R{c['R']}")
def test_wide_scan_random_shapes(pp, c, monkeypatch):
    """seeded random shapes in the regime of more than 64 columns (fp32 storage): extents that are no
    multiples of the 64-row tile or of the 16-column k-block, ranks with a ragged last n-tile, two wide
    passes above 128, k-splits, padded layouts, forced root counts — every MTTKRP and two exact sweeps
    against the oracle (a campaign sets PPALS_FUZZ_CASES / PPALS_FUZZ_SEED)"""
    if c["roots"] > 0 and c["roots"] <= len(c["lens"]) - 2:
        monkeypatch.setenv("PPALS_MSDT_ROOTS", str(c["roots"]))
    monkeypatch.setenv("PPALS_PAD_LAYOUT", str(c["pad"]))
    lens, R = c["lens"], c["R"]
    V, W = problem(lens, R, c["seed"], kind="r")
    G0 = O.init_factors(lens, R, 7 + c["seed"])
    c2 = pp.Context(0)
    t = pp.Tensor(c2, lens, 0).upload(V)
    s = pp.CP(c2, t, R)
    s.set_schedule(c["sched"])
    s.set_factors(W, G0)
    for m in range(len(lens)):
        assert relerr(s.mttkrp(m), O.mttkrp(V, W, m, 0)) < KTOL[0], (c, m)
    s.sweeps_dt(2)
    _, _, W_ref, _ = O.als_cp_dt(V, W, G0, tol=0.0, maxiter=1, resprint=1000)
    cond = max(np.linalg.cond(np.prod([w.T @ w for j, w in enumerate(W_ref) if j != i], axis=0))
               for i in range(len(lens)))
    for a, b in zip(s.get_factors(), W_ref):
        assert relerr(a, b) < 1e-5 + 3e-8 * cond, (c, relerr(a, b), cond)
    s.close()
    t.close()
    c2.close()
