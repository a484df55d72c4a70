"""bf16 tensor storage (PPALS_BF16) on the GPU.

Every comparison with the oracle runs the oracle on the bf16-rounded tensor (the download of the BF16
tensor, exact in fp64), so it bounds the arithmetic only, and the bars are those of fp32 storage in
tests/test_gpu_cp.py: 2e-6 per kernel, 1e-5 in the factors after sweeps. The drivers whose oracle
restatements take long (PP, -pp 2, the class-API optimizers, the low-rank ones) are compared with the
same run on F32 storage of the same bf16-exact values, which tests/test_gpu_cp.py holds to the
oracle. Parent-process tests use the numpy rounding of tests/bf16_util.py; torch stays out of this
process (tests/bf16_torch_cases.py runs those cases in children)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
from bf16_util import bf16_round, same_values

pytestmark = pytest.mark.gpu

F32, F64, BF16 = 0, 1, 3
KTOL = 2e-6
FTOL = 1e-5
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# the list of tests/test_gpu_cp.py, plus 70 columns (five 16-column passes of the bf16 kernels)
SHAPES = [
    ([8, 8, 8, 8], 3),
    ([5, 6, 7, 4], 3),
    ([20, 12, 16, 10], 10),
    ([16, 8, 12, 8], 20),
    ([8, 4, 8, 4], 40),
    ([24, 10, 9], 5),
    ([6, 5, 4, 3, 4], 4),
    ([4, 3, 4, 3, 2, 3], 2),
    ([70, 66, 5, 3], 6),
    ([3, 5, 40, 37], 6),
    ([16, 12, 10, 9], 70),
]


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


def bf16_tensor(pp, ctx, V):
    """(tensor, its values): V uploaded to BF16 storage and read back (exact in fp64)"""
    t = pp.Tensor(ctx, list(V.shape), BF16).upload(V)
    Vr = t.download()
    assert same_values(Vr, bf16_round(V))
    return t, Vr


def problem(lens, R, seed, kind="r2"):
    if kind == "r":
        V = O.build_V(O.init_factors(lens, R, 1000 + seed))
    else:
        V = O.fill_uniform(int(np.prod(lens)), 77 + seed, lo=0.5, hi=1.0).reshape(lens, order="F")
    return V, O.init_factors(lens, R, 2000 + seed)


# ---------------------------------------------------------------- storage: fills, upload, download
def test_upload_download_round_bit_for_bit(pp, ctx):
    lens = [9, 7, 6, 5]
    rng = np.random.default_rng(1)
    n = int(np.prod(lens))
    flat = rng.standard_normal(n) * np.exp(rng.uniform(-40, 40, n))
    flat[:6] = [np.inf, -np.inf, np.nan, 1 + 2.0 ** -8 + 2.0 ** -30, 2.0 ** -140, -0.0]
    flat[6:200] = (np.arange(194) * 2 + 1) * 2.0 ** -16 + 1.0   # ties of the second rounding
    V = flat.reshape(lens, order="F")
    t = pp.Tensor(ctx, lens, BF16).upload(V)
    assert same_values(t.download(), bf16_round(V))
    assert t.download().reshape(-1, order="F")[3] == 1.0
    t.close()


def test_fills_round_bit_for_bit(pp, ctx):
    lens = [13, 7, 6, 9]
    t = pp.Tensor(ctx, lens, BF16).fill_uniform(123, 0.5, 1.0)
    ref = O.fill_uniform(int(np.prod(lens)), 123, lo=0.5, hi=1.0).reshape(lens, order="F")
    assert same_values(t.download(), bf16_round(ref))
    assert abs(t.norm() - np.linalg.norm(bf16_round(ref))) < 1e-12 * np.linalg.norm(ref)
    # -tensor p: small integers, exact in bf16
    t64 = pp.Tensor(ctx, [4, 4, 4, 4], F64).fill_laplacian(4, 4)
    tl = pp.Tensor(ctx, [4, 4, 4, 4], BF16).fill_laplacian(4, 4)
    assert same_values(tl.download(), bf16_round(t64.download()))
    # -tensor r: the fp64 model rounded once per element (the model's last fp64 bit may differ from
    # the oracle's summation order: at most one bf16 step, and almost never)
    Wt = O.init_factors(lens, 4, 5)
    V = O.build_V(Wt)
    tc = pp.Tensor(ctx, lens, BF16).fill_cp(Wt)
    got, want = tc.download(), bf16_round(V)
    assert np.mean(got == want) > 0.999
    assert np.all(np.abs(got - want) <= 2.0 ** -7 * np.abs(want))
    s = pp.CP(ctx, tc, 4)
    s.set_factors(Wt)
    assert abs(s.residual() - np.linalg.norm(got - V)) < 1e-9 * np.linalg.norm(V)
    # -tensor c: the model, then the noise added to the stored value and rounded again
    tn = pp.Tensor(ctx, lens, BF16).fill_collinear(4, seed=3)
    t6 = pp.Tensor(ctx, lens, F64).fill_collinear(4, seed=3)
    assert relerr(tn.download(), t6.download()) < 2.0 ** -8
    for x in (t, t64, tl, tc, tn, t6):
        x.close()
    s.close()


def test_tucker_is_refused(pp, ctx):
    t = pp.Tensor(ctx, [6, 5, 4], BF16).fill_uniform(1)
    with pytest.raises(pp.PpalsError, match="error -5.*bf16"):
        pp.Tucker(ctx, t, [2, 2, 2])
    t.close()


# ---------------------------------------------------------------- kernels against the oracle
@pytest.mark.parametrize("lens,key", [([16, 16, 16, 16], "ab"), ([40, 24, 1200], "ab")])
def test_the_matrix_core_scan_runs(pp, ctx, lens, key):
    """the suffix scans of aligned shapes run on the bf16 matrix cores, not on the fp64 fallbacks: with
    a tensor of ones and factor entries 1/3, the fallback's fp64 products are exact to ~1e-16, while the
    three bf16 pieces of the Khatri-Rao value (1/3)^k carry it to ~2^-24 — the result must show that
    rounding (and stay inside the kernel bar). [40, 24, 1200]: the kept node of 960 rows reduces over
    1200 — the K-split path"""
    R = 3
    t = pp.Tensor(ctx, lens, BF16).upload(np.ones(lens))
    s = pp.CP(ctx, t, R)
    W = [np.full((n, R), 1.0 / 3.0, order="F") for n in lens]
    s.set_factors(W)
    V = np.ones(lens)
    got = s.tree_node(key)
    want = O.tree_node(V, W, key).ravel(order="F")
    err = relerr(got, want)
    assert 1e-12 < err < KTOL, err
    s.close()
    t.close()



@pytest.mark.parametrize("vt", [1, 0])
@pytest.mark.parametrize("lens,R", SHAPES)
def test_tree_nodes_and_mttkrp(pp, ctx, lens, R, vt, monkeypatch):
    """vt=1: the second resident layout (every first-level node a suffix scan on the bf16 matrix
    cores); vt=0: the prefix form of the right node"""
    monkeypatch.setenv("PPALS_TRANSPOSED_COPY", str(vt))
    V, W = problem(lens, R, 1)
    t, V = bf16_tensor(pp, ctx, V)
    s = pp.CP(ctx, t, R)
    s.set_factors(W)
    N = len(lens)
    for key, info in O.dimension_tree(N).items():
        if len(info["parent"]) != N or len(key) == 1:
            continue
        got = s.tree_node(key)
        want = O.tree_node(V, W, key).ravel(order="F")
        assert relerr(got, want) < KTOL, (key, relerr(got, want))
    for mode in range(N):
        assert relerr(s.mttkrp(mode), O.mttkrp(V, W, mode, 0)) < KTOL, mode
    s.close()
    t.close()


@pytest.mark.parametrize("lens,R", [([8, 8, 8, 8], 3), ([12, 10, 9, 11], 10), ([9, 8, 7], 4),
                                    ([5, 4, 3, 4, 3], 2)])
def test_pp_operators(pp, ctx, lens, R):
    V, W = problem(lens, R, 2)
    t, V = bf16_tensor(pp, ctx, V)
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
        assert relerr(got, want) < KTOL, (key, relerr(got, want))
    s.close()
    t.close()


@pytest.mark.parametrize("lens,R", [([6, 5, 7, 6], 3), ([50, 50, 40, 36], 4), ([9, 40, 33, 7, 5], 17)])
def test_padded_layouts(pp, ctx, lens, R, monkeypatch):
    """the padded resident layouts (tests/padded_cases.py's shapes, padding forced): compact results"""
    monkeypatch.setenv("PPALS_PAD_LAYOUT", "1")
    V, W = problem(lens, R, 4, "r")
    t, V = bf16_tensor(pp, ctx, V)
    s = pp.CP(ctx, t, R)
    s.set_factors(W)
    for mode in range(len(lens)):
        assert relerr(s.mttkrp(mode), O.mttkrp(V, W, mode, 0)) < KTOL, mode
    G = O.init_factors(lens, R, 99)
    _, _, W_ref, _ = O.als_cp_dt(V, W, G, tol=0.0, maxiter=2, resprint=1000)
    s.set_factors(W, G)
    s.sweeps_dt(3)
    for a, b in zip(s.get_factors(), W_ref):
        assert relerr(a, b) < FTOL, relerr(a, b)
    s.close()
    t.close()


@pytest.mark.parametrize("schedule", ["msdt", "dt"])
@pytest.mark.parametrize("lens,R", [([12, 10, 9, 11], 4), ([16, 16, 16, 16], 10), ([14, 9, 11], 3),
                                    ([9, 7, 8, 6, 5], 2), ([16, 12, 10, 9], 40)])
def test_dt_sweeps_match_oracle(pp, ctx, lens, R, schedule):
    V, W = problem(lens, R, 3, "r")
    t, V = bf16_tensor(pp, ctx, V)
    G = O.init_factors(lens, R, 99)
    K = 5
    _, _, W_ref, _ = O.als_cp_dt(V, W, G, tol=0.0, maxiter=K - 1, resprint=1000)
    s = pp.CP(ctx, t, R)
    s.set_schedule(schedule)
    s.set_factors(W, G)
    s.sweeps_dt(K)
    for a, b in zip(s.get_factors(), W_ref):
        assert relerr(a, b) < FTOL, relerr(a, b)
    s.close()
    t.close()


# ---------------------------------------------------------------- drivers: BF16 == F32 of the same values
def both_storages(pp, ctx, lens, R, seed, body):
    """run `body(session)` on BF16 storage and on F32 storage of the same bf16-exact tensor, from
    the same factors; returns the two (result, factors, gradients)"""
    V, W = problem(lens, R, seed, "r")
    V = bf16_round(V)
    G = O.init_factors(lens, R, 97)
    out = []
    for dtype in (BF16, F32):
        t = pp.Tensor(ctx, lens, dtype).upload(V)
        assert same_values(t.download(), V)
        s = pp.CP(ctx, t, R)
        s.set_factors(W, G)
        res = body(s, np.linalg.norm(V))
        Wg, Gg = s.get_factors(with_grad=True)
        out.append((res, Wg, Gg))
        s.close()
        t.close()
    return out


def assert_same_run(out, tol=FTOL):
    (r1, W1, G1), (r2, W2, G2) = out
    assert r1 == r2, (r1, r2)
    for a, b in zip(W1, W2):
        assert relerr(a, b) < tol, relerr(a, b)


def test_run_dt(pp, ctx):
    out = both_storages(pp, ctx, [10, 9, 8, 7], 3, 4,
                        lambda s, Vn: s.run_dt(tol=1e-7 * Vn, maxiter=60, resprint=1000))
    assert_same_run(out)


@pytest.mark.parametrize("lens,R", [([12, 11, 10, 9], 3), ([14, 12, 10], 3), ([7, 6, 6, 5, 5], 2)])
def test_run_pp(pp, ctx, lens, R):
    out = both_storages(pp, ctx, lens, R, 5, lambda s, Vn: s.run_pp(tol=1e-6 * Vn, tol_init=0.1,
                                                                    maxiter=40, resprint=1000))
    assert_same_run(out)


def test_run_pp_partupdate(pp, ctx):
    out = both_storages(pp, ctx, [9, 8, 7, 6], 2, 12,
                        lambda s, Vn: s.run_pp_partupdate(tol=1e-7 * Vn, tol_init=0.1, maxiter=40,
                                                          resprint=1000, update_percentage=0.5))
    assert_same_run(out)


def test_pp_bench_mode(pp, ctx):
    out = both_storages(pp, ctx, [12, 11, 10, 9], 3, 6,
                        lambda s, Vn: (s.run_dt(maxiter=1, bench=1, resprint=1000),
                                       s.run_pp(tol_init=0.05, maxiter=1, bench=1, resprint=1000)))
    assert_same_run(out, tol=1e-4)


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_cpd_als_each_optimizer(pp, ctx, kind):
    out = both_storages(pp, ctx, [12, 10, 8, 6], 5, 7,
                        lambda s, Vn: s.cpd_als(kind, tol=1e-9, maxiter=4, resprint=1000))
    assert_same_run(out)


@pytest.mark.parametrize("kind", [3, 4])
def test_cpd_als_lr(pp, ctx, kind):
    out = both_storages(pp, ctx, [10, 9, 8, 7], 4, 8,
                        lambda s, Vn: s.cpd_als_lr(kind, 2, 0, tol=1e-9 * Vn, maxiter=6, resprint=1000))
    assert_same_run(out, tol=1e-4)


def test_headline_bf16_and_f32_storage_agree(pp, ctx):
    """s = 200, order 4, R = 10, 5 multi-sweep sweeps: the bf16 kernels at full size against the fp32
    ones on the same values (factor entries +-1/2 and +-1: every model value is a multiple of 1/16
    of magnitude at most 10, exact in bf16, so F32 and BF16 storage hold the same tensor)"""
    lens, R = [200, 200, 200, 200], 10
    rng = np.random.default_rng(11)
    Wt = [np.asfortranarray(rng.choice([-1.0, -0.5, 0.5, 1.0], size=(200, R))) for _ in range(4)]
    W0 = O.init_factors(lens, R, 2000)
    G0 = O.init_factors(lens, R, 3000)
    got = []
    for dtype in (BF16, F32):
        t = pp.Tensor(ctx, lens, dtype).fill_cp(Wt)
        s = pp.CP(ctx, t, R)
        s.set_schedule("msdt")
        s.set_factors(W0, G0)
        s.sweeps_dt(5)
        got.append(s.get_factors())
        s.close()
        t.close()
    for a, b in zip(*got):
        assert relerr(a, b) < FTOL, relerr(a, b)


def test_rows_past_32bit_offsets_match_f32_storage(pp, ctx):
    """a scan whose k-block spans >= 2^31 bytes (2^25 rows in front of the contracted mode: the
    64-bit-address form of the bf16 scan, as configs[3] runs it) against F32 storage of the same
    bf16-exact values (factor entries 1/2 and 1: model values are multiples of 1/16 up to 4, and no
    sums with cancellation, so both storages sit within 1e-7 of the exact result)"""
    lens, R = [512, 256, 256, 4], 4
    rng = np.random.default_rng(5)
    Wt = [np.asfortranarray(rng.choice([0.5, 1.0], size=(n, R))) for n in lens]
    W0 = O.init_factors(lens, R, 2000)
    got = []
    for dtype in (BF16, F32):
        t = pp.Tensor(ctx, lens, dtype).fill_cp(Wt)
        s = pp.CP(ctx, t, R)
        s.set_factors(W0)
        # the level-1 PP operator that keeps a, b, c: one scan of 2^25 rows x 4 columns
        got.append((s.pp_operator("abc"), [s.mttkrp(m) for m in range(4)]))
        s.close()
        t.close()
    assert relerr(got[0][0], got[1][0]) < KTOL, relerr(got[0][0], got[1][0])
    for m in range(4):
        assert relerr(got[0][1][m], got[1][1][m]) < KTOL, (m, relerr(got[0][1][m], got[1][1][m]))


# ---------------------------------------------------------------- torch views, P = 2 shards (children)
def run_child(args, timeout, **env):
    e = dict(os.environ, **env)
    e["PYTHONNOUSERSITE"] = "1"
    p = subprocess.run([sys.executable] + args, cwd=ROOT, env=e, capture_output=True, text=True,
                       timeout=timeout)
    assert p.returncode == 0, f"exit {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-6000:]}"
    return p.stdout


@pytest.mark.parametrize("case", ["from_torch", "rounding", "export", "views"])
def test_torch_cases(case):
    out = run_child([os.path.join(HERE, "bf16_torch_cases.py"), case], 300)
    assert f"bf16 case {case}: ok" in out


def test_sharded_p2_matches_unsharded():
    """P = 2 ranks (threads, tests/hipsim's communicator) on the HIP kernels: MTTKRP, DT under both
    schedules and the PP driver match the unsharded oracle on the bf16-rounded tensor"""
    subprocess.check_call(["make", "-s", "-j", "4", "-C", os.path.join(HERE, "hipsim")])
    out = run_child([os.path.join(HERE, "bf16_sharded_rank.py"), "2"], 900, OMP_NUM_THREADS="4",
                    PPALS_ORACLE_THREADS="4")
    assert "all 2 ranks: OK" in out
