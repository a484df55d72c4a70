"""The CP normal equations with lambda != 0 and with an indefinite S, on every route the engine has
for S^-1 and for the mode update, against the fp64 oracle (run with -m gpu on an MI355X).

Every mode update solves W = M S^-1 with S = Hadamard_{j != mode}(W_j^T W_j) + lambda I. The
reference's S^-1 is the untruncated SVD inverse V diag(1/s) U^T (common.cxx:710-725,
O.svd_solve), whatever the signs of S's eigenvalues. Which kernels form it depends on R:

  R <= 64     one-wave Gauss-Jordan; two-sided Jacobi when a pivot is not positive
              (PPALS_FORCE_JACOBI=1 forces it)
  65 .. 128   block Gauss-Jordan on the matrix cores (PPALS_GJ_SCALAR=1: scalar sweeps in LDS);
              when a pivot is not positive, the conditional one-sided Jacobi + V Sigma^-2 W^T
              (PPALS_FORCE_EIGINV=2 runs it ungated, =1 takes dsyevd after a host read-back)
  129 .. 137  scalar sweeps in LDS, dsyevd when a pivot is not positive
  >= 138      sweeps out of global memory, dsyevd when a pivot is not positive

The direct solves use an order-3 problem whose mode-0 system has a spectrum chosen by the test:
W_2 = ones / sqrt(rows) makes G_2 = 1 1^T, and W_1 = U diag(sqrt(d)) Q^T with orthonormal U makes
H = G_1 o G_2 = Q diag(d) Q^T, so S = Q diag(d + lambda) Q^T. The environment switches are read when
a context is created: a fresh context per setting."""
import numpy as np
import pytest

import numpy_ref as NR
import oracle_lib as O

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


def relerr(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


# ------------------------------------------------------------------------------------------------
# direct solves: CP.gram_system(0, lam)

# spd: lambda = +0.125, d over 1 .. 1e3; one_negative: lambda < 0 turns one eigenvalue negative,
# cond <= 8; pm_pairs: lambda = -1 leaves half the spectrum negative, in +/- pairs of equal
# magnitude (singular vectors that are not eigenvectors); gap: O.init_factors, lambda = minus the
# midpoint of the widest gap in H's spectrum
SOLVE_CASES = ["spd", "one_negative", "pm_pairs", "gap"]


def crafted_system(R, case):
    """(lens, W, lam, S_want, cond) with the spectrum `case` asks for; asserts its own inertia"""
    rows1 = R + 3
    lens = [5, rows1, 6]
    if case == "gap":
        W = O.init_factors(lens, R, 17)
        e = np.linalg.eigvalsh(O.gram_hadamard(W, 0))
        if R == 1:
            lam, neg = -2.0 * e[0], 1
        else:
            k = int(np.argmax(np.diff(e)))
            lam, neg = -0.5 * (e[k] + e[k + 1]), k + 1
    else:
        rng = np.random.default_rng(1000 + R)
        Q, _ = np.linalg.qr(rng.standard_normal((R, R)))
        U, _ = np.linalg.qr(rng.standard_normal((rows1, R)))
        if case == "spd":
            d, lam, neg = np.logspace(0.0, 3.0, R), 0.125, 0
        elif case == "one_negative":
            d, lam, neg = np.concatenate([[1.0], np.linspace(3.0, 10.0, R - 1)]), -2.0, 1
        else:
            m = np.linspace(0.3, 0.9, R // 2)
            d, lam, neg = np.concatenate([1.0 + m, 1.0 - m, [1.5] * (R % 2)]), -1.0, R // 2
        W1 = (U * np.sqrt(d)) @ Q.T
        W = [O.init_factors(lens, R, 5)[0], np.asfortranarray(W1),
             np.full((lens[2], R), 1.0 / np.sqrt(lens[2]), order="F")]
    S_want = O.gram_hadamard(W, 0, lam)
    e = np.linalg.eigvalsh(S_want)
    assert np.sum(e < 0) == neg, (case, R, e)
    cond = np.max(np.abs(e)) / np.min(np.abs(e))
    assert cond <= 1e5, (case, R, cond)
    return lens, W, lam, S_want, cond


def check_solve(pp, c, R, case):
    lens, W, lam, S_want, cond = crafted_system(R, case)
    t = pp.Tensor(c, lens, 1)   # (the Grams alone: the tensor stays unfilled)
    s = pp.CP(c, t, R)
    s.set_factors(W)
    S, Si = s.gram_system(0, lam)
    s.close()
    t.close()
    assert np.all(np.isfinite(S)) and np.all(np.isfinite(Si))
    assert relerr(S, S_want) < 1e-13
    e_inv = relerr(Si, O.svd_solve(np.eye(R), S_want))
    e_id = relerr(Si @ S_want, np.eye(R))
    assert e_inv < 1e-10 * cond, (case, R, e_inv, cond)
    assert e_id < 1e-10 * cond, (case, R, e_id, cond)
    assert relerr(Si, Si.T) < 1e-13


# the odd sizes give the Jacobi tournaments a bye; 64 / 65, 128 / 129, 137 / 138 straddle the routes
SOLVE_R = [1, 3, 33, 63, 64, 65, 100, 127, 128, 129, 137, 138, 150]


@pytest.mark.parametrize("case", SOLVE_CASES)
@pytest.mark.parametrize("R", SOLVE_R)
def test_gram_system_lambda_and_indefinite(pp, ctx, R, case):
    """S and S^-1 with lambda != 0, definite or not, on the default route for R"""
    check_solve(pp, ctx, R, case)


def _switches():
    out = []
    for R in (1, 3, 33, 63, 64):
        out.append((R, "PPALS_FORCE_JACOBI=1"))
    for R in (65, 100, 127, 128):
        out += [(R, "PPALS_GJ_SCALAR=1"), (R, "PPALS_FORCE_EIGINV=2"), (R, "PPALS_FORCE_EIGINV=1"),
                (R, "PPALS_GJ_SCALAR=1,PPALS_FORCE_EIGINV=2")]
    for R in (129, 137, 138, 150):
        out.append((R, "PPALS_FORCE_EIGINV=1"))
    return out


def _context(pp, env, monkeypatch):
    for kv in env.split(","):
        k, v = kv.split("=")
        monkeypatch.setenv(k, v)
    return pp.Context(0)


@pytest.mark.parametrize("case", SOLVE_CASES)
@pytest.mark.parametrize("R,env", _switches())
def test_gram_system_lambda_and_indefinite_switched(pp, R, env, case, monkeypatch):
    """the same on the routes the environment switches select (forced fallbacks, scalar sweeps)"""
    c = _context(pp, env, monkeypatch)
    try:
        check_solve(pp, c, R, case)
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------
# mode updates: sweeps_dt(K, lam) against O.als_cp_dt(..., lam=lam), fp64 storage

# name: (lens, R, environment). The routes of HipOps::cp_mode_update / cp_mode_update_blocked:
SWEEP_ROUTES = {
    "small": ([12, 10, 9, 11], 4, ""),          # msdt: S, S^-1 prepared beside the contraction
    "staged": ([48, 40, 36], 40, ""),           # 33..64: fused, M and W staged in LDS
    "unstaged": ([96, 70, 66], 64, ""),         # fused, the stage does not fit, rows x R <= 6144
    "long_mode": ([3, 10, 12, 1800], 10, ""),   # the stage does not fit, rows x R > 6144: row-parallel
    "above_64": ([80, 75, 72], 70, ""),         # unfused, S^-1 by block Gauss-Jordan (+ fallback)
    "above_137": ([141, 24, 22], 140, ""),      # unfused, S^-1 out of global memory (+ dsyevd)
    "blocked": ([12, 10, 8, 12], 4, "PPALS_TEST_BLOCKED_UPDATE=2"),
    "force_jacobi": ([12, 10, 9, 11], 4, "PPALS_FORCE_JACOBI=1"),
    "above_64_eiginv": ([80, 75, 72], 70, "PPALS_FORCE_EIGINV=2"),
}
PLAIN_ROUTES = [k for k, v in SWEEP_ROUTES.items() if not v[2]]
SWITCHED_ROUTES = [k for k, v in SWEEP_ROUTES.items() if v[2]]


def sweep_problem(lens, R):
    V = O.build_V(O.init_factors(lens, R, 1100))
    return V, O.init_factors(lens, R, 2100), O.init_factors(lens, R, 99)


def replay_systems(V, W, lam):
    """one exact sweep in numpy (numpy_ref's own steps): the S of every mode update"""
    W, Ss = [w.copy() for w in W], []
    for i in range(V.ndim):
        M = NR._mttkrp(V, W, i)
        S = NR._S(W, i, lam)
        Ss.append(S)
        W[i] = M @ NR._svd_inverse(S)
    return Ss


def negative_lambda(V, W):
    """a lambda < 0 inside a gap of mode 0's spectrum (S indefinite there) that keeps every mode's S
    of the sweep away from singular: the best of the five widest gaps"""
    e = np.linalg.eigvalsh(O.gram_hadamard(W, 0))
    if len(e) == 1:
        cands = [-2.0 * e[0]]
    else:
        gaps = np.argsort(np.diff(e))[::-1][:5]
        cands = [-0.5 * (e[k] + e[k + 1]) for k in gaps]

    def worst(lam):
        return min(np.min(np.abs(ev)) / np.max(np.abs(ev))
                   for ev in (np.linalg.eigvalsh(S) for S in replay_systems(V, W, lam)))
    return max(cands, key=worst)


def sweeps_case(pp, c, route, schedule, sign):
    lens, R, _ = SWEEP_ROUTES[route]
    V, W, G = sweep_problem(lens, R)
    if sign > 0:
        K = 3
        lam = 0.05 * np.trace(O.gram_hadamard(W, 0)) / R
        _, _, W_ref, _ = O.als_cp_dt(V, W, G, tol=0.0, maxiter=K - 1, lam=lam, resprint=1000)
        kappa = max(np.linalg.cond(O.gram_hadamard(W_ref, i, lam)) for i in range(len(lens)))
    else:
        K = 1
        lam = negative_lambda(V, W)
        Ss = replay_systems(V, W, lam)
        ev = [np.linalg.eigvalsh(S) for S in Ss]
        assert np.min(ev[0]) < 0 < np.max(ev[0]), ev[0]          # mode 0's S is indefinite
        ratio = min(np.min(np.abs(x)) / np.max(np.abs(x)) for x in ev)
        assert ratio >= 1e-6, ratio
        kappa = 1.0 / ratio
        _, _, W_ref, _ = O.als_cp_dt(V, W, G, tol=0.0, maxiter=K - 1, lam=lam, resprint=1000)
    bar = 1e-11 * kappa * K
    # the oracle's factors at lambda and at 0 must differ by far more than the bar: a route that
    # dropped lambda fails
    _, _, W_0, _ = O.als_cp_dt(V, W, G, tol=0.0, maxiter=K - 1, resprint=1000)
    assert max(relerr(a, b) for a, b in zip(W_ref, W_0)) > 100 * bar, (lam, kappa)
    t = pp.Tensor(c, lens, 1).upload(V)
    s = pp.CP(c, t, R)
    s.set_schedule(schedule)
    s.set_factors(W, G)
    s.sweeps_dt(K, lam)
    W_got = s.get_factors()
    s.close()
    t.close()
    for i, (a, b) in enumerate(zip(W_got, W_ref)):
        assert np.all(np.isfinite(a))
        assert relerr(a, b) < bar, (route, schedule, lam, i, relerr(a, b), bar, kappa)


@pytest.mark.parametrize("sign", [1, -1])
@pytest.mark.parametrize("schedule", ["msdt", "dt"])
@pytest.mark.parametrize("route", PLAIN_ROUTES)
def test_sweeps_with_lambda(pp, ctx, route, schedule, sign):
    """K exact sweeps with lambda > 0, one with lambda < 0 (S indefinite), on every mode-update
    route and both schedules"""
    sweeps_case(pp, ctx, route, schedule, sign)


@pytest.mark.parametrize("sign", [1, -1])
@pytest.mark.parametrize("schedule", ["msdt", "dt"])
@pytest.mark.parametrize("route", SWITCHED_ROUTES)
def test_sweeps_with_lambda_switched(pp, route, schedule, sign, monkeypatch):
    c = _context(pp, SWEEP_ROUTES[route][2], monkeypatch)
    try:
        sweeps_case(pp, c, route, schedule, sign)
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------
# drivers with lambda > 0 against the oracle's drivers with the same lambda (fp64 storage)

DRIVER_LAM = 0.5


def driver_problem(lens, R, seed):
    V = O.build_V(O.init_factors(lens, R, 1000 + seed))
    return V, O.init_factors(lens, R, 2000 + seed), O.init_factors(lens, R, 3000 + seed)


def compare_rows(r1, r2, vn, rtol):
    assert len(r1) == len(r2), (len(r1), len(r2))
    for a, b in zip(r1, r2):
        assert a[0] == b[0] and a[1] == b[1] and a[4] == b[4], (a, b)
        assert abs(a[2] - b[2]) <= rtol * abs(a[2]) + 1e-9 * vn, (a, b)
        assert abs(a[5] - b[5]) <= rtol * abs(a[5]) + 1e-9 * vn, (a, b)


def lambda_matters(ref_fn):
    W_l, W_0 = ref_fn(DRIVER_LAM), ref_fn(0.0)
    assert max(relerr(a, b) for a, b in zip(W_l, W_0)) > 1e-3


@pytest.mark.parametrize("driver", ["dt", "pp", "pp_partupdate"])
def test_drivers_with_lambda(pp, ctx, driver, tmp_path):
    """alsCP_DT, alsCP_PP and alsCP_PP_partupdate with lambda > 0: iteration count, CSV rows and
    final factors as the oracle's with the same lambda"""
    lens, R = [10, 9, 8, 7], 3
    V, W, G = driver_problem(lens, R, 21)
    vn = np.linalg.norm(V)
    c_ref, c_got = str(tmp_path / "ref.csv"), str(tmp_path / "got.csv")
    if driver == "dt":
        kw = dict(tol=1e-7 * vn, maxiter=40, resprint=5)
        ref = lambda lam, csv=None: O.als_cp_dt(V, W, G, lam=lam, csv=csv, **kw)
    elif driver == "pp":
        kw = dict(tol=1e-7 * vn, tol_init=0.1, maxiter=40, resprint=1)
        ref = lambda lam, csv=None: O.als_cp_pp(V, W, G, lam=lam, csv=csv, **kw)
    else:
        kw = dict(tol=1e-7 * vn, tol_init=0.1, maxiter=40, resprint=1, update_percentage=0.5)
        ref = lambda lam, csv=None: O.als_cp_pp_partupdate(V, W, G, lam=lam, csv=csv, **kw)
    lambda_matters(lambda lam: ref(lam)[2])
    rc_ref, it_ref, W_ref, _ = ref(DRIVER_LAM, c_ref)
    t = pp.Tensor(ctx, lens, 1).upload(V)
    s = pp.CP(ctx, t, R)
    s.set_factors(W, G)
    run = {"dt": s.run_dt, "pp": s.run_pp, "pp_partupdate": s.run_pp_partupdate}[driver]
    rc, it = run(lam=DRIVER_LAM, csv=c_got, **kw)
    W_got = s.get_factors()
    s.close()
    t.close()
    assert (bool(rc), it) == (bool(rc_ref), it_ref)
    h1, r1 = O.read_csv(c_ref)
    h2, r2 = O.read_csv(c_got)
    assert h1 == h2
    if driver != "dt":
        assert any(r[4] == 1 for r in r2), "PP phase never entered"
    compare_rows(r1, r2, vn, 1e-5)
    for a, b in zip(W_got, W_ref):
        assert relerr(a, b) < 1e-6, relerr(a, b)


@pytest.mark.parametrize("kind", [1, 2, 3, 4])
def test_class_api_with_lambda(pp, ctx, kind, tmp_path):
    """CPD::als (DT and MSDT optimizers) and the low-rank optimizers with lambda > 0"""
    lens, R = [8, 7, 6, 5], 3
    V, W, G = driver_problem(lens, R, 22)
    vn = np.linalg.norm(V)
    c_ref, c_got = str(tmp_path / "ref.csv"), str(tmp_path / "got.csv")
    kw = dict(tol=1e-9 * vn, resprint=1)
    if kind <= 2:
        ref = lambda lam, csv=None: O.cpd_als(V, W, G, kind, maxsweep=8, lam=lam, csv=csv, **kw)
    else:
        ref = lambda lam, csv=None: O.cpd_als_lr(V, W, G, kind, 2, maxsweep=8, lam=lam, csv=csv, **kw)
    lambda_matters(lambda lam: ref(lam)[3])
    rc_ref, sw_ref, it_ref, W_ref, _ = ref(DRIVER_LAM, c_ref)
    t = pp.Tensor(ctx, lens, 1).upload(V)
    s = pp.CP(ctx, t, R)
    s.set_factors(W, G)
    if kind <= 2:
        rc, sw, it = s.cpd_als(kind, maxiter=8, lam=DRIVER_LAM, csv=c_got, **kw)
    else:
        rc, sw, it = s.cpd_als_lr(kind, 2, maxiter=8, lam=DRIVER_LAM, csv=c_got, **kw)
    W_got = s.get_factors()
    s.close()
    t.close()
    assert (rc, it) == (rc_ref, it_ref) and abs(sw - sw_ref) < 1e-12
    _, r1 = O.read_csv(c_ref)
    _, r2 = O.read_csv(c_got)
    compare_rows(r1, r2, vn, 1e-5)
    for a, b in zip(W_got, W_ref):
        assert relerr(a, b) < 1e-7, relerr(a, b)
