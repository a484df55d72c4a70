"""bench.py's own N > 1 code path on the CPU: the process group, the communicator-id hand-over,
init_comm, measure() with its barrier / max-over-ranks, and (`--full`) the sub-records — two ranks
over gloo and the engine's host stand-in (PPALS_BENCH_BACKEND=hostsim). What the driver's 8-GPU run
executes for the first time on hardware is executed here first (TEST INFRASTRUCTURE: the numbers
mean nothing)."""
import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("world", [2, 3, 8])
def test_bench_multi_rank_path_on_the_host_stand_in(world, tmp_path):
    import hostsim_util
    hostsim_util.load()  # build once, before the ranks race for it
    port = free_port()
    procs = []
    workload = "cp4_s12_r3" if world < 8 else "cp4_s16_r3"   # (8 ranks: 2 rows of the leading mode each)
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OMP_NUM_THREADS="2" if world < 8 else "1",
                   PPALS_BENCH_BACKEND="hostsim")
        procs.append(subprocess.Popen(
            [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(world), "--steps", "3",
             "--warmup", "1", "--workload", workload, "--dtype", "f64", "--full", "--no-cpu-baseline",
             "--dump-outputs", str(tmp_path / "multi")],
            env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=300))
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    for r, (p, (out, err)) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {r} failed:\n{out[-2000:]}\n{err[-3000:]}"
    lines = [ln for ln in outs[0][0].splitlines() if ln.startswith("{")]
    assert len(lines) == 1, outs[0][0]
    assert not any(ln.startswith("{") for o, _ in outs[1:] for ln in o.splitlines())  # rank 0 only
    d = json.loads(lines[0])
    assert d["n_gpus"] == world and d["rccl_ranks"] == world and d["steps"] == 3 and d["warmup"] == 1
    assert d["scaling"] == "strong" and d["value"] > 0 and d["ms_per_step"] > 0
    assert "REHEARSAL" in d["data"]
    assert f"x{world}" in d["config"]["sharding"]
    rs = d["sub_records"]["reduce_scatter_plan"]
    assert rs["value"] > 0 and "reduce-scatter" in rs["comm_plan"]
    # the N > 1 line carries BASELINE configs[3] and the N-GPU leg of configs[4] (shrunken here)
    c4 = d["sub_records"]["cfg4_sharded"]
    assert "error" not in c4, c4
    assert c4["rccl_ranks"] == world
    for plan in ("allreduce_plan", "reduce_scatter_plan"):
        assert c4[plan]["steps"] == 5 and c4[plan]["value"] > 0 and c4[plan]["ms_per_step"] > 0
    g = [c4[p_]["final_gradnorm"] for p_ in ("allreduce_plan", "reduce_scatter_plan")]
    assert abs(g[0] - g[1]) < 1e-8 * abs(g[0])       # same iterates on both collective plans
    c5 = d["sub_records"]["cfg5_tucker_sharded"]
    assert "error" not in c5, c5
    assert c5["rccl_ranks"] == world and c5["hosvd_ms"] > 0 and c5["ms_per_hooi_sweep"] > 0
    # the same ALS iterates on every shard plan: the run ends at the same gradient norm as one rank
    env = dict(os.environ, PPALS_BENCH_BACKEND="hostsim", OMP_NUM_THREADS="2")
    env.pop("RANK", None), env.pop("WORLD_SIZE", None)
    one = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3",
                          "--warmup", "1", "--workload", workload, "--dtype", "f64",
                          "--no-cpu-baseline", "--no-config-records", "--dump-outputs", str(tmp_path / "one")],
                         env=env, capture_output=True,
                         text=True, timeout=300)
    assert one.returncode == 0, one.stderr[-3000:]
    d1 = json.loads([ln for ln in one.stdout.splitlines() if ln.startswith("{")][0])
    assert abs(d1["final_gradnorm"] - d["final_gradnorm"]) < 1e-8 * d1["final_gradnorm"]
    assert abs(d1["final_rel_residual"] - d["final_rel_residual"]) < 1e-9
    # --dump-outputs: the sharded run hands back the same full factors and gradients as one rank
    import numpy as np
    names = sorted(os.listdir(tmp_path / "one"))
    assert len(names) == 10 and sorted(os.listdir(tmp_path / "multi")) == names
    for n in names:
        a, b = np.load(tmp_path / "multi" / n), np.load(tmp_path / "one" / n)
        assert a.shape == b.shape and np.linalg.norm(a - b) <= 1e-9 * np.linalg.norm(b), n


def _bench_dump(out_dir, steps, warmup, flags=("--no-cpu-baseline", "--no-config-records")):
    env = dict(os.environ, PPALS_BENCH_BACKEND="hostsim", OMP_NUM_THREADS="2")
    env.pop("RANK", None), env.pop("WORLD_SIZE", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", str(warmup), "--workload", "cp4_s12_r3", "--dtype", "f64",
                        *flags, "--dump-outputs", str(out_dir)],
                       env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_bench_plain_run_is_the_headline_alone(tmp_path):
    """a plain run measures the headline and nothing beside it; --full adds the sub-records and leaves
    the headline's iterates and dumped outputs as they are"""
    import numpy as np
    import hostsim_util
    hostsim_util.load()
    plain = _bench_dump(tmp_path / "plain", 3, 1, flags=())
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in plain, key
    assert plain["steps"] == 3 and plain["warmup"] == 1 and plain["value"] > 0
    assert "sub_records" not in plain and "cpu_baseline" not in plain
    full = _bench_dump(tmp_path / "full", 3, 1, flags=("--full", "--no-cpu-baseline"))
    assert full["sub_records"]["dt_schedule_f64"]["value"] > 0 and "cold" in full["sub_records"]
    assert full["final_gradnorm"] == plain["final_gradnorm"]
    assert full["final_rel_residual"] == plain["final_rel_residual"]
    names = sorted(os.listdir(tmp_path / "plain"))
    assert len(names) == 10 and sorted(os.listdir(tmp_path / "full")) == names
    for n in names:
        assert np.array_equal(np.load(tmp_path / "full" / n), np.load(tmp_path / "plain" / n)), n


def test_bench_dump_outputs_are_the_timed_sweeps(tmp_path):
    """--dump-outputs DIR: the factors, gradients, gradient norm and residual after exactly
    warmup + steps sweeps from the seeded start (the fp64 oracle's iterates), the same on every run;
    --steps is the number of timed sweeps and ms_per_step the time of one"""
    import numpy as np
    import oracle_lib as O
    import hostsim_util
    hostsim_util.load()
    lens, R, steps, warmup = [12, 12, 12, 12], 3, 3, 1
    d = _bench_dump(tmp_path / "a", steps, warmup)
    assert d["steps"] == steps and d["warmup"] == warmup and d["ms_per_step"] > 0
    assert abs(d["ms_per_step"] * d["value"] - 1e3) < 1e-6 * 1e3
    names = sorted(f.name for f in (tmp_path / "a").iterdir())
    assert names == sorted([f"W{i}.npy" for i in range(4)] + [f"gradW{i}.npy" for i in range(4)]
                           + ["gradnorm.npy", "residual.npy"])
    got = {n[:-4]: np.load(tmp_path / "a" / n) for n in names}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    V = O.build_V(O.init_factors(lens, R, 1000))
    _, _, W_ref, G_ref = O.als_cp_dt(V, O.init_factors(lens, R, 2000), O.init_factors(lens, R, 3000),
                                     tol=0.0, maxiter=warmup + steps - 1, resprint=10 ** 9)
    for i in range(4):
        assert got[f"W{i}"].shape == (lens[i], R)
        assert np.linalg.norm(got[f"W{i}"] - W_ref[i]) < 1e-9 * np.linalg.norm(W_ref[i])
        assert np.linalg.norm(got[f"gradW{i}"] - G_ref[i]) < 1e-9 * np.linalg.norm(G_ref[i])
    assert abs(float(got["gradnorm"]) - d["final_gradnorm"]) <= 1e-12 * d["final_gradnorm"]
    assert abs(float(got["residual"]) - O.residual(V, W_ref)) < 1e-9 * np.linalg.norm(V)
    # the same arguments give the same outputs
    _bench_dump(tmp_path / "b", steps, warmup)
    for n in names:
        assert np.array_equal(np.load(tmp_path / "b" / n), got[n[:-4]]), n
