"""Centring and scaling in place on the host stand-in (tests/preprocess_cases.py): the C ABI, the engine-side code
(tensor_center and the rest, the generation bump, the refusals) and the fp64 host twins of the four device ops in
ops.h, through hostsim_util.load(), F64 / F32 storage, host offsets. A back end without device views answers
PPALS_DEVICE with PPALS_ERR_UNSUPPORTED; a context of more than one rank is refused through the gloo stand-in
communicator."""
import os
import subprocess
import sys

import numpy as np
import pytest

import hostsim_util
import preprocess_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = (PC.F64, PC.F32)
CASES = [(lens, dt, mode) for lens, dt in PC.cases(DTYPES) for mode in range(len(lens))]
IDS = [f"{PC.DTNAME[dt]}-{'x'.join(map(str, lens))}-m{mode}" for lens, dt, mode in CASES]


@pytest.fixture(scope="module")
def pp():
    return hostsim_util.load()


@pytest.fixture(scope="module")
def ctx(pp):
    c = pp.Context(0)
    yield c
    c.close()


def test_every_route_has_a_shape():
    assert set(PC.ROUTES.values()) == PC.ALL_ROUTES
    for lens, dt in PC.cases((PC.F32, PC.F64, PC.BF16)):
        for mode in range(len(lens)):
            assert PC.ROUTES[(PC.DTNAME[dt], tuple(lens), mode)] == PC.route(dt, lens, mode)


@pytest.mark.parametrize("lens,dt,mode", CASES, ids=IDS)
def test_center_and_shift(pp, ctx, lens, dt, mode):
    V0, centred, off = PC.check_center_host(pp, ctx, lens, dt, mode)
    PC.check_shift(pp, ctx, lens, dt, mode, V0, centred, off)


@pytest.mark.parametrize("lens,dt,mode", CASES, ids=IDS)
def test_sumsq_scale_rescale(pp, ctx, lens, dt, mode):
    PC.check_scale(pp, ctx, lens, dt, mode)


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: PC.DTNAME[d])
@pytest.mark.parametrize("lens,a,b", [([7, 6, 5], 0, 1), ([7, 6, 5], 2, 0), ([33, 20, 12], 1, 2), ([40, 30], 1, 0)])
def test_centring_survives_scaling(pp, ctx, lens, a, b, dt):
    PC.check_property(pp, ctx, lens, dt, a, b)


def test_planted_offsets(pp, ctx):
    PC.check_planted(pp, ctx)


@pytest.mark.parametrize("schedule", ["dt", "msdt"])
@pytest.mark.parametrize("lens,dt,R", [([16, 16, 16, 16], PC.F32, 10), ([12, 10, 9], PC.F64, 3)])
def test_cp_session_sees_the_new_contents(pp, ctx, lens, dt, R, schedule):
    V = np.asfortranarray(0.5 + np.random.default_rng(3).random(lens))
    PC.check_cp_session(pp, ctx, lens, dt, R, schedule, V)


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: PC.DTNAME[d])
def test_tucker_session_sees_the_new_contents(pp, ctx, dt):
    lens = [12, 10, 9]
    PC.check_tucker_session(pp, ctx, lens, dt, [3, 3, 3], np.asfortranarray(0.5 + np.random.default_rng(4).random(lens)))


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: PC.DTNAME[d])
def test_refusals(pp, ctx, dt):
    host = np.zeros(9 * 8 * 7)
    PC.check_refusals(pp, ctx, dt, device_cases=[("device offsets", host.ctypes.data, PC.ERR_UNSUPPORTED)])


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: PC.DTNAME[d])
def test_preprocess_record(pp, ctx, dt):
    PC.check_preprocess(pp, ctx, dt)


_RANK = r"""
import os, sys
import numpy as np
import torch.distributed as dist
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import hostsim_util
import preprocess_cases as PC
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
pp = hostsim_util.load()
ctx = pp.Context(0)
uid, cbs, calls = hostsim_util.gloo_comm_uid(rank, world)
ctx.init_comm(rank, world, uid)
lens = [8, 5, 4]
t = pp.Tensor(ctx, lens, pp.F64).upload(PC.data(lens))
V0 = t.download()
lib, buf = pp.lib(), np.zeros(200)
import ctypes as C
p = buf.ctypes.data_as(C.POINTER(C.c_double))
for name, call in (("ppals_tensor_center", lambda: lib.ppals_tensor_center(t._h, 1, p, 0, None)),
                   ("ppals_tensor_center", lambda: lib.ppals_tensor_center(t._h, 1, None, 0, None)),
                   ("ppals_tensor_shift", lambda: lib.ppals_tensor_shift(t._h, 1, p, 0, C.c_double(1.0), None)),
                   ("ppals_tensor_slice_sumsq", lambda: lib.ppals_tensor_slice_sumsq(t._h, 1, p)),
                   ("ppals_tensor_scale", lambda: lib.ppals_tensor_scale(t._h, 1, p)),
                   ("ppals_tensor_rescale", lambda: lib.ppals_tensor_rescale(t._h, 1, p))):
    rc = call()
    assert rc == PC.ERR_UNSUPPORTED, (name, rc)
    assert lib.ppals_last_error().decode().startswith(name + ": "), lib.ppals_last_error()
assert PC.bits(t.download()) == PC.bits(V0)
t.close()
ctx.close()
dist.barrier()
print("RANK_OK", rank)
"""


def test_more_than_one_rank_is_refused(tmp_path):
    import socket
    hostsim_util.load()  # (built once, before the ranks start)
    script = tmp_path / "prep_rank.py"
    script.write_text(_RANK)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([sys.executable, str(script), ROOT], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=120)[0] for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and f"RANK_OK {r}" in o, o
