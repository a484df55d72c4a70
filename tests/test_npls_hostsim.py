"""N-PLS regression on the host stand-in (tests/npls_cases.py): the C ABI, the engine-side code (npls_fit / npls_predict:
the formulation that never deflates, against the deflating reference of tests/npls_ref.py), the refusals, and the fp64
host twins of the four device ops in ops.h, through hostsim_util.load(), F64 / F32 storage. A context of more than
one rank is refused through the gloo stand-in communicator."""
import os
import subprocess
import sys

import pytest

import hostsim_util
import npls_cases as NC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = (NC.F64, NC.F32)
OPS = [(lens, dt, mode) for lens in NC.SHAPES for dt in DTYPES for mode in range(len(lens))]
OPS_IDS = [f"{NC.DTNAME[dt]}-{'x'.join(map(str, lens))}-m{mode}" for lens, dt, mode in OPS]


@pytest.fixture(scope="module")
def pp():
    return hostsim_util.load()


@pytest.fixture(scope="module")
def ctx(pp):
    c = pp.Context(0)
    yield c
    c.close()


def test_every_route_has_a_shape():
    for dt in (NC.F32, NC.F64, NC.BF16):
        for op, routes in NC.ALL_ROUTES.items():
            assert NC.routes_by_dtype(op, dt) == routes, (op, NC.DTNAME[dt])


def test_binding_exports_the_entry_points(pp):
    import ppals
    for name in ("ppals_npls_fit", "ppals_npls_destroy", "ppals_npls_dims", "ppals_npls_get", "ppals_npls_predict",
                 "ppals_tensor_contract_mode", "ppals_tensor_slice_inner"):
        assert name in ppals.EXPORTS and hasattr(pp.lib(), name)


@pytest.mark.parametrize("lens,dt,mode", OPS, ids=OPS_IDS)
def test_contract_and_slice_inner(pp, ctx, lens, dt, mode):
    NC.check_ops(pp, ctx, lens, dt, mode)


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: NC.DTNAME[d])
@pytest.mark.parametrize("case", NC.FIT_CASES, ids=[c[0] for c in NC.FIT_CASES])
def test_fit_and_predict(pp, ctx, case, dt):
    NC.check_fit(pp, ctx, case, dt)


def test_fit_ends_where_nothing_is_left(pp, ctx):
    NC.check_ends_early(pp, ctx, NC.F64)


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: NC.DTNAME[d])
def test_cp_session_stays_live(pp, ctx, dt):
    NC.check_cp_session_stays_live(pp, ctx, dt)


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: NC.DTNAME[d])
def test_refusals(pp, ctx, dt):
    NC.check_refusals(pp, ctx, dt)


_RANK = r"""
import os, sys
import ctypes as C
import numpy as np
import torch.distributed as dist
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import hostsim_util
import npls_cases as NC
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
pp = hostsim_util.load()
one = pp.Context(0)
t1 = pp.Tensor(one, [8, 5, 4], pp.F64).upload(NC.data([8, 5, 4]))
model = pp.NPLS().fit(t1, np.arange(5.0) - 2.0, 1, 1)
ctx = pp.Context(0)
uid, cbs, calls = hostsim_util.gloo_comm_uid(rank, world)
ctx.init_comm(rank, world, uid)
lens = [8, 5, 4]
t = pp.Tensor(ctx, lens, pp.F64).upload(NC.data(lens))
V0 = t.download()
lib, buf, out = pp.lib(), np.zeros(400), C.c_void_p()
p = buf.ctypes.data_as(C.POINTER(C.c_double))
for name, call in (("ppals_npls_fit", lambda: lib.ppals_npls_fit(t._h, 1, p, 1, 1, None, C.byref(out))),
                   ("ppals_npls_predict", lambda: lib.ppals_npls_predict(model._h, t._h, 1, p, None)),
                   ("ppals_tensor_contract_mode", lambda: lib.ppals_tensor_contract_mode(t._h, 1, p, 1, p)),
                   ("ppals_tensor_slice_inner", lambda: lib.ppals_tensor_slice_inner(t._h, 1, p, 1, p))):
    rc = call()
    assert rc == NC.ERR_UNSUPPORTED, (name, rc)
    assert lib.ppals_last_error().decode().startswith(name + ": "), lib.ppals_last_error()
    assert not out.value
assert NC.bits(t.download()) == NC.bits(V0)
t.close()
ctx.close()
dist.barrier()
print("RANK_OK", rank)
"""


def test_more_than_one_rank_is_refused(tmp_path):
    import socket
    hostsim_util.load()  # (built once, before the ranks start)
    script = tmp_path / "npls_rank.py"
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
