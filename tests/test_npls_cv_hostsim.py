"""N-PLS cross-validation and the wide-column passes on the host stand-in (tests/npls_cv_cases.py): the C ABI, the
engine-side code (npls_crossval: the training mask in Y_res, the centring in the scores, no deflation, against the
per-segment reference cv_ref), the group split, the refusals, and the defaults of Ops::npls_contract_wide /
npls_slice_inner_wide in ops.h, through hostsim_util.load() and tests/npls_wide_shim, F64 / F32 storage. A context of
more than one rank is refused through the gloo stand-in communicator."""
import os
import subprocess
import sys

import pytest

import hostsim_util
import npls_cv_cases as CV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = (CV.F64, CV.F32)
NEW = ("ppals_npls_crossval", "ppals_tensor_contract_columns", "ppals_tensor_slice_inner_columns")
WIDE = [(lens, mode, dt) for lens, mode in CV.WIDE_SHAPES for dt in DTYPES]
WIDE_IDS = [f"{CV.DTNAME[dt]}-{i}" for i in CV.WIDE_IDS for dt in DTYPES]


@pytest.fixture(scope="module")
def pp():
    return hostsim_util.load()


@pytest.fixture(scope="module")
def ctx(pp):
    c = pp.Context(0)
    yield c
    c.close()


def test_every_route_has_a_shape():
    for op in CV.OPS:
        assert {CV.wide_route(op, lens, mode, Cn) for lens, mode in CV.WIDE_SHAPES for Cn in CV.WIDE_COLUMNS} == CV.ALL_WIDE_ROUTES, op


def test_binding_exports_the_entry_points(pp):
    import ppals
    for name in NEW:
        assert name in ppals.EXPORTS and hasattr(pp.lib(), name)


@pytest.mark.parametrize("lens,mode,dt", WIDE, ids=WIDE_IDS)
def test_wide_ops(pp, ctx, lens, mode, dt):
    CV.check_wide_ops(pp, ctx, lens, dt, mode)


def test_wide_ops_through_the_shim():
    """the shim's build against the stand-in: the defaults of ops.h on host arrays, guards untouched (no route log)"""
    lib = CV.load_shim(hostsim=True)
    for lens, mode in (([16, 33, 2], 1), ([40, 30], 0)):
        CV.check_wide_routes(lib, lens, mode, CV.F32, logged=False)
    lib.npls_wide_shim_close()


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: CV.DTNAME[d])
@pytest.mark.parametrize("case", CV.CV_CASES + [CV.GROUP_CASE], ids=[c[0] for c in CV.CV_CASES + [CV.GROUP_CASE]])
def test_crossval(pp, ctx, case, dt):
    CV.check_cv(pp, ctx, case, dt)


def test_raw_and_centred_tensor_agree(pp, ctx):
    CV.check_centered_agrees(pp, ctx)


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: CV.DTNAME[d])
def test_segment_with_constant_training_y(pp, ctx, dt):
    CV.check_constant_segment(pp, ctx, dt)


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: CV.DTNAME[d])
def test_cp_session_stays_live(pp, ctx, dt):
    CV.check_cp_session_stays_live(pp, ctx, dt)


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: CV.DTNAME[d])
def test_refusals(pp, ctx, dt):
    CV.check_refusals(pp, ctx, dt)


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
ctx = pp.Context(0)
uid, cbs, calls = hostsim_util.gloo_comm_uid(rank, world)
ctx.init_comm(rank, world, uid)
lens = [8, 5, 4]
t = pp.Tensor(ctx, lens, pp.F64).upload(NC.data(lens))
V0 = t.download()
lib, buf = pp.lib(), np.full(400, -7.0)
seg = (np.arange(5) % 2).astype(np.int32)
p, sp = buf.ctypes.data_as(C.POINTER(C.c_double)), seg.ctypes.data_as(C.POINTER(C.c_int32))
for name, call in (("ppals_npls_crossval", lambda: lib.ppals_npls_crossval(t._h, 1, p, 1, 1, sp, 2, 1, None, p, None, None, None, None)),
                   ("ppals_tensor_contract_columns", lambda: lib.ppals_tensor_contract_columns(t._h, 1, p, 1, p)),
                   ("ppals_tensor_slice_inner_columns", lambda: lib.ppals_tensor_slice_inner_columns(t._h, 1, p, 1, p))):
    rc = call()
    assert rc == NC.ERR_UNSUPPORTED, (name, rc)
    assert lib.ppals_last_error().decode().startswith(name + ": "), lib.ppals_last_error()
    assert np.all(buf == -7.0)
assert NC.bits(t.download()) == NC.bits(V0)
t.close()
ctx.close()
dist.barrier()
print("RANK_OK", rank)
"""


def test_more_than_one_rank_is_refused(tmp_path):
    import socket
    hostsim_util.load()  # (built once, before the ranks start)
    script = tmp_path / "npls_cv_rank.py"
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
