"""bf16 tensor storage (PPALS_BF16) on a CPU-only box.

* csrc/bf16.h (the host half of the rounding and the three-piece split), built with g++ under ASan +
  UBSan: the rounding of fp64 values is torch's CPU float64 -> bfloat16 cast bit for bit, and
  hi + mid + lo reproduces an fp64 value to 2^-24 relative.
* The numpy restatement the GPU tests use (tests/bf16_util.py) agrees with torch too.
* The host stand-in cannot hold a bf16 tensor: ppals_tensor_create refuses it with
  PPALS_ERR_UNSUPPORTED.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import bf16_util
import hostsim_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pairwise-perturbation_amd", "csrc")

DRIVER = r"""
#include <cstdio>
#include <cstring>
#include "bf16.h"
using namespace ppals;

int main(int argc, char **argv) {
  // stdin: raw fp64 values; stdout: per value the rounded bits and the three split pieces
  double x;
  while (std::fread(&x, 8, 1, stdin) == 1) {
    uint16_t r[4];
    r[0] = bf16s(x).u;
    bf16_split3(x, &r[1], &r[2], &r[3]);
    double back = (double)bf16s(x);
    std::fwrite(r, 2, 4, stdout);
    std::fwrite(&back, 8, 1, stdout);
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("bf16")
    src, exe = d / "bf16_driver.cpp", d / "bf16_driver"
    src.write_text(DRIVER)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, "-o", str(exe), str(src)])
    return str(exe)


def run(driver, x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    p = subprocess.run([driver], input=x.tobytes(), capture_output=True, env=env, timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    rec = np.frombuffer(p.stdout, dtype=np.dtype([("b", "<u2", 4), ("back", "<f8")]))
    assert rec.shape == x.shape
    return rec["b"], rec["back"]


def values():
    rng = np.random.default_rng(7)
    parts = [
        rng.standard_normal(20000) * np.exp(rng.uniform(-30, 30, 20000)),
        rng.uniform(-1, 1, 5000),
        # ties of the second rounding (exact fp32 values halfway between two bf16 values), both parities
        (np.arange(1, 2000, dtype=np.float64) * 2 + 1) * 2.0 ** -16 + 1.0,
        -((np.arange(1, 2000, dtype=np.float64) * 2 + 1) * 2.0 ** -16 + 1.0),
        # the double rounding: fp64 just above a tie rounds to the tie in fp32 first
        np.array([1 + 2.0 ** -8 + 2.0 ** -30, 1 + 2.0 ** -8 + 2.0 ** -20, 1 + 2.0 ** -8 - 2.0 ** -30]),
        # fp32 subnormals, the normal/subnormal edge, overflow to inf, fp64 values below fp32's range
        rng.uniform(-1, 1, 2000) * 2.0 ** -130, np.array([2.0 ** -126, 2.0 ** -127, 2.0 ** -149, 2.0 ** -151]),
        np.array([3.4e38, -3.4e38, 3.3895e38, 1e300, -1e300, 1e-300, 0.0, -0.0]),
        np.array([np.inf, -np.inf, np.nan, -np.nan]),
    ]
    return np.concatenate(parts)


TORCH_CAST = r"""
import sys
import numpy as np
import torch
x = np.fromfile(sys.argv[1], dtype=np.float64)
torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().tofile(sys.argv[2])
"""


def torch_bf16_bits(x, tmp_path):
    """torch's CPU float64 -> bfloat16 cast of x, in a child process (torch stays out of this one)"""
    src, dst = tmp_path / "x.f64", tmp_path / "b.u16"
    np.ascontiguousarray(x, dtype=np.float64).tofile(src)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    p = subprocess.run([sys.executable, "-c", TORCH_CAST, str(src), str(dst)], capture_output=True,
                       text=True, env=env, timeout=300)
    if p.returncode != 0 and "No module named 'torch'" in p.stderr:
        pytest.skip("torch is not installed")
    assert p.returncode == 0, p.stderr[-4000:]
    return np.fromfile(dst, dtype=np.uint16)


def test_rounding_matches_torch_bit_for_bit(driver, tmp_path):
    x = values()
    b, back = run(driver, x)
    want = torch_bf16_bits(x, tmp_path)
    nan = np.isnan(x)
    assert np.array_equal(b[~nan, 0], want[~nan])
    assert np.all(np.isnan(back[nan])) and np.all((b[nan, 0] & 0x7FFF) > 0x7F80)
    assert np.all((want[nan] & 0x7FFF) > 0x7F80)
    # the numpy restatement of the GPU tests is the same rounding
    assert np.array_equal(bf16_util.bf16_bits(x)[~nan], want[~nan])
    assert bf16_util.same_values(bf16_util.bf16_round(x), back)
    # torch's own double rounding, as the issue states it
    assert back[np.flatnonzero(x == 1 + 2.0 ** -8 + 2.0 ** -30)[0]] == 1.0


def test_three_piece_split_reproduces_fp64(driver):
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.standard_normal(20000) * np.exp(rng.uniform(-20, 20, 20000)),
                        rng.uniform(0.5, 1.0, 5000), [1.0, -1.0, 0.0, 1 / 3, np.pi]])
    b, _ = run(driver, x)
    w = (b[:, 1:].astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    s = w[:, 0] + w[:, 1] + w[:, 2]
    assert np.all(np.abs(s - x) <= 2.0 ** -24 * np.abs(x))
    # the pieces are ordered: |mid| <= ulp(hi)/2, |lo| <= ulp(mid)/2 (non-zero hi)
    nz = w[:, 0] != 0
    assert np.all(np.abs(w[nz, 1]) <= np.abs(w[nz, 0]) * 2.0 ** -8)


def test_hostsim_refuses_bf16_storage():
    pp = hostsim_util.load()
    ctx = pp.Context(0)
    with pytest.raises(pp.PpalsError, match="error -5.*bf16"):
        pp.Tensor(ctx, [4, 5, 6], pp.BF16)
    # and the other storage types still work there
    t = pp.Tensor(ctx, [4, 5, 6], pp.F32)
    t.close()
    ctx.close()
