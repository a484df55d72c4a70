"""The plan arithmetic of the weighted step's second side view (csrc/device_view.h: dv_model_side,
dv_side_along_a) on a CPU-only box.

A small driver around device_view.h, built with g++ under ASan + UBSan, cuts a box with dv_model_box, groups
its modes the way the step does (group A = the shard's leading modes, group B = the rest, any order), derives
the weights' strides and offset with dv_model_side, and walks every (a, b) the way the offset kernels do
(flat index of a group, first listed mode fastest), printing (shard offset, data offset, weights offset). A
numpy brute force over the box must give the same triples, each shard element of the rank's rows once: random
shapes, strides (zeros included), boxes and P = 1..4 shards."""
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pairwise-perturbation_amd", "csrc")

DRIVER = r"""
#include <cstdio>
#include <iostream>
#include <vector>
#include "device_view.h"
using namespace ppals;

static int64_t offset(const ModelGroup &g, const int64_t *st, int64_t idx) {
  int64_t v = 0;
  for (int m = 0; m < g.n; m++) {
    const int64_t q = idx / g.len[m], c = idx - q * g.len[m];
    v += c * st[m];
    idx = q;
  }
  return v;
}

int main() {
  std::string cmd;
  while (std::cin >> cmd) {
    if (cmd == "side") {  // side order g[] row0 l0 lo[] len[] dst[] wst[] nA permB[order - nA... by mode id]
      int order;
      std::cin >> order;
      int64_t g[DV_MAX_ORDER], lo[DV_MAX_ORDER], len[DV_MAX_ORDER], ds[DV_MAX_ORDER], ws[DV_MAX_ORDER], row0, l0;
      for (int i = 0; i < order; i++) std::cin >> g[i];
      std::cin >> row0 >> l0;
      for (int i = 0; i < order; i++) std::cin >> lo[i];
      for (int i = 0; i < order; i++) std::cin >> len[i];
      for (int i = 0; i < order; i++) std::cin >> ds[i];
      for (int i = 0; i < order; i++) std::cin >> ws[i];
      int nA;
      std::cin >> nA;
      int bmodes[DV_MAX_ORDER];
      for (int i = 0; i < order - nA; i++) std::cin >> bmodes[i];
      ViewArgs a, w;
      std::string err;
      if (!dv_check_args(DV_IMPORT, order, g, DV_F64, lo, len, ds, &a, &err) ||
          !dv_check_args(DV_IMPORT, order, g, DV_F64, lo, len, ws, &w, &err)) {
        std::printf("refused %s\nend\n", err.c_str());
        continue;
      }
      ModelBox bx;
      if (!dv_model_box(a, g, row0, l0, &bx)) {
        std::printf("empty\nend\n");
        continue;
      }
      ModelPlan mp;
      for (int m = 0; m < nA; m++) mp.ga.add(bx, m);
      for (int i = 0; i < order - nA; i++) mp.gb.add(bx, bmodes[i]);
      mp.voff = bx.voff;
      mp.roff = bx.roff;
      const ModelSide s = dv_model_side(w, bx, mp);
      std::printf("box %lld %lld\n", (long long)mp.ga.count, (long long)mp.gb.count);
      for (int64_t b = 0; b < mp.gb.count; b++)
        for (int64_t x = 0; x < mp.ga.count; x++)
          std::printf("%lld %lld %lld\n", (long long)(mp.roff + offset(mp.ga, mp.ga.rs, x) + offset(mp.gb, mp.gb.rs, b)),
                      (long long)(mp.voff + offset(mp.ga, mp.ga.vs, x) + offset(mp.gb, mp.gb.vs, b)),
                      (long long)(s.off + offset(s.ga, s.ga.vs, x) + offset(s.gb, s.gb.vs, b)));
      std::printf("end\n");
    } else if (cmd == "along") {  // along sa sb
      long long sa, sb;
      std::cin >> sa >> sb;
      std::printf("%d\n", dv_side_along_a(sa, sb) ? 1 : 0);
    }
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("wlsdv")
    src, exe = d / "wls_dv_driver.cpp", d / "wls_dv_driver"
    src.write_text(DRIVER)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, "-o", str(exe), str(src)])
    return str(exe)


def run(driver, lines):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    out = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True,
                         env=env, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    assert "runtime error" not in out.stderr, out.stderr[-4000:]
    return out.stdout.splitlines()


def brute(g, row0, l0, lo, ln, ds, ws):
    """(shard index, data offset, weights offset) of every box element in rows [row0, row0 + l0)"""
    N = len(g)
    rsf = [1] + [0] * (N - 1)
    for i in range(1, N):
        rsf[i] = rsf[i - 1] * (l0 if i == 1 else g[i - 1])
    out = []
    for j in itertools.product(*[range(n) for n in ln]):
        a = [lo[i] + j[i] for i in range(N)]
        if not row0 <= a[0] < row0 + l0:
            continue
        out.append(((a[0] - row0) + sum(a[i] * rsf[i] for i in range(1, N)),
                    sum(j[i] * ds[i] for i in range(N)), sum(j[i] * ws[i] for i in range(N))))
    return np.array(out, dtype=np.int64).reshape(-1, 3)


def random_strides(rng, ln):
    """a permuted dense layout with a step here and there, some modes broadcast (stride 0)"""
    N = len(ln)
    st, reach = [0] * N, 1
    for m in rng.permutation(N):
        st[m] = reach * int(rng.integers(1, 3))
        reach = st[m] * max(ln[m], 1)
    for m in range(N):
        if rng.random() < 0.25:
            st[m] = 0
    return st


def test_side_offsets_match_brute_force(driver):
    rng = np.random.default_rng(11)
    cases, lines = [], []
    for _ in range(300):
        N = int(rng.integers(2, 6))
        g = [int(rng.integers(1, 7)) for _ in range(N)]
        lo = [int(rng.integers(0, n)) for n in g]
        ln = [int(rng.integers(1, n - l + 1)) for n, l in zip(g, lo)]
        P = int(rng.integers(1, 5))
        rows = -(-g[0] // P)
        rank = int(rng.integers(0, P))
        row0 = min(rank * rows, g[0])
        l0 = max(0, min(rows, g[0] - row0))
        if l0 == 0:
            continue
        ds, ws = random_strides(rng, ln), random_strides(rng, ln)
        nA = int(rng.integers(1, N))
        bm = [int(m) for m in nA + rng.permutation(N - nA)]
        cases.append((g, row0, l0, lo, ln, ds, ws))
        lines.append(" ".join(str(x) for x in ["side", N, *g, row0, l0, *lo, *ln, *ds, *ws, nA, *bm]))
    out = run(driver, lines)
    i = 0
    for g, row0, l0, lo, ln, ds, ws in cases:
        want = brute(g, row0, l0, lo, ln, ds, ws)
        head = out[i].split()
        i += 1
        got = []
        while out[i] != "end":
            got.append([int(x) for x in out[i].split()])
            i += 1
        i += 1
        if head[0] == "empty":
            assert want.shape[0] == 0
            continue
        assert head[0] == "box", out[i - 2]
        got = np.array(got, dtype=np.int64).reshape(-1, 3)
        assert int(head[1]) * int(head[2]) == got.shape[0] == want.shape[0]
        assert len(set(got[:, 0])) == got.shape[0]          # each shard element once
        key = np.argsort(got[:, 0])
        wkey = np.argsort(want[:, 0])
        assert np.array_equal(got[key], want[wkey]), (g, row0, l0, lo, ln, ds, ws)
    assert i == len(out)


def test_how_a_side_view_is_read(driver):
    cases = [((1, 1), 1), ((1, 40), 1), ((1, 0), 1),      # unit-stride along a: in the store pass
             ((40, 1), 0), ((0, 1), 0),                   # its unit-stride run along b: through LDS
             ((0, 0), 1), ((0, 40), 1), ((40, 0), 1),     # a broadcast: one address for all lanes, along a
             ((12, 40), 1)]                               # no unit-stride run at all: along a
    out = run(driver, [f"along {sa} {sb}" for (sa, sb), _ in cases])
    assert [int(x) for x in out] == [w for _, w in cases]
