"""The host half of ppals_tensor_import_device / _export_device (csrc/device_view.h) on a CPU-only box.

* A small driver around device_view.h, built with g++ under ASan + UBSan, walks each copy plan the way
  its kernel does (kernels_io.hip.h: streaming rows and their 4-element vectors, 64 x 64 tiles, the
  per-element gather) and prints the (shard index, view offset) pairs; a numpy brute force over the box
  must give the same map, each shard element once. Random shapes, every ordering of the strides, steps,
  broadcast modes, boxes, P = 1..8 shards.
* The byte span (checked int64), the allocation bound and the export overlap rule.
* Through the host stand-in: a bad box / dtype / stride is PPALS_ERR_ARG; well-formed arguments reach
  the Ops default and come back PPALS_ERR_UNSUPPORTED (the stand-in has no device memory).
"""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import hostsim_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pairwise-perturbation_amd", "csrc")

DRIVER = r"""
#include <cstdio>
#include <iostream>
#include <vector>
#include "device_view.h"
using namespace ppals;

static void emit(const ViewPlan &p, int64_t v, int64_t r) {
  std::printf("%lld %lld\n", (long long)(p.roff + r), (long long)(p.voff + v));
}

int main() {
  std::string cmd;
  while (std::cin >> cmd) {
    if (cmd == "plan") {  // plan dir order g[] row0 l0 lo[] len[] st[]
      int dir, order;
      std::cin >> dir >> order;
      int64_t g[8], lo[8], len[8], st[8], row0, l0;
      for (int i = 0; i < order; i++) std::cin >> g[i];
      std::cin >> row0 >> l0;
      for (int i = 0; i < order; i++) std::cin >> lo[i];
      for (int i = 0; i < order; i++) std::cin >> len[i];
      for (int i = 0; i < order; i++) std::cin >> st[i];
      ViewArgs a;
      std::string err;
      if (!dv_check_args(dir, order, g, DV_F32, lo, len, st, &a, &err)) {
        std::printf("refused %s\nend\n", err.c_str());
        continue;
      }
      const ViewPlan p = dv_plan(a, g, row0, l0);
      std::printf("kind %d nd %d count %lld\n", p.kind, p.nd, (long long)p.count);
      if (p.kind == DV_STREAM) {
        bool vec = p.vs[0] == 1 && p.rs[0] == 1 && p.nd > 1 && p.n[0] % 4 == 0;
        for (int m = 1; m < p.nd; m++) vec = vec && p.vs[m] % 4 == 0 && p.rs[m] % 4 == 0;
        if (vec) {  // k_io_stream<VEC = true>, nd > 1
          const int64_t per_row = p.n[0] / 4, nv = per_row * (p.count / p.n[0]);
          for (int64_t u = 0; u < nv; u++) {
            const int64_t row = u / per_row, c = (u - row * per_row) * 4;
            int64_t v = c, r = c;
            dv_decode(p, 1, p.nd, row, v, r);
            for (int k = 0; k < 4; k++) emit(p, v + k, r + k);
          }
        } else {  // k_io_stream<VEC = false> (nd == 1 with VEC is the same map)
          for (int64_t e = 0; e < p.count; e++) {
            const int64_t row = e / p.n[0], c = e - row * p.n[0];
            int64_t v = c * p.vs[0], r = c * p.rs[0];
            dv_decode(p, 1, p.nd, row, v, r);
            emit(p, v, r);
          }
        }
      } else if (p.kind == DV_TILE) {  // k_io_tile
        int64_t FA, tA, tB, tiles;
        dv_tile_grid(p, &FA, &tA, &tB, &tiles);
        const int64_t nB = p.n[p.fk], rsB = p.rs[p.fk];
        for (int64_t t = 0; t < tiles; t++) {
          const int64_t ta = t % tA, tr = t / tA, tb = tr % tB, bt = tr / tB;
          int64_t bv = 0, br = 0;
          dv_decode(p, p.fk + 1, p.nd, bt, bv, br);
          const int64_t a0 = ta * DV_TILE_DIM, b0 = tb * DV_TILE_DIM;
          const int na = (int)std::min<int64_t>(DV_TILE_DIM, FA - a0);
          const int nb = (int)std::min<int64_t>(DV_TILE_DIM, nB - b0);
          int64_t av[DV_TILE_DIM], ar[DV_TILE_DIM];
          for (int i = 0; i < DV_TILE_DIM; i++) {
            av[i] = bv;
            ar[i] = br;
            if (i < na) dv_decode(p, 0, p.fk, a0 + i, av[i], ar[i]);
          }
          for (int a = 0; a < na; a++)
            for (int b = 0; b < nb; b++) emit(p, av[a] + b0 + b, ar[a] + (b0 + b) * rsB);
        }
      } else if (p.kind == DV_GATHER) {  // k_io_gather
        for (int64_t e = 0; e < p.count; e++) {
          int64_t v = 0, r = 0;
          dv_decode(p, 0, p.nd, e, v, r);
          emit(p, v, r);
        }
      }
      std::printf("end\n");
    } else if (cmd == "span") {  // span order len[] st[] esize
      int order, esize;
      std::cin >> order;
      int64_t len[8], st[8], out = -1;
      for (int i = 0; i < order; i++) std::cin >> len[i];
      for (int i = 0; i < order; i++) std::cin >> st[i];
      std::cin >> esize;
      const bool ok = dv_span_bytes(order, len, st, esize, &out);
      std::printf("%d %lld\n", ok ? 1 : 0, (long long)(ok ? out : -1));
    } else if (cmd == "alloc") {  // alloc ptr span base size
      unsigned long long ptr, base, size;
      long long span;
      std::cin >> ptr >> span >> base >> size;
      std::printf("%d\n", dv_in_allocation(ptr, span, base, size) ? 1 : 0);
    } else if (cmd == "overlap") {  // overlap order len[] st[]
      int order;
      std::cin >> order;
      int64_t len[8], st[8];
      for (int i = 0; i < order; i++) std::cin >> len[i];
      for (int i = 0; i < order; i++) std::cin >> st[i];
      std::printf("%d\n", dv_no_self_overlap(order, len, st) ? 1 : 0);
    }
    std::fflush(stdout);
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("dv")
    src, exe = d / "dv_driver.cpp", d / "dv_driver"
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


def plan_cmd(direction, g, row0, l0, lo, ln, st):
    return " ".join(str(x) for x in ["plan", direction, len(g), *g, row0, l0, *lo, *ln, *st])


def parse_plans(lines):
    res, i = [], 0
    while i < len(lines):
        head = lines[i].split()
        i += 1
        if head[0] == "refused":
            res.append(None)
            assert lines[i] == "end"
            i += 1
            continue
        kind, count = int(head[1]), int(head[5])
        pairs = []
        while lines[i] != "end":
            r, v = lines[i].split()
            pairs.append((int(r), int(v)))
            i += 1
        i += 1
        res.append((kind, count, np.array(pairs, dtype=np.int64).reshape(-1, 2)))
    return res


def brute(g, row0, l0, lo, ln, st):
    """(shard index, view offset) of every box element in rows [row0, row0 + l0)"""
    N = len(g)
    rsf = [1] + [0] * (N - 1)
    for i in range(1, N):
        rsf[i] = rsf[i - 1] * (l0 if i == 1 else g[i - 1])
    pairs = []
    for j in itertools.product(*[range(n) for n in ln]):
        a = [lo[i] + j[i] for i in range(N)]
        if not row0 <= a[0] < row0 + l0:
            continue
        r = (a[0] - row0) + sum(a[i] * rsf[i] for i in range(1, N))
        v = sum(j[i] * st[i] for i in range(N))
        pairs.append((r, v))
    return np.array(pairs, dtype=np.int64).reshape(-1, 2)


def random_cases(rng, ncases):
    cases = []
    for _ in range(ncases):
        N = int(rng.integers(1, 5))
        g = [int(x) for x in rng.integers(1, 8, size=N)]
        if rng.random() < 0.3:
            g[0] = int(rng.integers(1, 70))
        if rng.random() < 0.2 and N > 1:
            g[-1] = int(rng.integers(60, 140))   # more than one 64-wide tile
        lo, ln = [], []
        for s in g:
            if rng.random() < 0.5:
                lo.append(0)
                ln.append(s)
            else:
                a = int(rng.integers(0, s))
                lo.append(a)
                ln.append(int(rng.integers(1, s - a + 1)))
        # a strided parent of the box: a random mode order, steps, padding, broadcast modes
        order = list(rng.permutation(N))
        st, acc = [0] * N, 1
        for m in order:
            step = int(rng.choice([1, 1, 1, 2, 3]))
            st[m] = acc * step
            acc = st[m] * max(ln[m], 1) + int(rng.choice([0, 0, 1, 5]))
        for m in range(N):
            if rng.random() < 0.1:
                st[m] = 0
        P = int(rng.integers(1, 9))
        blk = -(-g[0] // P)
        p = int(rng.integers(0, P))
        row0 = min(p * blk, g[0])
        l0 = max(0, min(blk, g[0] - row0))
        if l0 == 0:
            row0, l0 = 0, g[0]
        cases.append((g, row0, l0, lo, ln, st))
    return cases


def check_cases(driver, cases, direction=0):
    res = parse_plans(run(driver, [plan_cmd(direction, *c) for c in cases]))
    kinds = set()
    for c, got in zip(cases, res):
        assert got is not None, c
        kind, count, pairs = got
        want = brute(*c)
        assert count == len(want), (c, count, len(want))
        assert len(pairs) == len(want), (c, kind, len(pairs), len(want))
        if len(want):
            assert len(np.unique(pairs[:, 0])) == len(pairs), (c, kind, "a shard element twice")
            a = pairs[np.lexsort(pairs.T[::-1])]
            b = want[np.lexsort(want.T[::-1])]
            assert np.array_equal(a, b), (c, kind)
            kinds.add(kind)
    return kinds


def test_plan_maps_match_brute_force(driver):
    kinds = check_cases(driver, random_cases(np.random.default_rng(7), 400))
    assert kinds == {1, 2, 3}, kinds   # streaming, tiled and gathered plans all exercised


def test_every_stride_ordering_every_shard(driver):
    g = [5, 3, 4, 6]
    cases = []
    for perm in itertools.permutations(range(4)):
        st, acc = [0] * 4, 1
        for m in perm:
            st[m] = acc
            acc *= g[m]
        for P in range(1, 9):
            blk = -(-g[0] // P)
            for p in range(P):
                row0 = p * blk
                if row0 >= g[0]:
                    continue
                cases.append((g, row0, min(blk, g[0] - row0), [0] * 4, g, st))
    kinds = check_cases(driver, cases)
    assert kinds >= {1, 2}


def test_torch_layouts_and_real_data_extents(driver):
    """C-contiguous (reversed) strides with tiny leading extents, step slices, broadcasts"""
    cases = []
    for g in ([3, 8, 8, 72], [33, 5, 4, 3], [1, 9, 8], [200, 1, 7], [3, 2, 70], [67, 65]):
        N = len(g)
        rev = [int(np.prod(g[i + 1:])) for i in range(N)]
        cases.append((g, 0, g[0], [0] * N, g, rev))                        # x
        cases.append((g, 0, g[0], [0] * N, g, [2 * s for s in rev]))         # x[..., ::2] of a wider parent
        cases.append((g, 0, g[0], [0] * N, g, [0] + rev[1:]))                # x.expand along mode 0
        half = g[-1] // 2 or 1
        cases.append((g, 0, g[0], [0] * (N - 1) + [g[-1] - half], g[:-1] + [half], rev))  # a slab
    check_cases(driver, cases)


def test_export_plans_and_overlap_rule(driver):
    cases = [c for c in random_cases(np.random.default_rng(11), 200)
             if all(s > 0 or n == 1 for s, n in zip(c[5], c[4]))]
    check_cases(driver, cases, direction=1)
    lines = run(driver, [
        "overlap 2 3 4 1 3",      # dense: fine
        "overlap 2 3 4 4 1",      # transposed dense: fine
        "overlap 2 3 4 1 2",      # rows overlap
        "overlap 2 3 4 0 3",      # broadcast on an extent 3
        "overlap 2 1 4 0 3",      # a zero stride on an extent of 1 writes nothing twice
        "overlap 3 2 2 2 1 1 4",  # the same stride twice: aliased
        "overlap 2 0 4 0 0",      # empty
        "overlap 2 3 5 2 7",      # step 2, rows 7 apart: fine
        "overlap 2 11 6 2 21",    # step 2 over 11 (last offset 20), rows 21 apart: fine
        "overlap 2 11 6 2 20",    # the same rows 20 apart: (10, 0) and (0, 1) collide
        "overlap 3 2 3 4 30 1 3", # sorted 1 (x3), 3 (x4), 30 (x2): 3 > 2, 30 > 11: fine
        "overlap 3 2 3 4 11 1 3", # 11 <= 2 + 9
    ])
    assert lines == ["1", "1", "0", "0", "1", "0", "1", "1", "1", "0", "1", "0"]


def test_span_arithmetic(driver):
    big = 2 ** 62
    lines = run(driver, [
        "span 2 3 4 1 3 4",             # (2 + 9 + 1) * 4
        "span 2 3 4 12 1 8",            # (24 + 3 + 1) * 8
        "span 1 5 0 2",                 # broadcast: one element
        "span 2 0 4 1 3 4",             # empty box
        f"span 1 3 {big} 4",            # 2 * 2^62 overflows
        f"span 1 2 {big} 4",            # 2^62 + 1 elements fit, their bytes do not
        f"span 2 2 2 {big} {big} 1",           # the sum overflows
        f"span 1 2 {2 ** 61} 2",        # (2^61 + 1) * 2 fits
    ])
    assert lines == ["1 48", "1 224", "1 2", "1 0", "0 -1", "0 -1", "0 -1",
                     f"1 {(2 ** 61 + 1) * 2}"]


def test_allocation_bound(driver):
    base, size = 0x7F0000000000, 4096
    lines = run(driver, [
        f"alloc {base} 4096 {base} {size}",          # exactly the allocation
        f"alloc {base + 8} 4088 {base} {size}",      # ends at its end
        f"alloc {base + 8} 4089 {base} {size}",      # one byte past
        f"alloc {base - 4} 8 {base} {size}",         # starts before it
        f"alloc {base + 4096} 0 {base} {size}",      # empty at the end
        f"alloc {base + 4097} 0 {base} {size}",      # past the end
        f"alloc {base + 16} 9223372036854775807 {base} {size}",
    ])
    assert lines == ["1", "1", "0", "0", "1", "0", "0"]


def test_refusals_before_the_copy(driver):
    g = [4, 5, 6]
    lines = run(driver, [
        plan_cmd(0, g, 0, 4, [0, 0, 0], [4, 5, 7], [1, 4, 20]),   # past the extent
        plan_cmd(0, g, 0, 4, [-1, 0, 0], [2, 5, 6], [1, 4, 20]),  # negative lo
        plan_cmd(0, g, 0, 4, [0, 0, 0], [4, 5, 6], [1, -4, 20]),  # negative stride
        plan_cmd(1, g, 0, 4, [0, 0, 0], [4, 5, 6], [1, 0, 20]),   # export onto a broadcast
        plan_cmd(0, g, 0, 4, [0, 0, 0], [4, 5, 6], [1, 0, 20]),   # import from one: fine
    ])
    res = parse_plans(lines)
    assert res[:4] == [None] * 4 and res[4] is not None


# ---------------------------------------------------------------- through the host stand-in
@pytest.fixture(scope="module")
def pp():
    return hostsim_util.load()


def test_hostsim_check_and_copy_codes(pp):
    ctx = pp.Context(0)
    t = pp.Tensor(ctx, [4, 5, 6], pp.F32)
    fake = 0x10000   # never dereferenced: the stand-in stops at its pointer query
    ARG, UNSUP = -3, -5
    dense = [30, 6, 1]
    assert t.check_view(0, fake, pp.F32, [4, 5, 6], dense) == UNSUP
    assert t.check_view(1, fake, pp.F64, [4, 5, 6], dense) == UNSUP
    assert t.check_view(0, fake, pp.BF16, [2, 5, 6], dense, lo=[2, 0, 0]) == UNSUP
    assert t.check_view(0, fake, pp.F32, [4, 5, 7], dense) == ARG            # box past the extent
    assert t.check_view(0, fake, pp.F32, [3, 5, 6], dense, lo=[2, 0, 0]) == ARG
    assert t.check_view(0, fake, 7, [4, 5, 6], dense) == ARG                 # bad dtype
    assert t.check_view(1, fake, pp.F16, [4, 5, 6], dense) == ARG            # f16 destination
    assert t.check_view(0, fake, pp.F32, [4, 5, 6], [30, -6, 1]) == ARG      # negative stride
    assert t.check_view(1, fake, pp.F32, [4, 5, 6], [30, 0, 1]) == ARG       # overlapping export
    assert t.check_view(0, fake, pp.F32, [4, 5, 6], [2 ** 62, 6, 1]) == ARG  # span overflows
    assert t.check_view(0, 0, pp.F32, [4, 5, 6], dense) == ARG               # NULL pointer
    assert t.check_view(2, fake, pp.F32, [4, 5, 6], dense) == ARG            # bad direction
    with pytest.raises(pp.PpalsError, match="error -3"):
        t.import_device(fake, pp.F32, [4, 5, 7], dense)
    with pytest.raises(pp.PpalsError, match="error -5"):
        t.import_device(fake, pp.F32, [4, 5, 6], dense)
    with pytest.raises(pp.PpalsError, match="error -5"):
        t.export_device(fake, pp.F32, [4, 5, 6], dense)
    with pytest.raises(pp.PpalsError, match="modes"):
        t.import_device(fake, pp.F32, [4, 5], dense[:2])
    lib = pp.lib()
    n = C.c_int64 * 3
    # NULL box (the whole tensor) and NULL strides (dense, first index fastest)
    assert lib.ppals_tensor_check_device_view(t._h, 0, C.c_void_p(fake), pp.F32, None, None, None) == UNSUP
    assert lib.ppals_tensor_check_device_view(t._h, 0, C.c_void_p(fake), pp.F32, n(0, 0, 0), None,
                                              None) == ARG
    assert lib.ppals_tensor_check_device_view(None, 0, C.c_void_p(fake), pp.F32, None, None, None) == ARG
    t.close()
    ctx.close()
