// kernels_shape.hip.h — the shaped non-negative mode update of a CP session (Ops::cp_mode_update_shape_ragged):
// every column of the factor is replaced, one after the other, by the least-squares projection of its HALS
// target onto the non-negative unimodal, non-decreasing or non-increasing sequences (Bro & Sidiropoulos 1998),
// for every start of a session in THREE launches whatever the number of starts, the ranks and the rows:
//   1. k_shape_grad        (row tiles x starts)  grad = -M + W_old S, its tile sums, S when asked
//   2. k_shape_columns     (one workgroup per start)  the column loop
//   3. k_cp_finish_nn_ragged of kernels_nn.hip.h  (tile sums and the Gram of the new W)
// hadamard_entry and wave_sum come from kernels_small.hip.h. All arithmetic is fp64; no atomics, every sum in a
// fixed order, so the same state gives the same bits; a start reads and writes its own columns only.
#pragma once
#include "kernels_nn.hip.h"

namespace ppals {

// Launch 1: the gradient half of k_cp_update_ortho_ragged (one wave per tile of 64 rows, a lane one row, S as
// R x R and the tile's rows of W_old as sW[q * 64 + lane] in LDS: (R^2 + 64 R) doubles).
__global__ __launch_bounds__(64) void k_shape_grad(
    const double *__restrict__ Gall, int N, int mode, StartTable t, double lambda,
    const double *__restrict__ M, int64_t ldm, const double *__restrict__ W, int64_t ldw,
    double *__restrict__ grad, int64_t ldg, int64_t rows, double *__restrict__ gradsq_part,
    double *__restrict__ S_out) {
  extern __shared__ double lds[];
  const int b = blockIdx.y;
  const int R = t.col[b + 1] - t.col[b];
  const int64_t c0 = t.col[b], so = t.sq[b];
  Gall += N * so;
  M += c0 * ldm;
  W += c0 * ldw;
  grad += c0 * ldg;
  double *sS = lds;          // R x R, column-major (symmetric)
  double *sW = lds + R * R;  // R x 64
  const int lane = threadIdx.x;
  for (int e = lane; e < R * R; e += 64) {
    const double v = hadamard_entry(Gall, N, mode, R, lambda, e);
    sS[e] = v;
    if (S_out && blockIdx.x == 0) S_out[so + e] = v;
  }
  const int64_t x = (int64_t)blockIdx.x * 64 + lane;
  const bool live = x < rows;
  for (int q = 0; q < R; q++) sW[q * 64 + lane] = live ? W[x + ldw * q] : 0.0;
  __syncthreads();
  double gs = 0;
  if (live) {
    for (int r = 0; r < R; r++) {
      const double *sc = sS + r * R;
      double acc = 0;
      for (int q = 0; q < R; q++) acc += sW[q * 64 + lane] * sc[q];
      const double gv = -M[x + ldm * r] + acc;
      grad[x + ldg * r] = gv;
      gs += gv * gv;
    }
  }
  gs = wave_sum(gs);
  if (lane == 0) gradsq_part[(int64_t)b * gridDim.x + blockIdx.x] = gs;
}

// The work arrays of one start in launch 2, n = rows: in LDS behind S while 8 R^2 + shape_work_bytes(n) fits
// in kShapeLdsBytes (ops.h), else in a global scratch of the same layout — one code path, two pointers.
//   v[n] | err0[n] err1[n] | sum0[n] sq0[n] | sum1[n] sq1[n] | start0[n + 1] start1[n + 1] (ints)
// 64 n + 8 bytes. Pass 0 runs over the rows upwards, pass 1 downwards, each on a wave of its own.
struct ShapeWork {
  double *v, *err[2], *sum[2], *sq[2];
  int *start[2];
};
__device__ __forceinline__ ShapeWork shape_work(double *base, int64_t n) {
  ShapeWork w;
  w.v = base;
  w.err[0] = base + n;
  w.err[1] = base + 2 * n;
  w.sum[0] = base + 3 * n;
  w.sq[0] = base + 4 * n;
  w.sum[1] = base + 5 * n;
  w.sq[1] = base + 6 * n;
  w.start[0] = (int *)(base + 7 * n);
  w.start[1] = w.start[0] + (n + 1);
  return w;
}

// v of lane j (uniform over the wave) to every lane: two v_readlane, no trip through the LDS crossbar
__device__ __forceinline__ double shape_bcast(double v, int j) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), j);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), j);
  return __hiloint2double(hi, lo);
}
// 1 / c for a count c: the hardware reciprocal and two Newton steps (fp64 throughout; within an ulp or two of the
// quotient). Only the split errors use it — they choose p; the fit itself divides properly (shape_emit).
__device__ __forceinline__ double shape_inv(double c) {
  double r = __builtin_amdgcn_rcp(c);
  r = fma(fma(-c, r, 1.0), r, r);
  return fma(fma(-c, r, 1.0), r, r);
}

// Pool-adjacent-violators over the m entries a[k] = v[rev ? n - 1 - k : k], k < m, by ONE wave whose lanes all
// run the same serial program on the same values: 64 entries are fetched at a time, a lane each, and handed
// round by shape_bcast. The top block lives in uniform registers and the up to 64 blocks under it in a WINDOW
// of per-lane registers (lane i holds block base + i; a push is a select on the lane number, a pop a v_readlane), so a step
// touches memory only when the window runs full (its 64 blocks are spilled, a lane each) or empty (the 64 below
// are fetched back): the chain of pooling decisions holds no memory round trip, and no division either — means
// are compared by cross-multiplication (counts are positive).
// The blocks of the non-decreasing fit end up in memory as (sum, start): block j covers the entries
// [start[j], start[j + 1]), start[depth] = m; the return value is the depth.
// ERR: also sq per block and err[k] = the error of the fit of the entries 0 .. k CLIPPED at `floor` (the bounded
// isotonic fit is the unbounded one clipped): the blocks below the top are final for that prefix, so
// err[k] = err[top's start - 1] + the top's own error sq - 2 c sum + c^2 count, c = max(mean, floor). Every lane
// stores err[k] (the same value to the same address), so a lane that fetches it back reads its own store.
template <bool ERR>
__device__ __forceinline__ int shape_pava(const double *v, int64_t n, bool rev, int m, double *ssum, double *ssq,
                                          int *sstart, double *err, double floor, int lane) {
  int depth = 0, base = 0;  // blocks below the top: [0, base) in memory, [base, depth) in the window
  double rsum = 0, rsq = 0, rbelow = 0;
  int rstart = 0;
  bool has = false;  // a top block
  double tsum = 0, tsq = 0, tcnt = 0, below = 0, last = 0;  // below: err under the top; last: err[pos - 1]
  int tstart = 0;
  for (int k0 = 0; k0 < m; k0 += 64) {
    const int k = k0 + lane;
    const double mine = k < m ? v[rev ? n - 1 - k : k] : 0.0;
    const int lim = m - k0 < 64 ? m - k0 : 64;
    for (int j = 0; j < lim; j++) {
      const int pos = k0 + j;
      const double x = shape_bcast(mine, j);
      double bs = x, bq = x * x, bcnt = 1.0, bbelow = last;
      int bstart = pos;
      while (has && tsum * bcnt >= bs * tcnt) {
        bs += tsum;
        bcnt += tcnt;
        bstart = tstart;
        if (ERR) {
          bq += tsq;
          bbelow = below;
        }
        if (depth > 0) {
          if (depth == base) {  // the window is empty: the 64 blocks below come back
            base -= 64;
            rsum = ssum[base + lane];
            rstart = sstart[base + lane];
            if (ERR) {
              rsq = ssq[base + lane];
              rbelow = rstart > 0 ? err[rstart - 1] : 0.0;
            }
          }
          depth--;
          const int i = depth - base;
          tsum = shape_bcast(rsum, i);
          tstart = __builtin_amdgcn_readlane(rstart, i);
          tcnt = (double)(bstart - tstart);
          if (ERR) {
            tsq = shape_bcast(rsq, i);
            below = shape_bcast(rbelow, i);
          }
        } else {
          has = false;
        }
      }
      if (has) {  // the old top goes below the new one
        if (depth - base == 64) {  // the window is full: its blocks go to memory
          ssum[base + lane] = rsum;
          sstart[base + lane] = rstart;
          if (ERR) ssq[base + lane] = rsq;
          base += 64;
        }
        const int i = depth - base;
        rsum = lane == i ? tsum : rsum;
        rstart = lane == i ? tstart : rstart;
        if (ERR) {
          rsq = lane == i ? tsq : rsq;
          rbelow = lane == i ? below : rbelow;
        }
        depth++;
      }
      tsum = bs;
      tcnt = bcnt;
      tstart = bstart;
      has = true;
      if (ERR) {
        tsq = bq;
        below = bbelow;
        const double mean = tsum * shape_inv(tcnt), c = mean > floor ? mean : floor;
        last = below + (tsq - 2.0 * c * tsum + c * c * tcnt);
        err[pos] = last;
      }
    }
  }
  if (lane < depth - base) {  // what is left in the window
    ssum[base + lane] = rsum;
    sstart[base + lane] = rstart;
  }
  if (has) {
    ssum[depth] = tsum;
    sstart[depth] = tstart;
    depth++;
  }
  sstart[depth] = m;
  return depth;
}

// the blocks of a pass into column w: block j's clipped mean to the rows of its entries; wave `wave` of
// `nwaves` takes the blocks j = wave, wave + nwaves, ..., its lanes the block's entries
__device__ __forceinline__ void shape_emit(double *w, int64_t n, bool rev, int depth, const double *ssum,
                                           const int *sstart, double floor, int wave, int nwaves, int lane) {
  for (int j = wave; j < depth; j += nwaves) {
    const int k0 = sstart[j], k1 = sstart[j + 1];
    const double mean = ssum[j] / (double)(k1 - k0), c = mean > floor ? mean : floor;
    for (int k = k0 + lane; k < k1; k += 64) w[rev ? n - 1 - k : k] = c;
  }
}

// Launch 2, one 1024-thread workgroup per start (StartTable by value): for r = 0 .. R_b - 1 in this order
//   d = S[r, r]; not a positive finite number: the column stays
//   v[x] = w[x, r] + (M[x, r] - sum_q w[x, q] S[q, r]) / d   with the W of this moment (all threads, rows strided)
//   some v[x] not finite: the column stays
//   INCREASING / DECREASING: one pass of shape_pava (wave 0), then shape_emit (all waves)
//   UNIMODAL: pass 0 on wave 0 and pass 1 on wave 1 give e(p) = err0[p] + err1[n - 2 - p], the error of "rows
//     0 .. p rise, rows p + 1 .. n - 1 fall"; the least e(p) wins, the smallest p on a tie (every thread takes
//     p strided, then a fixed-order reduction); the two passes again on [0, p] and on [p + 1, n) (later entries
//     pool a prefix's blocks away, so the first passes' stacks cannot be reused), then shape_emit of both.
// W is read and written in place: a column is written only after its v is complete, behind a barrier.
// dynamic LDS: S (R^2 doubles, R the largest rank of the launch) and, when `gwork` is null, the work arrays.
__global__ __launch_bounds__(1024) void k_shape_columns(
    const double *__restrict__ Gall, int N, int mode, StartTable t, double lambda,
    const double *__restrict__ M, int64_t ldm, double *W, int64_t ldw, int64_t rows, int shape, double floor,
    int rmax, double *gwork, int64_t gstride) {
  extern __shared__ double lds[];
  __shared__ double red_e[16];
  __shared__ int red_p[16];
  __shared__ int sh_depth[2];
  __shared__ int sh_p;
  const int b = blockIdx.x;
  const int R = t.col[b + 1] - t.col[b];
  const int64_t c0 = t.col[b], n = rows;
  Gall += (int64_t)N * t.sq[b];
  M += c0 * ldm;
  W += c0 * ldw;
  double *sS = lds;
  const ShapeWork wk = shape_work(gwork ? gwork + (int64_t)b * gstride : lds + rmax * rmax, n);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = blockDim.x >> 6;
  for (int e = tid; e < R * R; e += blockDim.x) sS[e] = hadamard_entry(Gall, N, mode, R, lambda, e);
  __syncthreads();
  for (int r = 0; r < R; r++) {
    const double *sc = sS + r * R;
    const double d = sc[r];
    if (!(d > 0.0) || d > 1.79769313486231570e308) continue;  // (uniform: every thread reads the same d)
    int bad = 0;
    for (int64_t x = tid; x < n; x += blockDim.x) {
      double acc = 0;
      for (int q = 0; q < R; q++) acc += W[x + ldw * q] * sc[q];
      const double v = W[x + ldw * r] + (M[x + ldm * r] - acc) / d;
      wk.v[x] = v;
      if (!(fabs(v) <= 1.79769313486231570e308)) bad = 1;
    }
    if (__syncthreads_or(bad)) continue;  // (uniform; the barrier also publishes v)
    double *wcol = W + ldw * r;
    if (shape != kShapeUnimodal) {
      const bool rev = shape == kShapeDecreasing;
      if (wave == 0) {
        const int depth = shape_pava<false>(wk.v, n, rev, (int)n, wk.sum[0], wk.sq[0], wk.start[0], wk.err[0], floor, lane);
        if (lane == 0) sh_depth[0] = depth;
      }
      __syncthreads();
      shape_emit(wcol, n, rev, sh_depth[0], wk.sum[0], wk.start[0], floor, wave, nwaves, lane);
      __syncthreads();
      continue;
    }
    if (wave < 2) shape_pava<true>(wk.v, n, wave == 1, (int)n, wk.sum[wave], wk.sq[wave], wk.start[wave], wk.err[wave], floor, lane);
    __syncthreads();
    double ebest = 0;
    int pbest = 0x7fffffff;
    for (int64_t p = tid; p < n; p += blockDim.x) {
      const double e = wk.err[0][p] + (p + 1 < n ? wk.err[1][n - 2 - p] : 0.0);
      if (pbest == 0x7fffffff || e < ebest) {
        ebest = e;
        pbest = (int)p;
      }
    }
    for (int off = 32; off > 0; off >>= 1) {
      const double eo = __shfl_down(ebest, off, 64);
      const int po = __shfl_down(pbest, off, 64);
      if (po != 0x7fffffff && (pbest == 0x7fffffff || eo < ebest || (eo == ebest && po < pbest))) {
        ebest = eo;
        pbest = po;
      }
    }
    if (lane == 0) {
      red_e[wave] = ebest;
      red_p[wave] = pbest;
    }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < nwaves; w++) {
        const double eo = red_e[w];
        const int po = red_p[w];
        if (po != 0x7fffffff && (pbest == 0x7fffffff || eo < ebest || (eo == ebest && po < pbest))) {
          ebest = eo;
          pbest = po;
        }
      }
      sh_p = pbest == 0x7fffffff ? 0 : pbest;
    }
    __syncthreads();
    const int p = sh_p;
    if (wave < 2) {
      const int m = wave == 0 ? p + 1 : (int)n - 1 - p;
      const int depth = shape_pava<false>(wk.v, n, wave == 1, m, wk.sum[wave], wk.sq[wave], wk.start[wave], wk.err[wave], floor, lane);
      if (lane == 0) sh_depth[wave] = depth;
    }
    __syncthreads();
    shape_emit(wcol, n, false, sh_depth[0], wk.sum[0], wk.start[0], floor, wave, nwaves, lane);
    shape_emit(wcol, n, true, sh_depth[1], wk.sum[1], wk.start[1], floor, wave, nwaves, lane);
    __syncthreads();
  }
}

}  // namespace ppals
