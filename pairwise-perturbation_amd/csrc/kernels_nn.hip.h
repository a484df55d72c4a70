// kernels_nn.hip.h — the non-negative (HALS) mode update of a CP session (Ops::cp_mode_update_nn) and of
// all starts of a multi-start session (Ops::cp_mode_update_nn_batched).
// hadamard_entry, wave_sum, block_sum, gram_pairs and k_sum_partials come from kernels_small.hip.h.
#pragma once
#include "kernels_small.hip.h"

namespace ppals {

// One pass of Cichocki-Phan HALS over the rows of one mode, fp64. A workgroup is ONE wave and owns a
// tile of 64 rows, a lane one row. Every workgroup forms S = Hadamard of the other modes' Grams
// + lambda I in LDS itself (N R^2 reads out of L2: nothing beside a launch), so no launch precedes this one.
//
// The lane's row lives in LDS, not in registers: sW[q * 64 + lane], so the 64 lanes of a read hit 64
// consecutive doubles (no bank conflict) and the rolled loops index it by q. A register array would
// need both loops unrolled — 2 * 64 * 64 multiply-adds of straight-line code at R = 64, more than
// the instruction cache — and one instantiation per rank bound. S[q, r] is the same address for
// every lane: an LDS broadcast. LDS: (R^2 + 64 R) doubles = 64 KB at R = 64, two workgroups per CU.
//
//   grad[x, r] = -M[x, r] + sum_q w_old[x, q] S[q, r]                       (pre-update row)
//   w[x, r]   <- max(nn_floor, w[x, r] + (M[x, r] - sum_q w[x, q] S[q, r]) / S[r, r])   r = 0 .. R-1
// (the second sum sees the entries already updated, q < r); a column whose S[r, r] is not a positive
// finite number stays. A lane reads and writes its own row of W only, so W is updated in place.
// gradsq_part[workgroup] = the tile's sum of grad^2, lanes added in the fixed order of wave_sum;
// k_sum_partials adds the tiles. Workgroup 0 stores S when asked.
//
// blockIdx.y is the start of a multi-start session (R columns per start, the layout of
// k_cp_mode_update_batched): start b reads its N Grams at Gall + b N R^2, owns columns [b R, (b+1) R) of M,
// W and grad, writes its tiles' sums to gradsq_part[b * gridDim.x + tile] and its S to S_out + b R^2.
// Nothing is shared between two starts. An ordinary session launches gridDim.y == 1: every offset is 0.
// (the body, for ONE workgroup on one start's pointers: k_cp_update_nn and k_cp_update_nn_ragged below)
__device__ __forceinline__ void cp_update_nn_body(
    const double *__restrict__ Gall, int N, int mode, int R, double lambda,
    const double *__restrict__ M, int64_t ldm, double *__restrict__ W, int64_t ldw,
    double *__restrict__ grad, int64_t ldg, int64_t rows, double *__restrict__ gradsq_part,
    double *__restrict__ S_out, double nn_floor) {
  extern __shared__ double lds[];
  double *sS = lds;           // R x R, column-major (symmetric)
  double *sW = lds + R * R;   // R x 64: the tile's rows, column q of lane l at q * 64 + l
  const int lane = threadIdx.x;
  for (int e = lane; e < R * R; e += 64) {
    const double v = hadamard_entry(Gall, N, mode, R, lambda, e);
    sS[e] = v;
    if (S_out && blockIdx.x == 0) S_out[e] = v;
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
    for (int r = 0; r < R; r++) {
      const double *sc = sS + r * R;
      const double d = sc[r];
      if (!(d > 0.0) || d > 1.79769313486231570e308) continue;
      double acc = 0;
      for (int q = 0; q < R; q++) acc += sW[q * 64 + lane] * sc[q];
      const double v = sW[r * 64 + lane] + (M[x + ldm * r] - acc) / d;
      const double w = v > nn_floor ? v : nn_floor;
      sW[r * 64 + lane] = w;
      W[x + ldw * r] = w;
    }
  }
  gs = wave_sum(gs);
  if (lane == 0) gradsq_part[blockIdx.x] = gs;
}

__global__ __launch_bounds__(64) void k_cp_update_nn(
    const double *__restrict__ Gall, int N, int mode, int R, double lambda,
    const double *__restrict__ M, int64_t ldm, double *__restrict__ W, int64_t ldw,
    double *__restrict__ grad, int64_t ldg, int64_t rows, double *__restrict__ gradsq_part,
    double *__restrict__ S_out, double nn_floor) {
  const int64_t b = blockIdx.y;
  cp_update_nn_body(Gall + b * N * R * R, N, mode, R, lambda, M + b * R * ldm, ldm, W + b * R * ldw, ldw,
                    grad + b * R * ldg, ldg, rows, gradsq_part + b * gridDim.x, S_out ? S_out + b * R * R : nullptr,
                    nn_floor);
}
// Rank-sweep sessions: blockIdx.y is a start of its own rank (StartTable by value, as
// k_cp_mode_update_ragged): R_b columns from col[b], Grams at Gall + N sq[b], S to S_out + sq[b]. The
// launch's LDS is sized for the largest rank; a start uses the front of it.
__global__ __launch_bounds__(64) void k_cp_update_nn_ragged(
    const double *__restrict__ Gall, int N, int mode, StartTable t, double lambda,
    const double *__restrict__ M, int64_t ldm, double *__restrict__ W, int64_t ldw,
    double *__restrict__ grad, int64_t ldg, int64_t rows, double *__restrict__ gradsq_part,
    double *__restrict__ S_out, double nn_floor) {
  const int b = blockIdx.y;
  const int64_t c0 = t.col[b], so = t.sq[b];
  cp_update_nn_body(Gall + N * so, N, mode, t.col[b + 1] - t.col[b], lambda, M + c0 * ldm, ldm, W + c0 * ldw, ldw,
                    grad + c0 * ldg, ldg, rows, gradsq_part + (int64_t)b * gridDim.x, S_out ? S_out + so : nullptr,
                    nn_floor);
}

// What follows the row kernel in a multi-start session, for all starts in ONE launch: workgroup b adds
// start b's `ntiles` tile sums into gradsq[b] (the order of k_sum_partials) and refreshes start b's Gram
// of the new W into Gall (the per-pair order of k_gram: 16 waves share the R (R + 1) / 2 pairs).
__global__ __launch_bounds__(1024) void k_cp_finish_nn_batched(
    const double *__restrict__ part, int ntiles, double *__restrict__ gradsq, const double *__restrict__ W,
    int64_t ldw, int64_t rows, int R, int N, int mode, double *__restrict__ Gall) {
  __shared__ double lds[17];
  const int64_t b = blockIdx.x;
  part += b * ntiles;
  double s = 0;
  for (int i = threadIdx.x; i < ntiles; i += blockDim.x) s += part[i];
  s = block_sum(s, lds);
  if (threadIdx.x == 0) gradsq[b] = s;
  gram_pairs(W + b * R * ldw, rows, ldw, R, Gall + (b * N + mode) * R * R, threadIdx.x >> 6, blockDim.x >> 6);
}

// The same for starts of different ranks (after k_cp_update_nn_ragged).
__global__ __launch_bounds__(1024) void k_cp_finish_nn_ragged(
    const double *__restrict__ part, int ntiles, double *__restrict__ gradsq, const double *__restrict__ W,
    int64_t ldw, int64_t rows, StartTable t, int N, int mode, double *__restrict__ Gall) {
  __shared__ double lds[17];
  const int b = blockIdx.x;
  const int R = t.col[b + 1] - t.col[b];
  part += (int64_t)b * ntiles;
  double s = 0;
  for (int i = threadIdx.x; i < ntiles; i += blockDim.x) s += part[i];
  s = block_sum(s, lds);
  if (threadIdx.x == 0) gradsq[b] = s;
  gram_pairs(W + (int64_t)t.col[b] * ldw, rows, ldw, R, Gall + (int64_t)N * t.sq[b] + (int64_t)mode * R * R,
             threadIdx.x >> 6, blockDim.x >> 6);
}

}  // namespace ppals
