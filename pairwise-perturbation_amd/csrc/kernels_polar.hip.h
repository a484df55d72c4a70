// kernels_polar.hip.h — the orthonormal mode update of a CP session (Ops::cp_mode_update_ortho_ragged):
// W <- M (M^T M)^(-1/2), the orthonormal polar factor of the mode's MTTKRP, for every start of a session
// in three launches whatever the number of starts, the ranks and the rows.
// gram_pairs, hadamard_entry, jacobi_eig_t, wave_sum and block_sum come from kernels_small.hip.h; the third
// launch is k_cp_finish_nn_ragged of kernels_nn.hip.h (tile sums and the Gram of the new W).
#pragma once
#include "kernels_nn.hip.h"

namespace ppals {

// Launch 1, one 1024-thread workgroup per start (StartTable by value, as k_cp_update_nn_ragged): the Gram
// route to the polar factor.
//   C = M_b^T M_b over all rows, every pair's sum in the order of gram_pairs (16 waves share the pairs);
//   C = U diag(theta) U^T by the parallel-ordered cyclic Jacobi of jacobi_eig_t, in LDS;
//   status[b] = 1 when the Jacobi converged, every theta is a positive finite number and
//   theta_min > theta_max * min_ratio (PPALS_ORTHO_MIN_RATIO), else 0: the start's factor then stays, and T
//   is not written;
//   T_b = U diag(theta^-1/2) U^T (R_b x R_b, symmetric, column-major) at T + sq[b].
// dynamic LDS: A[R][R+1], Q[R][R+1] | cs[64] doubles | red[18] doubles | pq[64] ints, R the largest rank
// of the launch — 67.5 KB at R = 64, so one workgroup per CU; a start of a smaller rank uses the front.
// C is gathered in Q's place with leading dimension R before the Jacobi initialises Q.
// (polar_factor_body: the workgroup's work on one matrix M of R columns, so that the slice polar factors of
// PARAFAC2, kernels_parafac2.hip.h, run the same code on a batch that a StartTable cannot carry)
__device__ inline void polar_factor_body(const double *__restrict__ M, int64_t ldm, int64_t rows, int R,
                                         double min_ratio, double *__restrict__ Tb, int *__restrict__ status_b,
                                         double *lds) {
  const int ldA = R + 1;
  double *A = lds;
  double *Q = A + R * ldA;
  double *cs = Q + R * ldA;
  double *red = cs + 64;
  int *pq = (int *)(red + 18);
  const int tid = threadIdx.x;
  gram_pairs(M, rows, ldm, R, Q, tid >> 6, blockDim.x >> 6);
  __syncthreads();
  for (int e = tid; e < R * R; e += blockDim.x) A[(e % R) * ldA + e / R] = Q[e];
  __syncthreads();
  jacobi_eig_t<1024>(A, Q, cs, pq, R, red);
  // jacobi_eig_t gives up after its last sweep without saying so: its own stopping test once more, so that a
  // C it did not diagonalise (NaNs, in practice) leaves the factor alone instead of yielding a wrong T
  double off = 0, dg = 0;
  for (int e = tid; e < R * R; e += blockDim.x) {
    const int i = e % R, j = e / R;
    const double a = A[i * ldA + j];
    if (i == j)
      dg += a * a;
    else
      off += a * a;
  }
  off = block_sum(off, red);
  dg = block_sum(dg, red);
  // the rule on theta: every thread reads the same sums and the same R diagonal entries, so `good` is uniform
  bool good = off <= 1e-30 * dg || off == 0.0;
  double tmin = 1.79769313486231570e308, tmax = 0.0;
  for (int k = 0; k < R; k++) {
    const double th = A[k * ldA + k];
    if (!(th > 0.0) || th > 1.79769313486231570e308) good = false;
    tmin = th < tmin ? th : tmin;
    tmax = th > tmax ? th : tmax;
  }
  if (good && tmin <= tmax * min_ratio) good = false;
  if (tid == 0) *status_b = good ? 1 : 0;
  if (!good) return;
  if (tid < R) cs[tid] = 1.0 / sqrt(A[tid * ldA + tid]);
  __syncthreads();
  for (int e = tid; e < R * R; e += blockDim.x) {  // T[i, j] = sum_k U[i, k] U[j, k] / sqrt(theta_k)
    const int i = e % R, j = e / R;
    double acc = 0;
    for (int k = 0; k < R; k++) acc += Q[i * ldA + k] * cs[k] * Q[j * ldA + k];
    Tb[e] = acc;
  }
}
__global__ __launch_bounds__(1024) void k_polar_factor(const double *__restrict__ M, int64_t ldm, int64_t rows,
                                                      StartTable t, double min_ratio, double *__restrict__ T,
                                                      int *__restrict__ status) {
  extern __shared__ double lds[];
  const int b = blockIdx.x;
  polar_factor_body(M + (int64_t)t.col[b] * ldm, ldm, rows, t.col[b + 1] - t.col[b], min_ratio, T + t.sq[b],
                    status + b, lds);
}

// Launch 2, a grid of (row tiles x starts); a workgroup is ONE wave on a tile of 64 rows, a lane one row, with
// the LDS layout of cp_update_nn_body: S (then T) as R x R, the tile's rows of W_old (then of M) as
// sW[q * 64 + lane]. LDS: (R^2 + 64 R) doubles = 64 KB at R = 64.
//   grad[x, r] = -M[x, r] + sum_q w_old[x, q] S[q, r]      (as for every kind; lambda enters S only)
//   gradsq_part[b * tiles + tile] = the tile's sum of grad^2, lanes added in the order of wave_sum
//   w[x, r]   <- sum_q M[x, q] T[q, r]                      when status[b] is 1; untouched otherwise
// Tile 0 stores S when asked. A lane reads and writes its own row only; nothing is shared between starts.
__global__ __launch_bounds__(64) void k_cp_update_ortho_ragged(
    const double *__restrict__ Gall, int N, int mode, StartTable t, double lambda,
    const double *__restrict__ M, int64_t ldm, double *__restrict__ W, int64_t ldw,
    double *__restrict__ grad, int64_t ldg, int64_t rows, double *__restrict__ gradsq_part,
    double *__restrict__ S_out, const double *__restrict__ T, const int *__restrict__ status) {
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
  if (!status[b]) return;  // (one value per start: uniform over the workgroup)
  __syncthreads();
  for (int e = lane; e < R * R; e += 64) sS[e] = T[so + e];
  for (int q = 0; q < R; q++) sW[q * 64 + lane] = live ? M[x + ldm * q] : 0.0;
  __syncthreads();
  if (live) {
    for (int r = 0; r < R; r++) {
      const double *tc = sS + r * R;
      double acc = 0;
      for (int q = 0; q < R; q++) acc += sW[q * 64 + lane] * tc[q];
      W[x + ldw * r] = acc;
    }
  }
}

}  // namespace ppals
