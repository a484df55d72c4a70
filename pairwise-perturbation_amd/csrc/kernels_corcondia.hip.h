// kernels_corcondia.hip.h — the factor side and the score of the core consistency diagnostic
// (CpEngine::core_consistency): the transposed pseudo-inverses P = W (W^T W)^-1 of every mode and start
// (Ops::cp_pinv_ragged) and sum (G - T)^2 of a start's core (Ops::core_score). All fp64.
// block_sum comes from kernels_small.hip.h.
#pragma once
#include "kernels_small.hip.h"

namespace ppals {

struct PinvArgs {
  const double *w[MAX_ORDER];
  double *p[MAX_ORDER];
  int64_t rows[MAX_ORDER];
};

// Workgroup (b, i, z) serves start b and mode i: it inverts the start's R_b x R_b Gram of that mode
// (Gall + N sq[b] + i R_b^2, as the session keeps it) in LDS by the in-place Gauss-Jordan sweeps of
// k_gram_system_lds — pivot row and column set aside, two barriers per pivot, no pivoting — and writes
//   P_i[x, col_b + r] = sum_q W_i[x, col_b + q] Ginv[q, r]
// for the row tiles z, z + gridDim.z, ... of 256 rows. The workgroups of one (b, i) invert the same
// matrix redundantly (R^3 flops against a launch), with the same bits, so none waits for another.
// A pivot that is not a positive finite number ends the sweeps (the test is made by every thread on the
// same LDS word: block-uniform): the block of P becomes zero and bad[b] = 1 — several workgroups may
// store that same 1. The table travels by value as in k_cp_mode_update_ragged.
// dynamic LDS: (Rmax^2 + 2 Rmax) doubles, Rmax the largest rank of the table (<= 64: 33.8 KB)
__global__ __launch_bounds__(256) void k_cp_pinv_ragged(const double *__restrict__ Gall, int N, StartTable t,
                                                        PinvArgs a, int *__restrict__ bad) {
  extern __shared__ __attribute__((aligned(16))) double lds_pinv[];
  const int b = blockIdx.x, mode = blockIdx.y;
  const int R = t.col[b + 1] - t.col[b];
  const int64_t c0 = t.col[b];
  double *A = lds_pinv;       // R x R, column-major
  double *prow = A + R * R;   // pivot row    A[k][*]
  double *pcol = prow + R;    // pivot column A[*][k]
  const int tid = threadIdx.x;
  const double *G = Gall + (int64_t)N * t.sq[b] + (int64_t)mode * R * R;
  for (int e = tid; e < R * R; e += blockDim.x) A[e] = G[e];
  __syncthreads();
  bool ok = true;
  for (int k = 0; k < R; k++) {
    const double p = A[k + R * k];
    if (tid < R) {
      prow[tid] = A[k + R * tid];
      pcol[tid] = A[tid + R * k];
    }
    __syncthreads();
    if (!(p > 0.0) || !(p <= 1.79769313486231570e308)) {  // the same word in every thread: uniform
      ok = false;
      break;
    }
    const double d = 1.0 / p;
    for (int e = tid; e < R * R; e += blockDim.x) {
      const int i = e % R, j = e / R;
      double v;
      if (i == k)
        v = (j == k) ? d : prow[j] * d;
      else if (j == k)
        v = -pcol[i] * d;
      else
        v = A[e] - pcol[i] * (prow[j] * d);
      A[e] = v;
    }
    __syncthreads();
  }
  if (ok) {  // symmetrise in place: the two triangles differ by rounding only
    for (int e = tid; e < R * R; e += blockDim.x) {
      const int i = e % R, j = e / R;
      if (i < j) {
        const double v = 0.5 * (A[i + R * j] + A[j + R * i]);
        A[i + R * j] = v;
        A[j + R * i] = v;
      }
    }
  } else if (tid == 0 && blockIdx.z == 0) {
    bad[b] = 1;
  }
  __syncthreads();
  const int64_t rows = a.rows[mode];
  const double *W = a.w[mode] + c0 * rows;
  double *P = a.p[mode] + c0 * rows;
  for (int64_t x0 = (int64_t)blockIdx.z * blockDim.x; x0 < rows; x0 += (int64_t)gridDim.z * blockDim.x) {
    const int64_t x = x0 + tid;
    if (x >= rows) continue;
    for (int r = 0; r < R; r++) {
      double acc = 0;
      if (ok)
        for (int q = 0; q < R; q++) acc += W[x + rows * q] * A[q + R * r];
      P[x + rows * r] = acc;
    }
  }
}

// ONE workgroup per launch, one launch per start: sum (G - T)^2 over the n = R^N entries of the core,
// T the superdiagonal of ones — entry e lies on it when e is a multiple of dstride = 1 + R + .. + R^(N-1).
// Thread t adds the entries t, t + 1024, ... in this order and block_sum adds the threads in its fixed
// order: the same core gives the same bits. *cc = 100 (1 - sum / R). *bad != 0: the start has no
// pseudo-inverse — *cc and every entry of the core become NaN.
__global__ __launch_bounds__(1024) void k_core_score(double *__restrict__ core, int64_t n, int R, int64_t dstride,
                                                     const int *__restrict__ bad, double *__restrict__ cc) {
  __shared__ double lds[17];
  const int tid = threadIdx.x;
  if (*bad) {  // (one word: block-uniform)
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    for (int64_t e = tid; e < n; e += blockDim.x) core[e] = nan;
    if (tid == 0) *cc = nan;
    return;
  }
  double s = 0;
  for (int64_t e = tid; e < n; e += blockDim.x) {
    const double d = core[e] - ((e % dstride) == 0 ? 1.0 : 0.0);
    s += d * d;
  }
  s = block_sum(s, lds);
  if (tid == 0) *cc = 100.0 * (1.0 - s / (double)R);
}

}  // namespace ppals
