// kernels_npls_wide.hip.h — the wide-column forms of the two tensor passes of N-PLS (Ops::npls_contract_wide /
// npls_slice_inner_wide; ppals_tensor_contract_columns / _slice_inner_columns, ppals_npls_crossval). The tensor is
// viewed as [L, I, T] around the sample mode, first index fastest, and only read:
//   contract:     Z[l,t,c] = sum_i   X[l,i,t] U[i,c]
//   slice_inner:  S[i,c]   = sum_l,t X[l,i,t] W[l,t,c]
// Both are GEMMs with one huge streamed operand and a thin fp64 one. X is widened to fp64 as stored; products and
// sums run on v_mfma_f64_16x16x4_f64 with the operand maps of kernels_parafac2.hip.h: A operand
// a[m = lane & 15][k = lane >> 4], B operand b[k = lane >> 4][n = lane & 15], D at (m = (lane >> 4) + 4 reg,
// n = lane & 15). A launch carries NT tiles of 16 columns (NT <= 4: 64 columns a read of X); padded rows and columns
// enter as zeros. Every sum runs in an order fixed by the shape, the tile count and the split, with no atomics; a
// split writes partial sums that k_npls_fold adds in split order.
//
// Two walks serve the four routes:
//   k_npls_wide_rows  after k_p2_project: the output rows are contiguous in X, the contracted index walks at stride
//                     s1. contract `wide.rows` (rows l, contracted i at stride L, a slab per t) and slice_inner
//                     `wide.lead` (L == 1: rows i, contracted t at stride I, t split over the blocks).
//   k_npls_wide_cols  after k_p2_compress: the contracted index is contiguous in X, the output index walks at stride
//                     s1. contract `wide.lead` (L == 1: contracted i, output t at stride I, i split over the blocks)
//                     and slice_inner `wide.rows` (contracted l, output i at stride L, accumulated over the slabs t,
//                     (l, t) split over the blocks).
#pragma once
#include "kernels_npls.hip.h"
#include "kernels_small.hip.h"

namespace ppals {

constexpr int NPLS_WIDE_COLS = 64;  // columns a read of X carries: four tiles of 16
constexpr int NPLS_WT = 64;         // output rows of a workgroup's tile
constexpr int NPLS_WCH = 32;        // the chunk of the contracted index staged in LDS
constexpr int NPLS_WLDX = 80;       // k_npls_wide_rows: leading dimension of the staged chunks [k][row], [k][column]
constexpr int NPLS_WLDC = 36;       // k_npls_wide_cols: leading dimension of the staged chunks [row][k], [column][k]
// (the pitches of kernels_parafac2.hip.h: 80 = 16 and 36 = 4 mod 32 bank pairs)

// Workgroup (tile, slab) = (blockIdx.x % tiles, blockIdx.x / tiles), split blockIdx.y of gridDim.y; 256 threads.
// out[row + n * slab + cstride * c + sstride * split] = sum over k in the split's range [K s / ns, K (s + 1) / ns) of
//   X[row + s1 * k + s2 * slab] * B[k + K * c],   row < n, c < nc <= 16 NT.
// Wave w owns rows [16 w, 16 w + 16) of the tile; X is read once, 64 consecutive rows per wave load. The tile goes
// through LDS on its way out so that a wave stores 64 consecutive rows of one column.
template <typename TX, int NT>
__global__ __launch_bounds__(256) void k_npls_wide_rows(const TX *__restrict__ X, int64_t s1, int64_t s2, int64_t n,
                                                        int64_t K, const double *__restrict__ B, int nc, int64_t tiles,
                                                        double *__restrict__ out, int64_t cstride, int64_t sstride) {
  constexpr int RP = 16 * NT;
  constexpr int STAGE = 2 * NPLS_WCH * NPLS_WLDX, GSZ = NPLS_WT * (RP + 1);
  __shared__ __attribute__((aligned(16))) double lds[STAGE > GSZ ? STAGE : GSZ];
  double *Xs = lds, *Bs = lds + NPLS_WCH * NPLS_WLDX, *Gs = lds;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l16 = lane & 15, g4 = lane >> 4;
  const int64_t slab = blockIdx.x / tiles, r0 = (int64_t)(blockIdx.x % tiles) * NPLS_WT;
  const int64_t k_lo = K * blockIdx.y / gridDim.y, k_hi = K * (blockIdx.y + 1) / gridDim.y;
  const TX *__restrict__ Xk = X + s2 * slab;
  f64x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; t++) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
  const int64_t xr = r0 + lane;  // the row this thread loads
  for (int64_t k0 = k_lo; k0 < k_hi; k0 += NPLS_WCH) {
    __syncthreads();  // the chunk before this one has been read
#pragma unroll
    for (int u = 0; u < NPLS_WCH / 4; u++) {
      const int kk = wave + 4 * u;
      const int64_t k = k0 + kk;
      Xs[kk * NPLS_WLDX + lane] = (xr < n && k < k_hi) ? (double)Xk[xr + s1 * k] : 0.0;
    }
    for (int e = tid; e < NPLS_WCH * RP; e += 256) {
      const int kk = e % NPLS_WCH, c = e / NPLS_WCH;
      const int64_t k = k0 + kk;
      Bs[kk * NPLS_WLDX + c] = (c < nc && k < k_hi) ? B[k + K * c] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int kc = 0; kc < NPLS_WCH; kc += 4) {
      const double a = Xs[(kc + g4) * NPLS_WLDX + 16 * wave + l16];
#pragma unroll
      for (int t = 0; t < NT; t++)
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Bs[(kc + g4) * NPLS_WLDX + 16 * t + l16], acc[t], 0, 0, 0);
    }
  }
  __syncthreads();  // the last chunk has been read: the tile takes its place
#pragma unroll
  for (int t = 0; t < NT; t++)
#pragma unroll
    for (int reg = 0; reg < 4; reg++) Gs[(16 * wave + g4 + 4 * reg) * (RP + 1) + 16 * t + l16] = acc[t][reg];
  __syncthreads();
  if (xr < n) {
    double *__restrict__ o = out + n * slab + sstride * blockIdx.y + xr;
    for (int c = wave; c < nc; c += 4) o[cstride * c] = Gs[lane * (RP + 1) + c];
  }
}

// Workgroup tile blockIdx.x of 64 output indices j, split blockIdx.y of gridDim.y; 256 threads. With nch =
// ceil(K / 32) chunks of the contracted index a slab and units = nch * slabs, the split takes the units
// [units s / ns, units (s + 1) / ns), unit u = chunk u % nch of slab u / nch:
// out[j + cstride * c + sstride * split] = sum over the split's (k, slab) of
//   X[k + s1 * j + s2 * slab] * B[k + K * slab + K * slabs * c],   j < n, c < nc <= 16 NT.
// Wave w owns the output indices [16 w, 16 w + 16) of the tile; X is read once, 32 consecutive k per half wave.
template <typename TX, int NT>
__global__ __launch_bounds__(256) void k_npls_wide_cols(const TX *__restrict__ X, int64_t s1, int64_t s2, int64_t n,
                                                        int64_t K, int64_t slabs, const double *__restrict__ B, int nc,
                                                        double *__restrict__ out, int64_t cstride, int64_t sstride) {
  constexpr int RP = 16 * NT;
  __shared__ __attribute__((aligned(16))) double lds[(NPLS_WT + RP) * NPLS_WLDC];
  double *Xs = lds, *Bs = lds + NPLS_WT * NPLS_WLDC;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l16 = lane & 15, g4 = lane >> 4;
  const int64_t j0 = (int64_t)blockIdx.x * NPLS_WT, bc = K * slabs;
  const int64_t nch = (K + NPLS_WCH - 1) / NPLS_WCH, units = nch * slabs;
  const int64_t u_lo = units * blockIdx.y / gridDim.y, u_hi = units * (blockIdx.y + 1) / gridDim.y;
  f64x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; t++) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
  const int lk = tid & 31, lj = tid >> 5;  // this thread's k of a chunk, and its first output index
  for (int64_t u = u_lo; u < u_hi; u++) {
    const int64_t slab = u / nch, k = (u % nch) * NPLS_WCH + lk;
    const TX *__restrict__ Xk = X + s2 * slab;
    const double *__restrict__ Bk = B + K * slab;
    __syncthreads();  // the chunk before this one has been read
#pragma unroll
    for (int q = 0; q < NPLS_WT / 8; q++) {
      const int jj = lj + 8 * q;
      const int64_t j = j0 + jj;
      Xs[jj * NPLS_WLDC + lk] = (k < K && j < n) ? (double)Xk[k + s1 * j] : 0.0;
    }
    for (int c = lj; c < RP; c += 8) Bs[c * NPLS_WLDC + lk] = (k < K && c < nc) ? Bk[k + bc * c] : 0.0;
    __syncthreads();
#pragma unroll
    for (int kc = 0; kc < NPLS_WCH; kc += 4) {
      const double b = Xs[(16 * wave + l16) * NPLS_WLDC + kc + g4];
#pragma unroll
      for (int t = 0; t < NT; t++)
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(Bs[(16 * t + l16) * NPLS_WLDC + kc + g4], b, acc[t], 0, 0, 0);
    }
  }
  const int64_t j = j0 + 16 * wave + l16;
  if (j < n) {
    double *__restrict__ o = out + sstride * blockIdx.y + j;
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
      for (int reg = 0; reg < 4; reg++) {
        const int c = 16 * t + g4 + 4 * reg;
        if (c < nc) o[cstride * c] = acc[t][reg];
      }
  }
}

}  // namespace ppals
