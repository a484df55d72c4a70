// kernels_slices.hip.h — the small kernels of the influence plot (Ops::residual_slices, fold_slice_sums,
// row_dots; include/ppals.h, "per-slice residuals and leverages"). The fused tensor pass is a MODE of
// k_rank_mfma (kernels_scan.hip.h); here: the general pass for what that one does not take, the fold of
// the partial sums of either, and the two kernels behind the pass. All sums fp64, no atomics, every
// order fixed by the geometry alone.
//
// Partial layout of a tensor pass (both routes), for one SLAB — nt consecutive row tiles (rows [row0, row0 +
// rows)) by nc consecutive k-chunks (columns [kc0, kc0 + kcols)):
//   rowpart[c * rp_ld + (m - row0)]   the sum of e^2 of row m over the columns of the slab's chunk c
//   colpart[t * cp_ld + (k - kc0)]    the sum of e^2 of column k over the rows of the slab's tile t
// (row0 and kc0 follow from the slab's first tile and chunk, which the pass kernels are told). k_slice_fold adds them
// in index order ONTO what the slabs before left: rowsq[m] is one running sum over all k-chunks in chunk
// order, colsq[k] one over all row tiles in tile order — however the tiles and chunks are cut into slabs.
// A pass of many k-chunks (few row tiles: up to 16 x the compute units of chunks) first adds every G consecutive
// chunks of a row (k_slice_group; G by the geometry alone, at most 64 groups, slabs cut at multiples of G), and
// the running sum is over the groups: a chain of at most G + 64 additions a row instead of one per chunk.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_small.hip.h"

namespace ppals {

constexpr int kSliceCols = 32;  // columns between two flushes of the general pass

// The general pass (bf16 storage, R > 32, odd M, an unaligned shard): a thread per row, 256 rows a
// workgroup, blockIdx.y = a chunk of kch columns (a multiple of kSliceCols). The thread keeps its row's sum
// over the chunk; a column's sum goes over the wave by shuffles, then over the four waves through LDS in
// wave order, kSliceCols columns per pair of barriers. RB > 0: the row of Q in RB registers (R <= RB);
// RB == 0: any rank, Q re-read per column (cache-resident). Correct, not fast.
template <typename TV, int RB>
__global__ __launch_bounds__(256) void k_slice_stream(const TV *__restrict__ V, int64_t M, int64_t K,
                                                      const double *__restrict__ Q,
                                                      const double *__restrict__ P, int R, int64_t kch,
                                                      int64_t tile0, int64_t chunk0, int64_t rp_ld,
                                                      int64_t cp_ld, double *__restrict__ rowpart,
                                                      double *__restrict__ colpart) {
  __shared__ double cs[4][kSliceCols];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t m = (tile0 + blockIdx.x) * 256 + threadIdx.x;
  const int64_t k0 = (chunk0 + blockIdx.y) * kch;
  const int64_t k1 = min(K, k0 + kch);
  const bool ok = m < M;
  double q[RB > 0 ? RB : 1];
  if constexpr (RB > 0) {
#pragma unroll
    for (int r = 0; r < RB; r++) q[r] = (ok && r < R) ? Q[m + M * r] : 0.0;
  }
  double racc = 0;
  for (int64_t kf = k0; kf < k1; kf += kSliceCols) {  // (uniform over the workgroup)
    const int nc = (int)min((int64_t)kSliceCols, k1 - kf);
    for (int c = 0; c < nc; c++) {
      const int64_t k = kf + c;
      double e2 = 0;
      if (ok) {
        double v = 0;
        if constexpr (RB > 0) {
#pragma unroll
          for (int r = 0; r < RB; r++)
            if (r < R) v += q[r] * P[k + K * r];
        } else {
          for (int r = 0; r < R; r++) v += Q[m + M * r] * P[k + K * r];
        }
        const double d = (double)V[m + M * k] - v;
        e2 = d * d;
      }
      racc += e2;
      const double w = wave_sum(e2);
      if (lane == 0) cs[wave][c] = w;
    }
    __syncthreads();
    if ((int)threadIdx.x < nc)
      colpart[(int64_t)blockIdx.x * cp_ld + (kf - chunk0 * kch) + threadIdx.x] =
          ((cs[0][threadIdx.x] + cs[1][threadIdx.x]) + cs[2][threadIdx.x]) + cs[3][threadIdx.x];
    __syncthreads();
  }
  if (ok) rowpart[(int64_t)blockIdx.y * rp_ld + (m - tile0 * 256)] = racc;
}

// the partial sums of one slab onto rowsq / colsq, in index order (layout at the top of this file);
// first_c / first_t != 0: the slab holds the first k-chunk / the first row tile (that sum starts from zero)
__global__ void k_slice_fold(const double *__restrict__ rowpart, int64_t nc, int64_t rp_ld, int64_t rows,
                             int64_t row0, int first_c, const double *__restrict__ colpart, int64_t nt,
                             int64_t cp_ld, int64_t kcols, int64_t kc0, int first_t,
                             double *__restrict__ rowsq, double *__restrict__ colsq) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < rows + kcols;
       e += (int64_t)gridDim.x * blockDim.x) {
    if (e < rows) {
      double s = first_c ? 0.0 : rowsq[row0 + e];
      for (int64_t c = 0; c < nc; c++) s += rowpart[c * rp_ld + e];
      rowsq[row0 + e] = s;
    } else {
      const int64_t k = e - rows;
      double s = first_t ? 0.0 : colsq[kc0 + k];
      for (int64_t t = 0; t < nt; t++) s += colpart[t * cp_ld + k];
      colsq[kc0 + k] = s;
    }
  }
}

// grp[g * rp_ld + r] = the sum of rowpart[c * rp_ld + r] over the chunks c of the slab's group g, in chunk order
__global__ void k_slice_group(const double *__restrict__ rowpart, int64_t nc, int64_t G, int64_t rp_ld,
                              int64_t rows, double *__restrict__ grp) {
  const int64_t ng = (nc + G - 1) / G;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < ng * rows;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t g = e / rows, r = e % rows, c1 = min(nc, (g + 1) * G);
    double s = 0;
    for (int64_t c = g * G; c < c1; c++) s += rowpart[c * rp_ld + r];
    grp[g * rp_ld + r] = s;
  }
}

// part[b] = sum x[b seg .. min(n, (b + 1) seg)): every thread its strided share in ascending order, then
// block_sum; k_sum_partials adds the parts
__global__ __launch_bounds__(256) void k_slice_total_parts(const double *__restrict__ x, int64_t n, int64_t seg,
                                                           double *__restrict__ part) {
  __shared__ double lds[17];
  const int64_t i0 = (int64_t)blockIdx.x * seg, i1 = min(n, i0 + seg);
  double s = 0;
  for (int64_t i = i0 + threadIdx.x; i < i1; i += blockDim.x) s += x[i];
  s = block_sum(s, lds);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// Ops::fold_slice_sums: workgroup b owns one output entry — index x of the j-th mode of the group — and
// adds the total / lens[j] entries of src whose j-th index is x: every thread its strided share in
// ascending order, then block_sum.
struct SliceFoldArgs {
  int64_t lens[MAX_ORDER];
  int n;
};
__global__ __launch_bounds__(256) void k_fold_slice_sums(const double *__restrict__ src, SliceFoldArgs a,
                                                         double *__restrict__ out) {
  __shared__ double lds[17];
  int64_t x = blockIdx.x, stride = 1, total = 1;
  int j = 0;
  while (j < a.n - 1 && x >= a.lens[j]) {
    x -= a.lens[j];
    stride *= a.lens[j];
    j++;
  }
  for (int i = 0; i < a.n; i++) total *= a.lens[i];
  const int64_t cnt = total / a.lens[j];
  double s = 0;
  for (int64_t e = threadIdx.x; e < cnt; e += blockDim.x)
    s += src[e % stride + stride * (x + a.lens[j] * (e / stride))];
  s = block_sum(s, lds);
  if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// Ops::row_dots: out[x] = sum_r P[x + ld r] W[x + ld r], r ascending
__global__ void k_row_dots(const double *__restrict__ P, const double *__restrict__ W, int64_t rows, int R,
                           int64_t ld, double *__restrict__ out) {
  for (int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; x < rows;
       x += (int64_t)gridDim.x * blockDim.x) {
    double s = 0;
    for (int r = 0; r < R; r++) s += P[x + ld * r] * W[x + ld * r];
    out[x] = s;
  }
}

}  // namespace ppals
