// kernels_parafac2.hip.h — the projection step of PARAFAC2 (Ops::parafac2_step) on a device
// view X of extents I x J x K with unit stride in mode 0, X_k = X[:, :, k]:
//   k_p2_project    Q_k = X_k A diag(C[k, :]) B^T          one pass over X, contraction over j
//   k_p2_polar      T_k = (Q_k^T Q_k)^(-1/2), status[k]    one workgroup per slice (polar_factor_body)
//   k_p2_apply      P_k = Q_k T_k where status[k] is 1
//   k_p2_compress   Y_k = P_k^T X_k                        one pass over X, contraction over i
//   k_p2_failed     the number of slices whose status is 0
// The ragged twins (k_p2_*_ragged, Ops::parafac2_step_ragged) run the same bodies on slices of unequal length:
// slice k has rows[k] rows, X_k[i, j] = X[xoff[k] + i + xcs[k] j], Q_k and P_k are column-major with leading
// dimension rows[k] at R roff[k], roff the prefix sum of rows. The grid of pass 1 and of the apply is the total
// number of row tiles, the slice slowest; a workgroup reads its slice from tile_slice[blockIdx.x] and its tile
// within the slice from tile0[slice], once, before its first chunk (one value per workgroup: scalar loads).
// The two passes over X widen its elements to fp64 and contract on v_mfma_f64_16x16x4_f64 with the operand
// maps of kernels_model.hip.h / kernels_fms.hip.h: A operand a[m = lane & 15][k = lane >> 4], B operand
// b[k = lane >> 4][n = lane & 15], D at (m = (lane >> 4) + 4 reg, n = lane & 15). The rank is padded to
// NT tiles of 16 (R <= 64: NT <= 4); padded rows and columns enter as zeros. Every sum runs in an order
// fixed by the shape alone, so the same state gives the same bits.
// block_sum and f64x4 come from kernels_small.hip.h, polar_factor_body from kernels_polar.hip.h.
#pragma once
#include "kernels_polar.hip.h"

namespace ppals {

constexpr int P2_TILE = 64;   // rows i of a projection tile, columns j of a compression tile
constexpr int P2_CH = 32;     // the chunk of the contracted index staged in LDS
constexpr int P2_LDX = 80;    // projection: leading dimension of the staged X chunk [j][i] and A chunk [j][r]
constexpr int P2_LDC = 36;    // compression: leading dimension of the staged X chunk [j][i] and P chunk [r][i]
// (80 = 16 mod 32 and 36 = 4 mod 32 bank pairs: the four k groups of an operand read, 16 lanes each, fall on
// bank pairs no more than two lanes share, which a 64-lane 8-byte read takes anyway)

__host__ __device__ inline size_t p2_project_lds(int R) {
  const int rp = (R + 15) / 16 * 16;
  const size_t stage = 2 * (size_t)P2_CH * P2_LDX;          // the X chunk and the A chunk
  const size_t g = (size_t)P2_TILE * (rp + 1);              // G in their place
  return sizeof(double) * ((stage > g ? stage : g) + (size_t)R * R);
}
__host__ __device__ inline size_t p2_compress_lds(int R) {
  const int rp = (R + 15) / 16 * 16;
  return sizeof(double) * ((size_t)P2_TILE * P2_LDC + (size_t)rp * P2_LDC + 17);
}

// Pass 1. Grid ceil(I / 64) x K (`tiles` row tiles per slice, the slice slowest), 256 threads. Wave w owns the
// rows [16 w, 16 w + 16) of the tile and NT accumulators G[16 rows][16 t ..]; X is read once, 64 consecutive i per
// wave load. The epilogue multiplies the
// 64 x R tile of G = X_k A by Mk = diag(C[k, :]) B^T (Mk[r][s] = C[k, r] B[s, r]) from LDS and stores
// Qk[i + I s] (k_p2_project: Qk = Q + I R k). The body serves both kernels; k, i0, Xk, s1 and I are one value
// per workgroup.
// dynamic LDS (p2_project_lds): Xs[32][80] | As[32][80], then G[64][16 NT + 1] in their place | Mk[R][R]
template <typename TX, int NT>
__device__ __forceinline__ void p2_project_body(const TX *__restrict__ Xk, int64_t s1, int64_t I, int64_t J, int R,
                                                const double *__restrict__ A, const double *__restrict__ B,
                                                const double *__restrict__ C, int64_t K, int64_t k, int64_t i0,
                                                double *__restrict__ Qk, double *lds_p2) {
  constexpr int RP = 16 * NT;
  const size_t stage = 2 * (size_t)P2_CH * P2_LDX, gsz = (size_t)P2_TILE * (RP + 1);
  double *Xs = lds_p2;
  double *As = Xs + P2_CH * P2_LDX;
  double *Gs = lds_p2;
  double *Mk = lds_p2 + (stage > gsz ? stage : gsz);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l16 = lane & 15, g4 = lane >> 4;
  for (int e = tid; e < R * R; e += 256) {
    const int r = e % R, s = e / R;
    Mk[e] = C[k + K * r] * B[s + (int64_t)R * r];
  }
  f64x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; t++) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
  const int64_t xi = i0 + lane;  // the row this thread loads
  for (int64_t j0 = 0; j0 < J; j0 += P2_CH) {
    __syncthreads();  // the chunk before this one has been read
#pragma unroll
    for (int u = 0; u < P2_CH / 4; u++) {
      const int jj = wave + 4 * u;
      const int64_t j = j0 + jj;
      Xs[jj * P2_LDX + lane] = (xi < I && j < J) ? (double)Xk[xi + s1 * j] : 0.0;
    }
    for (int e = tid; e < P2_CH * RP; e += 256) {
      const int jj = e % P2_CH, r = e / P2_CH;
      const int64_t j = j0 + jj;
      As[jj * P2_LDX + r] = (r < R && j < J) ? A[j + J * r] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int jc = 0; jc < P2_CH; jc += 4) {
      const double a = Xs[(jc + g4) * P2_LDX + 16 * wave + l16];
#pragma unroll
      for (int t = 0; t < NT; t++)
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, As[(jc + g4) * P2_LDX + 16 * t + l16], acc[t], 0, 0, 0);
    }
  }
  __syncthreads();  // the last chunk has been read: G takes its place
#pragma unroll
  for (int t = 0; t < NT; t++)
#pragma unroll
    for (int reg = 0; reg < 4; reg++) Gs[(16 * wave + g4 + 4 * reg) * (RP + 1) + 16 * t + l16] = acc[t][reg];
  __syncthreads();
  if (xi < I) {
    for (int s = wave; s < R; s += 4) {
      const double *mk = Mk + (size_t)R * s;
      double v = 0;
      for (int r = 0; r < R; r++) v += Gs[lane * (RP + 1) + r] * mk[r];
      Qk[xi + I * s] = v;
    }
  }
}
template <typename TX, int NT>
__global__ __launch_bounds__(256) void k_p2_project(const TX *__restrict__ X, int64_t s1, int64_t s2, int64_t I,
                                                    int64_t J, int R, const double *__restrict__ A,
                                                    const double *__restrict__ B, const double *__restrict__ C,
                                                    int64_t K, int tiles, double *__restrict__ Q) {
  extern __shared__ __attribute__((aligned(16))) double lds_p2[];
  const int64_t k = blockIdx.x / tiles, i0 = (int64_t)(blockIdx.x % tiles) * P2_TILE;
  p2_project_body<TX, NT>(X + s2 * k, s1, I, J, R, A, B, C, K, k, i0, Q + I * (int64_t)R * k, lds_p2);
}
// the ragged twin: grid = the total number of row tiles
template <typename TX, int NT>
__global__ __launch_bounds__(256) void k_p2_project_ragged(
    const TX *__restrict__ X, const int64_t *__restrict__ rows, const int64_t *__restrict__ roff,
    const int *__restrict__ tile0, const int *__restrict__ tile_slice, const int64_t *__restrict__ xoff,
    const int64_t *__restrict__ xcs, int64_t J, int R, const double *__restrict__ A, const double *__restrict__ B,
    const double *__restrict__ C, int64_t K, double *__restrict__ Q) {
  extern __shared__ __attribute__((aligned(16))) double lds_p2[];
  const int64_t k = tile_slice[blockIdx.x], i0 = (int64_t)((int)blockIdx.x - tile0[k]) * P2_TILE;
  p2_project_body<TX, NT>(X + xoff[k], xcs[k], rows[k], J, R, A, B, C, K, k, i0, Q + (int64_t)R * roff[k], lds_p2);
}

// The slice polar factors: workgroup k runs polar_factor_body on Q_k (I rows, leading dimension I) and writes
// T_k at T + R^2 k and status[k]. dynamic LDS: that of k_polar_factor.
__global__ __launch_bounds__(1024) void k_p2_polar(const double *__restrict__ Q, int64_t I, int R, double min_ratio,
                                                   double *__restrict__ T, int *__restrict__ status) {
  extern __shared__ double lds[];
  const int64_t k = blockIdx.x;
  polar_factor_body(Q + I * (int64_t)R * k, I, I, R, min_ratio, T + (int64_t)R * R * k, status + k, lds);
}
__global__ __launch_bounds__(1024) void k_p2_polar_ragged(const double *__restrict__ Q,
                                                          const int64_t *__restrict__ rows,
                                                          const int64_t *__restrict__ roff, int R, double min_ratio,
                                                          double *__restrict__ T, int *__restrict__ status) {
  extern __shared__ double lds[];
  const int64_t k = blockIdx.x, I = rows[k];
  polar_factor_body(Q + (int64_t)R * roff[k], I, I, R, min_ratio, T + (int64_t)R * R * k, status + k, lds);
}

// P_k = Q_k T_k for the slices whose status is 1; grid ceil(I / 64) x K as k_p2_project, 256 threads, a thread one
// row and every fourth column. dynamic LDS: T[R][R] | Q tile [R][64]
__device__ __forceinline__ void p2_apply_body(const double *__restrict__ Qk, const double *__restrict__ Tk,
                                              int64_t I, int R, int64_t i0, double *__restrict__ Pk, double *lds) {
  double *sT = lds, *sQ = lds + R * R;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t x = i0 + lane;
  for (int e = tid; e < R * R; e += 256) sT[e] = Tk[e];
  for (int q = wave; q < R; q += 4) sQ[q * 64 + lane] = x < I ? Qk[x + I * q] : 0.0;
  __syncthreads();
  if (x >= I) return;
  for (int s = wave; s < R; s += 4) {
    const double *tc = sT + R * s;
    double v = 0;
    for (int q = 0; q < R; q++) v += sQ[q * 64 + lane] * tc[q];
    Pk[x + I * s] = v;
  }
}
__global__ __launch_bounds__(256) void k_p2_apply(const double *__restrict__ Q, const double *__restrict__ T,
                                                  const int *__restrict__ status, int64_t I, int R, int tiles,
                                                  double *__restrict__ P) {
  extern __shared__ double lds[];
  const int64_t k = blockIdx.x / tiles;
  if (!status[k]) return;  // (one value per slice: uniform over the workgroup)
  p2_apply_body(Q + I * (int64_t)R * k, T + (int64_t)R * R * k, I, R, (int64_t)(blockIdx.x % tiles) * 64,
                P + I * (int64_t)R * k, lds);
}
__global__ __launch_bounds__(256) void k_p2_apply_ragged(const double *__restrict__ Q, const double *__restrict__ T,
                                                         const int *__restrict__ status,
                                                         const int64_t *__restrict__ rows,
                                                         const int64_t *__restrict__ roff,
                                                         const int *__restrict__ tile0,
                                                         const int *__restrict__ tile_slice, int R,
                                                         double *__restrict__ P) {
  extern __shared__ double lds[];
  const int64_t k = tile_slice[blockIdx.x];
  if (!status[k]) return;
  const int64_t o = (int64_t)R * roff[k];
  p2_apply_body(Q + o, T + (int64_t)R * R * k, rows[k], R, (int64_t)((int)blockIdx.x - tile0[k]) * 64, P + o, lds);
}

// Pass 2. Grid ceil(J / 64) x K (`tiles` column tiles per slice, the slice slowest), 256 threads. Wave w owns the
// columns [16 w, 16 w + 16) of the tile and NT accumulators Y[16 t ..][16 columns]; the contraction over i runs in
// chunks of 32 rows, X read once with 32 consecutive i per half wave, P_k tiled over i beside it. D (m = r, n = j)
// is rounded once to TY and stored at Y[r + R (j + J k)]. Every thread adds the squares of the X elements it loads
// and of the fp64 Y entries it holds; part[g] and part[gridDim.x + g], g = blockIdx.x, are the workgroup's sums.
// dynamic LDS (p2_compress_lds): Xs[64][36] | Ps[16 NT][36] | 17 doubles of block_sum
template <typename TX, typename TY, int NT>
__device__ __forceinline__ void p2_compress_body(const TX *__restrict__ Xk, int64_t s1, int64_t I, int64_t J, int R,
                                                 const double *__restrict__ Pk, int64_t k, int64_t j0,
                                                 TY *__restrict__ Y, double *__restrict__ part, double *lds_p2) {
  constexpr int RP = 16 * NT;
  double *Xs = lds_p2;
  double *Ps = Xs + P2_TILE * P2_LDC;
  double *red = Ps + RP * P2_LDC;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l16 = lane & 15, g4 = lane >> 4;
  f64x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; t++) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
  double sx = 0, sy = 0;
  const int li = tid & 31, lj = tid >> 5;  // this thread's row of a chunk, and its first column
  for (int64_t i0 = 0; i0 < I; i0 += P2_CH) {
    __syncthreads();  // the chunk before this one has been read
    const int64_t i = i0 + li;
#pragma unroll
    for (int u = 0; u < P2_TILE / 8; u++) {
      const int jj = lj + 8 * u;
      const int64_t j = j0 + jj;
      const double v = (i < I && j < J) ? (double)Xk[i + s1 * j] : 0.0;
      Xs[jj * P2_LDC + li] = v;
      sx += v * v;
    }
    for (int r = lj; r < RP; r += 8) Ps[r * P2_LDC + li] = (i < I && r < R) ? Pk[i + I * r] : 0.0;
    __syncthreads();
#pragma unroll
    for (int ic = 0; ic < P2_CH; ic += 4) {
      const double b = Xs[(16 * wave + l16) * P2_LDC + ic + g4];
#pragma unroll
      for (int t = 0; t < NT; t++)
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(Ps[(16 * t + l16) * P2_LDC + ic + g4], b, acc[t], 0, 0, 0);
    }
  }
  const int64_t j = j0 + 16 * wave + l16;
  if (j < J) {
    TY *__restrict__ y = Y + (int64_t)R * (j + J * k);
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
      for (int reg = 0; reg < 4; reg++) {
        const int r = 16 * t + g4 + 4 * reg;
        if (r < R) {
          const double v = acc[t][reg];
          sy += v * v;
          y[r] = (TY)v;
        }
      }
  }
  sx = block_sum(sx, red);
  sy = block_sum(sy, red);
  if (tid == 0) {
    part[blockIdx.x] = sx;
    part[(int64_t)gridDim.x + blockIdx.x] = sy;
  }
}
template <typename TX, typename TY, int NT>
__global__ __launch_bounds__(256) void k_p2_compress(const TX *__restrict__ X, int64_t s1, int64_t s2, int64_t I,
                                                     int64_t J, int R, const double *__restrict__ P, int tiles,
                                                     TY *__restrict__ Y, double *__restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) double lds_p2[];
  const int64_t k = blockIdx.x / tiles, j0 = (int64_t)(blockIdx.x % tiles) * P2_TILE;
  p2_compress_body<TX, TY, NT>(X + s2 * k, s1, I, J, R, P + I * (int64_t)R * k, k, j0, Y, part, lds_p2);
}
// the ragged twin: the same grid, the contraction of slice k runs to rows[k]
template <typename TX, typename TY, int NT>
__global__ __launch_bounds__(256) void k_p2_compress_ragged(const TX *__restrict__ X,
                                                            const int64_t *__restrict__ rows,
                                                            const int64_t *__restrict__ roff,
                                                            const int64_t *__restrict__ xoff,
                                                            const int64_t *__restrict__ xcs, int64_t J, int R,
                                                            const double *__restrict__ P, int tiles,
                                                            TY *__restrict__ Y, double *__restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) double lds_p2[];
  const int64_t k = blockIdx.x / tiles, j0 = (int64_t)(blockIdx.x % tiles) * P2_TILE;
  p2_compress_body<TX, TY, NT>(X + xoff[k], xcs[k], rows[k], J, R, P + (int64_t)R * roff[k], k, j0, Y, part, lds_p2);
}

// the number of slices that kept their projection, as a double beside the two sums
__global__ __launch_bounds__(1024) void k_p2_failed(const int *__restrict__ status, int64_t K,
                                                    double *__restrict__ out) {
  __shared__ double red[17];
  double n = 0;
  for (int64_t k = threadIdx.x; k < K; k += blockDim.x) n += status[k] ? 0.0 : 1.0;
  n = block_sum(n, red);
  if (threadIdx.x == 0) *out = n;
}

// the first R columns of the identity in every I x R slice of P
__global__ void k_p2_init(double *__restrict__ P, int64_t I, int R, int64_t K) {
  const int64_t total = I * R * K;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = e % I, r = (e / I) % R;
    P[e] = i == r ? 1.0 : 0.0;
  }
}

// the same in every rows[k] x R slice of a ragged P: grid = the total number of row tiles, 256 threads
__global__ __launch_bounds__(256) void k_p2_init_ragged(double *__restrict__ P, const int64_t *__restrict__ rows,
                                                        const int64_t *__restrict__ roff,
                                                        const int *__restrict__ tile0,
                                                        const int *__restrict__ tile_slice, int R) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t k = tile_slice[blockIdx.x], I = rows[k];
  const int64_t x = (int64_t)((int)blockIdx.x - tile0[k]) * 64 + lane;
  if (x >= I) return;
  double *__restrict__ Pk = P + (int64_t)R * roff[k];
  for (int s = wave; s < R; s += 4) Pk[x + I * s] = x == s ? 1.0 : 0.0;
}

}  // namespace ppals
