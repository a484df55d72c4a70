// kernels_npls.hip.h — the tensor ops of N-PLS regression (ppals_npls_fit / _predict, ppals_tensor_contract_mode /
// _slice_inner; Bro, J. Chemometrics 10 (1996) 47-61). The tensor is viewed as [L, I, T] around the sample mode,
// first index fastest; it is only read.
//   contract:     Z[l,t,c] = sum_i   X[l,i,t] U[i,c]      U: I x C, Z: L T C, both fp64, column c at L T c
//   slice_inner:  S[i,c]   = sum_l,t X[l,i,t] W[l,t,c]    W: L T C, S: I x C
//   outer_axpy:   A[e] += alpha prod_k w_k[e_k]           A an fp64 array of order K
//   argmax:       the first index of the largest |Z[e]|; a non-finite entry counts as +inf
//
// Arithmetic: an element is read as stored and widened to fp64; every product is accumulated by an explicit
// fma, and every sum runs in an order that depends on the shape and the route only (no atomics): the same state
// gives the same bits. A launch carries up to CW columns, each in registers of its own and through the same code,
// so column c of a C-column call has the bits of that column computed alone (CW = 1 or NPLS_CW, the launcher
// chunks).
//
// The walks:
//   k_npls_contract_runs  L < 64 (L == 1 included) and one t, L I elements, fits the run buffer: a workgroup loads
//                         NT consecutive t — one contiguous piece of memory — into LDS in 16-byte accesses and
//                         sums the NT L fibres there, G lanes a fibre and a tree over the G; the chunk of U sits
//                         in LDS beside it while I CW doubles fit 16 KiB.
//   k_npls_contract_long  L == 1 and a fibre beyond the run buffer: a workgroup a fibre, a tree over 256 lanes.
//   k_npls_contract_rows  otherwise: a thread owns VEC consecutive l of one t and walks i at stride L; where L T gives
//                         too few threads for the device, i is split over grid.y and the partial sums are folded
//                         in split order.
//   k_npls_si_flat        L < 64: [L, I] is one contiguous run of J = L I elements a t. X lanes along the run, 256 / X
//                         rows of t, a partial sum per (block, r = l + L i); the fold adds the blocks and the l of
//                         one i. No lane idles on a small L.
//   k_npls_si_rows        L >= 64: a block per (4 slices i, b) after k_sumsq_rows, lanes along l (vector loads where L
//                         and the base allow), the blocks b split t and, where that leaves the device short of
//                         work, l; a partial sum per (block, i).
//   k_npls_fold           S[i,c] = sum over blocks, then over l, in that order.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "bf16.h"
#include "kernels_prep.hip.h"

namespace ppals {

constexpr int NPLS_CW = 4;                  // columns a launch carries in registers
constexpr int NPLS_RUN_BYTES = 32 * 1024;   // run buffer of k_npls_contract_runs
constexpr int NPLS_FLAT_L = 64;             // below: the flat walks
constexpr int NPLS_MAX_DIMS = 8;
constexpr int NPLS_IB = 4;                  // slices a block of k_npls_si_rows works on
constexpr int NPLS_ULDS_BYTES = 16 * 1024;  // k_npls_contract_runs keeps a chunk of U in LDS up to this

// ------------------------------------------------------------------ contract
// grid.y = ns splits of i (split s takes i in [I s / ns, I (s + 1) / ns)): column c of split s goes to
// out + cstride * c + sstride * s — Z itself for ns == 1, partial sums that k_npls_fold adds in split order otherwise
template <typename T, int VEC, int CW>
__global__ __launch_bounds__(PREP_THREADS) void k_npls_contract_rows(const T *__restrict__ X, int64_t L, int64_t I,
                                                                     int64_t Tn, const double *__restrict__ U, int nc,
                                                                     double *__restrict__ out, int64_t cstride,
                                                                     int64_t sstride) {
  typedef prep_vec<T, VEC> vec;
  const int64_t Lv = L / VEC, n = Lv * Tn;
  const int64_t i_lo = I * blockIdx.y / gridDim.y, i_hi = I * (blockIdx.y + 1) / gridDim.y;
  double *Z = out + sstride * blockIdx.y;
  for (int64_t e = (int64_t)blockIdx.x * PREP_THREADS + threadIdx.x; e < n; e += (int64_t)gridDim.x * PREP_THREADS) {
    const int64_t l0 = (e % Lv) * VEC, t = e / Lv;
    const T *xp = X + l0 + L * I * t;
    double acc[CW][VEC];
#pragma unroll
    for (int c = 0; c < CW; c++)
#pragma unroll
      for (int k = 0; k < VEC; k++) acc[c][k] = 0;
#pragma unroll 4
    for (int64_t i = i_lo; i < i_hi; i++) {
      vec x;
      if (VEC > 1) {
        x = *reinterpret_cast<const vec *>(xp + L * i);
      } else {
        x.v[0] = xp[L * i];
      }
#pragma unroll
      for (int c = 0; c < CW; c++)
        if (c < nc) {
          const double u = U[i + I * c];
#pragma unroll
          for (int k = 0; k < VEC; k++) acc[c][k] = fma((double)x.v[k], u, acc[c][k]);
        }
    }
#pragma unroll
    for (int c = 0; c < CW; c++)
      if (c < nc) {
#pragma unroll
        for (int k = 0; k < VEC; k++) Z[l0 + k + L * t + cstride * c] = acc[c][k];
      }
  }
}

// NT consecutive t a run (NT L I elements, contiguous), G lanes a fibre (a power of two; NT L G <= 256 unless G == 1)
template <typename T, int CW>
__global__ __launch_bounds__(PREP_THREADS) void k_npls_contract_runs(const T *__restrict__ X, int L, int I, int64_t Tn,
                                                                     int NT, int G, const double *__restrict__ U, int nc,
                                                                     int ulds, double *__restrict__ Z) {
  extern __shared__ __attribute__((aligned(16))) char prep_smem[];
  constexpr int V16 = PrepVec16<T>::N;
  double *red = reinterpret_cast<double *>(prep_smem);                    // [CW][256]
  double *us = red + PREP_THREADS * CW;                                   // [CW][I] if ulds: the columns of U
  T *img = reinterpret_cast<T *>(us + (ulds ? (CW * I + 1) / 2 * 2 : 0));  // [V16 + NT * L * I], 16-byte aligned
  const int tid = threadIdx.x, fs = tid / G, g = tid % G, fpb = PREP_THREADS / G, LI = L * I;
  const int64_t nruns = (Tn + NT - 1) / NT, LT = (int64_t)L * Tn;
  if (ulds) {
    for (int e = tid; e < CW * I; e += PREP_THREADS) us[e] = e / I < nc ? U[(int64_t)e] : 0.0;  // (column c at I c, as in U)
    __syncthreads();
  }
  const double *Up = ulds ? us : U;
  for (int64_t run = blockIdx.x; run < nruns; run += gridDim.x) {
    const int64_t t0 = run * NT;
    const int nt = (int)(Tn - t0 < NT ? Tn - t0 : NT), n = nt * LI, nf = nt * L;
    const T *gp = X + t0 * LI;
    const int head = (int)(((16 - ((uintptr_t)gp & 15)) & 15) / sizeof(T));
    T *s = img + (V16 - head % V16) % V16;
    prep_run_copy<T, true>(const_cast<T *>(gp), s, n, head);
    __syncthreads();
    for (int fb = 0; fb < nf; fb += fpb) {
      const int f = fb + fs;
      const bool live = f < nf;
      double acc[CW];
#pragma unroll
      for (int c = 0; c < CW; c++) acc[c] = 0;
      if (live) {
        const T *base = s + f % L + LI * (f / L);
        for (int i = g; i < I; i += G) {
          const double x = (double)base[L * i];
#pragma unroll
          for (int c = 0; c < CW; c++)
            if (c < nc) acc[c] = fma(x, Up[i + (int64_t)I * c], acc[c]);
        }
      }
      if (G > 1) {
#pragma unroll
        for (int c = 0; c < CW; c++) red[c * PREP_THREADS + tid] = acc[c];
        for (int h = G / 2; h > 0; h >>= 1) {
          __syncthreads();
          if (g < h) {
#pragma unroll
            for (int c = 0; c < CW; c++) red[c * PREP_THREADS + tid] += red[c * PREP_THREADS + tid + h];
          }
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < CW; c++) acc[c] = red[c * PREP_THREADS + tid];
        __syncthreads();
      }
      if (live && g == 0) {
#pragma unroll
        for (int c = 0; c < CW; c++)
          if (c < nc) Z[t0 * L + f + LT * c] = acc[c];
      }
    }
    __syncthreads();  // the image is reloaded by the next run
  }
}

template <typename T, int CW>
__global__ __launch_bounds__(PREP_THREADS) void k_npls_contract_long(const T *__restrict__ X, int64_t I, int64_t Tn,
                                                                     const double *__restrict__ U, int nc,
                                                                     double *__restrict__ Z) {
  extern __shared__ __attribute__((aligned(16))) char prep_smem[];
  double *red = reinterpret_cast<double *>(prep_smem);  // [256]
  for (int64_t t = blockIdx.x; t < Tn; t += gridDim.x) {
    const T *gp = X + I * t;
    double acc[CW];
#pragma unroll
    for (int c = 0; c < CW; c++) acc[c] = 0;
    for (int64_t i = threadIdx.x; i < I; i += PREP_THREADS) {
      const double x = (double)gp[i];
#pragma unroll
      for (int c = 0; c < CW; c++)
        if (c < nc) acc[c] = fma(x, U[i + I * c], acc[c]);
    }
#pragma unroll
    for (int c = 0; c < CW; c++) {
      const double s = prep_block_sum(acc[c], red);
      if (threadIdx.x == 0 && c < nc) Z[t + Tn * c] = s;
    }
  }
}

// ------------------------------------------------------------------ slice_inner
// block (rc, b); XL lanes along r = l + L i (a power of two), 256 / XL rows of t strided by the nb blocks
template <typename T, int CW>
__global__ __launch_bounds__(PREP_THREADS) void k_npls_si_flat(const T *__restrict__ X, int64_t L, int64_t J, int64_t Tn,
                                                               int XL, const double *__restrict__ W, int nc,
                                                               double *__restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) char prep_smem[];
  double *red = reinterpret_cast<double *>(prep_smem);  // [CW][256]
  const int x = threadIdx.x % XL, y = threadIdx.x / XL, Y = PREP_THREADS / XL;
  const int64_t r = (int64_t)blockIdx.x * XL + x, nb = gridDim.y, LT = L * Tn;
  double acc[CW];
#pragma unroll
  for (int c = 0; c < CW; c++) acc[c] = 0;
  if (r < J) {
    const int64_t l = r % L;
    for (int64_t t = (int64_t)blockIdx.y * Y + y; t < Tn; t += nb * Y) {
      const double v = (double)X[r + J * t];
      const double *wp = W + l + L * t;
#pragma unroll
      for (int c = 0; c < CW; c++)
        if (c < nc) acc[c] = fma(v, wp[LT * c], acc[c]);
    }
  }
#pragma unroll
  for (int c = 0; c < CW; c++) red[c * PREP_THREADS + threadIdx.x] = acc[c];
  __syncthreads();
  if (y == 0 && r < J) {
#pragma unroll
    for (int c = 0; c < CW; c++)
      if (c < nc) {
        double s = 0;
        for (int yy = 0; yy < Y; yy++) s += red[c * PREP_THREADS + x + XL * yy];
        part[((int64_t)blockIdx.y * CW + c) * J + r] = s;
      }
  }
}

// block (ig, b): NPLS_IB consecutive slices i share every load of W; b = bt * nbl + bl, XL lanes along l (a power of
// two), VEC elements a lane, l strided by the nbl blocks, 256 / XL rows of t strided by the gridDim.y / nbl blocks
template <typename T, int VEC, int CW>
__global__ __launch_bounds__(PREP_THREADS) void k_npls_si_rows(const T *__restrict__ X, int64_t L, int64_t I, int64_t Tn,
                                                               int XL, int nbl, const double *__restrict__ W, int nc,
                                                               double *__restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) char prep_smem[];
  double *red = reinterpret_cast<double *>(prep_smem);  // [256]
  typedef prep_vec<T, VEC> vec;
  const int x = threadIdx.x % XL, y = threadIdx.x / XL, Y = PREP_THREADS / XL;
  const int64_t i0 = (int64_t)blockIdx.x * NPLS_IB, Lv = L / VEC, LT = L * Tn;
  const int64_t nbt = gridDim.y / nbl, bt = blockIdx.y / nbl, bl = blockIdx.y % nbl;
  const int ni = (int)(I - i0 < NPLS_IB ? I - i0 : NPLS_IB);
  double acc[NPLS_IB][CW];
#pragma unroll
  for (int q = 0; q < NPLS_IB; q++)
#pragma unroll
    for (int c = 0; c < CW; c++) acc[q][c] = 0;
  for (int64_t t = bt * Y + y; t < Tn; t += nbt * Y) {
    const T *gp = X + L * (i0 + I * t);
    const double *wp = W + L * t;
    for (int64_t l = bl * XL + x; l < Lv; l += (int64_t)nbl * XL) {
      vec a[NPLS_IB];
#pragma unroll
      for (int q = 0; q < NPLS_IB; q++)
        if (q < ni) {
          if (VEC > 1) {
            a[q] = *reinterpret_cast<const vec *>(gp + L * q + l * VEC);
          } else {
            a[q].v[0] = gp[L * q + l];
          }
        }
#pragma unroll
      for (int k = 0; k < VEC; k++)
#pragma unroll
        for (int c = 0; c < CW; c++)
          if (c < nc) {
            const double w = wp[l * VEC + k + LT * c];
#pragma unroll
            for (int q = 0; q < NPLS_IB; q++)
              if (q < ni) acc[q][c] = fma((double)a[q].v[k], w, acc[q][c]);
          }
    }
  }
#pragma unroll
  for (int q = 0; q < NPLS_IB; q++)
#pragma unroll
    for (int c = 0; c < CW; c++) {
      const double s = prep_block_sum(acc[q][c], red);
      if (threadIdx.x == 0 && c < nc && q < ni) part[((int64_t)blockIdx.y * CW + c) * I + i0 + q] = s;
    }
}

// S[i + I c] = sum_b sum_l part[(b CW + c) L I + l + L i], b outer, l inner
__global__ void k_npls_fold(const double *__restrict__ part, int nb, int CW, int64_t L, int64_t I, int nc,
                            double *__restrict__ S) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < I; i += (int64_t)gridDim.x * blockDim.x)
    for (int c = 0; c < nc; c++) {
      double s = 0;
      for (int b = 0; b < nb; b++) {
        const double *p = part + ((int64_t)b * CW + c) * L * I + L * i;
        for (int64_t l = 0; l < L; l++) s += p[l];
      }
      S[i + I * c] = s;
    }
}

// ------------------------------------------------------------------ outer_axpy
struct NplsOuter {
  int K;
  int64_t ext[NPLS_MAX_DIMS];
  const double *w[NPLS_MAX_DIMS];
};
__global__ void k_npls_outer_axpy(double *__restrict__ A, int64_t n, NplsOuter o, double alpha) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    int64_t rem = e;
    double p = 1.0;
    for (int k = 0; k < o.K; k++) {
      const int64_t ik = rem % o.ext[k];
      rem /= o.ext[k];
      p = k == 0 ? o.w[0][ik] : p * o.w[k][ik];
    }
    A[e] = fma(alpha, p, A[e]);
  }
}

// ------------------------------------------------------------------ argmax of |Z|
__device__ __forceinline__ double npls_mag(double z) {
  const double a = fabs(z);
  return a <= 1.7976931348623157e308 ? a : __longlong_as_double(0x7ff0000000000000LL);  // NaN and inf alike
}
__device__ __forceinline__ bool npls_better(double a, int64_t ia, double b, int64_t ib) {
  return a > b || (a == b && ia < ib);
}
// the block's best (value, index) in a tree; rv / ri: 256 entries of LDS each
__device__ __forceinline__ void npls_block_best(double &v, int64_t &ix, double *rv, int64_t *ri) {
  const int tid = threadIdx.x;
  rv[tid] = v;
  ri[tid] = ix;
  for (int s = PREP_THREADS / 2; s > 0; s >>= 1) {
    __syncthreads();
    if (tid < s && npls_better(rv[tid + s], ri[tid + s], rv[tid], ri[tid])) {
      rv[tid] = rv[tid + s];
      ri[tid] = ri[tid + s];
    }
  }
  __syncthreads();
  v = rv[0];
  ix = ri[0];
}
// pv / pi: one entry a block. An empty thread holds (-1, n): every entry beats it.
__global__ __launch_bounds__(PREP_THREADS) void k_npls_argmax_part(const double *__restrict__ Z, int64_t n,
                                                                   double *__restrict__ pv, int64_t *__restrict__ pi) {
  __shared__ double rv[PREP_THREADS];
  __shared__ int64_t ri[PREP_THREADS];
  double v = -1.0;
  int64_t ix = n;
  for (int64_t e = (int64_t)blockIdx.x * PREP_THREADS + threadIdx.x; e < n; e += (int64_t)gridDim.x * PREP_THREADS) {
    const double a = npls_mag(Z[e]);
    if (npls_better(a, e, v, ix)) {
      v = a;
      ix = e;
    }
  }
  npls_block_best(v, ix, rv, ri);
  if (threadIdx.x == 0) {
    pv[blockIdx.x] = v;
    pi[blockIdx.x] = ix;
  }
}
// out[0] = the largest magnitude, out[1] = its first index as a double (exact below 2^53)
__global__ __launch_bounds__(PREP_THREADS) void k_npls_argmax_fold(const double *__restrict__ pv,
                                                                   const int64_t *__restrict__ pi, int np, int64_t n,
                                                                   double *__restrict__ out) {
  __shared__ double rv[PREP_THREADS];
  __shared__ int64_t ri[PREP_THREADS];
  double v = -1.0;
  int64_t ix = n;
  for (int b = threadIdx.x; b < np; b += PREP_THREADS)
    if (npls_better(pv[b], pi[b], v, ix)) {
      v = pv[b];
      ix = pi[b];
    }
  npls_block_best(v, ix, rv, ri);
  if (threadIdx.x == 0) {
    out[0] = v;
    out[1] = (double)ix;
  }
}

}  // namespace ppals
