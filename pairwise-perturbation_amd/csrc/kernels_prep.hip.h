// kernels_prep.hip.h — PARAFAC preprocessing of the resident tensor in place (ppals_tensor_center / _shift /
// _slice_sumsq / _scale / _rescale): centring across a mode and scaling within a mode (Bro & Smilde,
// J. Chemometrics 17 (2003) 16-33). The tensor is viewed as [L, J, T], first index fastest; a fibre is the J
// elements with (l, t) fixed, a slice x the L T elements with j = x.
//
// Arithmetic, every kernel: an element is read as stored, widened to fp64, and the new value is rounded ONCE
// to the storage type by the cast the import uses ((float)x, bf16s(x)). Sums are formed in fp64 in an order
// that depends on the shape only — no atomics — so the same state gives the same bits.
//
// The walks (MODE: centre / shift by an offset per fibre / multiply by a factor per slice):
//   k_prep_lead       L == 1, fibres contiguous: a workgroup takes a run of whole fibres, loads it into LDS in
//                     16-byte pieces (scalar head and tail where the run is not aligned), works on it there
//                     with G lanes a fibre, and stores it the same way. One read, one write.
//   k_prep_lead_long  L == 1 and a fibre longer than the run buffer: a workgroup a fibre, two passes.
//   k_prep_rows       L > 1: lanes along l, a workgroup owns LX * VEC consecutive l of one t and walks j at
//                     stride L, JY = 256 / LX rows of j at a time. ONCHIP keeps what it read in LDS (every
//                     thread re-reads only its own elements: no barrier guards the image) and stores from
//                     there; otherwise the second pass re-reads the tensor.
// The slice sums of squares: k_sumsq_rows (L > 1) / k_sumsq_lead (L == 1) write one partial sum per (block,
// slice), k_fold_partials adds them in block order.
// All LDS is dynamic and every carve offset a multiple of 16.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "bf16.h"

namespace ppals {

enum PrepMode { PREP_CENTER = 0, PREP_SHIFT = 1, PREP_SCALE = 2 };
constexpr int PREP_THREADS = 256;
constexpr int PREP_ROWS_TILE_BYTES = 56 * 1024;  // on-chip image of a k_prep_rows tile
constexpr int PREP_LEAD_RUN_BYTES = 48 * 1024;   // run buffer of k_prep_lead

// elements of a 16-byte access
template <typename T>
struct PrepVec16 {
  static constexpr int N = 16 / (int)sizeof(T);
};
// elements a lane of k_prep_rows owns along l
template <typename T>
struct PrepRowsVec {
  static constexpr int N = sizeof(T) == 8 ? 2 : 4;
};
template <typename T, int N>
struct alignas(N * sizeof(T)) prep_vec {
  T v[N];
};

template <int MODE>
__device__ __forceinline__ double prep_apply(double v, double p, double alpha) {
  if (MODE == PREP_CENTER) return v - p;
  if (MODE == PREP_SHIFT) return v + alpha * p;  // alpha = +-1: alpha * p is exact, one rounding either way
  return v * p;
}

// the sum of the workgroup's 256 values in a fixed tree; red: 256 doubles of LDS. Ends with a barrier.
__device__ __forceinline__ double prep_block_sum(double v, double *red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  for (int s = PREP_THREADS / 2; s > 0; s >>= 1) {
    __syncthreads();
    if (tid < s) red[tid] += red[tid + s];
  }
  __syncthreads();
  const double r = red[0];
  __syncthreads();
  return r;
}

// ------------------------------------------------------------------ L == 1: runs of whole fibres through LDS
// n elements between global memory at g and the LDS image at s, 16 bytes a lane where both sides are aligned:
// `head` elements precede the first 16-byte boundary of g, and the caller placed s so that the same holds there.
template <typename T, bool LOAD>
__device__ __forceinline__ void prep_run_copy(T *g, T *s, int n, int head) {
  constexpr int V = PrepVec16<T>::N;
  typedef prep_vec<T, V> vec;
  const int tid = threadIdx.x;
  if (head > n) head = n;
  const int nv = (n - head) / V, tail0 = head + nv * V;
  if (tid < head) {
    if (LOAD) s[tid] = g[tid];
    else g[tid] = s[tid];
  }
  for (int u = tid; u < nv; u += PREP_THREADS) {
    if (LOAD) *reinterpret_cast<vec *>(s + head + u * V) = *reinterpret_cast<const vec *>(g + head + u * V);
    else *reinterpret_cast<vec *>(g + head + u * V) = *reinterpret_cast<const vec *>(s + head + u * V);
  }
  if (tail0 + tid < n) {
    if (LOAD) s[tail0 + tid] = g[tail0 + tid];
    else g[tail0 + tid] = s[tail0 + tid];
  }
}

// F fibres a run, G lanes a fibre (a power of two, F * G <= 256 unless G == 1). off: CENTER writes the means
// (may be null), SHIFT reads them; fac: SCALE's factors [J].
template <typename T, int MODE>
__global__ __launch_bounds__(PREP_THREADS) void k_prep_lead(T *__restrict__ V, int J, int64_t nfib, int F, int G,
                                                            double *__restrict__ off, const double *__restrict__ fac,
                                                            double alpha) {
  extern __shared__ __attribute__((aligned(16))) char prep_smem[];
  constexpr int V16 = PrepVec16<T>::N;
  double *red = reinterpret_cast<double *>(prep_smem);                       // [256]
  T *img = reinterpret_cast<T *>(prep_smem + 8 * PREP_THREADS);             // [V16 + F * J]
  const int tid = threadIdx.x, fs = tid / G, g = tid % G, fpb = PREP_THREADS / G;
  const int64_t nruns = (nfib + F - 1) / F;
  for (int64_t run = blockIdx.x; run < nruns; run += gridDim.x) {
    const int64_t f0 = run * F;
    const int nf = (int)(nfib - f0 < F ? nfib - f0 : F), n = nf * J;
    T *gp = V + f0 * J;
    const int head = (int)(((16 - ((uintptr_t)gp & 15)) & 15) / sizeof(T));
    T *s = img + (V16 - head % V16) % V16;  // element `head` of the run lands on a 16-byte boundary of LDS
    prep_run_copy<T, true>(gp, s, n, head);
    __syncthreads();
    for (int fb = 0; fb < nf; fb += fpb) {
      const int f = fb + fs;
      const bool live = f < nf;
      double p = 0;
      if (MODE == PREP_CENTER) {
        double acc = 0;
        if (live)
          for (int j = g; j < J; j += G) acc += (double)s[f * J + j];
        if (G > 1) {
          red[tid] = acc;
          for (int h = G / 2; h > 0; h >>= 1) {
            __syncthreads();
            if (g < h) red[tid] += red[tid + h];
          }
          __syncthreads();
          acc = red[tid - g];
          __syncthreads();
        }
        p = acc / (double)J;
        if (live && g == 0 && off) off[f0 + f] = p;
      } else if (MODE == PREP_SHIFT) {
        if (live) p = off[f0 + f];
      }
      if (live)
        for (int j = g; j < J; j += G) {
          if (MODE == PREP_SCALE) {
            p = fac[j];
            if (p == 1.0) continue;  // (a slice that stays: not even a NaN's payload moves)
          }
          s[f * J + j] = (T)prep_apply<MODE>((double)s[f * J + j], p, alpha);
        }
    }
    __syncthreads();
    prep_run_copy<T, false>(gp, s, n, head);
    __syncthreads();
  }
}

// a workgroup a fibre, two passes over it (the fibre does not fit the run buffer)
template <typename T, int MODE>
__global__ __launch_bounds__(PREP_THREADS) void k_prep_lead_long(T *__restrict__ V, int64_t J, int64_t nfib,
                                                                 double *__restrict__ off,
                                                                 const double *__restrict__ fac, double alpha) {
  extern __shared__ __attribute__((aligned(16))) char prep_smem[];
  double *red = reinterpret_cast<double *>(prep_smem);  // [256]
  const int tid = threadIdx.x;
  for (int64_t f = blockIdx.x; f < nfib; f += gridDim.x) {
    T *gp = V + f * J;
    double p = 0;
    if (MODE == PREP_CENTER) {
      double acc = 0;
      for (int64_t j = tid; j < J; j += PREP_THREADS) acc += (double)gp[j];
      p = prep_block_sum(acc, red) / (double)J;
      if (tid == 0 && off) off[f] = p;
    } else if (MODE == PREP_SHIFT) {
      p = off[f];
    }
    for (int64_t j = tid; j < J; j += PREP_THREADS) {
      if (MODE == PREP_SCALE) {
        p = fac[j];
        if (p == 1.0) continue;
      }
      gp[j] = (T)prep_apply<MODE>((double)gp[j], p, alpha);
    }
  }
}

// ------------------------------------------------------------------ L > 1: lanes along l, j at stride L
// VEC == 1: any L and alignment; VEC > 1 needs L % VEC == 0 and V aligned to VEC elements. ntl = tiles along l.
template <typename T, int VEC, int LX, int MODE, bool ONCHIP>
__global__ __launch_bounds__(PREP_THREADS) void k_prep_rows(T *__restrict__ V, int64_t L, int64_t J, int64_t Tn,
                                                            int64_t ntl, double *__restrict__ off,
                                                            const double *__restrict__ fac, double alpha) {
  extern __shared__ __attribute__((aligned(16))) char prep_smem[];
  constexpr int JY = PREP_THREADS / LX, BL = LX * VEC;
  typedef prep_vec<T, VEC> vec;
  double *part = reinterpret_cast<double *>(prep_smem);              // [JY][BL] (CENTER only)
  T *img = reinterpret_cast<T *>(prep_smem + 8 * JY * BL);           // [J][BL]  (CENTER && ONCHIP only)
  const int lx = threadIdx.x % LX, jy = threadIdx.x / LX;
  const int64_t ntiles = ntl * Tn;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t lb = tile % ntl, t = tile / ntl;
    const int64_t l0 = lb * BL + (int64_t)lx * VEC;
    const int nl = l0 >= L ? 0 : (L - l0 < VEC ? (int)(L - l0) : VEC);  // (VEC > 1: 0 or VEC)
    T *gp = V + l0 + L * J * t;
    double p[VEC];
#pragma unroll
    for (int k = 0; k < VEC; k++) p[k] = 0;
    if (MODE == PREP_CENTER) {
      double acc[VEC];
#pragma unroll
      for (int k = 0; k < VEC; k++) acc[k] = 0;
      if (nl > 0)
        for (int64_t j = jy; j < J; j += JY) {
          vec x;
          if (VEC > 1) {
            x = *reinterpret_cast<const vec *>(gp + L * j);
          } else {
            x.v[0] = gp[L * j];
          }
          if (ONCHIP) *reinterpret_cast<vec *>(img + j * BL + lx * VEC) = x;
#pragma unroll
          for (int k = 0; k < VEC; k++) acc[k] += (double)x.v[k];
        }
#pragma unroll
      for (int k = 0; k < VEC; k++) part[jy * BL + lx * VEC + k] = acc[k];
      __syncthreads();
#pragma unroll
      for (int k = 0; k < VEC; k++) {
        double s = 0;
        for (int y = 0; y < JY; y++) s += part[y * BL + lx * VEC + k];
        p[k] = s / (double)J;
      }
      if (off && jy == 0) {
#pragma unroll
        for (int k = 0; k < VEC; k++)
          if (k < nl) off[l0 + k + L * t] = p[k];
      }
    } else if (MODE == PREP_SHIFT) {
#pragma unroll
      for (int k = 0; k < VEC; k++)
        if (k < nl) p[k] = off[l0 + k + L * t];
    }
    if (nl > 0)
      for (int64_t j = jy; j < J; j += JY) {
        if (MODE == PREP_SCALE) {
          const double f = fac[j];
          if (f == 1.0) continue;
#pragma unroll
          for (int k = 0; k < VEC; k++) p[k] = f;
        }
        vec x;
        if (MODE == PREP_CENTER && ONCHIP) {
          x = *reinterpret_cast<const vec *>(img + j * BL + lx * VEC);
        } else if (VEC > 1) {
          x = *reinterpret_cast<const vec *>(gp + L * j);
        } else {
          x.v[0] = gp[L * j];
        }
#pragma unroll
        for (int k = 0; k < VEC; k++) x.v[k] = (T)prep_apply<MODE>((double)x.v[k], p[k], alpha);
        if (VEC > 1) {
          *reinterpret_cast<vec *>(gp + L * j) = x;
        } else {
          gp[L * j] = x.v[0];
        }
      }
    if (MODE == PREP_CENTER) __syncthreads();  // `part` is rewritten by the next tile
  }
}

// ------------------------------------------------------------------ slice sums of squares
// L > 1: block (j, b); X lanes along l (a power of two), 256 / X rows of t, t strided by the NB blocks of the slice
template <typename T, int VEC>
__global__ __launch_bounds__(PREP_THREADS) void k_sumsq_rows(const T *__restrict__ V, int64_t L, int64_t J, int64_t Tn,
                                                             int X, double *__restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) char prep_smem[];
  double *red = reinterpret_cast<double *>(prep_smem);
  typedef prep_vec<T, VEC> vec;
  const int x = threadIdx.x % X, y = threadIdx.x / X, Y = PREP_THREADS / X;
  const int64_t j = blockIdx.x, nb = gridDim.y, Lv = L / VEC;
  double acc = 0;
  for (int64_t t = (int64_t)blockIdx.y * Y + y; t < Tn; t += nb * Y) {
    const T *gp = V + L * (j + J * t);
    for (int64_t l = x; l < Lv; l += X) {
      const vec a = *reinterpret_cast<const vec *>(gp + l * VEC);
#pragma unroll
      for (int k = 0; k < VEC; k++) {
        const double d = (double)a.v[k];
        acc += d * d;
      }
    }
  }
  const double s = prep_block_sum(acc, red);
  if (threadIdx.x == 0) part[(int64_t)blockIdx.y * J + j] = s;
}

// L == 1: block (jc, b); X lanes along j (a power of two), one j a lane, 256 / X rows of t
template <typename T>
__global__ __launch_bounds__(PREP_THREADS) void k_sumsq_lead(const T *__restrict__ V, int64_t J, int64_t Tn, int X,
                                                             double *__restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) char prep_smem[];
  double *red = reinterpret_cast<double *>(prep_smem);
  const int x = threadIdx.x % X, y = threadIdx.x / X, Y = PREP_THREADS / X;
  const int64_t j = (int64_t)blockIdx.x * X + x, nb = gridDim.y;
  double acc = 0;
  if (j < J)
    for (int64_t t = (int64_t)blockIdx.y * Y + y; t < Tn; t += nb * Y) {
      const double d = (double)V[j + J * t];
      acc += d * d;
    }
  red[threadIdx.x] = acc;
  __syncthreads();
  if (y == 0 && j < J) {
    double s = 0;
    for (int yy = 0; yy < Y; yy++) s += red[x + X * yy];
    part[(int64_t)blockIdx.y * J + j] = s;
  }
}

// ss[j] = sum over the nb blocks, in block order
__global__ void k_fold_partials(const double *__restrict__ part, int nb, int64_t J, double *__restrict__ ss) {
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < J; j += (int64_t)gridDim.x * blockDim.x) {
    double s = 0;
    for (int b = 0; b < nb; b++) s += part[(int64_t)b * J + j];
    ss[j] = s;
  }
}

}  // namespace ppals
