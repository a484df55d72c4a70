// kernels_io.hip.h — copy / convert / permute between a strided device view and the resident shard
// (ppals_tensor_import_device / _export_device). The plan (device_view.h) orders the modes as the
// shard stores them; IMP = true reads the view and writes the shard, false the reverse. S is the
// element type read, D the type written; the view side may be f16 / bf16 (import only).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "bf16.h"
#include "device_view.h"

namespace ppals {

struct io_bf16 {
  uint16_t u;
};

template <typename D, typename S>
__device__ __forceinline__ D io_cvt(S x) {
  return (D)x;  // f32 <-> f64: exact widening, or the round-to-nearest-even (float) cast
}
template <>
__device__ __forceinline__ float io_cvt<float, io_bf16>(io_bf16 x) {
  return __uint_as_float((uint32_t)x.u << 16);
}
template <>
__device__ __forceinline__ double io_cvt<double, io_bf16>(io_bf16 x) {
  return (double)__uint_as_float((uint32_t)x.u << 16);
}

// bf16 storage (PPALS_BF16): a bf16 view copies bit for bit, f16 goes through its exact fp32 value
template <>
__device__ __forceinline__ bf16s io_cvt<bf16s, io_bf16>(io_bf16 x) {
  bf16s r;
  r.u = x.u;
  return r;
}
template <>
__device__ __forceinline__ bf16s io_cvt<bf16s, _Float16>(_Float16 x) {
  return bf16s((float)x);
}

template <typename T>
struct alignas(4 * sizeof(T)) io_vec4 {
  T v[4];
};

// (a) streaming: plan mode 0 is unit-stride in the view and the shard's fastest. VEC: 4 elements per
// access (both sides unit-stride along mode 0, every row start aligned to 4 elements, both pointers
// aligned to 4 * sizeof); otherwise one element per access. nd == 1 (the whole box one run, e.g. an
// identity layout) needs no index decoding.
template <bool IMP, bool VEC, typename S, typename D>
__global__ __launch_bounds__(256) void k_io_stream(const S *__restrict__ src, D *__restrict__ dst,
                                                   ViewPlan p) {
  const int64_t n0 = p.n[0];
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (int64_t)gridDim.x * blockDim.x;
  if (VEC) {
    if (p.nd == 1) {
      const int64_t nv = n0 >> 2;
      for (int64_t u = tid; u < nv; u += nth) {
        const io_vec4<S> a = reinterpret_cast<const io_vec4<S> *>(src)[u];
        io_vec4<D> b;
#pragma unroll
        for (int k = 0; k < 4; k++) b.v[k] = io_cvt<D>(a.v[k]);
        reinterpret_cast<io_vec4<D> *>(dst)[u] = b;
      }
      for (int64_t e = 4 * nv + tid; e < n0; e += nth) dst[e] = io_cvt<D>(src[e]);
    } else {
      const int64_t per_row = n0 >> 2, nv = per_row * (p.count / n0);
      for (int64_t u = tid; u < nv; u += nth) {
        const int64_t row = u / per_row, c = (u - row * per_row) * 4;
        int64_t v = c, r = c;
        dv_decode(p, 1, p.nd, row, v, r);
        const io_vec4<S> a = *reinterpret_cast<const io_vec4<S> *>(src + (IMP ? v : r));
        io_vec4<D> b;
#pragma unroll
        for (int k = 0; k < 4; k++) b.v[k] = io_cvt<D>(a.v[k]);
        *reinterpret_cast<io_vec4<D> *>(dst + (IMP ? r : v)) = b;
      }
    }
  } else {
    const int64_t vs0 = p.vs[0], rs0 = p.rs[0];
    for (int64_t e = tid; e < p.count; e += nth) {
      const int64_t row = e / n0, c = e - row * n0;
      int64_t v = c * vs0, r = c * rs0;
      dv_decode(p, 1, p.nd, row, v, r);
      dst[IMP ? r : v] = io_cvt<D>(src[IMP ? v : r]);
    }
  }
}

// (b) 64 x 64 tiles through LDS. Tile rows run over the flattened plan modes [0, fk) (A: the shard's
// fast side, offsets of the tile's 64 rows decoded once per tile into LDS), columns over plan mode fk
// (B: unit stride in the view); the other modes index the tiles. Reads and writes are both coalesced:
// the side that is contiguous along B is accessed with the lane index along B, the other with the lane
// index along A. The image is stored [64][65]: the column walk hits 64 different banks (4-byte types).
template <bool IMP, typename S, typename D>
__global__ __launch_bounds__(256) void k_io_tile(const S *__restrict__ src, D *__restrict__ dst,
                                                 ViewPlan p, int64_t FA, int64_t tA, int64_t tB,
                                                 int64_t tiles, int64_t rsB) {
  __shared__ D tile[DV_TILE_DIM][DV_TILE_DIM + 1];
  __shared__ int64_t av[DV_TILE_DIM], ar[DV_TILE_DIM];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;  // ty in [0, 4)
  int64_t nB = 1;
#pragma unroll
  for (int m = 0; m < DV_MAX_ORDER; m++)
    if (m == p.fk) nB = p.n[m];
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t ta = t % tA, tr = t / tA, tb = tr % tB, bt = tr / tB;
    int64_t bv = 0, br = 0;
    dv_decode(p, p.fk + 1, p.nd, bt, bv, br);
    const int64_t a0 = ta * DV_TILE_DIM, b0 = tb * DV_TILE_DIM;
    const int na = (int)min((int64_t)DV_TILE_DIM, FA - a0), nb = (int)min((int64_t)DV_TILE_DIM, nB - b0);
    if (threadIdx.x < DV_TILE_DIM) {
      int64_t v = bv, r = br;
      if ((int)threadIdx.x < na) dv_decode(p, 0, p.fk, a0 + threadIdx.x, v, r);
      av[threadIdx.x] = v;
      ar[threadIdx.x] = r;
    }
    __syncthreads();
    if (IMP) {  // view (unit stride along B) -> shard (contiguous along A)
#pragma unroll
      for (int i = 0; i < 16; i++) {
        const int a = ty + 4 * i;
        if (a < na && tx < nb) tile[a][tx] = io_cvt<D>(src[av[a] + b0 + tx]);
      }
      __syncthreads();
#pragma unroll
      for (int i = 0; i < 16; i++) {
        const int b = ty + 4 * i;
        if (tx < na && b < nb) dst[ar[tx] + (b0 + b) * rsB] = tile[tx][b];
      }
    } else {  // shard -> view
#pragma unroll
      for (int i = 0; i < 16; i++) {
        const int b = ty + 4 * i;
        if (tx < na && b < nb) tile[b][tx] = io_cvt<D>(src[ar[tx] + (b0 + b) * rsB]);
      }
      __syncthreads();
#pragma unroll
      for (int i = 0; i < 16; i++) {
        const int a = ty + 4 * i;
        if (a < na && tx < nb) dst[av[a] + b0 + tx] = tile[tx][a];
      }
    }
    __syncthreads();  // the image and the offsets are rewritten by the next tile
  }
}

// (c) per-element gather: the view has no unit-stride mode. Walks the shard's order.
template <bool IMP, typename S, typename D>
__global__ __launch_bounds__(256) void k_io_gather(const S *__restrict__ src, D *__restrict__ dst,
                                                   ViewPlan p) {
  const int64_t nth = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < p.count; e += nth) {
    int64_t v = 0, r = 0;
    dv_decode(p, 0, p.nd, e, v, r);
    dst[IMP ? r : v] = io_cvt<D>(src[IMP ? v : r]);
  }
}

}  // namespace ppals
