// pack_scan_bench.hip — does the one-n-tile fp32 scan get faster when it reads a lossless 28-bit copy
// of the tensor (24 low bits + a 4-bit offset from a per-block top byte, 3.5 B per element) instead
// of the fp32 words? cfg2 geometry, both forms of the scan the multi-sweep schedule runs:
//   suffix  M = 8e6 rows x K = 200            batched  M = 40 000 rows x K = 200 x 200 batches
// The library kernel k_scan_suffix_buf<float,1,5> and the packed kernel run on the same data,
// launches interleaved, and the results are compared bit for bit. Two byte arrangements of a block
// (4 waves x 64 lanes x 16 elements, the unit one workgroup consumes per iteration):
//   fmt 0  code plane (8 B per lane) at the head, then one 12-byte piece per lane and k-quad:
//          b64 + 4 x b96 loads; a short last k-block simply ends after its last present quad
//   fmt 1  per wave 3 x (64 lanes x 16 B) + 64 lanes x 8 B: 3 x b128 + b64 loads; the last k-block is
//          stored whole
// A lane's quad is three dwords: the low 24 bits of elements 0..2 in the low bytes, the three low
// bytes of element 3 in the top bytes; a code dword serves two quads (even nibbles / odd nibbles).
//   build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -o tools/pack_scan_bench tools/pack_scan_bench.hip
//   run:   tools/pack_scan_bench [rounds]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../pairwise-perturbation_amd/csrc/ops.h"
#include "../pairwise-perturbation_amd/csrc/kernels_scan.hip.h"
using namespace ppals;
#define CK(x)                                                                   \
  do {                                                                          \
    hipError_t e_ = (x);                                                        \
    if (e_ != hipSuccess) {                                                     \
      fprintf(stderr, "HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); \
      exit(1);                                                                  \
    }                                                                           \
  } while (0)

typedef unsigned int u32;
typedef u32 u32x2 __attribute__((ext_vector_type(2)));
typedef u32 u32x3 __attribute__((ext_vector_type(3)));
typedef u32 u32x4 __attribute__((ext_vector_type(4)));

constexpr int PKV_BLOCK = 256 * 16 * 7 / 2;  // bytes of a whole block: 14336
constexpr int PKV_CODES = 256 * 8;           // fmt 0: the code plane at the head of a block
constexpr int PKV_QUAD = 256 * 12;           // fmt 0: one k-quad of low parts
constexpr int PKV_WAVE = PKV_BLOCK / 4;       // fmt 1: one wave's part of a block

// bytes of one tile (all k-blocks of 256 rows)
static int64_t tile_bytes_of(int fmt, int64_t K) {
  const int64_t nkb = (K + 15) / 16, kfull = K / 16;
  if (fmt == 1 || kfull == nkb) return nkb * PKV_BLOCK;
  const int64_t nq = (K - kfull * 16 + 3) / 4;
  return kfull * PKV_BLOCK + PKV_CODES + nq * PKV_QUAD;
}

// the tensor of the headline run: a rank-10 model with factors ~ U(0,1), s = 200, order 4
__global__ void k_fill_model(float *p, int64_t n, const float *F) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n;
       e += (int64_t)gridDim.x * blockDim.x) {
    int64_t t = e;
    const int i0 = (int)(t % 200);
    t /= 200;
    const int i1 = (int)(t % 200);
    t /= 200;
    const int i2 = (int)(t % 200);
    const int i3 = (int)(t / 200);
    float s = 0.f;
    for (int r = 0; r < 10; r++)
      s += F[i0 * 10 + r] * F[2000 + i1 * 10 + r] * F[4000 + i2 * 10 + r] * F[6000 + i3 * 10 + r];
    p[e] = s;
  }
}
__global__ void k_fill(float *p, int64_t n, uint32_t seed) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n;
       e += (int64_t)gridDim.x * blockDim.x) {
    uint32_t h = (uint32_t)e * 2654435761u ^ seed;
    h ^= h >> 15;
    p[e] = 0.5f + (float)(h & 0xffff) * (0.5f / 65536.f);
  }
}

// the 16 fp32 words of (block gid, thread) in the scan's lane mapping; absent ones flagged
struct PkvLane {
  u32 e[4][4];
  bool ok[4][4];
};
__device__ inline PkvLane pkv_gather(const float *V, int64_t M, int64_t K, int64_t batch_stride, int n_mtiles,
                                   int nkb, int64_t gid, int tid) {
  const int lane = tid & 63, wave = tid >> 6, g = lane >> 4, j16 = lane & 15;
  const int64_t tile = gid / nkb;
  const int kb = (int)(gid % nkb);
  const int64_t mtile = tile % n_mtiles, batch = tile / n_mtiles;
  const int64_t m = (mtile * 4 + wave) * 64 + 4 * j16;
  PkvLane r;
  for (int u = 0; u < 4; u++) {
    const int64_t k = (int64_t)kb * 16 + 4 * u + g;
    for (int jj = 0; jj < 4; jj++) {
      r.ok[u][jj] = k < K && m + jj < M;
      r.e[u][jj] = r.ok[u][jj] ? __float_as_uint(V[batch * batch_stride + k * M + m + jj]) : 0u;
    }
  }
  return r;
}

// pre-pass: per block the smallest top byte (replicated into the four bytes of bases[gid]) and,
// over all blocks, the largest spread max - min (an integer maximum: order does not matter)
__global__ __launch_bounds__(256) void k_pkv_prepass(const float *V, int64_t M, int64_t K, int64_t batch_stride,
                                                    int n_mtiles, int nkb, u32 *bases, int *span) {
  __shared__ int smn[256], smx[256];
  const int64_t gid = blockIdx.x;
  const PkvLane r = pkv_gather(V, M, K, batch_stride, n_mtiles, nkb, gid, threadIdx.x);
  int mn = 255, mx = 0;
  for (int u = 0; u < 4; u++)
    for (int jj = 0; jj < 4; jj++)
      if (r.ok[u][jj]) {
        const int t = (int)(r.e[u][jj] >> 24);
        mn = min(mn, t);
        mx = max(mx, t);
      }
  smn[threadIdx.x] = mn;
  smx[threadIdx.x] = mx;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      smn[threadIdx.x] = min(smn[threadIdx.x], smn[threadIdx.x + s]);
      smx[threadIdx.x] = max(smx[threadIdx.x], smx[threadIdx.x + s]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    mn = smn[0];
    mx = smx[0];
    if (mx < mn) mn = mx = 0;
    bases[gid] = (u32)mn * 0x01010101u;
    atomicMax(span, mx - mn);
  }
}

template <int FMT>
__global__ __launch_bounds__(256) void k_pkv_pack(const float *V, int64_t M, int64_t K, int64_t batch_stride,
                                                 int n_mtiles, int nkb, int64_t tile_bytes, const u32 *bases,
                                                 char *out) {
  const int64_t gid = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const PkvLane r = pkv_gather(V, M, K, batch_stride, n_mtiles, nkb, gid, tid);
  const u32 base = bases[gid] & 0xffu;
  const int64_t tile = gid / nkb;
  const int kb = (int)(gid % nkb);
  char *blk = out + tile * tile_bytes + (int64_t)kb * PKV_BLOCK;
  u32 w[4][3], cw[2] = {0u, 0u};
  for (int u = 0; u < 4; u++) {
    u32 e[4];
    for (int jj = 0; jj < 4; jj++) {
      e[jj] = r.ok[u][jj] ? r.e[u][jj] : base << 24;  // absent: low part 0, code 0
      cw[u >> 1] |= ((e[jj] >> 24) - base) << (8 * jj + 4 * (u & 1));
    }
    for (int i = 0; i < 3; i++) w[u][i] = (e[i] & 0xffffffu) | (((e[3] >> (8 * i)) & 0xffu) << 24);
  }
  if (FMT == 0) {
    *reinterpret_cast<u32x2 *>(blk + wave * 512 + lane * 8) = u32x2{cw[0], cw[1]};
    for (int u = 0; u < 4; u++)
      if ((int64_t)kb * 16 + 4 * u < K) {
        u32 *q = reinterpret_cast<u32 *>(blk + PKV_CODES + u * PKV_QUAD + wave * 768 + lane * 12);
        q[0] = w[u][0];
        q[1] = w[u][1];
        q[2] = w[u][2];
      }
  } else {
    char *wv = blk + wave * PKV_WAVE;
    const u32 *d = &w[0][0];
    for (int i = 0; i < 3; i++)
      *reinterpret_cast<u32x4 *>(wv + i * 1024 + lane * 16) = u32x4{d[4 * i], d[4 * i + 1], d[4 * i + 2], d[4 * i + 3]};
    *reinterpret_cast<u32x2 *>(wv + 3072 + lane * 8) = u32x2{cw[0], cw[1]};
  }
}

// The packed form of k_scan_suffix_buf<float, 1, .> (no k-split, unpadded): the same persistent tile
// walk, next-tile prefetch, register double buffer, MFMA order, FLUSH and epilogue; only the source
// of the 16 fp32 values per lane and block differs. OPT bit 0: non-temporal tensor loads, bit 2:
// non-temporal result stores (as in the library kernel).
template <int FMT, int OPT>
__device__ __forceinline__ void scan_suffix_pkv_body(
    const char *__restrict__ Vp, const u32 *__restrict__ bases, int64_t tile_bytes, int64_t M, int64_t K,
    const float *__restrict__ P, int n_mtiles, int nkb, double *__restrict__ out, int64_t out_nstride,
    int64_t out_batch_stride, int ncols, int out32, int64_t ntiles) {
  typedef ScanTraits<float> TR;
  constexpr int VEC = 4, NT = 1, FLUSH = 4;
  constexpr int AUXV = (OPT & 1) ? 2 : 0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, j16 = lane & 15;
  const int voffP = (int)((g * 16 + j16) * VEC * (int)sizeof(float));
  const int voffC = FMT == 0 ? wave * 512 + lane * 8 : wave * PKV_WAVE + 3072 + lane * 8;
  const int voffL = FMT == 0 ? PKV_CODES + wave * 768 + lane * 12 : wave * PKV_WAVE + lane * 16;
  const __amdgpu_buffer_rsrc_t rsrcP = __builtin_amdgcn_make_buffer_rsrc(
      (void *)P, 0, (int)((int64_t)nkb * NT * (4 * 16 * VEC) * (int64_t)sizeof(float)), 0x00020000);

  struct Tile {
    int64_t m, obase;
    bool live;
  };
  auto decode = [&](int64_t id, Tile &t) {
    const unsigned b = (unsigned)id;
    const int mtile = (int)(b % (unsigned)n_mtiles);
    const int64_t batch = b / (unsigned)n_mtiles;
    const int64_t m0 = ((int64_t)mtile * 4 + wave) * (16 * VEC);
    t.live = m0 < M;  // wave-uniform
    t.m = m0 + (int64_t)VEC * j16;
    t.obase = batch * out_batch_stride;
  };
  struct Raw {
    u32 w[12], c[2], b;
    f32x4 p;
  };
#define PPALS_PKV_LOAD(tile_, kb_, r_)                                                                 \
  {                                                                                                   \
    const int t_ = __builtin_amdgcn_readfirstlane((int)(tile_));                                      \
    const int k_ = __builtin_amdgcn_readfirstlane((int)(kb_));                                        \
    const int64_t koff_ = (int64_t)k_ * PKV_BLOCK;                                                     \
    const __amdgpu_buffer_rsrc_t rs_ = __builtin_amdgcn_make_buffer_rsrc(                             \
        (void *)(Vp + (int64_t)t_ * tile_bytes + koff_), 0,                                           \
        (int)min(tile_bytes - koff_, (int64_t)PKV_BLOCK), 0x00020000);                                 \
    if constexpr (FMT == 0) {                                                                         \
      _Pragma("unroll") for (int u = 0; u < 4; u++) {                                                 \
        const u32x3 q_ = __builtin_amdgcn_raw_buffer_load_b96(rs_, voffL, u * PKV_QUAD, AUXV);         \
        r_.w[3 * u] = q_[0];                                                                          \
        r_.w[3 * u + 1] = q_[1];                                                                      \
        r_.w[3 * u + 2] = q_[2];                                                                      \
      }                                                                                               \
    } else {                                                                                          \
      _Pragma("unroll") for (int i = 0; i < 3; i++) {                                                 \
        const u32x4 q_ = __builtin_amdgcn_raw_buffer_load_b128(rs_, voffL, i * 1024, AUXV);           \
        r_.w[4 * i] = q_[0];                                                                          \
        r_.w[4 * i + 1] = q_[1];                                                                      \
        r_.w[4 * i + 2] = q_[2];                                                                      \
        r_.w[4 * i + 3] = q_[3];                                                                      \
      }                                                                                               \
    }                                                                                                 \
    const u32x2 c_ = __builtin_amdgcn_raw_buffer_load_b64(rs_, voffC, 0, AUXV);                       \
    r_.c[0] = c_[0];                                                                                  \
    r_.c[1] = c_[1];                                                                                  \
    r_.b = bases[(int64_t)t_ * nkb + k_];                                                             \
    r_.p = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(                           \
                                         rsrcP, voffP, k_ * (4 * 16 * VEC) * (int)sizeof(float), 0)); \
  }

  // the 16 fp32 words of a block: top bytes of a quad's four elements = base + code, one per byte
  // (no carries: <= 255), then one byte permute per element (three for the fourth)
  auto unpack = [](const Raw &r, f32x4 (&v)[4]) {
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const u32 cw = r.c[u >> 1];
      const u32 T = (((u & 1) ? cw >> 4 : cw) & 0x0f0f0f0fu) + r.b;
      const u32 w0 = r.w[3 * u], w1 = r.w[3 * u + 1], w2 = r.w[3 * u + 2];
      // v_perm_b32(hi, lo, sel): selector bytes 0..3 take lo's bytes, 4..7 hi's, 0x0c gives zero
      v[u][0] = __uint_as_float(__builtin_amdgcn_perm(T, w0, 0x04020100u));  // w0 & 0xffffff | T.b0 << 24
      v[u][1] = __uint_as_float(__builtin_amdgcn_perm(T, w1, 0x05020100u));
      v[u][2] = __uint_as_float(__builtin_amdgcn_perm(T, w2, 0x06020100u));
      v[u][3] = __uint_as_float(__builtin_amdgcn_perm(w1, w0, 0x0c0c0703u) |  // w0.b3, w1.b3, 0, 0
                                __builtin_amdgcn_perm(T, w2, 0x07030c0cu));   // 0, 0, w2.b3, T.b3
    }
  };

  Tile cur, nxt;
  int64_t id = blockIdx.x;
  for (; id < ntiles; id += gridDim.x) {
    decode(id, cur);
    if (cur.live) break;
  }
  if (id >= ntiles || nkb <= 0) return;
  f32x4 cv[4], cb;
  {
    Raw r0;
    PPALS_PKV_LOAD(id, 0, r0);
    unpack(r0, cv);
    cb = r0.p;
  }

  for (;;) {
    bool has_next = false;
    int64_t nid = id + gridDim.x;
    for (; nid < ntiles; nid += gridDim.x) {
      decode(nid, nxt);
      if (nxt.live) {
        has_next = true;
        break;
      }
    }
    f32x4 acc[VEC];
    double acc64[VEC][4];
#pragma unroll
    for (int a = 0; a < VEC; a++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        acc[a][r] = 0;
        acc64[a][r] = 0;
      }
    for (int kc = 0; kc < nkb; kc += FLUSH) {
      const int ke = min(nkb, kc + FLUSH);
      for (int kb = kc; kb < ke; kb++) {
        Raw nr;
        const bool same = kb + 1 < nkb;
        const int64_t pt = (same || !has_next) ? id : nid;
        const int pk = same ? kb + 1 : (has_next ? 0 : kb);
        PPALS_PKV_LOAD(pt, pk, nr);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < VEC; u++)
#pragma unroll
          for (int jj = 0; jj < VEC; jj++) acc[jj] = TR::mfma(cb[u], cv[u][jj], acc[jj]);
        // the scheduler must not pull the unpacking (and with it the wait for the loads just issued)
        // up between the MFMAs: the loads of block i+1 stay in flight under all MFMAs of block i
        __builtin_amdgcn_sched_barrier(0);
        unpack(nr, cv);
        cb = nr.p;
      }
#pragma unroll
      for (int a = 0; a < VEC; a++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          acc64[a][r] += (double)acc[a][r];
          acc[a][r] = 0;
        }
    }
    const ScanRowMap rm = scan_row_map<VEC>(cur.m, M, 0, 0);
    const bool vec_ok = (((cur.obase | out_nstride | rm.mo) & (VEC - 1)) == 0) && rm.nvalid == VEC;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int n = TR::row(lane, r);
      if (n < ncols && rm.nvalid > 0) {
        double val[VEC];
#pragma unroll
        for (int jj = 0; jj < VEC; jj++) val[jj] = acc64[jj][r];
        const int64_t idx = cur.obase + (int64_t)n * out_nstride + rm.mo;
        if (vec_ok && out32) {
          f32x4 ov;
#pragma unroll
          for (int jj = 0; jj < VEC; jj++) ov[jj] = (float)val[jj];
          if constexpr (OPT & 4)
            __builtin_nontemporal_store(ov, reinterpret_cast<f32x4 *>(reinterpret_cast<float *>(out) + idx));
          else
            *reinterpret_cast<f32x4 *>(reinterpret_cast<float *>(out) + idx) = ov;
        } else if (vec_ok) {
#pragma unroll
          for (int jj = 0; jj < VEC; jj += 2) {
            f64x2 ov = {val[jj], val[jj + 1]};
            if constexpr (OPT & 4)
              __builtin_nontemporal_store(ov, reinterpret_cast<f64x2 *>(out + idx + jj));
            else
              *reinterpret_cast<f64x2 *>(out + idx + jj) = ov;
          }
        } else {
#pragma unroll
          for (int jj = 0; jj < VEC; jj++)
            if (jj < rm.nvalid) scan_store(out, idx + jj, val[jj], out32);
        }
      }
    }
    if (!has_next) break;
    cur = nxt;
    id = nid;
  }
#undef PPALS_PKV_LOAD
}
#define PPALS_PKV_ARGS                                                                                             \
  const char *__restrict__ Vp, const u32 *__restrict__ bases, int64_t tile_bytes, int64_t M, int64_t K,           \
      const float *__restrict__ P, int n_mtiles, int nkb, double *__restrict__ out, int64_t out_nstride,          \
      int64_t out_batch_stride, int ncols, int out32, int64_t ntiles
#define PPALS_PKV_PASS Vp, bases, tile_bytes, M, K, P, n_mtiles, nkb, out, out_nstride, out_batch_stride, ncols, out32, ntiles
// as many waves per SIMD as the registers allow (4)
template <int FMT, int OPT>
__global__ __launch_bounds__(256) void k_scan_suffix_pkv(PPALS_PKV_ARGS) {
  scan_suffix_pkv_body<FMT, OPT>(PPALS_PKV_PASS);
}
// held at the 3 waves per SIMD of the library kernel
template <int FMT, int OPT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void k_scan_suffix_pkv3(PPALS_PKV_ARGS) {
  scan_suffix_pkv_body<FMT, OPT>(PPALS_PKV_PASS);
}

__global__ void k_count_diff(const u32 *a, const u32 *b, int64_t n, unsigned long long *cnt) {
  unsigned long long c = 0;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x)
    c += a[e] != b[e];
  if (c) atomicAdd(cnt, c);
}

struct Packed {
  char *data = nullptr;
  u32 *bases = nullptr;
  int64_t tile_bytes = 0, ntiles = 0, bytes = 0;
  int span = -1;
};
static Packed build_packed(int fmt, const float *V, int64_t M, int64_t K, int64_t T) {
  Packed p;
  const int n_mt = (int)((M + 255) / 256), nkb = (int)((K + 15) / 16);
  p.ntiles = (int64_t)n_mt * T;
  p.tile_bytes = tile_bytes_of(fmt, K);
  p.bytes = p.ntiles * p.tile_bytes;
  const int64_t nblocks = p.ntiles * nkb;
  int *span;
  CK(hipMalloc(&p.data, (size_t)p.bytes));
  CK(hipMalloc(&p.bases, sizeof(u32) * (size_t)nblocks));
  CK(hipMalloc(&span, sizeof(int)));
  CK(hipMemset(span, 0, sizeof(int)));
  hipLaunchKernelGGL(k_pkv_prepass, dim3((unsigned)nblocks), dim3(256), 0, 0, V, M, K, M * K, n_mt, nkb, p.bases, span);
  CK(hipMemcpy(&p.span, span, sizeof(int), hipMemcpyDeviceToHost));
  CK(hipFree(span));
  if (p.span >= 16) return p;
  if (fmt == 0)
    hipLaunchKernelGGL(k_pkv_pack<0>, dim3((unsigned)nblocks), dim3(256), 0, 0, V, M, K, M * K, n_mt, nkb, p.tile_bytes,
                       p.bases, p.data);
  else
    hipLaunchKernelGGL(k_pkv_pack<1>, dim3((unsigned)nblocks), dim3(256), 0, 0, V, M, K, M * K, n_mt, nkb, p.tile_bytes,
                       p.bases, p.data);
  CK(hipDeviceSynchronize());
  return p;
}

int main(int argc, char **argv) {
  const int64_t M = 8000000, Lb = 40000, Tb = 200;
  const int K = 200, R = 10, rounds = argc > 1 ? atoi(argv[1]) : 7;
  const int data = argc > 2 ? atoi(argv[2]) : 0;  // 0: the headline's rank-10 model, 1: uniform in [0.5, 1)
  const int nblk = (K + 15) / 16;
  hipDeviceProp_t prop;
  CK(hipGetDeviceProperties(&prop, 0));
  const int ncu = prop.multiProcessorCount;
  setvbuf(stdout, nullptr, _IONBF, 0);
  float *V, *P, *F, *Xref, *Xpk;
  const int64_t nout = M * R;
  CK(hipMalloc(&V, sizeof(float) * (size_t)M * K));
  CK(hipMalloc(&P, sizeof(float) * (size_t)nblk * 1024));
  CK(hipMalloc(&F, sizeof(float) * 8000));
  CK(hipMalloc(&Xref, sizeof(float) * (size_t)nout));
  CK(hipMalloc(&Xpk, sizeof(float) * (size_t)nout));
  std::vector<float> hf(8000);
  srand(1);
  for (auto &v : hf) v = (float)((rand() + 0.5) / ((double)RAND_MAX + 1.0));
  CK(hipMemcpy(F, hf.data(), sizeof(float) * 8000, hipMemcpyHostToDevice));
  // the Khatri-Rao operand: zero beyond K and beyond R columns, as k_krp_pack leaves it
  std::vector<float> hp((size_t)nblk * 1024, 0.f);
  for (int blk = 0; blk < nblk; blk++)
    for (int g = 0; g < 4; g++)
      for (int n = 0; n < 16; n++)
        for (int u = 0; u < 4; u++) {
          const int j = blk * 16 + 4 * u + g;
          if (j < K && n < R) hp[(((size_t)blk * 4 + g) * 16 + n) * 4 + u] = (float)((rand() + 0.5) / ((double)RAND_MAX + 1.0));
        }
  CK(hipMemcpy(P, hp.data(), sizeof(float) * hp.size(), hipMemcpyHostToDevice));
  if (data == 0)
    hipLaunchKernelGGL(k_fill_model, dim3(16384), dim3(256), 0, 0, V, M * K, F);
  else
    hipLaunchKernelGGL(k_fill, dim3(16384), dim3(256), 0, 0, V, M * K, 1u);
  CK(hipDeviceSynchronize());

  // [form][fmt]: form 0 = suffix, 1 = batched
  Packed pk[2][2];
  for (int form = 0; form < 2; form++)
    for (int fmt = 0; fmt < 2; fmt++) {
      pk[form][fmt] = form == 0 ? build_packed(fmt, V, M, K, 1) : build_packed(fmt, V, Lb, K, Tb);
      printf("packed form=%d fmt=%d: top-byte spread %d, %.4f B per element (%lld bytes)\n", form, fmt,
             pk[form][fmt].span, (double)pk[form][fmt].bytes / ((double)M * K), (long long)pk[form][fmt].bytes);
      if (pk[form][fmt].span >= 16) {
        printf("does not fit a window of 16: nothing to measure\n");
        return 2;
      }
    }

  constexpr int NVAR = 5;
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  const int n_mt = (int)((M + 255) / 256), n_mtb = (int)((Lb + 255) / 256);
  const dim3 gridf((unsigned)std::min<int64_t>(n_mt, (int64_t)ncu * 40));
  const dim3 gridb((unsigned)std::min<int64_t>((int64_t)n_mtb * Tb, (int64_t)ncu * 40));
  auto launch = [&](int form, int var, float *X) {
    const int64_t m = form == 0 ? M : Lb, nt = form == 0 ? (int64_t)n_mt : (int64_t)n_mtb * Tb;
    const int nm = form == 0 ? n_mt : n_mtb;
    const dim3 grid = form == 0 ? gridf : gridb;
    const int64_t nstride = form == 0 ? M : Lb * Tb, bstride = form == 0 ? 0 : Lb;
    if (var == 0)
      hipLaunchKernelGGL((k_scan_suffix_buf<float, 1, 5>), grid, dim3(256), 0, 0, V, m, (int64_t)K, m * K, P, nm, 1,
                         nblk, nblk, (double *)X, nstride, (int64_t)0, bstride, R, 1, nt);
    else {
      const Packed &q = pk[form][(var - 1) & 1];
      const void *kern = var == 1   ? (const void *)k_scan_suffix_pkv<0, 5>
                         : var == 2 ? (const void *)k_scan_suffix_pkv<1, 5>
                         : var == 3 ? (const void *)k_scan_suffix_pkv3<0, 5>
                                    : (const void *)k_scan_suffix_pkv3<1, 5>;
      const char *a_vp = q.data;
      const u32 *a_bases = q.bases;
      int64_t a_tb = q.tile_bytes, a_m = m, a_k = K, a_ns = nstride, a_bs = bstride, a_nt = nt;
      const float *a_p = P;
      int a_nm = nm, a_nkb = nblk, a_nc = R, a_o32 = 1;
      double *a_out = (double *)X;
      void *args[] = {&a_vp, &a_bases, &a_tb, &a_m, &a_k, &a_p, &a_nm, &a_nkb, &a_out, &a_ns, &a_bs, &a_nc, &a_o32, &a_nt};
      CK(hipLaunchKernel(kern, grid, dim3(256), args, 0, 0));
    }
  };

  // results first: bit for bit against the library kernel
  unsigned long long *cnt, hc;
  CK(hipMalloc(&cnt, sizeof(*cnt)));
  int bad = 0;
  for (int form = 0; form < 2; form++) {
    CK(hipMemset(Xref, 0xff, sizeof(float) * (size_t)nout));
    launch(form, 0, Xref);
    for (int var = 1; var < NVAR; var++) {
      CK(hipMemset(Xpk, 0xee, sizeof(float) * (size_t)nout));
      CK(hipMemset(cnt, 0, sizeof(*cnt)));
      launch(form, var, Xpk);
      hipLaunchKernelGGL(k_count_diff, dim3(4096), dim3(256), 0, 0, (const u32 *)Xref, (const u32 *)Xpk, nout, cnt);
      CK(hipMemcpy(&hc, cnt, sizeof(hc), hipMemcpyDeviceToHost));
      printf("form=%d variant=%d: %llu of %lld result words differ\n", form, var, hc, (long long)nout);
      bad += hc != 0;
    }
  }
  CK(hipGetLastError());

  std::vector<float> ms[2][NVAR];
  for (int r = 0; r < rounds + 1; r++)
    for (int form = 0; form < 2; form++)
      for (int var = 0; var < NVAR; var++) {
        CK(hipEventRecord(e0, 0));
        launch(form, var, var == 0 ? Xref : Xpk);
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        float t;
        CK(hipEventElapsedTime(&t, e0, e1));
        if (r > 0) ms[form][var].push_back(t);
      }
  const char *vn[NVAR] = {"1 plain fp32", "2 fmt0 b96/quad 4 waves", "3 fmt1 b128/lane 4 waves", "4 fmt0 b96/quad 3 waves",
                          "5 fmt1 b128/lane 3 waves"};
  for (int form = 0; form < 2; form++)
    for (int var = 0; var < NVAR; var++) {
      std::vector<float> s = ms[form][var];
      std::sort(s.begin(), s.end());
      const double med = s[s.size() / 2];
      const double src = var == 0 ? 4.0 * M * K : (double)pk[form][(var - 1) & 1].bytes;
      printf("%-8s %-26s median %.4f ms  min %.4f  max %.4f  source %.3f GB  %.2f TB/s  all:", form ? "batched" : "suffix",
             vn[var], med, s.front(), s.back(), src / 1e9, src / (med * 1e-3) / 1e12);
      for (float t : ms[form][var]) printf(" %.4f", t);
      printf("\n");
    }
  return bad ? 1 : 0;
}
