// kernels_model.hip.h — a decomposition's model, or its residual V - model, stored through a strided
// device view (ppals_cp_export_model_device / ppals_tucker_export_model_device, include/ppals.h).
//
// One kernel family: a thin-K product stored through a view (ModelPlan, device_view.h):
//   dst[voff + offA(a) + offB(b)] = sum_k Q[a + ldq*k] * P[(b % pL) + pLK*(b / pL) + pL*k]
// or, for the residual, V[roff + rA(a) + rB(b)] minus that sum, V the resident shard as stored.
// The products and sums are fp64 on v_mfma_f64_16x16x4_f64 and each element is rounded once to the
// destination type. A is the view's fast side: its modes are the view's unit-stride run, so a wave's
// stores walk consecutive addresses.
//
// Tiling: a workgroup owns 64 values of a (its Q rows stay in registers when K <= 4 * MAXRB) and walks
// 64 x 64 tiles along b. Wave w multiplies b rows [16w, 16w + 16) of the tile against the 4 column
// blocks of 16 a: the f64 MFMA layout (A operand = P: row lane&15, k lane>>4; B operand = Q: k lane>>4,
// column lane&15; D: column lane&15, row (lane>>4) + 4 reg) puts the lane's results at
// (b = 16w + (lane>>4) + 4 reg, a = 16t + lane&15). The tile goes through LDS ([b][a], fp64, padded
// row) and leaves with the lane index along a: 16-byte stores when the view allows them. The residual
// reads V along a when the shard is contiguous there, otherwise along b (lane index along b, into the
// LDS image) before the store pass — the two sides of the tile are then each accessed coalesced.
//
// The impute modes (ppals_cp_impute_device) turn the kernel round: dst is the resident shard itself
// (group A along the SHARD's fast side, the plan of dv_model_swapped) and the side read beside it is a
// mask view of one byte per element. The store pass keeps the lane index along a and stores the model,
// rounded once to the storage type, where the mask byte is 0: one plain vector store per lane under the
// lane's own predicate, nothing else of the shard is written. The mask bytes come in along a when the
// mask is unit-stride there, otherwise along b through a byte image in LDS (as the residual reads V).
// With the observed residual wanted, a lane whose byte is non-zero reads V instead and adds
// (V - model)^2 to its sum; the workgroup's sum goes to part[workgroup] and k_sum_partials adds those in
// a fixed order.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "bf16.h"
#include "device_view.h"
#include "kernels_small.hip.h"  // block_sum (hip_ops.hip includes ops.h ahead of the kernel headers)

namespace ppals {

typedef double mv_f64x4 __attribute__((ext_vector_type(4)));

constexpr int MV_TILE = 64;
// what k_model_view stores: the model, V - model, or the model into the shard where a mask byte is 0
// (MV_IMPUTE_SQ: and the sum of (V - model)^2 over the other elements)
enum { MV_MODEL = 0, MV_RESIDUAL = 1, MV_IMPUTE = 2, MV_IMPUTE_SQ = 3 };

// ov[i] / orr[i] = view / shard offset of flat index i of a mode group (first listed mode fastest)
__global__ __launch_bounds__(256) void k_model_offsets(ModelGroup g, int64_t *__restrict__ ov,
                                                       int64_t *__restrict__ orr) {
  const int64_t nth = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < g.count; e += nth) {
    int64_t idx = e, v = 0, r = 0;
#pragma unroll
    for (int m = 0; m < DV_MAX_ORDER; m++)
      if (m < g.n) {
        const int64_t q = idx / g.len[m], c = idx - q * g.len[m];
        v += c * g.vs[m];
        r += c * g.rs[m];
        idx = q;
      }
    ov[e] = v;
    orr[e] = r;
  }
}

template <typename T>
__device__ __forceinline__ double mv_load(const T *p) {
  return (double)*p;
}
template <>
__device__ __forceinline__ double mv_load<bf16s>(const bf16s *p) {
  return (double)__uint_as_float((uint32_t)p->u << 16);
}

template <typename T>
struct alignas(16) mv_vec {
  T v[16 / sizeof(T)];
};

// The store pass of the impute modes, lane index along a, shared by k_model_view and k_model_impute_wide:
// img the tile's fp64 image ([b][a]), mimg the byte image the mask goes through when it is not unit-stride
// along a, sav / sbv the shard's offsets and sar / sbr the mask's. SQ: the lanes of observed elements
// read V and add (V - model)^2 to acc.
template <typename D, bool SQ>
__device__ __forceinline__ void mv_impute_store(D *dst, const uint8_t *V, const ModelPlan &mp,
                                                const double (*img)[MV_TILE + 1],
                                                uint8_t (*mimg)[MV_TILE + 4], const int64_t *sav,
                                                const int64_t *sar, const int64_t *sbv, const int64_t *sbr,
                                                int64_t a0, int na, int nb, bool a_unit, bool v_along_a,
                                                double &acc) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // Every load of a pass is issued before anything depends on one (a rejected element reads the
  // tile's first, which exists): a load behind a branch, or behind a store it might alias, would
  // wait out one memory latency per row, 16 of them per tile.
  constexpr int NR = MV_TILE / 4;
  const int64_t m0 = mp.roff + sar[0] + sbr[0];
  if (!v_along_a) {  // the mask bytes with the lane index along b
    uint8_t mb[NR];
#pragma unroll
    for (int i = 0; i < NR; i++) {
      const int al = wave + 4 * i;
      mb[i] = V[(al < na && lane < nb) ? mp.roff + sar[al] + sbr[lane] : m0];
    }
#pragma unroll
    for (int i = 0; i < NR; i++) mimg[lane][wave + 4 * i] = mb[i];
    __syncthreads();
  }
  const int al = lane;
  const int64_t oa = a_unit ? a0 + al : sav[al < na ? al : 0];
  const int64_t o0 = mp.voff + sbv[0] + (a_unit ? a0 : sav[0]);
  // (in two halves of 8 rows: 16 rows of addresses and values in flight cost the second wave per SIMD)
#pragma unroll
  for (int h = 0; h < 2; h++) {
    constexpr int NH = NR / 2;
    uint8_t m[NH];
    D v[NH];
#pragma unroll
    for (int i = 0; i < NH; i++) {
      const int bl = wave + 4 * (NH * h + i);
      const bool ok = al < na && bl < nb;
      m[i] = v_along_a ? V[ok ? mp.roff + sbr[bl] + sar[al] : m0] : mimg[bl][al];
      if (SQ) v[i] = dst[ok ? mp.voff + sbv[bl] + oa : o0];
    }
#pragma unroll
    for (int i = 0; i < NH; i++) {
      const int bl = wave + 4 * (NH * h + i);
      if (al < na && bl < nb) {
        if (m[i] == 0) {
          dst[mp.voff + sbv[bl] + oa] = (D)img[bl][al];
        } else if (SQ) {
          const double r = mv_load(&v[i]) - img[bl][al];
          acc += r * r;
        }
      }
    }
  }
}

// The export modes (MV_MODEL, MV_RESIDUAL). D: destination element type (float / double); TV: the
// shard's storage type (read by the residual only); MAXRB: 4-wide contraction steps held in registers
// (more: Q is reloaded per chunk of MAXRB steps). flags: bit 0 the view is unit-stride over A
// (offA(a) = a); bit 1 16-byte stores (bit 0, and A, voff and every offB a multiple of the vector, dst
// aligned); bit 2 the shard is contiguous over A (rA(a) = a: the residual reads V in the store pass). V
// may be dst itself (the second pass of the two-pass residual, dst -= model: shard offsets = view
// offsets): every element is read and then written by the same thread, or read before and written
// after a barrier.
//
// The impute modes (MV_IMPUTE, MV_IMPUTE_SQ) run on the plan of dv_model_swapped, so every name above
// keeps its place and changes its tenant: dst (type D) is the shard, V (TV = uint8_t) the mask, the
// "view" offsets (tav, tbv, voff, bit 0) are the shard's and the "shard" offsets (tar, tbr, roff, bit 2)
// the mask's; bit 1 is never set. part: one sum per workgroup, MV_IMPUTE_SQ only.
// With Q in registers (MAXRB = 4) the impute modes ask for two waves per SIMD, as the export modes get
// unasked; without the bound the compiler went past 256 registers (one wave per SIMD, one workgroup
// per CU). MAXRB = 16 (R > 16) spills in every mode, the export's included.
template <typename D, typename TV, int MODE, int MAXRB>
__global__ __launch_bounds__(256, (MODE >= MV_IMPUTE && MAXRB <= 4) ? 2 : 1) void k_model_view(
    D *dst, const TV *V, const double *__restrict__ Q, const double *__restrict__ P, int K, ModelPlan mp,
    const int64_t *__restrict__ tav, const int64_t *__restrict__ tar, const int64_t *__restrict__ tbv,
    const int64_t *__restrict__ tbr, int flags, double *__restrict__ part) {
  constexpr bool RES = MODE == MV_RESIDUAL, IMP = MODE == MV_IMPUTE || MODE == MV_IMPUTE_SQ;
  __shared__ double img[MV_TILE][MV_TILE + 1];
  __shared__ uint8_t mimg[IMP ? MV_TILE : 1][IMP ? MV_TILE + 4 : 1];
  double acc = 0.0;  // MV_IMPUTE_SQ: this thread's share of the observed residual
  __shared__ int64_t sav[MV_TILE], sar[MV_TILE], sbv[MV_TILE], sbr[MV_TILE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, j16 = lane & 15;
  const int64_t A = mp.ga.count, B = mp.gb.count, a0 = (int64_t)blockIdx.x * MV_TILE;
  const int na = (int)min((int64_t)MV_TILE, A - a0);
  const int RB = (K + 3) / 4;
  const bool a_unit = flags & 1, vec_st = flags & 2, v_along_a = flags & 4;
  const int64_t nbt = (B + MV_TILE - 1) / MV_TILE;

  // q[t][rb] = Q[a0 + 16t + j16, 4 (c0 + rb) + g] of the rank chunk that starts at step c0 (0 outside)
  double q[4][MAXRB];
#define PPALS_MV_LOAD_Q(c0_)                                                     \
  _Pragma("unroll") for (int t = 0; t < 4; t++) {                                \
    const int64_t a_ = a0 + 16 * t + j16;                                        \
    _Pragma("unroll") for (int rb = 0; rb < MAXRB; rb++) {                       \
      const int k_ = 4 * ((c0_) + rb) + g;                                       \
      q[t][rb] = (a_ < A && k_ < K) ? Q[a_ + mp.ldq * (int64_t)k_] : 0.0;        \
    }                                                                            \
  }
  if (RB <= MAXRB) PPALS_MV_LOAD_Q(0);
  if (threadIdx.x < MV_TILE) {
    const int i = threadIdx.x;
    sav[i] = i < na ? tav[a0 + i] : 0;
    sar[i] = i < na ? tar[a0 + i] : 0;
  }
  // pn[rb] = P[b, 4 rb + g] of this lane's row b = 16 wave + j16 of tile tb_ (0 outside); loaded a tile
  // ahead, with the tile's b offsets (threads 64..127), so that their latency hides behind a tile's work
#define PPALS_MV_LOAD_P(tb_, c0_, pn_)                                                   \
  {                                                                                      \
    const int64_t b_ = (tb_) * MV_TILE + 16 * wave + j16;                                \
    const bool ok_ = (tb_) < nbt && b_ < B;                                              \
    const int64_t q_ = ok_ ? b_ / mp.pL : 0;                                             \
    const double *pr_ = P + (ok_ ? (b_ - q_ * mp.pL) + mp.pLK * q_ : 0);                 \
    _Pragma("unroll") for (int rb = 0; rb < MAXRB; rb++) {                               \
      const int k_ = 4 * ((c0_) + rb) + g;                                               \
      pn_[rb] = (ok_ && k_ < K) ? pr_[mp.pL * (int64_t)k_] : 0.0;                        \
    }                                                                                    \
  }
  double pn[MAXRB];
  int64_t nbv = 0, nbr = 0;
  const int ib = (int)threadIdx.x - MV_TILE;  // threads 64..127: the b offsets
  auto load_b = [&](int64_t tb_) {
    const int64_t bb = tb_ * MV_TILE + ib;
    const bool ok = ib >= 0 && ib < MV_TILE && tb_ < nbt && bb < B;
    nbv = ok ? tbv[bb] : 0;
    nbr = ok ? tbr[bb] : 0;
  };
  if (RB <= MAXRB) PPALS_MV_LOAD_P((int64_t)blockIdx.y, 0, pn);
  load_b(blockIdx.y);

  for (int64_t tb = blockIdx.y; tb < nbt; tb += gridDim.y) {
    const int64_t b0 = tb * MV_TILE;
    const int nb = (int)min((int64_t)MV_TILE, B - b0);
    if (ib >= 0 && ib < MV_TILE) {
      sbv[ib] = nbv;
      sbr[ib] = nbr;
    }
    load_b(tb + gridDim.y);
    mv_f64x4 d[4];
#pragma unroll
    for (int t = 0; t < 4; t++) d[t] = mv_f64x4{0.0, 0.0, 0.0, 0.0};
    if (RB <= MAXRB) {
      double pa[MAXRB];
#pragma unroll
      for (int rb = 0; rb < MAXRB; rb++) pa[rb] = pn[rb];
      PPALS_MV_LOAD_P(tb + gridDim.y, 0, pn);
#pragma unroll
      for (int rb = 0; rb < MAXRB; rb++) {
        if (rb < RB) {
#pragma unroll
          for (int t = 0; t < 4; t++)
            d[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[rb], q[t][rb], d[t], 0, 0, 0);
        }
      }
    } else {  // more rank steps than registers: Q and P chunk by chunk
      for (int c0 = 0; c0 < RB; c0 += MAXRB) {
        PPALS_MV_LOAD_Q(c0);
        double pa[MAXRB];
        PPALS_MV_LOAD_P(tb, c0, pa);
#pragma unroll
        for (int rb = 0; rb < MAXRB; rb++) {
          if (c0 + rb < RB) {
#pragma unroll
            for (int t = 0; t < 4; t++)
              d[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[rb], q[t][rb], d[t], 0, 0, 0);
          }
        }
      }
    }
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
      for (int r = 0; r < 4; r++) img[16 * wave + g + 4 * r][16 * t + j16] = d[t][r];
    __syncthreads();
    if (RES && !v_along_a) {  // V - model with the lane index along b
      for (int i = 0; i < MV_TILE / 4; i++) {
        const int al = wave + 4 * i, bl = lane;
        if (al < na && bl < nb) img[bl][al] = mv_load(V + (mp.roff + sar[al] + sbr[bl])) - img[bl][al];
      }
      __syncthreads();
    }
    // the store pass, lane index along a
    if constexpr (IMP) {
      mv_impute_store<D, MODE == MV_IMPUTE_SQ>(dst, V, mp, img, mimg, sav, sar, sbv, sbr, a0, na, nb, a_unit,
                                               v_along_a, acc);
    } else if (vec_st) {
      constexpr int VW = 16 / sizeof(D), TPR = MV_TILE / VW, RPP = 256 / TPR;
      const int al = (threadIdx.x % TPR) * VW;
      for (int bl = threadIdx.x / TPR; bl < nb; bl += RPP) {
        if (al < na) {
          mv_vec<D> o;
#pragma unroll
          for (int e = 0; e < VW; e++) {
            double x = img[bl][al + e];
            if (RES && v_along_a) x = mv_load(V + (mp.roff + sbr[bl] + a0 + al + e)) - x;
            o.v[e] = (D)x;
          }
          *reinterpret_cast<mv_vec<D> *>(dst + (mp.voff + sbv[bl] + a0 + al)) = o;
        }
      }
    } else {
      const int al = lane;
      for (int bl = wave; bl < nb; bl += 4) {
        if (al < na) {
          double x = img[bl][al];
          if (RES && v_along_a) x = mv_load(V + (mp.roff + sbr[bl] + sar[al])) - x;
          dst[mp.voff + sbv[bl] + (a_unit ? a0 + al : sav[al])] = (D)x;
        }
      }
    }
    __syncthreads();  // the image and the b offsets are rewritten by the next tile
  }
  if constexpr (MODE == MV_IMPUTE_SQ) {
    acc = block_sum(acc, &img[0][0]);
    if (threadIdx.x == 0) part[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = acc;
  }
#undef PPALS_MV_LOAD_Q
#undef PPALS_MV_LOAD_P
}

// The impute modes for K > 16 without spilling (ppals_tucker_impute_device: K is the leading mode's core
// rank, 17 .. 112). Same contract as the impute modes of k_model_view (the plan of dv_model_swapped, flags
// bits 0 and 2, part: one sum per workgroup with SQ), the same tiling, the same order of the sums over k
// and the same store pass; what differs is where the operands live:
//   Q: the workgroup's 64 rows, all K columns (rounded up to 4, zeros outside), staged ONCE in LDS as
//      qs[k][a] with rows of MW_LDQ = 80 doubles. The MFMA's B operand reads (k = 4 rb + (lane >> 4),
//      a = 16 t + (lane & 15)) with ds_read_b64, whose banks are (address / 4) % 64 per 32-lane half: a
//      half holds 16 consecutive a of two neighbouring k, at doubles 80 k + a and 80 (k + 1) + a, i.e.
//      32 different residues mod 32 because 80 = 16 mod 32. An unpadded row (64) would be 2-way. (Where
//      the compiler pairs two of a lane's reads into ds_read2_b64, that instruction serves 16 consecutive
//      lanes at a time, 16 consecutive a of one k: conflict-free under its rule too.)
//   P: from global memory, MW_CH = 4 steps (16 k) per lane at a time, the next chunk (of this tile, or the
//      first of the workgroup's next tile) loaded before the MFMAs of the current one.
// All LDS is dynamic (one region, so the image is 16-byte aligned whatever the statics would total):
// mw_lds_bytes(K) = 640 B per k of Q + 39680 B (the 64 x 65 fp64 image, 4 x 64 offsets, the byte image):
// 51.25 KB at K = 17 .. 20, 108.75 KB at K = 112 = MW_KMAX, the largest core rank the sweeps admit. The
// launch bound asks for 3 waves per SIMD (at most 168 registers; the kernel takes about 150, no scratch),
// i.e. 3 workgroups per CU; of the CU's 160 KB the LDS admits 3 up to K = 20, 2 up to K = 64 and 1
// above (mw_wgs_per_cu, which sizes the grid).
constexpr int MW_LDQ = MV_TILE + 16;
constexpr int MW_CH = 4;
constexpr int MW_KMAX = 112;
constexpr size_t MW_LDS_FIXED = sizeof(double) * MV_TILE * (MV_TILE + 1) + sizeof(int64_t) * 4 * MV_TILE +
                                (size_t)MV_TILE * (MV_TILE + 4);
inline size_t mw_lds_bytes(int K) { return sizeof(double) * MW_LDQ * (size_t)(4 * ((K + 3) / 4)) + MW_LDS_FIXED; }
inline int mw_wgs_per_cu(int K) { return (int)std::min<size_t>(3, (size_t)160 * 1024 / mw_lds_bytes(K)); }

template <typename D, bool SQ>
__global__ __launch_bounds__(256, 3) void k_model_impute_wide(
    D *dst, const uint8_t *V, const double *__restrict__ Q, const double *__restrict__ P, int K, ModelPlan mp,
    const int64_t *__restrict__ tav, const int64_t *__restrict__ tar, const int64_t *__restrict__ tbv,
    const int64_t *__restrict__ tbr, int flags, double *__restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) unsigned char mw_lds[];
  const int RB = (K + 3) / 4;
  double *qs = reinterpret_cast<double *>(mw_lds);  // [4 RB][MW_LDQ]
  double(*img)[MV_TILE + 1] = reinterpret_cast<double(*)[MV_TILE + 1]>(qs + (size_t)4 * RB * MW_LDQ);
  int64_t *sav = reinterpret_cast<int64_t *>(img + MV_TILE), *sar = sav + MV_TILE, *sbv = sar + MV_TILE,
          *sbr = sbv + MV_TILE;
  uint8_t(*mimg)[MV_TILE + 4] = reinterpret_cast<uint8_t(*)[MV_TILE + 4]>(sbr + MV_TILE);
  double acc = 0.0;  // SQ: this thread's share of the observed residual
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, j16 = lane & 15;
  const int64_t A = mp.ga.count, B = mp.gb.count, a0 = (int64_t)blockIdx.x * MV_TILE;
  const int na = (int)min((int64_t)MV_TILE, A - a0);
  const bool a_unit = flags & 1, v_along_a = flags & 4;
  const int64_t nbt = (B + MV_TILE - 1) / MV_TILE;

  for (int e = threadIdx.x; e < 4 * RB * MV_TILE; e += 256) {  // the Q image: 4 rows of k per pass
    const int k = e / MV_TILE, al = e % MV_TILE;
    qs[k * MW_LDQ + al] = (al < na && k < K) ? Q[a0 + al + mp.ldq * (int64_t)k] : 0.0;
  }
  if (threadIdx.x < MV_TILE) {
    const int i = threadIdx.x;
    sav[i] = i < na ? tav[a0 + i] : 0;
    sar[i] = i < na ? tar[a0 + i] : 0;
  }
  // this lane's row b = 16 wave + j16 of tile tb_ in P (nullptr outside), and a chunk of it:
  // p[rb] = P[b, 4 (c0 + rb) + g] (0 outside)
  auto p_row = [&](int64_t tb_) -> const double * {
    const int64_t b_ = tb_ * MV_TILE + 16 * wave + j16;
    if (tb_ >= nbt || b_ >= B) return nullptr;
    const int64_t q_ = b_ / mp.pL;
    return P + ((b_ - q_ * mp.pL) + mp.pLK * q_);
  };
  auto p_chunk = [&](const double *row, int c0, double(&p)[MW_CH]) {
#pragma unroll
    for (int rb = 0; rb < MW_CH; rb++) {
      const int k_ = 4 * (c0 + rb) + g;
      p[rb] = (row && k_ < K) ? row[mp.pL * (int64_t)k_] : 0.0;
    }
  };
  int64_t nbv = 0, nbr = 0;
  const int ib = (int)threadIdx.x - MV_TILE;  // threads 64..127: the b offsets, a tile ahead
  auto load_b = [&](int64_t tb_) {
    const int64_t bb = tb_ * MV_TILE + ib;
    const bool ok = ib >= 0 && ib < MV_TILE && tb_ < nbt && bb < B;
    nbv = ok ? tbv[bb] : 0;
    nbr = ok ? tbr[bb] : 0;
  };
  const double *prow = p_row(blockIdx.y);
  double pn[MW_CH];
  p_chunk(prow, 0, pn);
  load_b(blockIdx.y);
  __syncthreads();  // the Q image is complete

  for (int64_t tb = blockIdx.y; tb < nbt; tb += gridDim.y) {
    const int nb = (int)min((int64_t)MV_TILE, B - tb * MV_TILE);
    if (ib >= 0 && ib < MV_TILE) {
      sbv[ib] = nbv;
      sbr[ib] = nbr;
    }
    load_b(tb + gridDim.y);
    const double *pnext = p_row(tb + gridDim.y);
    mv_f64x4 d[4];
#pragma unroll
    for (int t = 0; t < 4; t++) d[t] = mv_f64x4{0.0, 0.0, 0.0, 0.0};
    for (int c0 = 0; c0 < RB; c0 += MW_CH) {
      double pa[MW_CH];
#pragma unroll
      for (int rb = 0; rb < MW_CH; rb++) pa[rb] = pn[rb];
      if (c0 + MW_CH < RB)
        p_chunk(prow, c0 + MW_CH, pn);
      else
        p_chunk(pnext, 0, pn);
#pragma unroll
      for (int rb = 0; rb < MW_CH; rb++) {
        if (c0 + rb < RB) {
          const double *qk = qs + (4 * (c0 + rb) + g) * MW_LDQ + j16;
#pragma unroll
          for (int t = 0; t < 4; t++)
            d[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[rb], qk[16 * t], d[t], 0, 0, 0);
        }
      }
    }
    prow = pnext;
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
      for (int r = 0; r < 4; r++) img[16 * wave + g + 4 * r][16 * t + j16] = d[t][r];
    __syncthreads();
    mv_impute_store<D, SQ>(dst, V, mp, img, mimg, sav, sar, sbv, sbr, a0, na, nb, a_unit, v_along_a, acc);
    __syncthreads();  // the image and the b offsets are rewritten by the next tile
  }
  if constexpr (SQ) {
    acc = block_sum(acc, &img[0][0]);
    if (threadIdx.x == 0) part[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = acc;
  }
}

}  // namespace ppals
