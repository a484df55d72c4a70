// kernels_tucker_slices.hip.h — the tensor pass of a Tucker session's influence plot (Ops::model_slice_sums;
// include/ppals.h, "Tucker: residual, per-slice residuals and leverages"): with
//   e(a, b) = V[roff + rA(a) + rB(b)] - sum_{k<K} Q[a + ldq*k] * P[(b % pL) + pLK*(b / pL) + pL*k]
// (V the resident shard as stored, everything else fp64; the plan of TuckerEngine::impute: group A is mode
// 0, the shard's fast side, group B the other modes in the shard's order) it keeps
//   asq[a] = sum_b e^2,   bsq[b] = sum_a e^2
// and stores nothing else. The products and differences run on v_mfma_f64_16x16x4_f64 with the tiling, the
// MFMA layout and the order of the sum over k of the imputation (kernels_model.hip.h): a workgroup owns 64
// values of a and walks 64 x 64 tiles along b, tile tb = blockIdx.y, blockIdx.y + gridDim.y, ...; the tile
// goes through the LDS image ([b][a], fp64) and is read back with the lane index along a, where V is read.
//   k_model_slices       K <= 16: the workgroup's rows of Q in registers. Any larger K as well, Q and P then
//                        reloaded in chunks of 16 k per tile (K > 112, which set_factors admits and no
//                        sweep does: correct, not fast, and without scratch).
//   k_model_slices_wide  16 < K <= 112: Q staged once in LDS, the layout of k_model_impute_wide.
//
// Sums, all fp64, no atomics. In the pass over a tile the thread (lane = a, wave w) owns rows b = w + 4 i of
// the tile: it adds e^2 to its running row sum (over all the tiles the workgroup walks, in walking order) and
// puts e^2 back into the image. After a barrier thread t adds the 16 values a = 16 (t & 3) .. + 15 of column
// b = t >> 2 in ascending a; the four quarters are added as (q0 + q1) + (q2 + q3). At the end the four waves'
// row sums are added in wave order.
//
// Partial layout of ONE launch — nt consecutive row tiles [t0, t0 + nt) (rows [64 t0, 64 t0 + rows)) by all B
// columns of the slab, gridDim.y = gy workgroups a row tile:
//   rowpart[y * rp_ld + (a - 64 t0)]   the sum of e^2 of row a over the tiles y, y + gy, ... of the slab
//   colpart[(t - t0) * B + b]          the sum of e^2 of column b over the 64 rows of tile t
// k_slice_fold (kernels_slices.hip.h) adds them in index order ONTO what came before: asq[a] is one running
// sum over the slabs in slab order and, within a slab, over y; bsq[b] one over all row tiles in tile order,
// however the tiles are cut into launches. gy follows from the slab's geometry alone (Ops::model_slice_sums),
// so a cap on the partials that cuts a slab's row tiles into several launches changes no bit.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "kernels_model.hip.h"

namespace ppals {

// The pass over one tile whose model is in img (after a barrier): see the top of this file. colpart points at
// the tile's first column. Ends with the column stores; the caller's barrier follows before img is rewritten.
template <typename TV>
__device__ __forceinline__ void ts_tile_sums(const TV *__restrict__ V, int64_t roff, double (*img)[MV_TILE + 1],
                                             const int64_t *sar, const int64_t *sbr, int na, int nb,
                                             double &racc, double *__restrict__ colpart) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  constexpr int NR = MV_TILE / 4, NH = NR / 2;
  const int al = lane;
  // Every load of a pass is issued before anything depends on one (mv_impute_store); an element outside
  // the tile reads the tile's first, which exists. In two halves of 8 rows, as there.
  const int64_t v0 = roff + sar[0] + sbr[0];
  const int64_t oa = sar[al < na ? al : 0];
#pragma unroll
  for (int h = 0; h < 2; h++) {
    TV v[NH];
#pragma unroll
    for (int i = 0; i < NH; i++) {
      const int bl = wave + 4 * (NH * h + i);
      v[i] = V[(al < na && bl < nb) ? roff + sbr[bl] + oa : v0];
    }
#pragma unroll
    for (int i = 0; i < NH; i++) {
      const int bl = wave + 4 * (NH * h + i);
      const double e = mv_load(&v[i]) - img[bl][al];
      const double e2 = (al < na && bl < nb) ? e * e : 0.0;
      racc += e2;
      img[bl][al] = e2;
    }
  }
  __syncthreads();
  const int cb = threadIdx.x >> 2, cq = threadIdx.x & 3;
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < 16; j++) s += img[cb][16 * cq + j];
  s += __shfl_xor(s, 1, 64);
  s += __shfl_xor(s, 2, 64);
  if (cq == 0 && cb < nb) colpart[cb] = s;
}

// the four waves' row sums in wave order (red: 4 x 64 doubles of LDS that nothing else uses any more)
__device__ __forceinline__ void ts_row_sums(double racc, double *red, int na, double *__restrict__ rowpart) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  red[wave * MV_TILE + lane] = racc;
  __syncthreads();
  if ((int)threadIdx.x < na)
    rowpart[threadIdx.x] = ((red[threadIdx.x] + red[MV_TILE + threadIdx.x]) + red[2 * MV_TILE + threadIdx.x]) +
                           red[3 * MV_TILE + threadIdx.x];
}

// TV: the shard's storage type (float / double). tar / tbr: the shard offsets of the flat indices of groups
// A and B (k_model_offsets). t0: the first row tile of the launch. Two waves per SIMD are asked for, as the
// imputation's K <= 16 route asks.
constexpr int TS_RB = 4;  // 4-wide contraction steps held in registers
template <typename TV>
__global__ __launch_bounds__(256, 2) void k_model_slices(
    const TV *__restrict__ V, const double *__restrict__ Q, const double *__restrict__ P, int K, ModelPlan mp,
    const int64_t *__restrict__ tar, const int64_t *__restrict__ tbr, int64_t t0, int64_t rp_ld,
    double *__restrict__ rowpart, double *__restrict__ colpart) {
  __shared__ double img[MV_TILE][MV_TILE + 1];
  __shared__ int64_t sar[MV_TILE], sbr[MV_TILE];
  double racc = 0.0;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int g = lane >> 4, j16 = lane & 15;
  const int64_t A = mp.ga.count, B = mp.gb.count, a0 = (t0 + blockIdx.x) * MV_TILE;
  const int na = (int)min((int64_t)MV_TILE, A - a0);
  const int RB = (K + 3) / 4;
  const int64_t nbt = (B + MV_TILE - 1) / MV_TILE;

  // q[t][rb] = Q[a0 + 16t + j16, 4 (c0 + rb) + g] of the rank chunk that starts at step c0 (0 outside)
  double q[4][TS_RB];
  auto load_q = [&](int c0) {
#pragma unroll
    for (int t = 0; t < 4; t++) {
      const int64_t a_ = a0 + 16 * t + j16;
#pragma unroll
      for (int rb = 0; rb < TS_RB; rb++) {
        const int k_ = 4 * (c0 + rb) + g;
        q[t][rb] = (a_ < A && k_ < K) ? Q[a_ + mp.ldq * (int64_t)k_] : 0.0;
      }
    }
  };
  // p[rb] = P[b, 4 (c0 + rb) + g] of this lane's row b = 16 wave + j16 of tile tb_ (0 outside)
  auto load_p = [&](int64_t tb_, int c0, double(&p)[TS_RB]) {
    const int64_t b_ = tb_ * MV_TILE + 16 * wave + j16;
    const bool ok_ = tb_ < nbt && b_ < B;
    const int64_t q_ = ok_ ? b_ / mp.pL : 0;
    const double *pr_ = P + (ok_ ? (b_ - q_ * mp.pL) + mp.pLK * q_ : 0);
#pragma unroll
    for (int rb = 0; rb < TS_RB; rb++) {
      const int k_ = 4 * (c0 + rb) + g;
      p[rb] = (ok_ && k_ < K) ? pr_[mp.pL * (int64_t)k_] : 0.0;
    }
  };
  if (RB <= TS_RB) load_q(0);
  if (threadIdx.x < MV_TILE) sar[threadIdx.x] = (int)threadIdx.x < na ? tar[a0 + threadIdx.x] : 0;
  // the next tile's P rows and b offsets (threads 64..127) are loaded a tile ahead
  double pn[TS_RB];
  int64_t nbr = 0;
  const int ib = (int)threadIdx.x - MV_TILE;
  auto load_b = [&](int64_t tb_) {
    const int64_t bb = tb_ * MV_TILE + ib;
    nbr = (ib >= 0 && ib < MV_TILE && tb_ < nbt && bb < B) ? tbr[bb] : 0;
  };
  if (RB <= TS_RB) load_p((int64_t)blockIdx.y, 0, pn);
  load_b(blockIdx.y);

  for (int64_t tb = blockIdx.y; tb < nbt; tb += gridDim.y) {
    const int nb = (int)min((int64_t)MV_TILE, B - tb * MV_TILE);
    if (ib >= 0 && ib < MV_TILE) sbr[ib] = nbr;
    load_b(tb + gridDim.y);
    mv_f64x4 d[4];
#pragma unroll
    for (int t = 0; t < 4; t++) d[t] = mv_f64x4{0.0, 0.0, 0.0, 0.0};
    if (RB <= TS_RB) {
      double pa[TS_RB];
#pragma unroll
      for (int rb = 0; rb < TS_RB; rb++) pa[rb] = pn[rb];
      load_p(tb + gridDim.y, 0, pn);
#pragma unroll
      for (int rb = 0; rb < TS_RB; rb++) {
        if (rb < RB) {
#pragma unroll
          for (int t = 0; t < 4; t++)
            d[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[rb], q[t][rb], d[t], 0, 0, 0);
        }
      }
    } else {  // more rank steps than registers: Q and P chunk by chunk
      for (int c0 = 0; c0 < RB; c0 += TS_RB) {
        load_q(c0);
        double pa[TS_RB];
        load_p(tb, c0, pa);
#pragma unroll
        for (int rb = 0; rb < TS_RB; rb++) {
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
    ts_tile_sums(V, mp.roff, img, sar, sbr, na, nb, racc, colpart + (int64_t)blockIdx.x * B + tb * MV_TILE);
    __syncthreads();  // the image and the b offsets are rewritten by the next tile
  }
  ts_row_sums(racc, &img[0][0], na, rowpart + (int64_t)blockIdx.y * rp_ld + (int64_t)blockIdx.x * MV_TILE);
}

// 16 < K <= MW_KMAX: Q in LDS as k_model_impute_wide holds it (qs[k][a], rows of MW_LDQ doubles: the bank
// argument is there), P from global memory MW_CH steps at a time, a chunk ahead. All LDS is dynamic:
// ts_lds_bytes(K) = 640 B per k of Q + 34304 B (the 64 x 65 fp64 image and the two offset tables): 46 KB at
// K = 17 .. 20, 103.5 KB at K = 112. The launch bound asks for 3 waves per SIMD, as the imputation's; of the
// CU's 160 KB the LDS admits 3 workgroups up to K = 28, 2 up to K = 72 and 1 above (ts_wgs_per_cu).
constexpr size_t TS_LDS_FIXED = sizeof(double) * MV_TILE * (MV_TILE + 1) + sizeof(int64_t) * 2 * MV_TILE;
inline size_t ts_lds_bytes(int K) { return sizeof(double) * MW_LDQ * (size_t)(4 * ((K + 3) / 4)) + TS_LDS_FIXED; }
inline int ts_wgs_per_cu(int K) { return (int)std::min<size_t>(3, (size_t)160 * 1024 / ts_lds_bytes(K)); }

template <typename TV>
__global__ __launch_bounds__(256, 3) void k_model_slices_wide(
    const TV *__restrict__ V, const double *__restrict__ Q, const double *__restrict__ P, int K, ModelPlan mp,
    const int64_t *__restrict__ tar, const int64_t *__restrict__ tbr, int64_t t0, int64_t rp_ld,
    double *__restrict__ rowpart, double *__restrict__ colpart) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ts_lds[];
  const int RB = (K + 3) / 4;
  double *qs = reinterpret_cast<double *>(ts_lds);  // [4 RB][MW_LDQ]
  double(*img)[MV_TILE + 1] = reinterpret_cast<double(*)[MV_TILE + 1]>(qs + (size_t)4 * RB * MW_LDQ);
  int64_t *sar = reinterpret_cast<int64_t *>(img + MV_TILE), *sbr = sar + MV_TILE;
  double racc = 0.0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, j16 = lane & 15;
  const int64_t A = mp.ga.count, B = mp.gb.count, a0 = (t0 + blockIdx.x) * MV_TILE;
  const int na = (int)min((int64_t)MV_TILE, A - a0);
  const int64_t nbt = (B + MV_TILE - 1) / MV_TILE;

  for (int e = threadIdx.x; e < 4 * RB * MV_TILE; e += 256) {  // the Q image: 4 rows of k per pass
    const int k = e / MV_TILE, al = e % MV_TILE;
    qs[k * MW_LDQ + al] = (al < na && k < K) ? Q[a0 + al + mp.ldq * (int64_t)k] : 0.0;
  }
  if (threadIdx.x < MV_TILE) sar[threadIdx.x] = (int)threadIdx.x < na ? tar[a0 + threadIdx.x] : 0;
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
  int64_t nbr = 0;
  const int ib = (int)threadIdx.x - MV_TILE;  // threads 64..127: the b offsets, a tile ahead
  auto load_b = [&](int64_t tb_) {
    const int64_t bb = tb_ * MV_TILE + ib;
    nbr = (ib >= 0 && ib < MV_TILE && tb_ < nbt && bb < B) ? tbr[bb] : 0;
  };
  const double *prow = p_row(blockIdx.y);
  double pn[MW_CH];
  p_chunk(prow, 0, pn);
  load_b(blockIdx.y);
  __syncthreads();  // the Q image is complete

  for (int64_t tb = blockIdx.y; tb < nbt; tb += gridDim.y) {
    const int nb = (int)min((int64_t)MV_TILE, B - tb * MV_TILE);
    if (ib >= 0 && ib < MV_TILE) sbr[ib] = nbr;
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
    ts_tile_sums(V, mp.roff, img, sar, sbr, na, nb, racc, colpart + (int64_t)blockIdx.x * B + tb * MV_TILE);
    __syncthreads();  // the image and the b offsets are rewritten by the next tile
  }
  ts_row_sums(racc, &img[0][0], na, rowpart + (int64_t)blockIdx.y * rp_ld + (int64_t)blockIdx.x * MV_TILE);
}

}  // namespace ppals
