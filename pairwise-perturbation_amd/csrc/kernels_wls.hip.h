// kernels_wls.hip.h — the majorization step of weighted CP (ppals_cp_wls_device, include/ppals.h): the
// resident shard rewritten with the working tensor of Kiers' majorization,
//   z = x           where h >= 1            (loss (x - m)^2)
//   z = m           where h <= 0 or NaN     (loss 0; x is not used)
//   z = fma(h, x - m, m)   otherwise        (loss h (x - m)^2)
// m the fp64 model sum_k Q[a, k] P[b, k] of the current factors, x and h the elements of two strided side
// views (data and weights, type TS) widened to fp64, z rounded once to the storage type D. Every element
// of the box is stored, so nothing is predicated and the loss costs no stream of its own: x and m are
// both in registers.
//
// Tiling, MFMA layout and the order of the sum over k are those of k_model_impute_wide
// (kernels_model.hip.h): a workgroup owns 64 values of a (group A, the SHARD's fast side), stages its Q
// rows once in LDS (qs[k][a], rows of MW_LDQ doubles), and walks 64 x 64 tiles along b; wave w multiplies
// b rows [16w, 16w + 16) against the 4 column blocks of 16 a in 4-wide v_mfma_f64_16x16x4_f64 steps, k
// ascending, P prefetched MW_CH steps at a time. With h in {0, 1} the stored values are therefore the
// imputation's, bit for bit. One kernel covers 1 <= K <= WL_KMAX = 128.
//
// The plan is the imputation's (dv_model_swapped: the kernel's "view" offsets tav / tbv / voff are the
// shard's, its "shard" offsets tax / tbx / roff the data view's) with a third table taw / tbw / woff for the
// weights (ModelSide, device_view.h). Each side view is read in one of two ways (dv_side_along_a):
//   along a: in the store pass, the lane index along a as for the stores. With the 16-byte store pass
//            (flags bit 1) a side that is unit-stride and aligned over A (bit 4 / bit 7) comes in as one
//            vector of VW elements per lane, any other as VW loads at its own offsets;
//   along b: before the store pass, the lane index along b (the view's unit-stride run leads group B), and
//            through LDS. Both sides along b: the arithmetic is done there, into the fp64 image, and the
//            store pass only rounds and stores. One side along b: its values wait in a typed image
//            (TS[64][65]) for the store pass, which reads the other side.
// A stride of 0 is one address for all lanes, in either pass: no path of its own. All loads of a pass
// (or of a half of it) are issued before anything depends on one; a lane outside the tile reads the
// tile's first element, which exists.
//
// The store pass: 16-byte stores, VW = 4 fp32 / 2 fp64 consecutive a per lane, when the shard is
// unit-stride over A and aligned (flags bit 1), else one element per lane at the shard's offsets.
//
// LDS, all dynamic:  wl_lds_bytes(K, side) = 640 B per k of Q (K rounded up to 4) + 33280 B (the 64 x 65
// fp64 image) + 3072 B (6 x 64 offsets) + side, side = 64 * 65 * sizeof(TS) when exactly one side view is
// read along b, else 0: at K <= 16 at most 10240 + 36352 + 33280 = 79872 B, so two workgroups fit the
// CU's 160 KiB (163840 B) under every layout; 151552 B at K = 128 with a typed fp64 image. The launch
// bound asks for 2 waves per SIMD (256 registers); no instantiation spills.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "device_view.h"
#include "kernels_model.hip.h"

namespace ppals {

constexpr int WL_KMAX = 128;
constexpr size_t WL_LDS_FIXED = sizeof(double) * MV_TILE * (MV_TILE + 1) + sizeof(int64_t) * 6 * MV_TILE;
inline size_t wl_lds_bytes(int K, size_t side_elem /* 0: no typed image */) {
  return sizeof(double) * MW_LDQ * (size_t)(4 * ((K + 3) / 4)) + WL_LDS_FIXED +
         side_elem * MV_TILE * (MV_TILE + 1);
}
inline int wl_wgs_per_cu(size_t lds) { return (int)std::max<size_t>(1, std::min<size_t>(2, (size_t)160 * 1024 / lds)); }

enum {
  WL_A_UNIT = 1, WL_VEC_ST = 2,
  WL_X_ALONG_A = 4, WL_X_UNIT = 8, WL_X_VEC = 16,
  WL_H_ALONG_A = 32, WL_H_UNIT = 64, WL_H_VEC = 128
};

// ov[i] = offset of flat index i of a mode group under the strides g.vs (the third table: the weights)
__global__ __launch_bounds__(256) void k_model_offsets_side(ModelGroup g, int64_t *__restrict__ ov) {
  const int64_t nth = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < g.count; e += nth) {
    int64_t idx = e, v = 0;
#pragma unroll
    for (int m = 0; m < DV_MAX_ORDER; m++)
      if (m < g.n) {
        const int64_t q = idx / g.len[m], c = idx - q * g.len[m];
        v += c * g.vs[m];
        idx = q;
      }
    ov[e] = v;
  }
}

// the per-element rule; adds the element's loss to acc
__device__ __forceinline__ double wl_rule(double x, double h, double m, double &acc) {
  if (!(h > 0.0)) return m;  // h <= 0 or NaN: x is not looked at
  const double d = x - m;
  if (h >= 1.0) {
    acc += d * d;
    return x;
  }
  acc += h * (d * d);
  return __fma_rn(h, d, m);
}

template <typename TS, int VW>
struct alignas((VW * sizeof(TS) > 16) ? 16 : VW * sizeof(TS)) wl_vec {
  TS v[VW];
};

// What the store pass reads of one side view: its pointer, offsets and how it comes in.
template <typename TS>
struct WlSide {
  const TS *p;
  const int64_t *sa, *sb;  // LDS: offsets of the tile's a / b
  int64_t off;             // roff / woff
  bool in_lds, unit, vec;  // in the typed image; offA(a) = a; one vector per lane
};

// One side's VW elements of row bl for this lane (al .. al + VW - 1), from global memory. ok: inside the tile.
template <typename TS, int VW>
__device__ __forceinline__ void wl_load(const WlSide<TS> &s, int64_t a0, int al, int bl, bool ok, TS (&o)[VW]) {
  if (VW > 1 && s.vec) {
    const wl_vec<TS, VW> t =
        *reinterpret_cast<const wl_vec<TS, VW> *>(s.p + (s.off + s.sb[ok ? bl : 0] + a0 + (ok ? al : 0)));
#pragma unroll
    for (int e = 0; e < VW; e++) o[e] = t.v[e];
  } else {
#pragma unroll
    for (int e = 0; e < VW; e++) {
      const int ae = ok ? al + e : 0;
      o[e] = s.p[s.off + s.sb[ok ? bl : 0] + (s.unit ? a0 + ae : s.sa[ae])];
    }
  }
}

// The store pass. VW = 1: lane index along a, rows wave, wave + 4, ...; VW > 1: 64 / VW lanes a row, 16-byte
// stores. done: the image already holds z (both sides were read along b).
template <typename D, typename TS, int VW>
__device__ __forceinline__ void wl_store(D *dst, const ModelPlan &mp, const double (*img)[MV_TILE + 1],
                                         const TS (*simg)[MV_TILE + 1], const int64_t *sav, const int64_t *sbv,
                                         const WlSide<TS> &X, const WlSide<TS> &H, int64_t a0, int na, int nb,
                                         bool a_unit, bool done, double &acc) {
  constexpr int TPR = MV_TILE / VW, RPP = 256 / TPR, NR = MV_TILE / RPP, CH = NR < 8 ? NR : 8;
  const int al = ((int)threadIdx.x % TPR) * VW, br = (int)threadIdx.x / TPR;
#pragma unroll
  for (int c = 0; c < NR; c += CH) {
    TS xv[CH][VW], hv[CH][VW];
    if (!done) {
#pragma unroll
      for (int i = 0; i < CH; i++) {
        const int bl = br + RPP * (c + i);
        const bool ok = al < na && bl < nb;
        if (!X.in_lds) wl_load<TS, VW>(X, a0, al, bl, ok, xv[i]);
        if (!H.in_lds) wl_load<TS, VW>(H, a0, al, bl, ok, hv[i]);
      }
    }
#pragma unroll
    for (int i = 0; i < CH; i++) {
      const int bl = br + RPP * (c + i);
      if (al < na && bl < nb) {
        mv_vec<D> o;
#pragma unroll
        for (int e = 0; e < VW; e++) {
          double z = img[bl][al + e];
          if (!done) {
            const double x = X.in_lds ? (double)simg[bl][al + e] : (double)xv[i][e];
            const double h = H.in_lds ? (double)simg[bl][al + e] : (double)hv[i][e];
            z = wl_rule(x, h, z, acc);
          }
          o.v[e] = (D)z;
        }
        if (VW > 1)
          *reinterpret_cast<mv_vec<D> *>(dst + (mp.voff + sbv[bl] + a0 + al)) = o;
        else
          dst[mp.voff + sbv[bl] + (a_unit ? a0 + al : sav[al])] = o.v[0];
      }
    }
  }
}

template <typename D, typename TS>
__global__ __launch_bounds__(256, 2) void k_model_wls(
    D *dst, const TS *Xp, const TS *Hp, const double *__restrict__ Q, const double *__restrict__ P, int K,
    ModelPlan mp, int64_t woff, const int64_t *__restrict__ tav, const int64_t *__restrict__ tax,
    const int64_t *__restrict__ taw, const int64_t *__restrict__ tbv, const int64_t *__restrict__ tbx,
    const int64_t *__restrict__ tbw, int flags, double *__restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) unsigned char wl_lds[];
  const int RB = (K + 3) / 4;
  double *qs = reinterpret_cast<double *>(wl_lds);  // [4 RB][MW_LDQ]
  double(*img)[MV_TILE + 1] = reinterpret_cast<double(*)[MV_TILE + 1]>(qs + (size_t)4 * RB * MW_LDQ);
  int64_t *sav = reinterpret_cast<int64_t *>(img + MV_TILE), *sax = sav + MV_TILE, *saw = sax + MV_TILE,
          *sbv = saw + MV_TILE, *sbx = sbv + MV_TILE, *sbw = sbx + MV_TILE;
  TS(*simg)[MV_TILE + 1] = reinterpret_cast<TS(*)[MV_TILE + 1]>(sbw + MV_TILE);  // (one side along b only)
  double acc = 0.0;  // this thread's share of the loss
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, j16 = lane & 15;
  const int64_t A = mp.ga.count, B = mp.gb.count, a0 = (int64_t)blockIdx.x * MV_TILE;
  const int na = (int)min((int64_t)MV_TILE, A - a0);
  const bool a_unit = flags & WL_A_UNIT, vec_st = flags & WL_VEC_ST;
  const bool x_b = !(flags & WL_X_ALONG_A), h_b = !(flags & WL_H_ALONG_A), both_b = x_b && h_b;
  const int64_t nbt = (B + MV_TILE - 1) / MV_TILE;
  const WlSide<TS> X{Xp, sax, sbx, mp.roff, x_b, (flags & WL_X_UNIT) != 0, (flags & WL_X_VEC) != 0};
  const WlSide<TS> H{Hp, saw, sbw, woff, h_b, (flags & WL_H_UNIT) != 0, (flags & WL_H_VEC) != 0};

  for (int e = threadIdx.x; e < 4 * RB * MV_TILE; e += 256) {  // the Q image: 4 rows of k per pass
    const int k = e / MV_TILE, al = e % MV_TILE;
    qs[k * MW_LDQ + al] = (al < na && k < K) ? Q[a0 + al + mp.ldq * (int64_t)k] : 0.0;
  }
  if (threadIdx.x < MV_TILE) {
    const int i = threadIdx.x;
    sav[i] = i < na ? tav[a0 + i] : 0;
    sax[i] = i < na ? tax[a0 + i] : 0;
    saw[i] = i < na ? taw[a0 + i] : 0;
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
  int64_t nbv = 0, nbx = 0, nbw = 0;
  const int ib = (int)threadIdx.x - MV_TILE;  // threads 64..127: the b offsets, a tile ahead
  auto load_b = [&](int64_t tb_) {
    const int64_t bb = tb_ * MV_TILE + ib;
    const bool ok = ib >= 0 && ib < MV_TILE && tb_ < nbt && bb < B;
    nbv = ok ? tbv[bb] : 0;
    nbx = ok ? tbx[bb] : 0;
    nbw = ok ? tbw[bb] : 0;
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
      sbx[ib] = nbx;
      sbw[ib] = nbw;
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
    if (x_b || h_b) {  // the side views whose unit-stride run lies along b: lane index along b
      constexpr int NH = MV_TILE / 8;
      const int bl = lane;
      const int64_t x0 = X.off + sax[0] + sbx[0], h0 = H.off + saw[0] + sbw[0];
#pragma unroll
      for (int hf = 0; hf < 2; hf++) {
        TS xv[NH], hv[NH];
#pragma unroll
        for (int i = 0; i < NH; i++) {
          const int al = wave + 4 * (NH * hf + i);
          const bool ok = al < na && bl < nb;
          if (x_b) xv[i] = Xp[ok ? X.off + sax[al] + sbx[bl] : x0];
          if (h_b) hv[i] = Hp[ok ? H.off + saw[al] + sbw[bl] : h0];
        }
#pragma unroll
        for (int i = 0; i < NH; i++) {
          const int al = wave + 4 * (NH * hf + i);
          if (both_b) {
            if (al < na && bl < nb) img[bl][al] = wl_rule((double)xv[i], (double)hv[i], img[bl][al], acc);
          } else {
            simg[bl][al] = x_b ? xv[i] : hv[i];
          }
        }
      }
      __syncthreads();
    }
    if (vec_st)
      wl_store<D, TS, 16 / sizeof(D)>(dst, mp, img, simg, sav, sbv, X, H, a0, na, nb, a_unit, both_b, acc);
    else
      wl_store<D, TS, 1>(dst, mp, img, simg, sav, sbv, X, H, a0, na, nb, a_unit, both_b, acc);
    __syncthreads();  // the images and the b offsets are rewritten by the next tile
  }
  acc = block_sum(acc, &img[0][0]);
  if (threadIdx.x == 0) part[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = acc;
}

}  // namespace ppals
