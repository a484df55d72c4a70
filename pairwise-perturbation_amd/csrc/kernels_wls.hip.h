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
constexpr int WL_HIST_BINS = 2048;  // (kernels_huber.hip.h: the quantile's histogram follows the images in LDS)
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

// What a kernel built on the tile loop (kernels_wls_tile.hip.h, the body of k_model_wls below) does with an
// element (x, h, m): the compile-time policy KIND, and HAS_H = false for a family without a weights view
// (h = 1 everywhere: no H pointer, no third offset table). WL_WLS is the rule above; the other two live in kernels_huber.hip.h. WlCtx is the state a rule
// keeps per thread: a rule touches only its own members, the rest never exist in the compiled kernel.
enum { WL_WLS = 0, WL_HUBER = 1, WL_HIST = 2 };
struct WlCtx {
  double acc = 0.0;    // this thread's share of the loss
  double c = 0.0;      // WL_HUBER: the clipping threshold
  double nclip = 0.0;  // WL_HUBER: this thread's count of clipped elements (exact: an integer in a double)
  uint32_t *hist = nullptr;  // WL_HIST: the workgroup's histogram in LDS, and the pass (kernels_huber.hip.h)
  uint32_t prefix = 0, mask = 0;
  int pshift = 31, shift = 0;
};
template <int KIND>
__device__ __forceinline__ double wl_apply(double x, double h, double m, WlCtx &cx);
template <>
__device__ __forceinline__ double wl_apply<WL_WLS>(double x, double h, double m, WlCtx &cx) {
  return wl_rule(x, h, m, cx.acc);
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
// stores. done: the image already holds z (both sides were read along b). WL_HIST stores nothing.
template <typename D, typename TS, int VW, int KIND, bool HAS_H>
__device__ __forceinline__ void wl_store(D *dst, const ModelPlan &mp, const double (*img)[MV_TILE + 1],
                                         const TS (*simg)[MV_TILE + 1], const int64_t *sav, const int64_t *sbv,
                                         const WlSide<TS> &X, const WlSide<TS> &H, int64_t a0, int na, int nb,
                                         bool a_unit, bool done, WlCtx &cx) {
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
        if (HAS_H && !H.in_lds) wl_load<TS, VW>(H, a0, al, bl, ok, hv[i]);
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
            const double h = !HAS_H ? 1.0 : H.in_lds ? (double)simg[bl][al + e] : (double)hv[i][e];
            z = wl_apply<KIND>(x, h, z, cx);
          }
          o.v[e] = (D)z;
        }
        if (KIND == WL_HIST) continue;
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
  constexpr int KIND = WL_WLS;
  constexpr bool HAS_H = true;
  WlCtx cx;
#include "kernels_wls_tile.hip.h"
}

}  // namespace ppals
