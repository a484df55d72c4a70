// kernels_huber.hip.h — robust CP (ppals_cp_huber_device, ppals_cp_abs_residual_quantile; include/ppals.h):
// two more rules on the tile loop of the weighted step (kernels_wls_tile.hip.h), each with and without a
// weights view.
//
// k_model_huber<D, TS, HAS_H>: the working tensor of Huber's loss rho_c under Kiers' majorization,
//   z = m                           where h <= 0 or NaN      (loss 0; x is not used)
//   a = |x - m| <= c (or NaN):      the weighted step's rule, by its own code (wl_rule): with c = +inf the
//                                   stored bits and the loss are those of k_model_wls
//   a > c, dc = copysign(c, x - m): z = m + dc (h >= 1) or fma(h, dc, m); loss min(h, 1) c (2 a - c); clipped
// A workgroup writes two partials: its loss, and npart further on its clipped count, an integer kept exactly
// in a double. HAS_H = false is the family without a weights view (h = 1): no H pointer, no third offset
// table, 8 B per element (fp32 / fp32) in place of 12; the data side keeps both ways of being read, and with
// it along b the arithmetic is done there, so no typed image is ever needed: wl_lds_bytes(K, 0).
//
// k_model_absres_hist<TS, HAS_H>: one pass of a radix select over the keys of a_e = (float)|x_e - m_e|, e the
// elements with h > 0. The tile loop without the store pass; both sides are read as the step reads them. A key
// is the fp32 pattern of a_e (31 bits; every NaN is 0x7fc00000, above +inf). A pass counts, by
// bin = (key >> shift) & mask, the keys with key >> pshift == prefix (pshift = 31, prefix = 0: all), into a
// histogram of WL_HIST_BINS uint32 in LDS behind the images, and adds its non-zero bins to the global uint64
// histogram once, with integer atomics: the counts do not depend on the grid or the order of arrival.
// Residuals crowd into a few exponent bins, so the lanes of a wave first agree on their distinct bins
// (ballot / readlane) and one lane adds the popcount: an LDS atomic per distinct bin of a wave, not per lane.
#pragma once
#include "kernels_wls.hip.h"

namespace ppals {

template <>
__device__ __forceinline__ double wl_apply<WL_HUBER>(double x, double h, double m, WlCtx &cx) {
  if (!(h > 0.0)) return m;  // h <= 0 or NaN: x is not looked at
  const double d = x - m, a = fabs(d);
  if (!(a > cx.c)) return wl_rule(x, h, m, cx.acc);  // (NaN too) the weighted step's operations, in its order
  const double dc = copysign(cx.c, d), l = cx.c * (2.0 * a - cx.c);
  cx.nclip += 1.0;
  if (h >= 1.0) {
    cx.acc += l;
    return m + dc;
  }
  cx.acc += h * l;
  return __fma_rn(h, dc, m);
}

constexpr uint32_t HB_NAN_KEY = 0x7fc00000u;
__device__ __forceinline__ uint32_t hb_key(double x, double m) {
  const float a = (float)fabs(x - m);  // the fp64 difference rounded to nearest fp32
  return a != a ? HB_NAN_KEY : __float_as_uint(a);
}

// Called under divergence (lanes outside the tile are not here): ballot sees the active lanes only.
template <>
__device__ __forceinline__ double wl_apply<WL_HIST>(double x, double h, double m, WlCtx &cx) {
  const uint32_t key = hb_key(x, m);
  const bool sel = h > 0.0 && (key >> cx.pshift) == cx.prefix;
  const uint32_t bin = (key >> cx.shift) & cx.mask;
  unsigned long long todo = __ballot(sel);
  const int lane = threadIdx.x & 63;
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const uint32_t b = (uint32_t)__builtin_amdgcn_readlane((int)bin, leader);
    const unsigned long long same = __ballot(sel && bin == b);
    if (lane == leader) atomicAdd(&cx.hist[b], (uint32_t)__popcll(same));
    todo &= ~same;
  }
  return m;
}

template <typename D, typename TS>
__global__ __launch_bounds__(256, 2) void k_model_huber(
    D *dst, const TS *Xp, const TS *Hp, const double *__restrict__ Q, const double *__restrict__ P, int K,
    ModelPlan mp, int64_t woff, const int64_t *__restrict__ tav, const int64_t *__restrict__ tax,
    const int64_t *__restrict__ taw, const int64_t *__restrict__ tbv, const int64_t *__restrict__ tbx,
    const int64_t *__restrict__ tbw, int flags, double c, double *__restrict__ part) {
  constexpr int KIND = WL_HUBER;
  constexpr bool HAS_H = true;
  WlCtx cx;
  cx.c = c;
#include "kernels_wls_tile.hip.h"
}

template <typename D, typename TS>
__global__ __launch_bounds__(256, 2) void k_model_huber_now(
    D *dst, const TS *Xp, const double *__restrict__ Q, const double *__restrict__ P, int K, ModelPlan mp,
    const int64_t *__restrict__ tav, const int64_t *__restrict__ tax, const int64_t *__restrict__ tbv,
    const int64_t *__restrict__ tbx, int flags, double c, double *__restrict__ part) {
  constexpr int KIND = WL_HUBER;
  constexpr bool HAS_H = false;
  const TS *const Hp = nullptr;  // (what the family does without: never read)
  const int64_t *const taw = nullptr, *const tbw = nullptr, woff = 0;
  WlCtx cx;
  cx.c = c;
#include "kernels_wls_tile.hip.h"
}

// (D of the tile loop only sets the width of a lane's run in the "store" pass: TS gives 16 bytes of the views)
template <typename TS, bool HAS_H>
__global__ __launch_bounds__(256, 2) void k_model_absres_hist(
    const TS *Xp, const TS *Hp, const double *__restrict__ Q, const double *__restrict__ P, int K, ModelPlan mp,
    int64_t woff, const int64_t *__restrict__ tax, const int64_t *__restrict__ taw,
    const int64_t *__restrict__ tbx, const int64_t *__restrict__ tbw, int flags, int pshift, uint32_t prefix,
    int shift, uint32_t mask, unsigned long long *__restrict__ ghist) {
  constexpr int KIND = WL_HIST;
  using D = TS;
  D *const dst = nullptr;  // (never read: nothing is stored)
  const int64_t *const tav = nullptr, *const tbv = nullptr;
  double *const part = nullptr;
  WlCtx cx;
  cx.pshift = pshift;
  cx.prefix = prefix;
  cx.shift = shift;
  cx.mask = mask;
#include "kernels_wls_tile.hip.h"
  __syncthreads();  // (the last tile's barrier already ordered the LDS atomics; this one is for the reader)
  for (int e = threadIdx.x; e < WL_HIST_BINS; e += 256) {
    const uint32_t n = cx.hist[e];
    if (n) atomicAdd(&ghist[e], (unsigned long long)n);
  }
}

}  // namespace ppals
