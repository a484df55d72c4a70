// hip_ops.hip — the product implementation of ppals::Ops: hand-written HIP kernels for gfx950,
// launched on one engine-owned stream. No CPU fallback: construction throws without a HIP device.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <chrono>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <map>
#include <type_traits>
#include <vector>

#include "hip_ops.h"
#include "roctx_ranges.h"
#include "preload_policy.h"
#include "kernels_scan.hip.h"
#include "kernels_pack.hip.h"
#include "kernels_small.hip.h"
#include "kernels_nn.hip.h"
#include "kernels_polar.hip.h"
#include "kernels_shape.hip.h"
#include "kernels_holdout.hip.h"
#include "kernels_corcondia.hip.h"
#include "kernels_fms.hip.h"
#include "kernels_slices.hip.h"
#include "kernels_eig.hip.h"
#include "kernels_io.hip.h"
#include "kernels_model.hip.h"
#include "kernels_tucker_slices.hip.h"
#include "kernels_wls.hip.h"
#include "kernels_huber.hip.h"
#include "kernels_parafac2.hip.h"
#include "kernels_bf16.hip.h"
#include "kernels_prep.hip.h"
#include "kernels_npls.hip.h"
#include "kernels_npls_wide.hip.h"

namespace ppals {
#define HIP_CHECK(expr)                                                                       \
  do {                                                                                        \
    hipError_t _e = (expr);                                                                   \
    if (_e != hipSuccess)                                                                     \
      throw std::runtime_error(std::string("HIP error: ") + hipGetErrorString(_e) + " at " + \
                               __FILE__ + ":" + std::to_string(__LINE__) + " (" #expr ")");  \
  } while (0)

// workgroup size of k_chol_m for an n x 2n elimination (a barrier per pivot: fewer waves, cheaper barrier)
static inline unsigned k_chol_threads(int n) {
  (void)n;  // measured: 256 threads at n = 20 make the launch 17.8 -> 22.3 us (the per-pivot update,
            // not the barrier, is the longer part); 1024 with LDS-only barriers: see below
  return 1024u;
}
static inline int grid_for(int64_t n, int block, int cap = 4096) {
  int64_t g = (n + block - 1) / block;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return (int)g;
}

// A reduction over n units (k-blocks, columns) in the `want` splits a launcher asks for (at least 1):
// per = units per split, at least min_per and rounded up to a multiple of align; nsplit = the splits
// that leaves non-empty.
struct KSplit {
  int nsplit;
  int64_t per;
};
static inline KSplit k_split(int64_t n, int64_t want, int64_t min_per = 1, int64_t align = 1) {
  want = std::max<int64_t>(want, 1);
  int64_t per = std::max((n + want - 1) / want, min_per);
  per = (per + align - 1) / align * align;
  return {(int)((n + per - 1) / per), per};
}

// Compile-time dispatch of a launch: f(std::integral_constant) for the first of Vs equal to v, or for
// the last of Vs when none is. Instantiates f for exactly the listed values.
template <auto V, auto... Vs, typename T, typename F>
static inline void dispatch(T v, F &&f) {
  if constexpr (sizeof...(Vs) == 0)
    f(std::integral_constant<decltype(V), V>());
  else if (v == V)
    f(std::integral_constant<decltype(V), V>());
  else
    dispatch<Vs...>(v, f);
}

// The vendor eigensolver libraries, process-wide. See hip_preload_eigensolver (hip_ops.h).
struct EigLibs {
  void *blas = nullptr, *solver = nullptr;
};
static bool g_hip_runtime_up = false;  // set by the first HipOps (this library's own use of the runtime)
static EigLibs &eig_libs() {
  static EigLibs l;
  if (l.blas && l.solver) return l;
  switch (late_preload_policy(false, g_hip_runtime_up, getenv("PPALS_STRICT_PRELOAD"))) {
    case kPreloadRefuse: throw Unsupported(late_preload_message());
    case kPreloadWarn: fprintf(stderr, "%s\n", late_preload_message()); fflush(stderr); break;
    default: break;
  }
  l.blas = dlopen("librocblas.so.5", RTLD_NOW | RTLD_GLOBAL);
  if (!l.blas) l.blas = dlopen("librocblas.so", RTLD_NOW | RTLD_GLOBAL);
  l.solver = dlopen("librocsolver.so.0", RTLD_NOW | RTLD_GLOBAL);
  if (!l.solver) l.solver = dlopen("librocsolver.so", RTLD_NOW | RTLD_GLOBAL);
  if (!l.blas || !l.solver)
    throw std::runtime_error(std::string("ppals: cannot load rocSOLVER: ") + dlerror());
  return l;
}

class HipOps : public Ops {
 public:
  explicit HipOps(int device) {
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
      throw std::runtime_error(
          "ppals: no HIP device available (the engine has no CPU fallback; hipGetDeviceCount: " +
          std::string(e == hipSuccess ? "0 devices" : hipGetErrorString(e)) + ")");
    if (device < 0 || device >= ndev)
      throw std::runtime_error("ppals: device index out of range");
    dev_ = device;
    g_hip_runtime_up = true;
    HIP_CHECK(hipSetDevice(dev_));
    HIP_CHECK(hipStreamCreateWithFlags(&st_, hipStreamNonBlocking));
    hipDeviceProp_t prop;
    HIP_CHECK(hipGetDeviceProperties(&prop, dev_));
    ncu_ = prop.multiProcessorCount;
    HIP_CHECK(hipFuncSetAttribute((const void *)k_gram_system,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
    HIP_CHECK(hipFuncSetAttribute((const void *)k_cp_update,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
    HIP_CHECK(hipFuncSetAttribute((const void *)k_top_eig_small,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 152 * 1024));
    HIP_CHECK(hipFuncSetAttribute((const void *)k_cp_mode_update<false, false>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 152 * 1024));
    HIP_CHECK(hipFuncSetAttribute((const void *)k_cp_mode_update<true, true>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 152 * 1024));
    HIP_CHECK(hipFuncSetAttribute((const void *)k_cp_mode_update_batched<false, false>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 152 * 1024));
    HIP_CHECK(hipFuncSetAttribute((const void *)k_cp_mode_update_batched<true, true>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 152 * 1024));
    HIP_CHECK(hipFuncSetAttribute((const void *)k_cp_mode_update_ragged<false, false>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 152 * 1024));
    HIP_CHECK(hipFuncSetAttribute((const void *)k_cp_mode_update_ragged<true, true>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 152 * 1024));
    if (const char *v = getenv("PPALS_FORCE_JACOBI")) force_jacobi_ = atoi(v);
    if (const char *v = getenv("PPALS_EIG_FAST")) {
      eig_fast_ = atoi(v);  // 0: always the full solver; 2: warm steps as usual, cold starts on the full solver
      eig_cold_ = eig_fast_ != 2;
    }
    if (const char *v = getenv("PPALS_EIG_DEBUG")) eig_debug_ = atoi(v);
    if (const char *v = getenv("PPALS_EIG_SIGMA_SCALE")) eig_sigma_scale_ = atof(v);
    if (const char *v = getenv("PPALS_FORCE_EIGINV")) force_eiginv_ = atoi(v);
    HIP_CHECK(hipFuncSetAttribute((const void *)k_chol_rinv,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 72 * 1024));
    HIP_CHECK(hipFuncSetAttribute((const void *)k_chol_m,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 152 * 1024));
    HIP_CHECK(hipFuncSetAttribute((const void *)k_rr_apply,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 152 * 1024));
    if (const char *v = getenv("PPALS_SYM_LDS_MIN")) sym_lds_min_ = std::max(32, atoi(v));
    if (const char *v = getenv("PPALS_EIG_DEFER")) {
      eig_defer_ok_ = atoi(v);
      handover_ok_ = eig_defer_ok_ != 2;  // (2: deferred, the second stream handed over by events)
    }
    if (const char *v = getenv("PPALS_EIG_DEFER_FAIL")) eig_defer_fail_ = atoi(v);
    if (const char *v = getenv("PPALS_SCAN_TAIL")) scan_tail_on_ = atoi(v) != 0;
    if (const char *v = getenv("PPALS_SCAN_WIDE")) wide_enabled_ = atoi(v) != 0;
    if (const char *v = getenv("PPALS_COLD_SUBSPACE_FROM")) cold_subspace_from_ = std::max(65, atoi(v));
    if (const char *v = getenv("PPALS_PERSIST_MULT")) persist_mult_ = std::max(1, atoi(v));  // (probe: tools/runs/r05_m.sh)
    HIP_CHECK(hipFuncSetAttribute((const void *)k_rmult_chol,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 152 * 1024));
    HIP_CHECK(hipFuncSetAttribute((const void *)k_jacobi_onesided,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 152 * 1024));
    HIP_CHECK(hipFuncSetAttribute((const void *)k_rr_small,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 152 * 1024));
    HIP_CHECK(hipFuncSetAttribute((const void *)k_gram_system_lds,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 152 * 1024));
    HIP_CHECK(hipFuncSetAttribute((const void *)k_gram_system_mfma,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 152 * 1024));
    const int mw_max = (int)mw_lds_bytes(MW_KMAX);
    HIP_CHECK(hipFuncSetAttribute((const void *)k_model_impute_wide<float, false>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, mw_max));
    HIP_CHECK(hipFuncSetAttribute((const void *)k_model_impute_wide<float, true>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, mw_max));
    HIP_CHECK(hipFuncSetAttribute((const void *)k_model_impute_wide<double, false>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, mw_max));
    HIP_CHECK(hipFuncSetAttribute((const void *)k_model_impute_wide<double, true>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, mw_max));
    const int ts_max = (int)ts_lds_bytes(MW_KMAX);
    HIP_CHECK(hipFuncSetAttribute((const void *)k_model_slices_wide<float>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, ts_max));
    HIP_CHECK(hipFuncSetAttribute((const void *)k_model_slices_wide<double>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, ts_max));
    const int wl_max = (int)wl_lds_bytes(WL_KMAX, sizeof(double));
    HIP_CHECK(hipFuncSetAttribute((const void *)k_model_wls<float, float>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, wl_max));
    HIP_CHECK(hipFuncSetAttribute((const void *)k_model_wls<float, double>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, wl_max));
    HIP_CHECK(hipFuncSetAttribute((const void *)k_model_wls<double, float>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, wl_max));
    HIP_CHECK(hipFuncSetAttribute((const void *)k_model_wls<double, double>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, wl_max));
    const void *huber_kernels[] = {
        (const void *)k_model_huber<float, float>,      (const void *)k_model_huber<float, double>,
        (const void *)k_model_huber<double, float>,     (const void *)k_model_huber<double, double>,
        (const void *)k_model_huber_now<float, float>,  (const void *)k_model_huber_now<float, double>,
        (const void *)k_model_huber_now<double, float>, (const void *)k_model_huber_now<double, double>,
        (const void *)k_model_absres_hist<float, true>, (const void *)k_model_absres_hist<float, false>,
        (const void *)k_model_absres_hist<double, true>, (const void *)k_model_absres_hist<double, false>};
    for (const void *k : huber_kernels)
      HIP_CHECK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    wl_max + (int)(sizeof(uint32_t) * WL_HIST_BINS)));
    // (the on-chip centring tile: 56 KiB of image + 8 KiB of partial sums at VEC = 4 is the whole 64 KiB)
    HIP_CHECK(hipFuncSetAttribute((const void *)k_prep_rows<float, 4, 16, PREP_CENTER, true>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
    HIP_CHECK(hipFuncSetAttribute((const void *)k_prep_rows<bf16s, 4, 16, PREP_CENTER, true>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
    HIP_CHECK(hipFuncSetAttribute((const void *)k_prep_rows<double, 2, 16, PREP_CENTER, true>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
    if (const char *v = getenv("PPALS_GJ_SCALAR")) gj_scalar_ = atoi(v);
    HIP_CHECK(hipFuncSetAttribute((const void *)k_fms_cross, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)fms_lds_bytes(FMS_MAXC, FMS_MAXC, false)));
    HIP_CHECK(hipFuncSetAttribute((const void *)k_polar_factor, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  96 * 1024));  // (67.5 KB at R = 64)
    HIP_CHECK(hipFuncSetAttribute((const void *)k_shape_columns, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)kShapeLdsBytes));
    HIP_CHECK(hipFuncSetAttribute((const void *)k_p2_polar, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
    HIP_CHECK(hipFuncSetAttribute((const void *)k_p2_polar_ragged, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  96 * 1024));
    const void *p2_wide[] = {(const void *)k_p2_project<float, 4>, (const void *)k_p2_project<double, 4>,
                             (const void *)k_p2_project_ragged<float, 4>,
                             (const void *)k_p2_project_ragged<double, 4>};
    for (const void *k : p2_wide)  // (R > 48: 72 KB at R = 64; every other instantiation stays below 64 KB)
      HIP_CHECK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p2_project_lds(64)));
  }
  ~HipOps() override {
    hipSetDevice(dev_);
    hipStreamSynchronize(st_);
    if (st2_) hipStreamSynchronize(st2_);  // (checks of deferred steps still read the slots' buffers)
    for (auto &ev : events_) {
      hipEventDestroy(ev.a);
      hipEventDestroy(ev.b);
    }
    for (auto &t : timers_) {
      hipEventDestroy(t.a);
      hipEventDestroy(t.b);
    }
    if (ws_mttv_) hipFree(ws_mttv_);
    if (ws_pack_) hipFree(ws_pack_);
    if (pack_stats_) hipFree(pack_stats_);
    if (ws_mv_) hipFree(ws_mv_);
    if (ws_hist_) hipFree(ws_hist_);
    if (ws_slab_) hipFree(ws_slab_);
    if (ws_krp_) hipFree(ws_krp_);
    if (ws_part_) hipFree(ws_part_);
    if (ws_small_) hipFree(ws_small_);
    if (ws_big_) hipFree(ws_big_);
    if (ws_big2_) hipFree(ws_big2_);
    if (ws_eig_) hipFree(ws_eig_);
    if (ws_orth_) hipFree(ws_orth_);
    if (ws_pow_) hipFree(ws_pow_);
    if (ws_cold_) hipFree(ws_cold_);
    if (ws_cold2_) hipFree(ws_cold2_);
    if (ws_cholm_) hipFree(ws_cholm_);
    if (ws_gsfb_) hipFree(ws_gsfb_);
    if (ws_jac_) hipFree(ws_jac_);
    if (eig_host_) hipHostFree(eig_host_);
    if (ws_part2_) hipFree(ws_part2_);
    for (auto &kv : eig_state_) {
      if (kv.second.Q) hipFree(kv.second.Q);
      if (kv.second.Qn) hipFree(kv.second.Qn);
      free_lazy(kv.second);
    }
    for (auto &kv : eig_small_)
      if (kv.second.Q) hipFree(kv.second.Q);
    if (st2_) hipStreamDestroy(st2_);
    if (handover_) hipFree(handover_);
    if (io_ev_in_) hipEventDestroy(io_ev_in_);
    if (io_ev_out_) hipEventDestroy(io_ev_out_);
    hipStreamDestroy(st_);
  }

  void *alloc(size_t bytes) override {
    void *p = nullptr;
    HIP_CHECK(hipSetDevice(dev_));
    HIP_CHECK(hipMalloc(&p, bytes ? bytes : 8));
    return p;
  }
  void free(void *p) override {
    if (p) {
      hipStreamSynchronize(st_);
      hipFree(p);
    }
  }
  void h2d(void *dst, const void *src, size_t bytes) override {
    HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st_));
    HIP_CHECK(hipStreamSynchronize(st_));
  }
  void d2h(void *dst, const void *src, size_t bytes) override {
    HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipStreamSynchronize(st_));
  }
  void d2d(void *dst, const void *src, size_t bytes) override {
    HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st_));
  }
  void zero(void *p, size_t bytes) override { HIP_CHECK(hipMemsetAsync(p, 0, bytes, st_)); }
  void sync() override { HIP_CHECK(hipStreamSynchronize(st_)); }
  void *stream() override { return (void *)st_; }
  void bind() override { HIP_CHECK(hipSetDevice(dev_)); }
  bool supports_storage(int dt) override { return dt == F32 || dt == F64 || dt == BF16; }

  // ------------------------------------------------------------------ generation / norms
  void fill_uniform(void *V, int dt, int64_t l0, int64_t g0, int64_t row0, int64_t rest,
                    uint64_t seed, double lo, double hi) override {
    int64_t n = l0 * rest;
    int g = grid_for(n, 256, 16384);
    if (dt == F32)
      hipLaunchKernelGGL(k_fill_uniform<float>, dim3(g), dim3(256), 0, st_, (float *)V, l0, g0,
                         row0, rest, seed, lo, hi);
    else if (dt == BF16)
      hipLaunchKernelGGL(k_fill_uniform<bf16s>, dim3(g), dim3(256), 0, st_, (bf16s *)V, l0, g0,
                         row0, rest, seed, lo, hi);
    else
      hipLaunchKernelGGL(k_fill_uniform<double>, dim3(g), dim3(256), 0, st_, (double *)V, l0, g0,
                         row0, rest, seed, lo, hi);
    HIP_CHECK(hipGetLastError());
  }

  void fill_laplacian(void *V, int dt, int64_t l0, int64_t g0, int64_t row0, int64_t rest,
                      int ndigits, int s) override {
    int g = grid_for(l0 * rest, 256, 16384);
    if (dt == F32)
      hipLaunchKernelGGL(k_fill_laplacian<float>, dim3(g), dim3(256), 0, st_, (float *)V, l0, g0,
                         row0, rest, ndigits, s);
    else if (dt == BF16)
      hipLaunchKernelGGL(k_fill_laplacian<bf16s>, dim3(g), dim3(256), 0, st_, (bf16s *)V, l0, g0,
                         row0, rest, ndigits, s);
    else
      hipLaunchKernelGGL(k_fill_laplacian<double>, dim3(g), dim3(256), 0, st_, (double *)V, l0, g0,
                         row0, rest, ndigits, s);
    HIP_CHECK(hipGetLastError());
  }
  void add_uniform_noise(void *V, int dt, int64_t l0, int64_t g0, int64_t row0, int64_t rest,
                         uint64_t seed, double lo, double hi, double alpha) override {
    int g = grid_for(l0 * rest, 256, 16384);
    if (dt == F32)
      hipLaunchKernelGGL((k_uniform_noise<float, 0>), dim3(g), dim3(256), 0, st_, (float *)V, l0,
                         g0, row0, rest, seed, lo, hi, alpha, (double *)nullptr);
    else if (dt == BF16)
      hipLaunchKernelGGL((k_uniform_noise<bf16s, 0>), dim3(g), dim3(256), 0, st_, (bf16s *)V, l0,
                         g0, row0, rest, seed, lo, hi, alpha, (double *)nullptr);
    else
      hipLaunchKernelGGL((k_uniform_noise<double, 0>), dim3(g), dim3(256), 0, st_, (double *)V, l0,
                         g0, row0, rest, seed, lo, hi, alpha, (double *)nullptr);
    HIP_CHECK(hipGetLastError());
  }
  void uniform_sumsq(int64_t l0, int64_t g0, int64_t row0, int64_t rest, uint64_t seed, double lo,
                     double hi, double *out) override {
    int g = grid_for(l0 * rest, 256, 4096);
    double *part = (double *)ensure(ws_part_, ws_part_sz_, sizeof(double) * g);
    hipLaunchKernelGGL((k_uniform_noise<double, 1>), dim3(g), dim3(256), 0, st_, (double *)nullptr,
                       l0, g0, row0, rest, seed, lo, hi, 0.0, part);
    hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(1024), 0, st_, part, g, out);
    HIP_CHECK(hipGetLastError());
  }

  // the launch geometry of k_rank_mfma (MODE 3 walks the one of MODE 1 in slabs); false: shape not covered
  struct RankPlan {
    int nkb, nchunk, per, rem, RB;
    int64_t n_mtiles;
  };
  template <typename TV>
  bool rank_plan(int mode, const void *V, int64_t M, int64_t K, int R, RankPlan &pl) {
    constexpr int VEC = ScanTraits<TV>::VEC;
    if (R > 32 || M % VEC != 0 || M < VEC || (((uintptr_t)V) & 15) != 0 || K < 1)
      return false;
    const int64_t nkb64 = (K + 15) / 16;
    if (nkb64 > 0x7fffffff) return false;
    const int nkb = (int)nkb64;
    const int64_t n_mtiles = (M + 64 * VEC - 1) / (64 * VEC);
    // enough workgroups to fill the chip several times, chunks of >= 8 column blocks
    // (workgroups per CU x 4 .. 128 instead of 16: 1.60-1.73 ms for the whole [diffV] call at cfg2,
    // 1.61 at 16 — tools/k10_probe.py, profiles/r03z_k10_geometry.txt: the geometry is not the lever)
    const KSplit ks = k_split(nkb, std::min<int64_t>(nkb, ((int64_t)ncu_ * 16 + n_mtiles - 1) / n_mtiles),
                              std::min(nkb, 8));
    const int nchunk = ks.nsplit, per = (int)ks.per;
    if (n_mtiles > 0x7fffffff || nchunk > 65535) return false;
    // residual: a remainder of 1 or 2 ranks goes to the vector pipe instead of a padded matrix-core
    // step (kernels_scan.hip.h, REM), its P columns in LDS — if a chunk's share of them fits
    // (measured, tools/k10_probe.py at cfg2, profiles/r04I_k10_probe.txt: R = 10 1.28 -> 1.26 ms, R = 9
    // 1.17 ms, R = 13 1.38 ms against ~1.5 ms with a padded fourth step; two ranks beside three or four
    // steps — R = 14: 1.63 ms, R = 18: 1.78 ms — lose to padding: 2 waves per SIMD)
    int rem = ((mode == 1 || mode == 3) && R > 4 && R <= 17 && (R % 4 == 1 || (R % 4 == 2 && R <= 10))) ? R % 4 : 0;
    if (sizeof(double) * (size_t)per * 16 * rem > 48 * 1024) rem = 0;
    pl = {nkb, nchunk, per, rem, mode == 2 ? 1 : (R - rem + 3) / 4, n_mtiles};
    return true;
  }
  // K10 on the matrix cores (kernels_scan.hip.h: k_rank_mfma); false: shape not covered
  template <typename TV, int MODE>
  bool rank_mfma(void *V, int64_t M, int64_t K, const double *Q, const double *P, int R,
                 double *out) {
    RankPlan pl;
    if (!rank_plan<TV>(MODE, V, M, K, R, pl)) return false;
    const int nkb = pl.nkb, nchunk = pl.nchunk, per = pl.per, rem = pl.rem, RB = pl.RB;
    const int64_t n_mtiles = pl.n_mtiles;
    double *Ppk = nullptr;
    if (MODE != 2) {
      Ppk = (double *)ensure(ws_pack_, ws_pack_sz_, sizeof(double) * (size_t)nkb * RB * 64);
      hipLaunchKernelGGL(k_rank_pack, dim3(grid_for((int64_t)nkb * RB * 64, 256)), dim3(256), 0, st_,
                         P, K, R - rem, RB, nkb, Ppk);
    }
    dim3 grid((unsigned)n_mtiles, (unsigned)nchunk);
    double *part = nullptr;
    const int64_t npart = (int64_t)n_mtiles * nchunk;
    if (MODE != 0) part = (double *)ensure(ws_part_, ws_part_sz_, npart * sizeof(double));
    prof_begin(1, (double)M * K * sizeof(TV));
    const size_t lds_rem = sizeof(double) * (size_t)per * 16 * rem;
    const bool remk = MODE == 1 && rem != 0;  // the instantiation chosen below
    route("rank.mfma mode=%d dt=%s R=%d maxrb=%d rem=%d tiles=%lld chunks=%d per=%d", MODE, sname<TV>(), R,
          remk ? (RB <= 2 ? 2 : 4) : RB <= 3 ? 3 : RB <= 4 ? 4 : 8, remk ? rem : 0, (long long)n_mtiles, nchunk, per);
    bool done = false;
    if constexpr (MODE == 1) {
      if (rem) {
        auto launch_rem = [&](auto mrb, auto rm) {
          hipLaunchKernelGGL((k_rank_mfma<TV, 1, mrb, rm>), grid, dim3(256), lds_rem, st_, (TV *)V, M, K, Q, Ppk,
                             R, RB, per, nkb, part, P);
        };
        if (RB <= 2)
          dispatch<1, 2>(rem, [&](auto rm) { launch_rem(std::integral_constant<int, 2>(), rm); });
        else
          launch_rem(std::integral_constant<int, 4>(), std::integral_constant<int, 1>());
        done = true;
      }
    }
    if (done) {
    } else if (RB <= 3)
      hipLaunchKernelGGL((k_rank_mfma<TV, MODE, 3>), grid, dim3(256), 0, st_, (TV *)V, M, K, Q, Ppk, R,
                         RB, per, nkb, part);
    else if (RB <= 4)
      hipLaunchKernelGGL((k_rank_mfma<TV, MODE, 4>), grid, dim3(256), 0, st_, (TV *)V, M, K, Q, Ppk, R,
                         RB, per, nkb, part);
    else
      hipLaunchKernelGGL((k_rank_mfma<TV, MODE, 8>), grid, dim3(256), 0, st_, (TV *)V, M, K, Q, Ppk, R,
                         RB, per, nkb, part);
    prof_end();
    HIP_CHECK(hipGetLastError());
    if (MODE != 0) {
      hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(1024), 0, st_, part, (int)npart, out);
      HIP_CHECK(hipGetLastError());
    }
    return true;
  }
  // generation / residual for 32 < R <= 256 on the matrix cores (k_rank_split); false: not covered
  template <typename TV, int MODE>
  bool rank_split(void *V, int64_t M, int64_t K, const double *Q, const double *P, int R,
                  double *out) {
    constexpr int VEC = ScanTraits<TV>::VEC;
    if (R <= 32 || R > 256 || M % VEC != 0 || M < VEC ||
        (((uintptr_t)V) & 15) != 0 || K < 1)
      return false;
    const int RB = (R + 3) / 4;
    const int64_t nkb64 = (K + 15) / 16;
    if (nkb64 > 0x7fffffff) return false;
    const int nkb = (int)nkb64;
    double *Ppk = (double *)ensure(ws_pack_, ws_pack_sz_, sizeof(double) * (size_t)nkb * RB * 64);
    hipLaunchKernelGGL(k_rank_pack, dim3(grid_for((int64_t)nkb * RB * 64, 256)), dim3(256), 0, st_, P,
                       K, R, RB, nkb, Ppk);
    const int64_t n_mtiles = (M + 16 * VEC - 1) / (16 * VEC);
    const KSplit ks = k_split(nkb, std::min<int64_t>(nkb, ((int64_t)ncu_ * 8 + n_mtiles - 1) / n_mtiles),
                              std::min(nkb, 8));
    const int nchunk = ks.nsplit, per = (int)ks.per;
    if (n_mtiles > 0x7fffffff || nchunk > 65535) return false;
    dim3 grid((unsigned)n_mtiles, (unsigned)nchunk);
    const int64_t npart = (int64_t)n_mtiles * nchunk;
    double *part = MODE == 1 ? (double *)ensure(ws_part_, ws_part_sz_, npart * sizeof(double)) : nullptr;
    prof_begin(1, (double)M * K * sizeof(TV));
    const int rbw = (RB + 3) / 4;
    route("rank.split mode=%d dt=%s R=%d maxrbw=%d tiles=%lld chunks=%d per=%d", MODE, sname<TV>(), R,
          rbw <= 4 ? 4 : rbw <= 8 ? 8 : 16, (long long)n_mtiles, nchunk, per);
    if (rbw <= 4)
      hipLaunchKernelGGL((k_rank_split<TV, MODE, 4>), grid, dim3(256), 0, st_, (TV *)V, M, K, Q, Ppk, R,
                         RB, per, nkb, part);
    else if (rbw <= 8)
      hipLaunchKernelGGL((k_rank_split<TV, MODE, 8>), grid, dim3(256), 0, st_, (TV *)V, M, K, Q, Ppk, R,
                         RB, per, nkb, part);
    else
      hipLaunchKernelGGL((k_rank_split<TV, MODE, 16>), grid, dim3(256), 0, st_, (TV *)V, M, K, Q, Ppk,
                         R, RB, per, nkb, part);
    prof_end();
    HIP_CHECK(hipGetLastError());
    if (MODE == 1) {
      hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(1024), 0, st_, part, (int)npart, out);
      HIP_CHECK(hipGetLastError());
    }
    return true;
  }
  template <typename TV, int MODE>
  void rank_stream(void *V, int64_t M, int64_t K, const double *Q, const double *P, int R,
                   double *out) {
    // (a bf16 tensor: the per-element kernels below, whose fp64 model is rounded once per element)
    if constexpr (!std::is_same<TV, bf16s>::value) {
      if (rank_mfma<TV, MODE>(V, M, K, Q, P, R, out)) return;
      if constexpr (MODE != 2)
        if (rank_split<TV, MODE>(V, M, K, Q, P, R, out)) return;
    }
    int kch = 32;
    while ((K + kch - 1) / kch > 65535) kch *= 2;
    dim3 grid((unsigned)((M + 255) / 256), (unsigned)((K + kch - 1) / kch));
    double *part = nullptr;
    int64_t npart = (int64_t)grid.x * grid.y;
    if (MODE != 0) part = (double *)ensure(ws_part_, ws_part_sz_, npart * sizeof(double));
    TV *v = (TV *)V;
    route("rank.stream mode=%d dt=%s R=%d rb=%d kch=%d", MODE, sname<TV>(), R,
          R > 64 ? 0 : R <= 16 ? 16 : R <= 32 ? 32 : 64, kch);
    if (R > 64)
      hipLaunchKernelGGL((k_rank_stream_any<TV, MODE>), grid, dim3(256), 0, st_, v, M, K, Q, P, R,
                         kch, part);
    else if (R <= 16)
      hipLaunchKernelGGL((k_rank_stream<TV, 16, MODE>), grid, dim3(256), 0, st_, v, M, K, Q, P, R,
                         kch, part);
    else if (R <= 32)
      hipLaunchKernelGGL((k_rank_stream<TV, 32, MODE>), grid, dim3(256), 0, st_, v, M, K, Q, P, R,
                         kch, part);
    else
      hipLaunchKernelGGL((k_rank_stream<TV, 64, MODE>), grid, dim3(256), 0, st_, v, M, K, Q, P, R,
                         kch, part);
    HIP_CHECK(hipGetLastError());
    if (MODE != 0) {
      hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(1024), 0, st_, part, (int)npart, out);
      HIP_CHECK(hipGetLastError());
    }
  }
  void fill_rank(void *V, int dt, int64_t M, int64_t K, const double *Q, const double *P,
                 int R) override {
    if (dt == F32)
      rank_stream<float, 0>(V, M, K, Q, P, R, nullptr);
    else if (dt == BF16)
      rank_stream<bf16s, 0>(V, M, K, Q, P, R, nullptr);
    else
      rank_stream<double, 0>(V, M, K, Q, P, R, nullptr);
  }
  void residual_sq(const void *V, int dt, int64_t M, int64_t K, const double *Q, const double *P,
                   int R, double *out) override {
    RoctxRange roctx_("K10 residual / norm stream");
    void *v = const_cast<void *>(V);
    if (Q == nullptr) {
      if (dt == F32)
        rank_stream<float, 2>(v, M, K, nullptr, nullptr, 0, out);
      else if (dt == BF16)
        rank_stream<bf16s, 2>(v, M, K, nullptr, nullptr, 0, out);
      else
        rank_stream<double, 2>(v, M, K, nullptr, nullptr, 0, out);
    } else {
      if (dt == F32)
        rank_stream<float, 1>(v, M, K, Q, P, R, out);
      else if (dt == BF16)
        rank_stream<bf16s, 1>(v, M, K, Q, P, R, out);
      else
        rank_stream<double, 1>(v, M, K, Q, P, R, out);
    }
  }
  // ---- the influence plot: the residual's pass keeping its row and column sums (ops.h, residual_slices)
  // The walk in slabs both routes share. The pass geometry — n_tiles row tiles of rpt rows by nchunk k-chunks of
  // cpc columns — is fixed by the shape alone; the cap only cuts it into slabs of nt tiles x nc chunks whose
  // partial sums (8 (nt min(K, nc cpc) + nc nt rpt) bytes, and 1/G of the row part again) fit: whole row tiles
  // while one fits, otherwise one tile's chunks, in multiples of the row fold's group G. k_slice_group and
  // k_slice_fold add every slab's partials onto rowsq / colsq in an order of the geometry alone, so the cap
  // changes no bit. launch(tile0, nt, chunk0, nc, rp_ld, cp_ld, rowpart, colpart) runs the pass of one slab;
  // each is bracketed in the launch profile with the bytes of its part of the tensor.
  template <typename F>
  void slice_slabs(int64_t M, int64_t K, int64_t n_tiles, int64_t rpt, int64_t nchunk, int64_t cpc, size_t elem,
                   size_t cap, void *&work, size_t &work_bytes, double *rowsq, double *colsq, double *total,
                   F &&launch) {
    const int64_t G = (nchunk + 63) / 64;  // chunks per group of the row fold (kernels_slices.hip.h)
    const int nparts = (int)std::min<int64_t>(1024, (K + 8191) / 8192);  // of the two-level total
    const int64_t words = (int64_t)(cap / sizeof(double)) - nparts, one = K + (nchunk + (G > 1 ? 64 : 0)) * rpt;
    int64_t nt = 1, nc = nchunk;
    if (one <= words)
      nt = std::min(n_tiles, words / one);
    else
      nc = std::min(nchunk, std::max<int64_t>(1, words / ((cpc + 2 * rpt) * G)) * G);
    const int64_t rp_ld = std::min(M, nt * rpt), cp_ld = std::min(K, nc * cpc), ngs = G > 1 ? (nc + G - 1) / G : 0;
    const int64_t seg = (K + nparts - 1) / nparts;
    const size_t need = sizeof(double) * (size_t)((nc + ngs) * rp_ld + nt * cp_ld + nparts);
    if (need > work_bytes) {  // (the caller's buffer, exactly what is needed: it is held to a cap)
      free(work);
      work = nullptr;
      work_bytes = 0;
      work = alloc(need);
      work_bytes = need;
    }
    double *rowpart = (double *)work;
    double *colpart = rowpart + nc * rp_ld, *grp = colpart + nt * cp_ld, *parts = grp + ngs * rp_ld;
    route("slices_slabs:%lldx%lld", (long long)((n_tiles + nt - 1) / nt), (long long)((nchunk + nc - 1) / nc));
    for (int64_t t0 = 0; t0 < n_tiles; t0 += nt)
      for (int64_t c0 = 0; c0 < nchunk; c0 += nc) {
        const int64_t ntc = std::min(nt, n_tiles - t0), ncc = std::min(nc, nchunk - c0);
        const int64_t row0 = t0 * rpt, rows = std::min(M - row0, ntc * rpt);
        const int64_t kc0 = c0 * cpc, kcols = std::min(K - kc0, ncc * cpc);
        prof_begin(1, (double)rows * (double)kcols * elem);
        launch(t0, ntc, c0, ncc, rp_ld, cp_ld, rowpart, colpart);
        prof_end();
        HIP_CHECK(hipGetLastError());
        const int64_t ngc = (ncc + G - 1) / G;
        if (G > 1)
          hipLaunchKernelGGL(k_slice_group, dim3(grid_for(ngc * rows, 256)), dim3(256), 0, st_, rowpart, ncc, G, rp_ld,
                             rows, grp);
        hipLaunchKernelGGL(k_slice_fold, dim3(grid_for(rows + kcols, 256)), dim3(256), 0, st_, G > 1 ? grp : rowpart,
                           G > 1 ? ngc : ncc, rp_ld, rows, row0, c0 == 0 ? 1 : 0, colpart, ntc, cp_ld, kcols, kc0,
                           t0 == 0 ? 1 : 0, rowsq, colsq);
        HIP_CHECK(hipGetLastError());
      }
    hipLaunchKernelGGL(k_slice_total_parts, dim3(nparts), dim3(256), 0, st_, colsq, K, seg, parts);
    hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(1024), 0, st_, parts, nparts, total);
    HIP_CHECK(hipGetLastError());
  }
  // the fused route: MODE 3 of k_rank_mfma, on the shapes and with the geometry, the packed P and the REM
  // remainder of the residual (rank_plan); false: shape not covered
  template <typename TV>
  bool slices_mfma(const void *V, int64_t M, int64_t K, const double *Q, const double *P, int R, double *rowsq,
                   double *colsq, double *total, size_t cap, void *&work, size_t &wb) {
    constexpr int VEC = ScanTraits<TV>::VEC;
    RankPlan pl;
    if (!rank_plan<TV>(3, V, M, K, R, pl)) return false;
    const int RB = pl.RB, rem = pl.rem, per = pl.per, nkb = pl.nkb;
    double *Ppk = (double *)ensure(ws_pack_, ws_pack_sz_, sizeof(double) * (size_t)nkb * RB * 64);
    hipLaunchKernelGGL(k_rank_pack, dim3(grid_for((int64_t)nkb * RB * 64, 256)), dim3(256), 0, st_, P, K, R - rem, RB,
                       nkb, Ppk);
    const size_t lds_rem = sizeof(double) * (size_t)per * 16 * rem;
    route("slices_mfma:%s,R%d,RB%d,rem%d,tiles%lld,chunks%d", tname<TV>(), R, RB, rem, (long long)pl.n_mtiles,
          pl.nchunk);
    slice_slabs(M, K, pl.n_mtiles, 64 * VEC, pl.nchunk, (int64_t)per * 16, sizeof(TV), cap, work, wb, rowsq, colsq, total,
                [&](int64_t t0, int64_t nt, int64_t c0, int64_t nc, int64_t rp_ld, int64_t cp_ld, double *rowpart,
                    double *colpart) {
                  const dim3 grid((unsigned)nt, (unsigned)nc);
                  auto go = [&](auto mrb, auto rm) {
                    hipLaunchKernelGGL((k_rank_mfma<TV, 3, mrb, rm>), grid, dim3(256), lds_rem, st_, (TV *)V, M, K, Q,
                                       Ppk, R, RB, per, nkb, rowpart, P, colpart, (int)t0, (int)c0, rp_ld, cp_ld);
                  };
                  std::integral_constant<int, 0> none{};
                  if (rem && RB <= 2)
                    dispatch<1, 2>(rem, [&](auto rm) { go(std::integral_constant<int, 2>(), rm); });
                  else if (rem)
                    go(std::integral_constant<int, 4>(), std::integral_constant<int, 1>());
                  else if (RB <= 3)
                    go(std::integral_constant<int, 3>(), none);
                  else if (RB <= 4)
                    go(std::integral_constant<int, 4>(), none);
                  else
                    go(std::integral_constant<int, 8>(), none);
                });
    return true;
  }
  // the general route (k_slice_stream): 256-row tiles, enough k-chunks to fill the chip
  template <typename TV>
  void slices_stream(const void *V, int64_t M, int64_t K, const double *Q, const double *P, int R, double *rowsq,
                     double *colsq, double *total, size_t cap, void *&work, size_t &wb) {
    const int64_t n_tiles = (M + 255) / 256;
    const int64_t want = std::min<int64_t>((K + kSliceCols - 1) / kSliceCols,
                                           std::max<int64_t>(1, ((int64_t)ncu_ * 8 + n_tiles - 1) / n_tiles));
    const KSplit ks = k_split(K, want, 1, kSliceCols);
    const int64_t kch = ks.per, nchunk = ks.nsplit;
    route("slices_stream:%s,R%d,tiles%lld,chunks%lld", std::is_same<TV, bf16s>::value ? "bf16" : tname<TV>(), R,
          (long long)n_tiles, (long long)nchunk);
    slice_slabs(M, K, n_tiles, 256, nchunk, kch, sizeof(TV), cap, work, wb, rowsq, colsq, total,
                [&](int64_t t0, int64_t nt, int64_t c0, int64_t nc, int64_t rp_ld, int64_t cp_ld, double *rowpart,
                    double *colpart) {
                  const dim3 grid((unsigned)nt, (unsigned)nc);  // (nc <= 8 x the compute units)
                  auto go = [&](auto rb) {
                    hipLaunchKernelGGL((k_slice_stream<TV, rb>), grid, dim3(256), 0, st_, (const TV *)V, M, K, Q, P, R,
                                       kch, t0, c0, rp_ld, cp_ld, rowpart, colpart);
                  };
                  if (R <= 16)
                    go(std::integral_constant<int, 16>());
                  else if (R <= 64)
                    go(std::integral_constant<int, 64>());
                  else
                    go(std::integral_constant<int, 0>());
                });
  }
  template <typename TV>
  void slices_any(const void *V, int64_t M, int64_t K, const double *Q, const double *P, int R, double *rowsq,
                  double *colsq, double *total, size_t cap, void *&work, size_t &wb) {
    if constexpr (!std::is_same<TV, bf16s>::value)
      if (slices_mfma<TV>(V, M, K, Q, P, R, rowsq, colsq, total, cap, work, wb)) return;
    slices_stream<TV>(V, M, K, Q, P, R, rowsq, colsq, total, cap, work, wb);
  }
  void residual_slices(const void *V, int dt, int64_t M, int64_t K, const double *Q, const double *P, int R,
                       double *rowsq, double *colsq, double *total, size_t work_cap_bytes, void *&work,
                       size_t &work_bytes) override {
    RoctxRange roctx_("residual stream with slice sums");
    if (M < 1 || K < 1 || R < 1) throw std::runtime_error("ppals: residual_slices needs M, K, R >= 1");
    if (dt == F32)
      slices_any<float>(V, M, K, Q, P, R, rowsq, colsq, total, work_cap_bytes, work, work_bytes);
    else if (dt == BF16)
      slices_any<bf16s>(V, M, K, Q, P, R, rowsq, colsq, total, work_cap_bytes, work, work_bytes);
    else
      slices_any<double>(V, M, K, Q, P, R, rowsq, colsq, total, work_cap_bytes, work, work_bytes);
  }
  void fold_slice_sums(const double *src, const int64_t *lens, int n, double *out) override {
    if (n < 1 || n > MAX_ORDER) throw std::runtime_error("ppals: fold_slice_sums order out of range");
    SliceFoldArgs a;
    int64_t nout = 0;
    a.n = n;
    for (int j = 0; j < n; j++) nout += (a.lens[j] = lens[j]);
    if (nout > 0x7fffffff) throw std::runtime_error("ppals: fold_slice_sums: too many slices");
    route("fold_slice_sums:n%d", n);
    hipLaunchKernelGGL(k_fold_slice_sums, dim3((unsigned)nout), dim3(256), 0, st_, src, a, out);
    HIP_CHECK(hipGetLastError());
  }
  void row_dots(const double *P, const double *W, int64_t rows, int R, int64_t ld, double *out) override {
    hipLaunchKernelGGL(k_row_dots, dim3(grid_for(rows, 256)), dim3(256), 0, st_, P, W, rows, R, ld, out);
    HIP_CHECK(hipGetLastError());
  }
  void upload_shard(void *V, int dt, const double *host_full, int64_t l0, int64_t g0,
                    int64_t row0, int64_t rest) override {
    // stage `chunk` columns (each l0 contiguous rows of the shard) at a time through a device
    // fp64 buffer, converting to the tensor's storage type on the device
    const int64_t chunk_cols = std::max<int64_t>(1, (int64_t)(64 << 20) / (8 * l0));
    std::vector<double> host((size_t)(chunk_cols * l0));
    double *stage = (double *)alloc(sizeof(double) * chunk_cols * l0);
    for (int64_t c0 = 0; c0 < rest; c0 += chunk_cols) {
      int64_t nc = std::min(chunk_cols, rest - c0);
      for (int64_t c = 0; c < nc; c++)
        std::copy(host_full + (c0 + c) * g0 + row0, host_full + (c0 + c) * g0 + row0 + l0,
                  host.begin() + c * l0);
      h2d(stage, host.data(), sizeof(double) * nc * l0);
      int64_t n = nc * l0;
      if (dt == F32)
        hipLaunchKernelGGL(k_convert_rows<float>, dim3(grid_for(n, 256)), dim3(256), 0, st_,
                           (float *)V + c0 * l0, stage, n);
      else if (dt == BF16)
        hipLaunchKernelGGL(k_convert_rows<bf16s>, dim3(grid_for(n, 256)), dim3(256), 0, st_,
                           (bf16s *)V + c0 * l0, stage, n);
      else
        hipLaunchKernelGGL(k_convert_rows<double>, dim3(grid_for(n, 256)), dim3(256), 0, st_,
                           (double *)V + c0 * l0, stage, n);
      HIP_CHECK(hipGetLastError());
      sync();
    }
    free(stage);
  }

  void download_shard(const void *V, int dt, double *host_full, int64_t l0, int64_t g0,
                      int64_t row0, int64_t rest) override {
    const int64_t chunk_cols = std::max<int64_t>(1, (int64_t)(64 << 20) / (8 * l0));
    std::vector<double> host((size_t)(chunk_cols * l0));
    double *stage = (double *)alloc(sizeof(double) * chunk_cols * l0);
    for (int64_t c0 = 0; c0 < rest; c0 += chunk_cols) {
      const int64_t nc = std::min(chunk_cols, rest - c0), n = nc * l0;
      if (dt == F32)
        hipLaunchKernelGGL(k_widen_rows<float>, dim3(grid_for(n, 256)), dim3(256), 0, st_, stage,
                           (const float *)V + c0 * l0, n);
      else if (dt == BF16)
        hipLaunchKernelGGL(k_widen_rows<bf16s>, dim3(grid_for(n, 256)), dim3(256), 0, st_, stage,
                           (const bf16s *)V + c0 * l0, n);
      else
        hipLaunchKernelGGL(k_widen_rows<double>, dim3(grid_for(n, 256)), dim3(256), 0, st_, stage,
                           (const double *)V + c0 * l0, n);
      HIP_CHECK(hipGetLastError());
      d2h(host.data(), stage, sizeof(double) * n);
      for (int64_t c = 0; c < nc; c++)
        std::copy(host.begin() + c * l0, host.begin() + (c + 1) * l0,
                  host_full + (c0 + c) * g0 + row0);
    }
    free(stage);
  }

  // ------------------------------------------------------------------ device views
  bool device_ptr_info(const void *p, PtrInfo *out, std::string *why) override {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
      (void)hipGetLastError();
      *why = "unknown to the HIP runtime";
      return false;
    }
    out->device = at.device;
    out->is_device = at.type == hipMemoryTypeDevice && !at.isManaged && at.device == dev_;
    if (!out->is_device) {
      *why = at.isManaged || at.type == hipMemoryTypeManaged || at.type == hipMemoryTypeUnified
                 ? "managed memory"
             : at.type == hipMemoryTypeHost ? "host memory"
             : at.device != dev_ ? "memory of device " + std::to_string(at.device) + ", the context is on " +
                                       std::to_string(dev_)
                                 : "not device memory";
      return true;
    }
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) {
      (void)hipGetLastError();
      *why = "no allocation holds the pointer";
      out->is_device = false;
      return false;
    }
    out->base = (uint64_t)(uintptr_t)base;
    out->size = size;
    return true;
  }

  template <bool IMP, typename S, typename D>
  void io_launch(const ViewPlan &p, const S *src, D *dst) {
    if (p.kind == DV_STREAM) {
      bool vec = p.vs[0] == 1 && p.rs[0] == 1 && (uintptr_t)src % (4 * sizeof(S)) == 0 &&
                 (uintptr_t)dst % (4 * sizeof(D)) == 0;
      if (p.nd > 1) {
        vec = vec && p.n[0] % 4 == 0;
        for (int m = 1; m < p.nd; m++) vec = vec && p.vs[m] % 4 == 0 && p.rs[m] % 4 == 0;
      }
      const int g = grid_for(vec ? (p.count + 3) / 4 : p.count, 256, 16384);
      if (vec)
        hipLaunchKernelGGL((k_io_stream<IMP, true, S, D>), dim3(g), dim3(256), 0, st_, src, dst, p);
      else
        hipLaunchKernelGGL((k_io_stream<IMP, false, S, D>), dim3(g), dim3(256), 0, st_, src, dst, p);
    } else if (p.kind == DV_TILE) {
      int64_t FA, tA, tB, tiles;
      dv_tile_grid(p, &FA, &tA, &tB, &tiles);
      const int g = (int)std::min<int64_t>(tiles, 16384);
      hipLaunchKernelGGL((k_io_tile<IMP, S, D>), dim3(g), dim3(256), 0, st_, src, dst, p, FA, tA, tB,
                         tiles, p.rs[p.fk]);
    } else {
      hipLaunchKernelGGL((k_io_gather<IMP, S, D>), dim3(grid_for(p.count, 256, 16384)), dim3(256), 0,
                         st_, src, dst, p);
    }
    HIP_CHECK(hipGetLastError());
  }
  template <typename R>
  void io_import(const ViewPlan &p, const void *view, int vdt, R *V) {
    const char *s = (const char *)view;
    switch (vdt) {
      case DV_F32: io_launch<true>(p, (const float *)s + p.voff, V + p.roff); break;
      case DV_F64: io_launch<true>(p, (const double *)s + p.voff, V + p.roff); break;
      case DV_F16: io_launch<true>(p, (const _Float16 *)s + p.voff, V + p.roff); break;
      case DV_BF16: io_launch<true>(p, (const io_bf16 *)s + p.voff, V + p.roff); break;
      default: throw std::runtime_error("ppals: bad view dtype");
    }
  }
  template <typename R>
  void io_export(const ViewPlan &p, void *view, int vdt, const R *V) {
    if (vdt == DV_F32)
      io_launch<false>(p, V + p.roff, (float *)view + p.voff);
    else if (vdt == DV_F64)
      io_launch<false>(p, V + p.roff, (double *)view + p.voff);
    else
      throw std::runtime_error("ppals: bad view dtype");
  }
  void copy_view(const ViewPlan &p, int dir, void *view, int vdt, void *V, int dt,
                 void *caller_stream) override {
    HIP_CHECK(hipSetDevice(dev_));
    if (!io_ev_in_) {
      HIP_CHECK(hipEventCreateWithFlags(&io_ev_in_, hipEventDisableTiming));
      HIP_CHECK(hipEventCreateWithFlags(&io_ev_out_, hipEventDisableTiming));
    }
    hipStream_t cs = (hipStream_t)caller_stream;
    HIP_CHECK(hipEventRecord(io_ev_in_, cs));  // the view is ready once the caller's work so far is done
    HIP_CHECK(hipStreamWaitEvent(st_, io_ev_in_, 0));
    if (dir == DV_IMPORT) {
      if (dt == F32)
        io_import(p, view, vdt, (float *)V);
      else if (dt == BF16)
        io_import(p, view, vdt, (bf16s *)V);
      else
        io_import(p, view, vdt, (double *)V);
    } else {
      if (dt == F32)
        io_export(p, view, vdt, (const float *)V);
      else if (dt == BF16)
        io_export(p, view, vdt, (const bf16s *)V);
      else
        io_export(p, view, vdt, (const double *)V);
    }
    HIP_CHECK(hipEventRecord(io_ev_out_, st_));  // and the caller's later work waits for the copy
    HIP_CHECK(hipStreamWaitEvent(cs, io_ev_out_, 0));
  }
  hipEvent_t io_ev_in_ = nullptr, io_ev_out_ = nullptr;
  void io_events() {
    HIP_CHECK(hipSetDevice(dev_));
    if (!io_ev_in_) {
      HIP_CHECK(hipEventCreateWithFlags(&io_ev_in_, hipEventDisableTiming));
      HIP_CHECK(hipEventCreateWithFlags(&io_ev_out_, hipEventDisableTiming));
    }
  }
  void join_stream(void *caller_stream) override {
    io_events();
    HIP_CHECK(hipEventRecord(io_ev_in_, (hipStream_t)caller_stream));
    HIP_CHECK(hipStreamWaitEvent(st_, io_ev_in_, 0));
  }
  void release_stream(void *caller_stream) override {
    io_events();
    HIP_CHECK(hipEventRecord(io_ev_out_, st_));
    HIP_CHECK(hipStreamWaitEvent((hipStream_t)caller_stream, io_ev_out_, 0));
  }

  // ------------------------------------------------------------------ preprocessing in place (kernels_prep.hip.h)
  // The route rule, a plain formula on (dt, L, J) and the base alignment:
  //   L == 1: lead.runs while a fibre fits the run buffer, J * size <= 48 KiB; lead.long beyond.
  //   L  > 1: vec = L % VEC == 0 and V aligned to VEC elements (VEC = 4, 2, 4 for f32, f64, bf16); a tile is
  //           BL = vec ? 16 * VEC : 64 consecutive l; centring keeps the tile on chip (rows.lds) while
  //           J * BL * size <= 56 KiB and takes two passes (rows.twopass) beyond. shift and scale keep nothing.
  static int pow2_floor(int64_t x) {
    int p = 1;
    while (2 * (int64_t)p <= x) p *= 2;
    return p;
  }
  static int pow2_ceil(int64_t x, int cap) {
    int p = 1;
    while (p < x && p < cap) p *= 2;
    return p;
  }
  static const char *prep_name(int mode) { return mode == PREP_CENTER ? "center" : mode == PREP_SHIFT ? "shift" : "scale"; }
  template <typename TV, int MODE>
  void prep_lead(TV *V, int64_t J, int64_t T, double *off, const double *fac, double alpha) {
    const int64_t fib_bytes = J * (int64_t)sizeof(TV);
    if (fib_bytes > PREP_LEAD_RUN_BYTES) {
      route("prep.%s.%s.lead.long", prep_name(MODE), sname<TV>());
      hipLaunchKernelGGL((k_prep_lead_long<TV, MODE>), dim3((unsigned)std::min<int64_t>(T, 16384)), dim3(PREP_THREADS),
                         8 * PREP_THREADS, st_, V, J, T, off, fac, alpha);
      return;
    }
    // fibres a run: what the buffer holds, fewer while that leaves the device without work (4 runs a CU)
    int64_t F = std::max<int64_t>(1, PREP_LEAD_RUN_BYTES / fib_bytes);
    F = std::min(F, std::max<int64_t>(1, (T + 4 * ncu_ - 1) / (4 * (int64_t)ncu_)));
    const int G = F >= PREP_THREADS ? 1 : std::min(pow2_floor(PREP_THREADS / F), pow2_ceil(J, PREP_THREADS));
    if (G > 1) F = std::min<int64_t>(F, PREP_THREADS / G);
    const int64_t nruns = (T + F - 1) / F;
    const size_t lds = 8 * PREP_THREADS + (size_t)(PrepVec16<TV>::N + F * J) * sizeof(TV);
    route("prep.%s.%s.lead.runs F=%lld G=%d", prep_name(MODE), sname<TV>(), (long long)F, G);
    hipLaunchKernelGGL((k_prep_lead<TV, MODE>), dim3((unsigned)std::min<int64_t>(nruns, 16384)), dim3(PREP_THREADS),
                       (lds + 15) / 16 * 16, st_, V, (int)J, T, (int)F, G, off, fac, alpha);
  }
  template <typename TV, int MODE, int VEC, int LX>
  void prep_rows_launch(TV *V, int64_t L, int64_t J, int64_t T, double *off, const double *fac, double alpha) {
    constexpr int BL = LX * VEC;
    const int64_t ntl = (L + BL - 1) / BL;
    const bool onchip = MODE == PREP_CENTER && J * BL * (int64_t)sizeof(TV) <= PREP_ROWS_TILE_BYTES;
    const size_t lds = MODE != PREP_CENTER ? 0 : 8 * (size_t)PREP_THREADS * VEC + (onchip ? (size_t)J * BL * sizeof(TV) : 0);
    const dim3 grid((unsigned)std::min<int64_t>(ntl * T, 16384));
    route("prep.%s.%s.rows.%s vec=%d", prep_name(MODE), sname<TV>(),
          MODE != PREP_CENTER ? "stream" : onchip ? "lds" : "twopass", VEC > 1 ? 1 : 0);
    if (onchip)
      hipLaunchKernelGGL((k_prep_rows<TV, VEC, LX, MODE, MODE == PREP_CENTER>), grid, dim3(PREP_THREADS), lds, st_, V, L, J,
                         T, ntl, off, fac, alpha);
    else
      hipLaunchKernelGGL((k_prep_rows<TV, VEC, LX, MODE, false>), grid, dim3(PREP_THREADS), lds, st_, V, L, J, T, ntl,
                         off, fac, alpha);
  }
  template <typename TV, int MODE>
  void prep_typed(TV *V, int64_t L, int64_t J, int64_t T, double *off, const double *fac, double alpha) {
    if (L * J * T <= 0) return;
    constexpr int VEC = PrepRowsVec<TV>::N;
    if (L == 1)
      prep_lead<TV, MODE>(V, J, T, off, fac, alpha);
    else if (L % VEC == 0 && (uintptr_t)V % (VEC * sizeof(TV)) == 0)
      prep_rows_launch<TV, MODE, VEC, 16>(V, L, J, T, off, fac, alpha);
    else
      prep_rows_launch<TV, MODE, 1, 64>(V, L, J, T, off, fac, alpha);
    HIP_CHECK(hipGetLastError());
  }
  template <int MODE>
  void prep_dispatch(void *V, int dt, int64_t L, int64_t J, int64_t T, double *off, const double *fac, double alpha) {
    if (dt == F32)
      prep_typed<float, MODE>((float *)V, L, J, T, off, fac, alpha);
    else if (dt == BF16)
      prep_typed<bf16s, MODE>((bf16s *)V, L, J, T, off, fac, alpha);
    else
      prep_typed<double, MODE>((double *)V, L, J, T, off, fac, alpha);
  }
  void center_fibres(void *V, int dt, int64_t L, int64_t J, int64_t T, double *off) override {
    prep_dispatch<PREP_CENTER>(V, dt, L, J, T, off, nullptr, 0.0);
  }
  void shift_fibres(void *V, int dt, int64_t L, int64_t J, int64_t T, const double *off, double alpha) override {
    prep_dispatch<PREP_SHIFT>(V, dt, L, J, T, const_cast<double *>(off), nullptr, alpha);
  }
  void scale_slices(void *V, int dt, int64_t L, int64_t J, int64_t T, const double *fac) override {
    prep_dispatch<PREP_SCALE>(V, dt, L, J, T, nullptr, fac, 0.0);
  }
  // ss[j] from one partial sum per (block, slice), folded in block order. nb blocks a slice: enough for ~8
  // workgroups a CU, no more than there are rows of t, and nb * J partial sums capped at 64 MB.
  template <typename TV>
  void sumsq_typed(const TV *V, int64_t L, int64_t J, int64_t T, double *ss) {
    constexpr int VEC = PrepVec16<TV>::N;
    const bool vec = L > 1 && L % VEC == 0 && (uintptr_t)V % 16 == 0;
    const int X = L == 1 ? pow2_ceil(J, PREP_THREADS) : pow2_ceil(vec ? L / VEC : L, PREP_THREADS);
    const int Y = PREP_THREADS / X;
    const int64_t gx = L == 1 ? (J + X - 1) / X : J;
    int64_t nb = std::max<int64_t>(1, (8 * (int64_t)ncu_ + gx - 1) / gx);
    nb = std::min(nb, (T + Y - 1) / Y);
    nb = std::min(nb, std::max<int64_t>(1, ((int64_t)64 << 20) / (8 * J)));
    nb = std::min<int64_t>(nb, 65535);
    if (gx > 0x7fffffff) throw Unsupported("ppals: slice_sumsq supports at most 2^31 - 1 slices");
    double *part = (double *)ensure(ws_part_, ws_part_sz_, sizeof(double) * (size_t)nb * J);
    const dim3 grid((unsigned)gx, (unsigned)nb);
    route("prep.sumsq.%s.%s vec=%d X=%d nb=%lld", sname<TV>(), L == 1 ? "lead" : "rows", vec ? 1 : 0, X, (long long)nb);
    if (L == 1)
      hipLaunchKernelGGL((k_sumsq_lead<TV>), grid, dim3(PREP_THREADS), 8 * PREP_THREADS, st_, V, J, T, X, part);
    else if (vec)
      hipLaunchKernelGGL((k_sumsq_rows<TV, VEC>), grid, dim3(PREP_THREADS), 8 * PREP_THREADS, st_, V, L, J, T, X, part);
    else
      hipLaunchKernelGGL((k_sumsq_rows<TV, 1>), grid, dim3(PREP_THREADS), 8 * PREP_THREADS, st_, V, L, J, T, X, part);
    hipLaunchKernelGGL(k_fold_partials, dim3(grid_for(J, 256)), dim3(256), 0, st_, part, (int)nb, J, ss);
    HIP_CHECK(hipGetLastError());
  }
  void slice_sumsq(const void *V, int dt, int64_t L, int64_t J, int64_t T, double *ss) override {
    if (J <= 0) return;
    if (L * T <= 0) {
      zero(ss, sizeof(double) * J);
      return;
    }
    if (dt == F32)
      sumsq_typed((const float *)V, L, J, T, ss);
    else if (dt == BF16)
      sumsq_typed((const bf16s *)V, L, J, T, ss);
    else
      sumsq_typed((const double *)V, L, J, T, ss);
  }

  // ------------------------------------------------------------------ N-PLS (kernels_npls.hip.h)
  // The route rule, a plain formula on (dt, L, I) and the base alignment; nothing in it looks at
  // the number of columns, so that a column has the same bits in whatever chunk it travels:
  //   contract:    L < 64 and one t (L * I * size) within the 32 KiB run buffer: runs; beyond it long for L == 1;
  //                everything else rows, vec = L % VEC == 0 and X aligned to VEC elements (VEC = 4, 2, 4 for f32,
  //                f64, bf16).
  //   slice_inner: L < 64: flat; else rows, vec = L % V16 == 0 and X aligned to 16 bytes (V16 = 4, 2, 8).
  template <typename TV, int CW>
  void npls_contract_chunk(const TV *X, int64_t L, int64_t I, int64_t T, const double *U, int nc, double *Z) {
    const int64_t run_bytes = L * I * (int64_t)sizeof(TV);
    if (L < NPLS_FLAT_L && run_bytes <= NPLS_RUN_BYTES) {
      int64_t NT = std::max<int64_t>(1, NPLS_RUN_BYTES / run_bytes);
      NT = std::min(NT, std::max<int64_t>(1, (T + 4 * ncu_ - 1) / (4 * (int64_t)ncu_)));
      const int64_t F = NT * L;
      const int G = F >= PREP_THREADS ? 1 : std::min(pow2_floor(PREP_THREADS / F), pow2_ceil(I, PREP_THREADS));
      const int64_t nruns = (T + NT - 1) / NT;
      const int ulds = I * NPLS_CW * (int64_t)sizeof(double) <= NPLS_ULDS_BYTES ? 1 : 0;  // (of a full chunk: not of C)
      const size_t lds = 8 * (size_t)PREP_THREADS * CW + (ulds ? 8 * (size_t)((CW * I + 1) / 2 * 2) : 0) +
                         (size_t)(PrepVec16<TV>::N + NT * L * I) * sizeof(TV);
      route("npls.contract.%s.runs NT=%lld G=%d ulds=%d", sname<TV>(), (long long)NT, G, ulds);
      hipLaunchKernelGGL((k_npls_contract_runs<TV, CW>), dim3((unsigned)std::min<int64_t>(nruns, 16384)), dim3(PREP_THREADS),
                         (lds + 15) / 16 * 16, st_, X, (int)L, (int)I, T, (int)NT, G, U, nc, ulds, Z);
    } else if (L == 1) {
      route("npls.contract.%s.long", sname<TV>());
      hipLaunchKernelGGL((k_npls_contract_long<TV, CW>), dim3((unsigned)std::min<int64_t>(T, 16384)), dim3(PREP_THREADS),
                         8 * PREP_THREADS, st_, X, I, T, U, nc, Z);
    } else {
      constexpr int VEC = PrepRowsVec<TV>::N;
      const bool vec = L % VEC == 0 && (uintptr_t)X % (VEC * sizeof(TV)) == 0;
      const int64_t n = (vec ? L / VEC : L) * T, LT = L * T, blocks = (n + PREP_THREADS - 1) / PREP_THREADS;
      // too few threads for the device and a long i: ns splits of i (at least 32 i each, the partial sums of a full
      // chunk within 64 MB), folded in split order
      int64_t ns = 1;
      if (blocks < 4 * (int64_t)ncu_ && I >= 64) {
        ns = std::min<int64_t>((4 * (int64_t)ncu_ + blocks - 1) / blocks, I / 32);
        ns = std::min(ns, std::max<int64_t>(1, ((int64_t)64 << 20) / (8 * LT * NPLS_CW)));
        ns = std::min<int64_t>(ns, 65535);
      }
      const dim3 grid((unsigned)std::min<int64_t>(blocks, 262144), (unsigned)ns);
      double *out = ns > 1 ? (double *)ensure(ws_part_, ws_part_sz_, sizeof(double) * (size_t)ns * CW * LT) : Z;
      const int64_t sstride = ns > 1 ? CW * LT : 0;
      route("npls.contract.%s.rows vec=%d ns=%lld", sname<TV>(), vec ? 1 : 0, (long long)ns);
      if (vec)
        hipLaunchKernelGGL((k_npls_contract_rows<TV, VEC, CW>), grid, dim3(PREP_THREADS), 0, st_, X, L, I, T, U, nc, out, LT,
                           sstride);
      else
        hipLaunchKernelGGL((k_npls_contract_rows<TV, 1, CW>), grid, dim3(PREP_THREADS), 0, st_, X, L, I, T, U, nc, out, LT,
                           sstride);
      if (ns > 1)
        hipLaunchKernelGGL(k_npls_fold, dim3(grid_for(LT, 256)), dim3(256), 0, st_, out, (int)ns, CW, (int64_t)1, LT, nc, Z);
    }
  }
  // nb blocks a row of partial sums: enough for ~8 workgroups a CU, no more than there are rows of t, the partial
  // sums of a full chunk capped at 64 MB
  int64_t npls_nb(int64_t gx, int64_t rows, int64_t T, int Y) {
    int64_t nb = std::max<int64_t>(1, (8 * (int64_t)ncu_ + gx - 1) / gx);
    nb = std::min(nb, (T + Y - 1) / Y);
    nb = std::min(nb, std::max<int64_t>(1, ((int64_t)64 << 20) / (8 * rows * NPLS_CW)));
    return std::min<int64_t>(nb, 65535);
  }
  template <typename TV, int CW>
  void npls_si_chunk(const TV *X, int64_t L, int64_t I, int64_t T, const double *W, int nc, double *S) {
    if (L < NPLS_FLAT_L) {
      const int64_t J = L * I;
      const int XL = pow2_ceil(J, PREP_THREADS), Y = PREP_THREADS / XL;
      const int64_t gx = (J + XL - 1) / XL, nb = npls_nb(gx, J, T, Y);
      if (gx > 0x7fffffff) throw Unsupported("ppals: slice_inner supports at most 2^31 - 1 rows of partial sums");
      double *part = (double *)ensure(ws_part_, ws_part_sz_, sizeof(double) * (size_t)nb * CW * J);
      route("npls.slice_inner.%s.flat X=%d nb=%lld", sname<TV>(), XL, (long long)nb);
      hipLaunchKernelGGL((k_npls_si_flat<TV, CW>), dim3((unsigned)gx, (unsigned)nb), dim3(PREP_THREADS),
                         8 * PREP_THREADS * CW, st_, X, L, J, T, XL, W, nc, part);
      hipLaunchKernelGGL(k_npls_fold, dim3(grid_for(I, 256)), dim3(256), 0, st_, part, (int)nb, CW, L, I, nc, S);
      return;
    }
    constexpr int VEC = PrepVec16<TV>::N;
    const bool vec = L % VEC == 0 && (uintptr_t)X % 16 == 0;
    const int64_t Lv = vec ? L / VEC : L;
    const int XL = pow2_ceil(Lv, PREP_THREADS), Y = PREP_THREADS / XL;
    const int64_t gx = (I + NPLS_IB - 1) / NPLS_IB, nbt = npls_nb(gx, I, T, Y);
    // where the rows of t leave the device short of work (T = 1: the sample mode last), the blocks split l as well
    int64_t nbl = 1;
    if (gx * nbt < 8 * (int64_t)ncu_) {
      nbl = std::min<int64_t>((8 * (int64_t)ncu_ + gx * nbt - 1) / (gx * nbt), (Lv + XL - 1) / XL);
      nbl = std::min(nbl, std::max<int64_t>(1, ((int64_t)64 << 20) / (8 * I * NPLS_CW * nbt)));
      nbl = std::max<int64_t>(1, std::min<int64_t>(nbl, 65535 / nbt));
    }
    const int64_t nb = nbt * nbl;
    if (gx > 0x7fffffff) throw Unsupported("ppals: slice_inner supports at most 2^33 - 4 slices");
    double *part = (double *)ensure(ws_part_, ws_part_sz_, sizeof(double) * (size_t)nb * CW * I);
    route("npls.slice_inner.%s.rows vec=%d X=%d nbt=%lld nbl=%lld", sname<TV>(), vec ? 1 : 0, XL, (long long)nbt, (long long)nbl);
    const dim3 grid((unsigned)gx, (unsigned)nb);
    if (vec)
      hipLaunchKernelGGL((k_npls_si_rows<TV, VEC, CW>), grid, dim3(PREP_THREADS), 8 * PREP_THREADS, st_, X, L, I, T, XL,
                         (int)nbl, W, nc, part);
    else
      hipLaunchKernelGGL((k_npls_si_rows<TV, 1, CW>), grid, dim3(PREP_THREADS), 8 * PREP_THREADS, st_, X, L, I, T, XL,
                         (int)nbl, W, nc, part);
    hipLaunchKernelGGL(k_npls_fold, dim3(grid_for(I, 256)), dim3(256), 0, st_, part, (int)nb, CW, (int64_t)1, I, nc, S);
  }
  // a single column goes alone, more in chunks of NPLS_CW
  template <typename TV>
  void npls_contract_typed(const TV *X, int64_t L, int64_t I, int64_t T, const double *U, int C, double *Z) {
    if (C == 1) npls_contract_chunk<TV, 1>(X, L, I, T, U, 1, Z);
    else
      for (int c0 = 0; c0 < C; c0 += NPLS_CW)
        npls_contract_chunk<TV, NPLS_CW>(X, L, I, T, U + I * c0, std::min(NPLS_CW, C - c0), Z + L * T * c0);
    HIP_CHECK(hipGetLastError());
  }
  template <typename TV>
  void npls_si_typed(const TV *X, int64_t L, int64_t I, int64_t T, const double *W, int C, double *S) {
    if (C == 1) npls_si_chunk<TV, 1>(X, L, I, T, W, 1, S);
    else
      for (int c0 = 0; c0 < C; c0 += NPLS_CW)
        npls_si_chunk<TV, NPLS_CW>(X, L, I, T, W + L * T * c0, std::min(NPLS_CW, C - c0), S + I * c0);
    HIP_CHECK(hipGetLastError());
  }
  void npls_contract(const void *X, int dt, int64_t L, int64_t I, int64_t T, const double *U, int C, double *Z) override {
    if (L * T <= 0 || C <= 0) return;
    if (I <= 0) {
      zero(Z, sizeof(double) * L * T * C);
      return;
    }
    // (profile slot 0, with the tensor scans: the bytes a chunk reads, once per chunk)
    prof_begin(0, (double)L * I * T * dtype_size(dt) * (C == 1 ? 1 : (C + NPLS_CW - 1) / NPLS_CW));
    if (dt == F32)
      npls_contract_typed((const float *)X, L, I, T, U, C, Z);
    else if (dt == BF16)
      npls_contract_typed((const bf16s *)X, L, I, T, U, C, Z);
    else
      npls_contract_typed((const double *)X, L, I, T, U, C, Z);
    prof_end();
  }
  void npls_slice_inner(const void *X, int dt, int64_t L, int64_t I, int64_t T, const double *W, int C, double *S) override {
    if (I <= 0 || C <= 0) return;
    if (L * T <= 0) {
      zero(S, sizeof(double) * I * C);
      return;
    }
    prof_begin(0, (double)L * I * T * dtype_size(dt) * (C == 1 ? 1 : (C + NPLS_CW - 1) / NPLS_CW));
    if (dt == F32)
      npls_si_typed((const float *)X, L, I, T, W, C, S);
    else if (dt == BF16)
      npls_si_typed((const bf16s *)X, L, I, T, W, C, S);
    else
      npls_si_typed((const double *)X, L, I, T, W, C, S);
    prof_end();
  }

  // ------------------------------------------------------------------ N-PLS, wide columns (kernels_npls_wide.hip.h)
  // The route rule, a plain formula on (L, I, T, C) ("Cross-validation"), the thresholds from
  // profiles/npls_cv_bench.md (a wide route is taken only where it did not lose to the narrow chunks):
  //   L == 1:      `wide.lead` for C > NPLS_CW and I >= 32 (below that a chunk of the contraction, or half a tile of
  //                output rows, is mostly padding: I = 3 lost), both ops;
  //   L >= 16:     `wide.rows` for C > 32 (contract: the narrow rows walk holds 0.67 of the HBM peak with four columns
  //                and wins up to C = 16) and for C > 8 (slice_inner);
  //   otherwise:   `narrow`, the ops above in their chunks of NPLS_CW.
  // A launch carries up to 64 columns in nt tiles of 16, C > 64 goes in chunks of 64. Where the output tiles alone
  // leave the device short of work the contracted index is split over grid.y into ns pieces (4 chunks of 32 each at
  // least, the partial sums of a launch within 64 MB) and k_npls_fold adds the pieces in split order.
  static bool npls_wide_geometry(bool contract, int64_t L, int64_t I, int C) {
    if (L == 1) return C > NPLS_CW && I >= 32;
    return L >= 16 && C > (contract ? 32 : 8);
  }
  int64_t npls_wide_ns(int64_t blocks, int64_t units, int64_t rows, int nc) {
    int64_t ns = std::max<int64_t>(1, (4 * (int64_t)ncu_ + blocks - 1) / blocks);
    ns = std::min(ns, std::max<int64_t>(1, units / 4));
    ns = std::min(ns, std::max<int64_t>(1, ((int64_t)64 << 20) / (8 * rows * nc)));
    return std::min<int64_t>(ns, 65535);
  }
  template <typename TX>
  void npls_wide_rows_launch(int nt, dim3 grid, const TX *X, int64_t s1, int64_t s2, int64_t n, int64_t K, const double *B,
                             int nc, int64_t tiles, double *out, int64_t cstride, int64_t sstride) {
    auto k = nt == 1 ? k_npls_wide_rows<TX, 1> : nt == 2 ? k_npls_wide_rows<TX, 2> : nt == 3 ? k_npls_wide_rows<TX, 3>
                                                                                              : k_npls_wide_rows<TX, 4>;
    hipLaunchKernelGGL(k, grid, dim3(256), 0, st_, X, s1, s2, n, K, B, nc, tiles, out, cstride, sstride);
  }
  template <typename TX>
  void npls_wide_cols_launch(int nt, dim3 grid, const TX *X, int64_t s1, int64_t s2, int64_t n, int64_t K, int64_t slabs,
                             const double *B, int nc, double *out, int64_t cstride, int64_t sstride) {
    auto k = nt == 1 ? k_npls_wide_cols<TX, 1> : nt == 2 ? k_npls_wide_cols<TX, 2> : nt == 3 ? k_npls_wide_cols<TX, 3>
                                                                                              : k_npls_wide_cols<TX, 4>;
    hipLaunchKernelGGL(k, grid, dim3(256), 0, st_, X, s1, s2, n, K, slabs, B, nc, out, cstride, sstride);
  }
  template <typename TX>
  void npls_contract_wide_typed(const TX *X, int64_t L, int64_t I, int64_t T, const double *U, int C, double *Z) {
    const int64_t LT = L * T;
    for (int c0 = 0; c0 < C; c0 += NPLS_WIDE_COLS) {
      const int nc = std::min(NPLS_WIDE_COLS, C - c0), nt = (nc + 15) / 16;
      const double *Uc = U + I * c0;
      double *Zc = Z + LT * c0;
      if (L > 1) {
        const int64_t tiles = (L + NPLS_WT - 1) / NPLS_WT;
        if (tiles * T > 0x7fffffff) throw Unsupported("ppals: the wide contraction supports at most 2^31 - 1 row tiles");
        route("npls.contract.%s.wide.rows nt=%d", sname<TX>(), nt);
        npls_wide_rows_launch<TX>(nt, dim3((unsigned)(tiles * T)), X, L, L * I, L, I, Uc, nc, tiles, Zc, LT, 0);
      } else {
        const int64_t blocks = (T + NPLS_WT - 1) / NPLS_WT, units = (I + NPLS_WCH - 1) / NPLS_WCH;
        if (blocks > 0x7fffffff) throw Unsupported("ppals: the wide contraction supports at most 2^31 - 1 row tiles");
        const int64_t ns = npls_wide_ns(blocks, units, T, nc);
        double *out = ns > 1 ? (double *)ensure(ws_part_, ws_part_sz_, sizeof(double) * (size_t)ns * nc * T) : Zc;
        route("npls.contract.%s.wide.lead nt=%d ns=%lld", sname<TX>(), nt, (long long)ns);
        npls_wide_cols_launch<TX>(nt, dim3((unsigned)blocks, (unsigned)ns), X, I, 0, T, I, 1, Uc, nc, out, T,
                                  ns > 1 ? nc * T : 0);
        if (ns > 1)
          hipLaunchKernelGGL(k_npls_fold, dim3(grid_for(T, 256)), dim3(256), 0, st_, out, (int)ns, nc, (int64_t)1, T, nc, Zc);
      }
    }
    HIP_CHECK(hipGetLastError());
  }
  template <typename TX>
  void npls_si_wide_typed(const TX *X, int64_t L, int64_t I, int64_t T, const double *W, int C, double *S) {
    const int64_t LT = L * T, blocks = (I + NPLS_WT - 1) / NPLS_WT;
    if (blocks > 0x7fffffff) throw Unsupported("ppals: the wide slice_inner supports at most 2^31 - 1 row tiles");
    for (int c0 = 0; c0 < C; c0 += NPLS_WIDE_COLS) {
      const int nc = std::min(NPLS_WIDE_COLS, C - c0), nt = (nc + 15) / 16;
      const double *Wc = W + LT * c0;
      double *Sc = S + I * c0;
      const int64_t units = L > 1 ? (L + NPLS_WCH - 1) / NPLS_WCH * T : (T + NPLS_WCH - 1) / NPLS_WCH;
      const int64_t ns = npls_wide_ns(blocks, units, I, nc);
      double *out = ns > 1 ? (double *)ensure(ws_part_, ws_part_sz_, sizeof(double) * (size_t)ns * nc * I) : Sc;
      const int64_t sstride = ns > 1 ? nc * I : 0;
      const dim3 grid((unsigned)blocks, (unsigned)ns);
      if (L > 1) {
        route("npls.slice_inner.%s.wide.rows nt=%d ns=%lld", sname<TX>(), nt, (long long)ns);
        npls_wide_cols_launch<TX>(nt, grid, X, L, L * I, I, L, T, Wc, nc, out, I, sstride);
      } else {
        route("npls.slice_inner.%s.wide.lead nt=%d ns=%lld", sname<TX>(), nt, (long long)ns);
        npls_wide_rows_launch<TX>(nt, grid, X, I, 0, I, T, Wc, nc, blocks, out, I, sstride);
      }
      if (ns > 1)
        hipLaunchKernelGGL(k_npls_fold, dim3(grid_for(I, 256)), dim3(256), 0, st_, out, (int)ns, nc, (int64_t)1, I, nc, Sc);
    }
    HIP_CHECK(hipGetLastError());
  }
  void npls_contract_wide(const void *X, int dt, int64_t L, int64_t I, int64_t T, const double *U, int C, double *Z) override {
    if (!npls_wide_geometry(true, L, I, C) || L * T <= 0 || I <= 0) {
      route("npls.contract.%s.wide.narrow", dt == F32 ? "f32" : dt == BF16 ? "bf16" : "f64");
      npls_contract(X, dt, L, I, T, U, C, Z);
      return;
    }
    prof_begin(0, (double)L * I * T * dtype_size(dt) * ((C + NPLS_WIDE_COLS - 1) / NPLS_WIDE_COLS));
    if (dt == F32)
      npls_contract_wide_typed((const float *)X, L, I, T, U, C, Z);
    else if (dt == BF16)
      npls_contract_wide_typed((const bf16s *)X, L, I, T, U, C, Z);
    else
      npls_contract_wide_typed((const double *)X, L, I, T, U, C, Z);
    prof_end();
  }
  void npls_slice_inner_wide(const void *X, int dt, int64_t L, int64_t I, int64_t T, const double *W, int C, double *S) override {
    if (!npls_wide_geometry(false, L, I, C) || L * T <= 0 || I <= 0) {
      route("npls.slice_inner.%s.wide.narrow", dt == F32 ? "f32" : dt == BF16 ? "bf16" : "f64");
      npls_slice_inner(X, dt, L, I, T, W, C, S);
      return;
    }
    prof_begin(0, (double)L * I * T * dtype_size(dt) * ((C + NPLS_WIDE_COLS - 1) / NPLS_WIDE_COLS));
    if (dt == F32)
      npls_si_wide_typed((const float *)X, L, I, T, W, C, S);
    else if (dt == BF16)
      npls_si_wide_typed((const bf16s *)X, L, I, T, W, C, S);
    else
      npls_si_wide_typed((const double *)X, L, I, T, W, C, S);
    prof_end();
  }
  void npls_outer_axpy(double *A, const int64_t *ext, int K, const double *const *w, double alpha) override {
    if (K < 1 || K > NPLS_MAX_DIMS) throw Unsupported("ppals: outer_axpy takes 1 to 8 vectors");
    NplsOuter o;
    o.K = K;
    int64_t n = 1;
    for (int k = 0; k < K; k++) {
      o.ext[k] = ext[k];
      o.w[k] = w[k];
      n *= ext[k];
    }
    if (n <= 0) return;
    hipLaunchKernelGGL(k_npls_outer_axpy, dim3(grid_for(n, 256, 16384)), dim3(256), 0, st_, A, n, o, alpha);
    HIP_CHECK(hipGetLastError());
  }
  void npls_argmax(const double *Z, int64_t n, double *out) override {
    if (n <= 0) return;
    const int np = grid_for(n, PREP_THREADS, 1024);
    char *ws = (char *)ensure(ws_part_, ws_part_sz_, 16 * (size_t)np);
    double *pv = (double *)ws;
    int64_t *pi = (int64_t *)(ws + 8 * (size_t)np);
    hipLaunchKernelGGL(k_npls_argmax_part, dim3(np), dim3(PREP_THREADS), 0, st_, Z, n, pv, pi);
    hipLaunchKernelGGL(k_npls_argmax_fold, dim3(1), dim3(PREP_THREADS), 0, st_, pv, pi, np, n, out);
    HIP_CHECK(hipGetLastError());
  }

  // ------------------------------------------------------------------ model through a view
  template <typename D, typename TV, int MODE>
  void mv_launch(dim3 grid, D *dst, const TV *V, const double *Q, const double *P, int K,
                 const ModelPlan &mp, const int64_t *tab, int flags, double *part = nullptr) {
    const int64_t A = mp.ga.count, B = mp.gb.count;
    const int64_t *tav = tab, *tar = tab + A, *tbv = tab + 2 * A, *tbr = tab + 2 * A + B;
    if (K <= 16)
      hipLaunchKernelGGL((k_model_view<D, TV, MODE, 4>), grid, dim3(256), 0, st_, dst, V, Q, P, K, mp,
                         tav, tar, tbv, tbr, flags, part);
    else
      hipLaunchKernelGGL((k_model_view<D, TV, MODE, 16>), grid, dim3(256), 0, st_, dst, V, Q, P, K, mp,
                         tav, tar, tbv, tbr, flags, part);
  }
  template <typename D>
  void mv_dispatch(dim3 grid, D *dst, const void *V, int dt, const double *Q, const double *P, int K,
                   bool residual, const ModelPlan &mp, const int64_t *tab, int flags) {
    if (!residual)
      mv_launch<D, float, MV_MODEL>(grid, dst, nullptr, Q, P, K, mp, tab, flags);
    else if (dt == F32)
      mv_launch<D, float, MV_RESIDUAL>(grid, dst, (const float *)V, Q, P, K, mp, tab, flags);
    else if (dt == BF16)
      mv_launch<D, bf16s, MV_RESIDUAL>(grid, dst, (const bf16s *)V, Q, P, K, mp, tab, flags);
    else
      mv_launch<D, double, MV_RESIDUAL>(grid, dst, (const double *)V, Q, P, K, mp, tab, flags);
  }
  void model_to_view(const ModelPlan &mp, const double *Q, const double *P, int K, bool residual,
                     void *view, int vdt, const void *V, int dt, void *caller_stream) override {
    HIP_CHECK(hipSetDevice(dev_));
    const int64_t A = mp.ga.count, B = mp.gb.count;
    if (A <= 0 || B <= 0) return;
    if (K < 1) throw std::runtime_error("ppals: model_to_view needs K >= 1");
    if (vdt != DV_F32 && vdt != DV_F64) throw std::runtime_error("ppals: bad model view dtype");
    dim3 grid;
    const int64_t *tab = mv_tables(mp, &grid);
    const int vw = vdt == DV_F32 ? 4 : 2;
    const bool a_unit = mp.ga.view_unit();
    bool vec = a_unit && A % vw == 0 && mp.voff % vw == 0 &&
               ((uintptr_t)view) % 16 == 0;
    for (int i = 0; i < mp.gb.n; i++)
      if (mp.gb.len[i] > 1 && mp.gb.vs[i] % vw != 0) vec = false;
    const int flags = (a_unit ? 1 : 0) | (vec ? 2 : 0) | (mp.ga.shard_unit() ? 4 : 0);
    if (!io_ev_in_) {
      HIP_CHECK(hipEventCreateWithFlags(&io_ev_in_, hipEventDisableTiming));
      HIP_CHECK(hipEventCreateWithFlags(&io_ev_out_, hipEventDisableTiming));
    }
    hipStream_t cs = (hipStream_t)caller_stream;
    HIP_CHECK(hipEventRecord(io_ev_in_, cs));  // the view is the caller's once its work so far is done
    HIP_CHECK(hipStreamWaitEvent(st_, io_ev_in_, 0));
    if (vdt == DV_F32)
      mv_dispatch<float>(grid, (float *)view, V, dt, Q, P, K, residual, mp, tab, flags);
    else
      mv_dispatch<double>(grid, (double *)view, V, dt, Q, P, K, residual, mp, tab, flags);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(io_ev_out_, st_));  // and the caller's later work waits for the stores
    HIP_CHECK(hipStreamWaitEvent(cs, io_ev_out_, 0));
  }

  // the offset tables of both groups of a plan, built on the engine stream (nothing of the caller's is
  // read), and a chip's worth of workgroups, each walking its share of the b tiles
  const int64_t *mv_tables(const ModelPlan &mp, dim3 *grid, int wgs_per_cu = 8) {
    const int64_t A = mp.ga.count, B = mp.gb.count;
    const int64_t ntA = (A + MV_TILE - 1) / MV_TILE, ntB = (B + MV_TILE - 1) / MV_TILE;
    if (ntA > 0x7fffffff) throw std::runtime_error("ppals: model view too wide");
    int64_t *tab = (int64_t *)ensure(ws_mv_, ws_mv_sz_, sizeof(int64_t) * 2 * (size_t)(A + B));
    hipLaunchKernelGGL(k_model_offsets, dim3(grid_for(A, 256)), dim3(256), 0, st_, mp.ga, tab, tab + A);
    hipLaunchKernelGGL(k_model_offsets, dim3(grid_for(B, 256)), dim3(256), 0, st_, mp.gb, tab + 2 * A,
                       tab + 2 * A + B);
    HIP_CHECK(hipGetLastError());
    const int64_t want = std::max<int64_t>(1, ((int64_t)ncu_ * wgs_per_cu + ntA - 1) / ntA);
    *grid = dim3((unsigned)ntA, (unsigned)std::min<int64_t>(std::min<int64_t>(want, ntB), 65535));
    return tab;
  }
  // Routes of the imputation: K <= 16, or a caller that keeps the route CP sessions have always had
  // (wide = false): the impute instantiations of k_model_view (MAXRB = 16 above K = 16: it spills).
  // wide and 16 < K <= MW_KMAX (Tucker sessions: K is the leading core rank): k_model_impute_wide, Q
  // in LDS. (K > MW_KMAX = 112, which set_factors admits and no sweep does: k_model_view again.)
  template <typename T>
  void impute_launch(dim3 grid, T *V, const uint8_t *mask, const double *Q, const double *P, int K,
                     const ModelPlan &mp, const int64_t *tab, int flags, double *part, bool wide) {
    if (!wide) {
      if (part)
        mv_launch<T, uint8_t, MV_IMPUTE_SQ>(grid, V, mask, Q, P, K, mp, tab, flags, part);
      else
        mv_launch<T, uint8_t, MV_IMPUTE>(grid, V, mask, Q, P, K, mp, tab, flags);
      return;
    }
    if constexpr (std::is_same<T, bf16s>::value) {
      throw std::runtime_error("ppals: the wide imputation stores F32 or F64");
    } else {
      const int64_t A = mp.ga.count, B = mp.gb.count;
      const int64_t *tav = tab, *tar = tab + A, *tbv = tab + 2 * A, *tbr = tab + 2 * A + B;
      const size_t lds = mw_lds_bytes(K);
      if (part)
        hipLaunchKernelGGL((k_model_impute_wide<T, true>), grid, dim3(256), lds, st_, V, mask, Q, P, K, mp,
                           tav, tar, tbv, tbr, flags, part);
      else
        hipLaunchKernelGGL((k_model_impute_wide<T, false>), grid, dim3(256), lds, st_, V, mask, Q, P, K, mp,
                           tav, tar, tbv, tbr, flags, part);
    }
  }
  void model_impute(const ModelPlan &plan, const double *Q, const double *P, int K, bool wide_k,
                    const void *mask, void *V, int dt, double *sumsq, void *caller_stream) override {
    HIP_CHECK(hipSetDevice(dev_));
    const int64_t A = plan.ga.count, B = plan.gb.count;
    if (A <= 0 || B <= 0) {
      if (sumsq) zero(sumsq, sizeof(double));
      return;
    }
    if (K < 1) throw std::runtime_error("ppals: model_impute needs K >= 1");
    const bool wide = wide_k && K > 16 && K <= MW_KMAX;
    const ModelPlan mp = dv_model_swapped(plan);  // the kernel's "view" is the shard, its "V" the mask
    dim3 grid;
    // (the wide kernel: two rounds of the workgroups its LDS lets a CU hold, so that Q is staged rarely)
    const int64_t *tab = wide ? mv_tables(mp, &grid, 2 * mw_wgs_per_cu(K)) : mv_tables(mp, &grid);
    const int64_t npart = (int64_t)grid.x * grid.y;
    if (sumsq && npart > 0x7fffffff) throw std::runtime_error("ppals: model view too wide");
    double *part = sumsq ? (double *)ensure(ws_part_, ws_part_sz_, sizeof(double) * npart) : nullptr;
    // bit 0: the shard is unit-stride over A; bit 2: the mask is (its bytes are read in the store pass)
    const int flags = (mp.ga.view_unit() ? 1 : 0) | (mp.ga.shard_unit() ? 4 : 0);
    if (!io_ev_in_) {
      HIP_CHECK(hipEventCreateWithFlags(&io_ev_in_, hipEventDisableTiming));
      HIP_CHECK(hipEventCreateWithFlags(&io_ev_out_, hipEventDisableTiming));
    }
    hipStream_t cs = (hipStream_t)caller_stream;
    HIP_CHECK(hipEventRecord(io_ev_in_, cs));  // the mask is ready once the caller's work so far is done
    HIP_CHECK(hipStreamWaitEvent(st_, io_ev_in_, 0));
    const uint8_t *m = (const uint8_t *)mask;
    if (dt == F32)
      impute_launch(grid, (float *)V, m, Q, P, K, mp, tab, flags, part, wide);
    else if (dt == BF16)
      impute_launch(grid, (bf16s *)V, m, Q, P, K, mp, tab, flags, part, wide);
    else
      impute_launch(grid, (double *)V, m, Q, P, K, mp, tab, flags, part, wide);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(io_ev_out_, st_));  // and the caller may change the mask after the reads
    HIP_CHECK(hipStreamWaitEvent(cs, io_ev_out_, 0));
    if (sumsq) {
      hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(1024), 0, st_, part, (int)npart, sumsq);
      HIP_CHECK(hipGetLastError());
    }
  }

  // ------------------------------------------------------------------ a Tucker session's slice sums
  // Routes (kernels_tucker_slices.hip.h), chosen by K as the imputation chooses: K <= 16 k_model_slices, Q in
  // registers; 16 < K <= MW_KMAX k_model_slices_wide, Q in LDS; above, k_model_slices again, in chunks of k.
  // The geometry — ntA row tiles, gy workgroups a tile — follows from the slab alone; the cap only cuts the
  // row tiles into launches of nt tiles whose partials (8 (nt B + gy 64 nt) bytes) fit, and k_slice_fold adds
  // every launch's partials onto asq / bsq in tile order, so the cap changes no bit.
  template <typename TV>
  void slice_sums_launch(const ModelPlan &mp, const double *Q, const double *P, int K, const TV *V, bool first,
                         double *asq, double *bsq, size_t cap, void *&work, size_t &work_bytes) {
    const int64_t A = mp.ga.count, B = mp.gb.count;
    const bool wide = K > 16 && K <= MW_KMAX;
    dim3 grid;
    const int64_t *tab = wide ? mv_tables(mp, &grid, 2 * ts_wgs_per_cu(K)) : mv_tables(mp, &grid);
    const int64_t *tar = tab + A, *tbr = tab + 2 * A + B;
    const int64_t ntA = grid.x, gy = grid.y;
    const int64_t one = B + gy * MV_TILE;  // doubles of partial sums a row tile
    const int64_t nt = std::max<int64_t>(1, std::min<int64_t>(ntA, (int64_t)(cap / sizeof(double)) / one));
    const int64_t rp_ld = nt * MV_TILE;
    const size_t need = sizeof(double) * (size_t)(nt * one);
    if (need > work_bytes) {  // (the caller's buffer, exactly what is needed: it is held to a cap)
      free(work);
      work = nullptr;
      work_bytes = 0;
      work = alloc(need);
      work_bytes = need;
    }
    double *rowpart = (double *)work, *colpart = rowpart + gy * rp_ld;
    route("model_slices:%s,K%d,%s,tiles%lld,gy%lld,launches%lld", tname<TV>(), K,
          wide ? "lds" : (K <= 16 ? "regs" : "chunks"), (long long)ntA, (long long)gy, (long long)((ntA + nt - 1) / nt));
    for (int64_t t0 = 0; t0 < ntA; t0 += nt) {
      const int64_t ntc = std::min(nt, ntA - t0), rows = std::min(A - t0 * MV_TILE, ntc * MV_TILE);
      const dim3 g((unsigned)ntc, (unsigned)gy);
      prof_begin(1, (double)rows * (double)B * sizeof(TV));
      if (wide)
        hipLaunchKernelGGL((k_model_slices_wide<TV>), g, dim3(256), ts_lds_bytes(K), st_, V, Q, P, K, mp, tar, tbr, t0,
                           rp_ld, rowpart, colpart);
      else
        hipLaunchKernelGGL((k_model_slices<TV>), g, dim3(256), 0, st_, V, Q, P, K, mp, tar, tbr, t0, rp_ld, rowpart,
                           colpart);
      prof_end();
      HIP_CHECK(hipGetLastError());
      hipLaunchKernelGGL(k_slice_fold, dim3(grid_for(rows + B, 256)), dim3(256), 0, st_, rowpart, gy, rp_ld, rows,
                         t0 * MV_TILE, first ? 1 : 0, colpart, ntc, B, B, (int64_t)0, t0 == 0 ? 1 : 0, asq, bsq);
      HIP_CHECK(hipGetLastError());
    }
  }
  void model_slice_sums(const ModelPlan &mp, const double *Q, const double *P, int K, const void *V, int dt,
                        bool first, double *asq, double *bsq, size_t work_cap_bytes, void *&work,
                        size_t &work_bytes) override {
    RoctxRange roctx_("model slice sums");
    HIP_CHECK(hipSetDevice(dev_));
    if (mp.ga.count <= 0 || mp.gb.count <= 0) return;
    if (K < 1) throw std::runtime_error("ppals: model_slice_sums needs K >= 1");
    if (dt == F32)
      slice_sums_launch(mp, Q, P, K, (const float *)V, first, asq, bsq, work_cap_bytes, work, work_bytes);
    else if (dt == F64)
      slice_sums_launch(mp, Q, P, K, (const double *)V, first, asq, bsq, work_cap_bytes, work, work_bytes);
    else
      throw std::runtime_error("ppals: model_slice_sums reads F32 or F64 storage");
  }

  // ------------------------------------------------------------------ the weighted step
  // flags of one side view of k_model_wls (`along_a`, `unit`, `vec` = the side's three bits): how it is
  // read (dv_side_along_a), whether offA(a) = a, and whether a lane's vw elements are one aligned vector
  static int wls_side_flags(const ModelGroup &ga, const ModelGroup &gb, const int64_t *sa, const int64_t *sb,
                            int64_t off, const void *p, int vw, bool vec_st, int along_a, int unit, int vec) {
    int first_a = 0, first_b = 0;  // (groups may hold modes of extent 1: their strides never count)
    while (first_a < ga.n && ga.len[first_a] <= 1) first_a++;
    while (first_b < gb.n && gb.len[first_b] <= 1) first_b++;
    const int64_t s_a = first_a < ga.n ? sa[first_a] : 0, s_b = first_b < gb.n ? sb[first_b] : 0;
    if (!dv_side_along_a(s_a, s_b)) return 0;
    int f = along_a;
    if (!ModelGroup::unit(ga.n, ga.len, sa)) return f;
    f |= unit;
    bool v = vec_st && off % vw == 0 && ((uintptr_t)p) % 16 == 0;
    for (int i = 0; i < gb.n; i++)
      if (gb.len[i] > 1 && sb[i] % vw != 0) v = false;
    return f | (v ? vec : 0);
  }
  // One launch of the tile loop of kernels_wls.hip.h: the weighted step (WL_WLS), the Huber step (WL_HUBER, `c`;
  // ws == nullptr: the family without a weights view) or a pass of the residual quantile's radix select
  // (WL_HIST: V is not touched, `ghist`). out (device, may be nullptr): the loss, and for WL_HUBER the clipped
  // count behind it.
  struct WlJob {
    int kind;
    const ModelSide *ws;
    const void *data, *weights;
    int vdt;
    void *V;
    int dt;
    double c;
    double *out;
    int pshift, shift;
    uint32_t prefix, mask;
    unsigned long long *ghist;
  };
  template <typename D, typename TS>
  void wl_launch(const WlJob &j, dim3 grid, size_t lds, const double *Q, const double *P, int K, const ModelPlan &mp,
                 const int64_t *tab, int flags, double *part) {
    const int64_t A = mp.ga.count, B = mp.gb.count;
    const int nt = j.ws ? 3 : 2;  // tables per group: the shard's, the data's, the weights'
    const int64_t *tav = tab, *tax = tab + A, *taw = tab + 2 * A, *tbv = tab + nt * A, *tbx = tbv + B, *tbw = tbx + B;
    D *V = (D *)j.V;
    const TS *X = (const TS *)j.data, *H = (const TS *)j.weights;
    const int64_t woff = j.ws ? j.ws->off : 0;
    if (j.kind == WL_WLS)
      hipLaunchKernelGGL((k_model_wls<D, TS>), grid, dim3(256), lds, st_, V, X, H, Q, P, K, mp, woff, tav, tax, taw, tbv,
                         tbx, tbw, flags, part);
    else if (j.kind == WL_HUBER && j.ws)
      hipLaunchKernelGGL((k_model_huber<D, TS>), grid, dim3(256), lds, st_, V, X, H, Q, P, K, mp, woff, tav, tax, taw,
                         tbv, tbx, tbw, flags, j.c, part);
    else if (j.kind == WL_HUBER)
      hipLaunchKernelGGL((k_model_huber_now<D, TS>), grid, dim3(256), lds, st_, V, X, Q, P, K, mp, tav, tax, tbv, tbx,
                         flags, j.c, part);
    else if constexpr (std::is_same<D, TS>::value) {
      if (j.ws)
        hipLaunchKernelGGL((k_model_absres_hist<TS, true>), grid, dim3(256), lds, st_, X, H, Q, P, K, mp, woff, tax, taw,
                           tbx, tbw, flags, j.pshift, j.prefix, j.shift, j.mask, j.ghist);
      else
        hipLaunchKernelGGL((k_model_absres_hist<TS, false>), grid, dim3(256), lds, st_, X, H, Q, P, K, mp, woff, tax, taw,
                           tbx, tbw, flags, j.pshift, j.prefix, j.shift, j.mask, j.ghist);
    }
  }
  void wl_run(const WlJob &j, const char *name, const ModelPlan &plan, const double *Q, const double *P, int K,
              void *caller_stream) {
    HIP_CHECK(hipSetDevice(dev_));
    const int64_t A = plan.ga.count, B = plan.gb.count;
    const int nout = j.kind == WL_HUBER ? 2 : 1;
    if (A <= 0 || B <= 0) {
      if (j.out) zero(j.out, sizeof(double) * nout);
      return;
    }
    const bool hist = j.kind == WL_HIST;
    if (K < 1 || K > WL_KMAX) throw std::runtime_error(std::string("ppals: ") + name + " needs 1 <= K <= 128");
    if ((!hist && j.dt != F32 && j.dt != F64) || (j.vdt != DV_F32 && j.vdt != DV_F64))
      throw std::runtime_error(std::string("ppals: ") + name + " stores F32 or F64 and reads F32 or F64 views");
    const ModelPlan mp = dv_model_swapped(plan);  // the kernel's "view" is the shard, its "shard" the data
    // (a histogram pass stores nothing: its lanes take 16-byte runs of the views whenever A allows whole runs)
    const int sdt = hist ? (j.vdt == DV_F32 ? F32 : F64) : j.dt;
    const int vw = sdt == F32 ? 4 : 2;
    const bool a_unit = hist || mp.ga.view_unit();
    bool vec_st = a_unit && A % vw == 0 && (hist || (mp.voff % vw == 0 && ((uintptr_t)j.V) % 16 == 0));
    for (int i = 0; i < mp.gb.n && !hist; i++)
      if (mp.gb.len[i] > 1 && mp.gb.vs[i] % vw != 0) vec_st = false;
    int flags = (a_unit ? WL_A_UNIT : 0) | (vec_st ? WL_VEC_ST : 0);
    flags |= wls_side_flags(mp.ga, mp.gb, mp.ga.rs, mp.gb.rs, mp.roff, j.data, vw, vec_st, WL_X_ALONG_A, WL_X_UNIT,
                            WL_X_VEC);
    if (j.ws)
      flags |= wls_side_flags(mp.ga, mp.gb, j.ws->ga.vs, j.ws->gb.vs, j.ws->off, j.weights, vw, vec_st, WL_H_ALONG_A,
                              WL_H_UNIT, WL_H_VEC);
    const bool one_b = j.ws && !(flags & WL_X_ALONG_A) != !(flags & WL_H_ALONG_A);
    const size_t lds = wl_lds_bytes(K, one_b ? (j.vdt == DV_F32 ? 4 : 8) : 0) +
                       (hist ? sizeof(uint32_t) * WL_HIST_BINS : 0);
    // the offset tables of both groups, built on the engine stream (nothing of the caller's is read), and
    // two rounds of the workgroups the LDS lets a CU hold, each walking its share of the b tiles
    const int64_t ntA = (A + MV_TILE - 1) / MV_TILE, ntB = (B + MV_TILE - 1) / MV_TILE;
    if (ntA > 0x7fffffff) throw std::runtime_error("ppals: model view too wide");
    const int nt = j.ws ? 3 : 2;
    int64_t *tab = (int64_t *)ensure(ws_mv_, ws_mv_sz_, sizeof(int64_t) * nt * (size_t)(A + B));
    hipLaunchKernelGGL(k_model_offsets, dim3(grid_for(A, 256)), dim3(256), 0, st_, mp.ga, tab, tab + A);
    if (j.ws) hipLaunchKernelGGL(k_model_offsets_side, dim3(grid_for(A, 256)), dim3(256), 0, st_, j.ws->ga, tab + 2 * A);
    hipLaunchKernelGGL(k_model_offsets, dim3(grid_for(B, 256)), dim3(256), 0, st_, mp.gb, tab + nt * A,
                       tab + nt * A + B);
    if (j.ws)
      hipLaunchKernelGGL(k_model_offsets_side, dim3(grid_for(B, 256)), dim3(256), 0, st_, j.ws->gb, tab + 3 * A + 2 * B);
    HIP_CHECK(hipGetLastError());
    const int64_t want = std::max<int64_t>(1, ((int64_t)ncu_ * 2 * wl_wgs_per_cu(lds) + ntA - 1) / ntA);
    const dim3 grid((unsigned)ntA, (unsigned)std::min<int64_t>(std::min<int64_t>(want, ntB), 65535));
    const int64_t npart = (int64_t)grid.x * grid.y;
    if (npart * nout > 0x7fffffff) throw std::runtime_error("ppals: model view too wide");
    double *part = hist ? nullptr : (double *)ensure(ws_part_, ws_part_sz_, sizeof(double) * npart * nout);
    const char *vn = j.vdt == DV_F32 ? "f32" : "f64";
    if (hist)
      route("model.absres_hist.%s%s K=%d flags=%d lds=%zu shift=%d", vn, j.ws ? "" : ".now", K, flags, lds, j.shift);
    else
      route("model.%s.%s.%s%s K=%d flags=%d lds=%zu", j.kind == WL_WLS ? "wls" : "huber", j.dt == F32 ? "f32" : "f64", vn,
            j.ws ? "" : ".now", K, flags, lds);
    if (!io_ev_in_) {
      HIP_CHECK(hipEventCreateWithFlags(&io_ev_in_, hipEventDisableTiming));
      HIP_CHECK(hipEventCreateWithFlags(&io_ev_out_, hipEventDisableTiming));
    }
    hipStream_t cs = (hipStream_t)caller_stream;
    HIP_CHECK(hipEventRecord(io_ev_in_, cs));  // the views are ready once the caller's work so far is done
    HIP_CHECK(hipStreamWaitEvent(st_, io_ev_in_, 0));
    if (sdt == F32 && j.vdt == DV_F32)
      wl_launch<float, float>(j, grid, lds, Q, P, K, mp, tab, flags, part);
    else if (sdt == F32)
      wl_launch<float, double>(j, grid, lds, Q, P, K, mp, tab, flags, part);
    else if (j.vdt == DV_F32)
      wl_launch<double, float>(j, grid, lds, Q, P, K, mp, tab, flags, part);
    else
      wl_launch<double, double>(j, grid, lds, Q, P, K, mp, tab, flags, part);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(io_ev_out_, st_));  // and the caller may change the views after the reads
    HIP_CHECK(hipStreamWaitEvent(cs, io_ev_out_, 0));
    for (int i = 0; j.out && i < nout; i++) {
      hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(1024), 0, st_, part + i * npart, (int)npart, j.out + i);
      HIP_CHECK(hipGetLastError());
    }
  }
  void model_wls(const ModelPlan &plan, const ModelSide &ws, const double *Q, const double *P, int K,
                 const void *data, const void *weights, int vdt, void *V, int dt, double *sumsq,
                 void *caller_stream) override {
    wl_run(WlJob{WL_WLS, &ws, data, weights, vdt, V, dt, 0.0, sumsq, 0, 0, 0, 0, nullptr}, "model_wls", plan, Q, P, K,
           caller_stream);
  }
  void model_huber(const ModelPlan &plan, const ModelSide *ws, const double *Q, const double *P, int K,
                   const void *data, const void *weights, int vdt, void *V, int dt, double c, double *loss_clipped,
                   void *caller_stream) override {
    wl_run(WlJob{WL_HUBER, ws, data, ws ? weights : nullptr, vdt, V, dt, c, loss_clipped, 0, 0, 0, 0, nullptr},
           "model_huber", plan, Q, P, K, caller_stream);
  }
  void model_absres_hist(const ModelPlan &plan, const ModelSide *ws, const double *Q, const double *P, int K,
                         const void *data, const void *weights, int vdt, int pshift, uint32_t prefix, int shift,
                         uint32_t mask, uint64_t *hist /* host, WL_HIST_BINS */, void *caller_stream) override {
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "");
    HIP_CHECK(hipSetDevice(dev_));
    unsigned long long *gh =
        (unsigned long long *)ensure(ws_hist_, ws_hist_sz_, sizeof(unsigned long long) * WL_HIST_BINS);
    zero(gh, sizeof(unsigned long long) * WL_HIST_BINS);
    wl_run(WlJob{WL_HIST, ws, data, ws ? weights : nullptr, vdt, nullptr, 0, 0.0, nullptr, pshift, shift, prefix, mask,
                 gh},
           "model_absres_hist", plan, Q, P, K, caller_stream);
    d2h(hist, gh, sizeof(unsigned long long) * WL_HIST_BINS);
  }

  // ------------------------------------------------------------------ PARAFAC2 (kernels_parafac2.hip.h)
  void parafac2_check() override {}
  void parafac2_init(double *P, int64_t I, int R, int64_t K) override {
    HIP_CHECK(hipSetDevice(dev_));
    hipLaunchKernelGGL(k_p2_init, dim3(grid_for(I * R * K, 256)), dim3(256), 0, st_, P, I, R, K);
    HIP_CHECK(hipGetLastError());
  }
  template <typename TX, int NT>
  void p2_launch(const Parafac2Step &s, int ti, int tj, double *part) {
    const TX *X = (const TX *)s.X;
    hipLaunchKernelGGL((k_p2_project<TX, NT>), dim3((unsigned)(ti * s.K)), dim3(256), p2_project_lds(s.R), st_, X, s.s1,
                       s.s2, s.I, s.J, s.R, s.A, s.B, s.C, s.K, ti, s.Q);
    const size_t lds_polar = sizeof(double) * (2 * (size_t)s.R * (s.R + 1) + 64 + 18) + sizeof(int) * 64;
    hipLaunchKernelGGL(k_p2_polar, dim3((unsigned)s.K), dim3(1024), lds_polar, st_, s.Q, s.I, s.R, s.min_ratio, s.T,
                       s.status);
    hipLaunchKernelGGL(k_p2_apply, dim3((unsigned)(ti * s.K)), dim3(256),
                       sizeof(double) * ((size_t)s.R * s.R + 64 * (size_t)s.R), st_, s.Q, s.T, s.status, s.I, s.R, ti,
                       s.P);
    if (s.dt == F32)
      hipLaunchKernelGGL((k_p2_compress<TX, float, NT>), dim3((unsigned)(tj * s.K)), dim3(256), p2_compress_lds(s.R),
                         st_, X, s.s1, s.s2, s.I, s.J, s.R, s.P, tj, (float *)s.Y, part);
    else
      hipLaunchKernelGGL((k_p2_compress<TX, double, NT>), dim3((unsigned)(tj * s.K)), dim3(256), p2_compress_lds(s.R),
                         st_, X, s.s1, s.s2, s.I, s.J, s.R, s.P, tj, (double *)s.Y, part);
  }
  // seven launches whatever the extents: project, polar, apply, compress, the two sums and the failed count
  // (the last three only when `out` is asked for)
  void parafac2_step(const Parafac2Step &s, void *caller_stream) override {
    HIP_CHECK(hipSetDevice(dev_));
    if (s.R < 2 || s.R > 64 || s.I < s.R || s.J < s.R || s.K < 1)
      throw std::runtime_error("ppals: parafac2_step needs 2 <= R <= min(64, I, J) and K >= 1");
    if ((s.dt != F32 && s.dt != F64) || (s.vdt != DV_F32 && s.vdt != DV_F64))
      throw std::runtime_error("ppals: parafac2_step stores F32 or F64 and reads an F32 or F64 view");
    const int64_t ti = (s.I + P2_TILE - 1) / P2_TILE, tj = (s.J + P2_TILE - 1) / P2_TILE;
    if (ti * s.K > 0x7fffffff || tj * s.K > 0x3fffffff) throw std::runtime_error("ppals: parafac2_step: too many tiles");
    const int64_t npart = tj * s.K;
    double *part = (double *)ensure(ws_part_, ws_part_sz_, sizeof(double) * 2 * npart);
    const int nt = (s.R + 15) / 16;
    route("parafac2.step.%s.%s R=%d nt=%d tiles=%dx%d lds=%zu,%zu", s.dt == F32 ? "f32" : "f64",
          s.vdt == DV_F32 ? "f32" : "f64", s.R, nt, (int)ti, (int)tj, p2_project_lds(s.R), p2_compress_lds(s.R));
    join_stream(caller_stream);  // the view is ready once the caller's work so far is done
    dispatch<1, 2, 3, 4>(nt, [&](auto NT) {
      if (s.vdt == DV_F32)
        p2_launch<float, NT()>(s, (int)ti, (int)tj, part);
      else
        p2_launch<double, NT()>(s, (int)ti, (int)tj, part);
    });
    HIP_CHECK(hipGetLastError());
    release_stream(caller_stream);  // and the caller may change the view after the reads
    if (s.out) {
      hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(1024), 0, st_, part, (int)npart, s.out);
      hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(1024), 0, st_, part + npart, (int)npart, s.out + 1);
      hipLaunchKernelGGL(k_p2_failed, dim3(1), dim3(1024), 0, st_, s.status, s.K, s.out + 2);
      HIP_CHECK(hipGetLastError());
    }
  }

  // the ragged step: the same seven launches, the first pass and the apply over the row tiles of all slices
  void parafac2_init_ragged(const Parafac2Ragged &s) override {
    HIP_CHECK(hipSetDevice(dev_));
    if (s.tiles < 1 || s.tiles > 0x7fffffff) throw std::runtime_error("ppals: parafac2_init_ragged: too many tiles");
    hipLaunchKernelGGL(k_p2_init_ragged, dim3((unsigned)s.tiles), dim3(256), 0, st_, s.P, s.rows, s.roff, s.tile0,
                       s.tile_slice, s.R);
    HIP_CHECK(hipGetLastError());
  }
  template <typename TX, int NT>
  void p2_launch_ragged(const Parafac2Ragged &s, int tj, double *part) {
    const TX *X = (const TX *)s.X;
    hipLaunchKernelGGL((k_p2_project_ragged<TX, NT>), dim3((unsigned)s.tiles), dim3(256), p2_project_lds(s.R), st_, X,
                       s.rows, s.roff, s.tile0, s.tile_slice, s.xoff, s.xcs, s.J, s.R, s.A, s.B, s.C, s.K, s.Q);
    const size_t lds_polar = sizeof(double) * (2 * (size_t)s.R * (s.R + 1) + 64 + 18) + sizeof(int) * 64;
    hipLaunchKernelGGL(k_p2_polar_ragged, dim3((unsigned)s.K), dim3(1024), lds_polar, st_, s.Q, s.rows, s.roff, s.R,
                       s.min_ratio, s.T, s.status);
    hipLaunchKernelGGL(k_p2_apply_ragged, dim3((unsigned)s.tiles), dim3(256),
                       sizeof(double) * ((size_t)s.R * s.R + 64 * (size_t)s.R), st_, s.Q, s.T, s.status, s.rows, s.roff,
                       s.tile0, s.tile_slice, s.R, s.P);
    if (s.dt == F32)
      hipLaunchKernelGGL((k_p2_compress_ragged<TX, float, NT>), dim3((unsigned)(tj * s.K)), dim3(256),
                         p2_compress_lds(s.R), st_, X, s.rows, s.roff, s.xoff, s.xcs, s.J, s.R, s.P, tj, (float *)s.Y,
                         part);
    else
      hipLaunchKernelGGL((k_p2_compress_ragged<TX, double, NT>), dim3((unsigned)(tj * s.K)), dim3(256),
                         p2_compress_lds(s.R), st_, X, s.rows, s.roff, s.xoff, s.xcs, s.J, s.R, s.P, tj, (double *)s.Y,
                         part);
  }
  void parafac2_step_ragged(const Parafac2Ragged &s, void *caller_stream) override {
    HIP_CHECK(hipSetDevice(dev_));
    if (s.R < 2 || s.R > 64 || s.J < s.R || s.K < 1 || s.tiles < s.K)
      throw std::runtime_error("ppals: parafac2_step_ragged needs 2 <= R <= min(64, J), K >= 1 and rows[k] >= 1");
    if ((s.dt != F32 && s.dt != F64) || (s.vdt != DV_F32 && s.vdt != DV_F64))
      throw std::runtime_error("ppals: parafac2_step_ragged stores F32 or F64 and reads an F32 or F64 view");
    const int64_t tj = (s.J + P2_TILE - 1) / P2_TILE;
    if (s.tiles > 0x7fffffff || tj * s.K > 0x3fffffff)
      throw std::runtime_error("ppals: parafac2_step_ragged: too many tiles");
    const int64_t npart = tj * s.K;
    double *part = (double *)ensure(ws_part_, ws_part_sz_, sizeof(double) * 2 * npart);
    const int nt = (s.R + 15) / 16;
    route("parafac2.step_ragged.%s.%s R=%d nt=%d tiles=%d,%d lds=%zu,%zu", s.dt == F32 ? "f32" : "f64",
          s.vdt == DV_F32 ? "f32" : "f64", s.R, nt, (int)s.tiles, (int)(tj * s.K), p2_project_lds(s.R),
          p2_compress_lds(s.R));
    join_stream(caller_stream);
    dispatch<1, 2, 3, 4>(nt, [&](auto NT) {
      if (s.vdt == DV_F32)
        p2_launch_ragged<float, NT()>(s, (int)tj, part);
      else
        p2_launch_ragged<double, NT()>(s, (int)tj, part);
    });
    HIP_CHECK(hipGetLastError());
    release_stream(caller_stream);
    if (s.out) {
      hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(1024), 0, st_, part, (int)npart, s.out);
      hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(1024), 0, st_, part + npart, (int)npart, s.out + 1);
      hipLaunchKernelGGL(k_p2_failed, dim3(1), dim3(1024), 0, st_, s.status, s.K, s.out + 2);
      HIP_CHECK(hipGetLastError());
    }
  }

  void *try_alloc(size_t bytes) override {
    void *p = nullptr;
    hipSetDevice(dev_);
    if (hipMalloc(&p, bytes ? bytes : 8) != hipSuccess) {
      (void)hipGetLastError();
      return nullptr;
    }
    return p;
  }
  void scan_store_mode(int mode) override { scan_nt_mode_ = mode; }
  void scan_packed_source(const PackedSrc *pk) override {
    scan_pk_ = pk ? *pk : PackedSrc();
  }
  PackedSrc scan_pk_;
  int64_t scan_pk_launches_ = 0;
  // PPALS_PK2_DECODE=branch (measurements only): the 26-bit scan adds its escape bits under a branch
  bool scan_pk2_branch_ = [] {
    const char *e = getenv("PPALS_PK2_DECODE");
    return e && std::string(e) == "branch";
  }();
  int64_t scan_packed_launches() override { return scan_pk_launches_; }
  int *pack_stats_ = nullptr;  // device words of the pre-pass: largest spread, escape blocks
  PackSurvey pack_survey(const void *src, int dt, int64_t L, int64_t J, int64_t T, void *bases) override {
    // what the packed scan route itself needs (scan_t): fp32, whole lanes of 4 rows, 16-byte aligned
    // rows, 32-bit tile ids and block counts
    const int64_t n_mtiles = (L + 255) / 256, nkb = (J + 15) / 16;
    PackSurvey sv;
    if (dt != F32 || L < 4 || L % 4 || J < 1 || T < 1 || (((uintptr_t)src) & 15) || n_mtiles * T > 0x7fffffff ||
        n_mtiles * T * nkb > 0x7fffffff)
      return sv;
    if (!pack_stats_) pack_stats_ = (int *)alloc(2 * sizeof(int));
    const unsigned nblocks = (unsigned)(n_mtiles * T * nkb);
    HIP_CHECK(hipMemsetAsync(pack_stats_, 0, 2 * sizeof(int), st_));
    hipLaunchKernelGGL(k_pk_prepass, dim3(nblocks), dim3(256), 0, st_, (const float *)src, L, J, (int)n_mtiles,
                       (int)nkb, (pk_u32 *)bases, pack_stats_);
    HIP_CHECK(hipGetLastError());
    int stats[2] = {0, 0};
    HIP_CHECK(hipMemcpyAsync(stats, pack_stats_, sizeof stats, hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipStreamSynchronize(st_));
    sv.spread = stats[0];
    sv.escapes = stats[1];
    return sv;
  }
  void pack_write(const void *src, int64_t L, int64_t J, int64_t T, int format, void *bases, void *data,
                  void *esc) override {
    const int64_t n_mtiles = (L + 255) / 256, nkb = (J + 15) / 16;
    const unsigned nblocks = (unsigned)(n_mtiles * T * nkb);
    hipLaunchKernelGGL(k_pk_side_words, dim3(1), dim3(1024), 0, st_, (pk_u32 *)bases, (int64_t)nblocks, format);
    HIP_CHECK(hipGetLastError());
    dispatch<PACK_FMT26, PACK_FMT28>(format, [&](auto fmt) {
      hipLaunchKernelGGL((k_pk_pack<fmt>), dim3(nblocks), dim3(256), 0, st_, (const float *)src, L, J, (int)n_mtiles,
                         (int)nkb, pack_tile_bytes(fmt, J), (const pk_u32 *)bases, (char *)data, (char *)esc);
    });
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(st_));
  }
  void scan_profile_slot(int slot) override { scan_slot_ = slot == 1 ? 1 : 0; }
  int scan_nt_mode_ = -1;
  size_t mem_available() override {
    size_t fr = 0, tot = 0;
    hipSetDevice(dev_);
    if (hipMemGetInfo(&fr, &tot) != hipSuccess) {
      (void)hipGetLastError();
      return (size_t)-1;
    }
    return fr;
  }
  void unpack_shards(const void *stage, int dt, int64_t s0, int64_t rest, int64_t blk, int P,
                     int64_t chunk_bytes, void *full) override {
    const int g = grid_for(s0 * rest, 256, 16384);
    if (dt == F32)
      hipLaunchKernelGGL(k_unpack_shards<float>, dim3(g), dim3(256), 0, st_, (const char *)stage,
                         s0, rest, blk, P, chunk_bytes, (float *)full);
    else if (dt == BF16)
      hipLaunchKernelGGL(k_unpack_shards<bf16s>, dim3(g), dim3(256), 0, st_, (const char *)stage,
                         s0, rest, blk, P, chunk_bytes, (bf16s *)full);
    else
      hipLaunchKernelGGL(k_unpack_shards<double>, dim3(g), dim3(256), 0, st_, (const char *)stage,
                         s0, rest, blk, P, chunk_bytes, (double *)full);
    HIP_CHECK(hipGetLastError());
  }
  void transpose2d(const void *src, int dt, int64_t rows, int64_t cols, void *dst) override {
    transpose_batched(src, dt, rows, cols, 1, dst);
  }
  void transpose_batched(const void *src, int dt, int64_t rows, int64_t cols, int64_t batch,
                         void *dst) override {
    const int64_t nb = ((rows + 63) / 64) * ((cols + 63) / 64);
    if (nb > 0x7fffffff) throw std::runtime_error("ppals: transpose grid too large");
    const size_t step = (size_t)rows * cols * dtype_size(dt);
    for (int64_t b0 = 0; b0 < batch; b0 += 65535) {  // grid.y limit
      const unsigned nby = (unsigned)std::min<int64_t>(65535, batch - b0);
      const char *s = (const char *)src + b0 * step;
      char *d = (char *)dst + b0 * step;
      if (dt == F32)
        hipLaunchKernelGGL(k_transpose<float>, dim3((unsigned)nb, nby), dim3(256), 0, st_,
                           (const float *)s, rows, cols, (float *)d);
      else if (dt == BF16)
        hipLaunchKernelGGL(k_transpose<bf16s>, dim3((unsigned)nb, nby), dim3(256), 0, st_,
                           (const bf16s *)s, rows, cols, (bf16s *)d);
      else
        hipLaunchKernelGGL(k_transpose<double>, dim3((unsigned)nb, nby), dim3(256), 0, st_,
                           (const double *)s, rows, cols, (double *)d);
    }
    HIP_CHECK(hipGetLastError());
  }

  // ------------------------------------------------------------------ KRP
  static KrpArgs krp_args(const FactorRef *f, int nf, int64_t *J) {
    KrpArgs a;
    int64_t j = 1;
    if (nf > MAX_ORDER) throw std::runtime_error("ppals: too many Khatri-Rao factors");
    for (int i = 0; i < nf; i++) {
      a.ptr[i] = f[i].ptr;
      a.rows[i] = f[i].rows;
      a.ld[i] = f[i].ld;
      j *= f[i].rows;
    }
    a.nf = nf;
    *J = j;
    return a;
  }
  void krp(double *out, const FactorRef *f, int nf, int col0, int ncols) override {
    int64_t J;
    KrpArgs a = krp_args(f, nf, &J);
    hipLaunchKernelGGL(k_krp, dim3(grid_for(J * ncols, 256)), dim3(256), 0, st_, out, a, J, col0,
                       ncols);
    HIP_CHECK(hipGetLastError());
  }

  // ------------------------------------------------------------------ scans
  template <typename TV>
  void scan_t(const TV *V, int64_t L, int64_t J, int64_t T, const FactorRef *f, int nf, int R,
              double *out, int64_t out_tstride, int64_t out_rstride, int out32, RowPad pad) {
    constexpr int VEC = ScanTraits<TV>::VEC;
    int64_t Jc;
    KrpArgs a = krp_args(f, nf, &Jc);
    if (Jc != J) throw std::runtime_error("ppals: scan_contract factor extents do not match J");
    if (pad.ld && (L % pad.ld || pad.ld % VEC || pad.valid > pad.ld || pad.valid <= 0 || L == 1))
      throw std::runtime_error("ppals: scan_contract padded rows inconsistent");
    const bool aligned_base = (((uintptr_t)V) & 15) == 0;
    // 65..128 columns of an fp32 tensor in ONE pass (k_scan_wide: MFMA-bound regime, the tensor tile
    // staged through LDS); whatever is left after whole passes of 128 goes the narrow way
    // (buffer loads: a k-block of 16 columns and the packed operand must be addressable with 32-bit offsets)
    const bool wide_ok = sizeof(TV) == 4 && wide_enabled_ && L > 1 && aligned_base && (L % 4 == 0) &&
                         L >= 4 && (double)L * J * T >= 1.0e6 && 16.0 * (double)L * 4.0 < 2.0e9 &&
                         ((double)J / 16.0 + 1.0) * 8.0 * 1024.0 < 2.0e9;
    int col_step = 64;
    for (int col0 = 0; col0 < R; col0 += col_step) {
      if (wide_ok && R - col0 > 64) {
        col_step = std::min(128, R - col0);
        if constexpr (sizeof(TV) == 4)
          scan_wide((const float *)V, L, J, T, a, col0, col_step, out, out_tstride, out_rstride, out32, pad);
        continue;
      }
      col_step = 64;
      const int ncols = std::min(64, R - col0);
      // n-tiles of 16 result columns: 3 for 33..48 columns (ranks such as 40, or the second
      // launch of R = 100 = 64 + 36) instead of padding them to 64 — these scans are MFMA-bound
      const int NT = ncols <= 16 ? 1 : (ncols <= 32 ? 2 : (ncols <= 48 ? 3 : 4));
      const int64_t nblk64 = (J + 4 * VEC - 1) / (4 * VEC);
      if (nblk64 > 0x7fffffff) throw std::runtime_error("ppals: contraction extent too large");
      const int nblk = (int)nblk64;
      const size_t pack_bytes = (size_t)nblk * NT * 4 * 16 * VEC * sizeof(TV);
      TV *P = (TV *)ensure(ws_pack_, ws_pack_sz_, pack_bytes);
      const bool prefix = (L == 1);
      hipLaunchKernelGGL(k_krp_pack<TV>, dim3(grid_for((int64_t)nblk * NT * 64 * VEC, 256)),
                         dim3(256), 0, st_, P, nblk, NT, prefix ? 1 : 0, a, J, col0, ncols);
      HIP_CHECK(hipGetLastError());
      double *o = out32 ? (double *)((float *)out + (int64_t)col0 * out_rstride)
                        : out + (int64_t)col0 * out_rstride;
      // algorithmic bytes of the launch: one read of the scanned tensor + the result it must write
      const double bytes = (double)L * (double)J * (double)T * sizeof(TV) +
                           (double)L * (double)T * ncols * (out32 ? 4.0 : 8.0);
      if (prefix) {
        // out[t + rs*n] = sum_j V[j + J*t] * B[j,n]      (M = J rows reduced, K = T columns)
        const int64_t M = J, K = T;
        const bool al = aligned_base && (M % VEC == 0);
        const int64_t ncolgrp = (K + 63) / 64;
        int want = 1;
        const int target = ncu_ * 4;
        if (ncolgrp < target) want = (int)std::min<int64_t>((target + ncolgrp - 1) / ncolgrp,
                                                            std::max(1, nblk / 64));
        const KSplit ks = k_split(nblk, want);
        const int nsplit = ks.nsplit, per = (int)ks.per;
        // (the slab of a k-split prefix scan is [split][ncols][K], its rows contiguous, where the
        // result's rows are out_tstride apart: not the suffix form of pass_dst)
        double *dst = o;
        int dst32 = out32;
        int64_t dst_ks = out_tstride, dst_ns = out_rstride, dst_ss = 0;
        if (nsplit > 1) {
          dst32 = 0;
          dst = (double *)ensure(ws_slab_, ws_slab_sz_, sizeof(double) * nsplit * ncols * K);
          dst_ks = 1;
          dst_ns = K;
          dst_ss = (int64_t)ncols * K;
        }
        if (al && M >= VEC)
          route("scan.%s.prefix.fast nt=%d nsplit=%d out32=%d", tname<TV>(), NT, nsplit, out32);
        else
          route("scan.%s.prefix.generic al=%d nt=%d nsplit=%d out32=%d", tname<TV>(), al ? 1 : 0, NT, nsplit, out32);
        dim3 grid((unsigned)ncolgrp, (unsigned)nsplit);
        dim3 grid_il((unsigned)((K + 15) / 16), (unsigned)nsplit);  // interleaved-waves variant
        prof_begin(scan_slot_, bytes);
        dispatch<1, 2, 3, 4>(NT, [&](auto nt) {
          if (al && M >= VEC)
            hipLaunchKernelGGL((k_scan_prefix_fast<TV, nt, 12>), grid_il, dim3(256), 0, st_, V, M, K, P, per,
                               nblk, dst, dst_ks, dst_ns, dst_ss, ncols, dst32);
          else
            dispatch<true, false>(al, [&](auto alv) {
              hipLaunchKernelGGL((k_scan_prefix<TV, nt, alv, 4>), grid, dim3(256), 0, st_, V, M, K, P, per,
                                 nblk, dst, dst_ks, dst_ns, dst_ss, ncols, dst32);
            });
        });
        prof_end();
        HIP_CHECK(hipGetLastError());
        slab_combine(nsplit, dst, dst_ss, K, ncols, o, out_tstride, out_rstride, out32);
      } else {
        // out[l + L*t + rs*n] = sum_j V[l + L*(j + J*t)] * B[j,n]   (M = L rows kept, K = J)
        const int64_t M = L, K = J;
        const bool al = aligned_base && (M % VEC == 0);
        const int64_t n_mtiles64 = (M + 64 * VEC - 1) / (64 * VEC);
        const int n_mtiles = (int)n_mtiles64;
        int want = 1;
        const int target = ncu_ * 8;
        if (T == 1 && n_mtiles < target)
          want = (int)std::min<int64_t>((target + n_mtiles - 1) / n_mtiles,
                                        std::max(1, nblk / 32));
        // a batched scan of a small tensor (the second-level mode products of a Tucker sweep:
        // 400 x 400 x 20 -> 2 row tiles x 20 batches = 40 workgroups, 29 us for 25.6 MB): K-split
        // down to 4 column blocks per workgroup until there are two workgroups per CU
        else if (T > 1 && n_mtiles64 * T < ncu_ && (double)M * T * ncols * nblk / 4 * 8.0 < 64e6)
          want = (int)std::min<int64_t>(((int64_t)ncu_ * 2 + n_mtiles64 * T - 1) / (n_mtiles64 * T),
                                        std::max(1, nblk / 4));
        const KSplit ks = k_split(nblk, want);
        const int nsplit = ks.nsplit, per = (int)ks.per;
        const PassDst d = pass_dst(nsplit, M, T, ncols, o, out32, out_rstride, out_tstride, pad);
        const int64_t nblocks = (int64_t)n_mtiles * nsplit * T;
        if (nblocks > 0x7fffffff) throw std::runtime_error("ppals: scan grid too large");
        dim3 grid((unsigned)nblocks);
        // persistent launch: ncu*40 workgroups (measured best of 3..40 per CU), each walks over its tiles
        // (fewer tiles than that: every workgroup would take exactly ONE tile and the launch loses what the
        // persistent form is for — the P = 8 shard of cfg2, 3906 tiles: 6 workgroups per CU walking 2.5
        // tiles each scan it in 156.3 us instead of 159.6-161.0, profiles/r05m_persist_mult_shard.txt)
        const int64_t pgrid = nblocks < (int64_t)ncu_ * persist_mult_ ? (int64_t)ncu_ * std::min(persist_mult_, 6)
                                                                       : (int64_t)ncu_ * persist_mult_;
        dim3 grid_p((unsigned)std::min<int64_t>(nblocks, pgrid));
        bool nts = nt_store(nsplit, (double)M * T * ncols * (d.out32 ? 4.0 : 8.0));
        // (Measured and rejected, tools/runs/r03_u.sh: second-level sums in fp32 for short
        // reductions — 16 NT registers fewer, the two-tile global-load kernel 174 -> 130 registers and
        // 2 -> 3 waves per SIMD, the one-tile buffer kernel 3 -> 4 waves: cfg4 36.0 / 36.7 -> 33.0 /
        // 33.6 sweeps/s, cfg2 no gain. More waves in flight make the mixed read/write stream worse.
        // Fewer do not help either: 64 KB of dynamic LDS per workgroup (2 instead of 3 workgroups per
        // CU) x 6..40 workgroups per CU in the persistent grid: profiles/r03v_occupancy_sweep.txt.)
        // buffer-load variant: needs 32-bit byte offsets inside one 16-column block
        const bool buf_ok = (16.0 * (double)M * sizeof(TV) < 2.0e9) && (pack_bytes < 2000000000ull);
        // Which KERNEL runs must not depend on the store kind: the engine's placement exploration tries
        // both kinds and keeps what the stopwatch prefers, and the tail-mode kernel (which has no
        // non-temporal instantiation) sums k in another order than the others — results would then vary
        // from run to run with timing noise. So the tail mode is decided first, and where it applies
        // the stores are ordinary whatever was asked for.
        const bool takes_buf = al && M >= VEC && buf_ok && (NT == 1 || sizeof(TV) == 8) &&
                               !(sizeof(TV) == 8 && nsplit > 1);
        const bool takes_tail = !takes_buf && al && M >= VEC && T == 1 && nsplit == 1 && NT <= 2 &&
                                d.row_ld == 0 && scan_tail_split<TV>(NT, n_mtiles) >= 0;
        if (takes_tail) nts = false;
        // the packed twin of this very scan (Ops::scan_packed_source): the one-n-tile fp32 buffer route,
        // unpadded and without k-split; the same result bits from 3.5 or 3.25 instead of 4 bytes per element
        bool takes_pk = false;
        if constexpr (sizeof(TV) == 4)
          takes_pk = takes_buf && NT == 1 && nsplit == 1 && d.row_ld == 0 && scan_pk_.data && scan_pk_.L == L &&
                     scan_pk_.J == J && scan_pk_.T == T;
        const bool pk26 = takes_pk && scan_pk_.format == PACK_FMT26;
        // (the profile counts the bytes the launch addresses: the packed source — blocks, side words and
        // the escape planes of a 26-bit twin — + the result)
        prof_begin(scan_slot_, takes_pk ? (double)pack_data_bytes(scan_pk_.format, L, J, T) +
                                              (double)pack_base_bytes(L, J, T) +
                                              (pk26 ? (double)scan_pk_.escapes * PACK26_ESC_BYTES : 0.0) +
                                              (double)L * (double)T * ncols * (out32 ? 4.0 : 8.0)
                                        : bytes);
        // (measured: with NT >= 2 the fp32 build of the buffer variant drops to 2 waves/SIMD and
        // loses to the global-load kernel, so it is used for one n-tile / fp64 storage only)
        // (and: K-split scans of an fp64 tensor — few, long work items of half-size blocks — run
        // at 0.80 of peak on the global-load kernel against 0.70 here: tools/r02_f64.sh)
        // (A two-tile launch of 2-3 workgroups per CU — the first mode product of a Tucker sweep at
        // cfg5, 625 tiles, 73 us — is a round and a quarter at 2 waves per SIMD; handing it to the
        // register-lean persistent form with 3 waves, k_scan_suffix_lean<2,4,0,3>, was measured:
        // 40 HOOI sweeps 0.0446 / 0.0443 s against 0.0442 / 0.0441 s. Not kept.)
        if (takes_tail)
          route("scan.%s.suffix.tail nt=%d from=%d", tname<TV>(), NT, scan_tail_split<TV>(NT, n_mtiles));
        else if (takes_pk)
          route("scan.%s.suffix.%s nt=1 nsplit=1 nts=%d pad=0 out32=%d", tname<TV>(), pk26 ? "pk2" : "pk", nts ? 1 : 0,
                out32);
        else if (takes_buf || (al && M >= VEC))
          route("scan.%s.suffix.%s nt=%d nsplit=%d nts=%d pad=%d out32=%d", tname<TV>(), takes_buf ? "buf" : "fast",
                NT, nsplit, nts ? 1 : 0, pad.ld ? 1 : 0, out32);
        else
          route("scan.%s.suffix.generic al=%d nt=%d nsplit=%d pad=%d out32=%d", tname<TV>(), al ? 1 : 0, NT, nsplit,
                pad.ld ? 1 : 0, out32);
        if (takes_tail) {
          // a round and a bit of resident workgroups (cfg5's 625 tiles on 512 slots: 0.49 of the HBM
          // peak): the tiles of the last, partial round as four quarter-length work items each
          // (kernels_scan.hip.h, TAIL MODE)
          const int tail_from = scan_tail_split<TV>(NT, n_mtiles);
          const int64_t strips = ((M + 16 * VEC - 1) / (16 * VEC)) - (int64_t)tail_from * 4;
          dim3 grid_t((unsigned)(tail_from + strips));
          const size_t lds_t = sizeof(double) * 3 * (size_t)(VEC * NT * 4) * 64;
          dispatch<1, 2>(NT, [&](auto nt) {
            hipLaunchKernelGGL((k_scan_suffix_fast<TV, nt, 9>), grid_t, dim3(256), lds_t, st_, V, M, K, M * K, P,
                               n_mtiles, nsplit, per, nblk, d.p, d.nstride, d.split_stride, d.batch_stride, ncols,
                               d.out32, (int64_t)0, (int64_t)0, tail_from);
          });
        } else if (takes_pk) {
          scan_pk_launches_++;
          if (pk26)
            // (bit 3, the branched escape decode, is the other side of the A/B in profiles/pack26_bench.md)
            dispatch<5, 1, 13, 9>((nts ? 5 : 1) | (scan_pk2_branch_ ? 8 : 0), [&](auto opt) {
              hipLaunchKernelGGL((k_scan_suffix_pk2<opt>), grid_p, dim3(256), 0, st_, (const char *)scan_pk_.data,
                                 (const unsigned int *)scan_pk_.bases, (const char *)scan_pk_.esc,
                                 pack_tile_bytes(PACK_FMT26, J), M, (const float *)P, n_mtiles, nblk, d.p, d.nstride,
                                 d.batch_stride, ncols, d.out32, nblocks);
            });
          else
            dispatch<5, 1>(nts ? 5 : 1, [&](auto opt) {
              hipLaunchKernelGGL((k_scan_suffix_pk<opt>), grid_p, dim3(256), 0, st_, (const char *)scan_pk_.data,
                                 (const unsigned int *)scan_pk_.bases, pack_tile_bytes(PACK_FMT28, J), M,
                                 (const float *)P, n_mtiles, nblk, d.p, d.nstride, d.batch_stride, ncols, d.out32,
                                 nblocks);
            });
        } else {
          dispatch<1, 2, 3, 4>(NT, [&](auto nt) {
            if (takes_buf)
              dispatch<5, 1>(nts ? 5 : 1, [&](auto opt) {
                hipLaunchKernelGGL((k_scan_suffix_buf<TV, nt, opt>), grid_p, dim3(256), 0, st_, V, M, K, M * K, P,
                                   n_mtiles, nsplit, per, nblk, d.p, d.nstride, d.split_stride, d.batch_stride,
                                   ncols, d.out32, nblocks, d.row_ld, d.row_valid);
              });
            else if (al && M >= VEC)
              dispatch<5, 1>(nts ? 5 : 1, [&](auto opt) {
                hipLaunchKernelGGL((k_scan_suffix_fast<TV, nt, opt>), grid, dim3(256), 0, st_, V, M, K, M * K, P,
                                   n_mtiles, nsplit, per, nblk, d.p, d.nstride, d.split_stride, d.batch_stride,
                                   ncols, d.out32, d.row_ld, d.row_valid);
              });
            else
              dispatch<true, false>(al, [&](auto alv) {
                hipLaunchKernelGGL((k_scan_suffix<TV, nt, alv>), grid, dim3(256), 0, st_, V, M, K, M * K, P,
                                   n_mtiles, nsplit, per, nblk, d.p, d.nstride, d.split_stride, d.batch_stride,
                                   ncols, d.out32, d.row_ld, d.row_valid);
              });
          });
        }
        prof_end();
        HIP_CHECK(hipGetLastError());
        slab_combine(nsplit, d.p, d.split_stride, M, ncols, o, 1, out_rstride, out32, pad, T, d.batch_stride,
                     out_tstride);
      }
    }
  }
  // One pass of the wide kernel over columns [col0, col0 + ncols), 64 < ncols <= 128 (fp32 tensor,
  // suffix / batched form): pack, launch, combine the k-splits.
  void scan_wide(const float *V, int64_t L, int64_t J, int64_t T, const KrpArgs &a, int col0, int ncols,
                 double *out, int64_t out_tstride, int64_t out_rstride, int out32, RowPad pad) {
    const int NT = (ncols + 15) / 16;
    const int64_t nblk64 = (J + 15) / 16;
    if (nblk64 > 0x7fffffff) throw std::runtime_error("ppals: contraction extent too large");
    const int nblk = (int)nblk64;
    const size_t pack_bytes = (size_t)nblk * NT * 256 * sizeof(float);
    float *P = (float *)ensure(ws_pack_, ws_pack_sz_, pack_bytes);
    hipLaunchKernelGGL(k_krp_pack<float>, dim3(grid_for((int64_t)nblk * NT * 256, 256)), dim3(256), 0, st_,
                       P, nblk, NT, 0, a, J, col0, ncols);
    HIP_CHECK(hipGetLastError());
    double *o = out32 ? (double *)((float *)out + (int64_t)col0 * out_rstride)
                      : out + (int64_t)col0 * out_rstride;
    const int64_t M = L, K = J;
    const int64_t n_mtiles64 = (M + 63) / 64;
    if (n_mtiles64 * T > 0x7fffffff) throw std::runtime_error("ppals: scan grid too large");
    const int n_mtiles = (int)n_mtiles64;
    // k-split: the launch is MFMA-bound, so what counts is how evenly its workgroups fill the resident
    // slots (a partial last round idles the matrix cores): take the split whose number of rounds is
    // closest below a whole number, a little in favour of fewer splits (slab traffic, the combine)
    const void *kernel = nullptr;
    dispatch<5, 6, 7, 8>(NT, [&](auto nt) { kernel = (const void *)k_scan_wide<nt, 1>; });
    const double slots = (double)ncu_ * occupancy(wide_occ_[NT - 1], kernel, 512, 0, 2);
    const int64_t tiles = n_mtiles64 * T;
    int want = 1;
    if ((double)tiles < 8.0 * slots) {
      double best = -1.0;
      const int ns_max = (int)std::min<int64_t>(24, std::max(1, nblk / 16));
      for (int ns = 1; ns <= ns_max; ns++) {
        const double rounds = (double)tiles * ns / slots;
        const double score = rounds / std::ceil(rounds) - 0.004 * ns;
        if (score > best) {
          best = score;
          want = ns;
        }
      }
    }
    const KSplit ks = k_split(nblk, want);
    const int nsplit = ks.nsplit, per = (int)ks.per;
    const PassDst d = pass_dst(nsplit, M, T, ncols, o, out32, out_rstride, out_tstride, pad);
    const int64_t nblocks = (int64_t)n_mtiles * nsplit * T;
    if (nblocks > 0x7fffffff) throw std::runtime_error("ppals: scan grid too large");
    const double bytes = (double)L * (double)J * (double)T * 4.0 + (double)L * (double)T * ncols * (out32 ? 4.0 : 8.0);
    route("scan.f32.wide nt=%d nsplit=%d pad=%d out32=%d", NT, nsplit, pad.ld ? 1 : 0, out32);
    prof_begin(scan_slot_, bytes);
    dispatch<5, 6, 7, 8>(NT, [&](auto nt) {
      hipLaunchKernelGGL((k_scan_wide<nt, 1>), dim3((unsigned)nblocks), dim3(512), 0, st_, V, M, K, M * K, P,
                         n_mtiles, nsplit, per, nblk, d.p, d.nstride, d.split_stride, d.batch_stride, ncols, d.out32,
                         d.row_ld, d.row_valid);
    });
    prof_end();
    HIP_CHECK(hipGetLastError());
    slab_combine(nsplit, d.p, d.split_stride, M, ncols, o, 1, out_rstride, out32, pad, T, d.batch_stride,
                 out_tstride);
  }
  int gj_scalar_ = 0;  // PPALS_GJ_SCALAR=1: the scalar in-LDS sweeps for 64 < R <= 128 (A/B, tests)
  bool wide_enabled_ = true;  // PPALS_SCAN_WIDE=0: chunks of 64 columns (A/B, tests)
  int wide_occ_[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // resident workgroups per CU of k_scan_wide<1..8>
  // Where the tail mode of k_scan_suffix_fast starts (first tile of the last, partial round of resident
  // workgroups), or -1: the launch fits one round, has many rounds (the tail is a small share), or its
  // last round is nearly full anyway. Resident workgroups per CU from the runtime's occupancy query
  // of the tail-mode instantiation (its LDS included).
  template <typename TV>
  int scan_tail_split(int NT, int n_mtiles) {
    constexpr int VEC = ScanTraits<TV>::VEC;
    if (!scan_tail_on_) return -1;
    const size_t lds_t = sizeof(double) * 3 * (size_t)(VEC * NT * 4) * 64;
    const int per_cu = occupancy(scan_tail_occ_[(sizeof(TV) == 8 ? 2 : 0) + (NT - 1)],
                                 NT == 1 ? (const void *)k_scan_suffix_fast<TV, 1, 9>
                                         : (const void *)k_scan_suffix_fast<TV, 2, 9>,
                                 256, lds_t, -1);
    if (per_cu < 0) return -1;
    const int slots = ncu_ * per_cu;
    if (n_mtiles <= slots || n_mtiles > 4 * slots) return -1;
    const int rem = n_mtiles % slots;
    if (rem == 0 || rem * 4 > slots * 3) return -1;   // (a last round that is 3/4 full is left alone)
    return n_mtiles - rem;
  }
  int scan_tail_occ_[4] = {0, 0, 0, 0};
  bool scan_tail_on_ = true;  // PPALS_SCAN_TAIL=0: no tail mode (A/B)
  // Scans of a bf16 tensor (kernels_bf16.hip.h): passes of up to 16 result columns; row-aligned suffix
  // and batched forms on the bf16 matrix cores, every other shape on the per-row fp64 kernels.
  void scan_bf16(const uint16_t *V, int64_t L, int64_t J, int64_t T, const FactorRef *f, int nf, int R,
                 double *out, int64_t out_tstride, int64_t out_rstride, int out32, RowPad pad) {
    int64_t Jk;
    const KrpArgs a = krp_args(f, nf, &Jk);
    if (Jk != J) throw std::runtime_error("ppals: scan factor extents do not match the tensor");
    const bool aligned_base = (((uintptr_t)V) & 15) == 0;
    const int64_t nblk64 = (J + BF16_KB - 1) / BF16_KB;
    const int64_t n_mtiles64 = (L + 511) / 512;
    const bool mfma_ok = L > 1 && aligned_base && L % 8 == 0 && nblk64 * BF16_MAX_NT * 3 * 1024 < 2000000000ll &&
                         n_mtiles64 * T <= 0x7fffffff;
    const bool big = (double)BF16_KB * L * 2.0 >= 2.0e9;  // a k-block past 32-bit buffer offsets
    const double bytes_v = (double)L * J * T * 2.0;
    for (int col0 = 0; col0 < R; col0 += 16 * BF16_MAX_NT) {
      const int ncols = std::min(16 * BF16_MAX_NT, R - col0);
      double *o = out32 ? (double *)((float *)out + (int64_t)col0 * out_rstride) : out + (int64_t)col0 * out_rstride;
      prof_begin(scan_slot_, bytes_v + (double)L * T * ncols * (out32 ? 4.0 : 8.0));
      if (mfma_ok) {
        const int NT = (ncols + 15) / 16;
        const int nblk = (int)nblk64;
        uint16_t *P = (uint16_t *)ensure(ws_pack_, ws_pack_sz_, (size_t)nblk * NT * 3 * 1024);
        hipLaunchKernelGGL(k_krp_pack_bf16, dim3(grid_for((int64_t)nblk * NT * 512, 256)), dim3(256), 0, st_, P,
                           nblk, NT, a, J, col0, ncols);
        HIP_CHECK(hipGetLastError());
        // K-split when the row tiles cannot fill the chip (a tree node of few rows and a long reduction:
        // order 4 at s = 200 keeps 40000 rows = 79 tiles; order 3 keeps s rows = 1 tile): the fp32
        // launcher's rule (scan_t), each split at least 16 k-blocks; partial sums through the slab
        const int64_t M = L;
        int want = 1;
        if (T == 1 && n_mtiles64 < (int64_t)ncu_ * 8)
          want = (int)std::min<int64_t>(((int64_t)ncu_ * 8 + n_mtiles64 - 1) / n_mtiles64,
                                        std::max(1, nblk / 16));
        else if (T > 1 && n_mtiles64 * T < ncu_ && (double)M * T * ncols * nblk / 4 * 8.0 < 64e6)
          want = (int)std::min<int64_t>(((int64_t)ncu_ * 2 + n_mtiles64 * T - 1) / (n_mtiles64 * T),
                                        std::max(1, nblk / 4));
        const KSplit ks = k_split(nblk, want);
        const int nsplit = ks.nsplit, per = (int)ks.per;
        if (n_mtiles64 * nsplit * T > 0x7fffffff) throw std::runtime_error("ppals: scan grid too large");
        const PassDst d = pass_dst(nsplit, M, T, ncols, o, out32, out_rstride, out_tstride, pad);
        const dim3 grid((unsigned)(n_mtiles64 * nsplit * T));
        const bool nts = nt_store(nsplit, (double)L * T * ncols * (out32 ? 4.0 : 8.0));
        route("scan.bf16.mfma nsplit=%d nts=%d pad=%d out32=%d", nsplit, nts ? 1 : 0, pad.ld ? 1 : 0, out32);
        dispatch<true, false>(nts, [&](auto ntsv) {
          dispatch<true, false>(big, [&](auto bigv) {
            hipLaunchKernelGGL((k_scan_suffix_bf16<BF16_MAX_NT, ntsv, bigv>), grid, dim3(256), 0, st_, V, L, J, P,
                               (int)n_mtiles64, nsplit, per, nblk, d.p, d.nstride, d.split_stride, d.batch_stride,
                               ncols, d.out32, d.row_ld, d.row_valid);
          });
        });
        HIP_CHECK(hipGetLastError());
        slab_combine(nsplit, d.p, d.split_stride, M, ncols, o, 1, out_rstride, out32, pad, T, d.batch_stride,
                     out_tstride);
      } else {
        double *B = (double *)ensure(ws_krp_, ws_krp_sz_, sizeof(double) * (size_t)J * ncols);
        krp(B, f, nf, col0, ncols);
        route("%s", L == 1 ? "scan.bf16.prefix" : "scan.bf16.rows");
        if (L == 1)
          hipLaunchKernelGGL(k_scan_bf16_prefix<16 * BF16_MAX_NT>, dim3((unsigned)std::min<int64_t>((T + 3) / 4, 65536)),
                             dim3(256), 0,
                             st_, V, J, T, B, ncols, o, out_tstride, out_rstride, out32);
        else
          hipLaunchKernelGGL(k_scan_bf16_rows<16 * BF16_MAX_NT>, dim3(grid_for(L * T, 256, 16384)), dim3(256), 0,
                             st_, V, L, J, T, B, ncols, o, out_tstride, out_rstride, out32, pad.ld, pad.valid);
      }
      prof_end();
      HIP_CHECK(hipGetLastError());
    }
  }
  using Ops::scan_contract;
  void scan_contract(const void *V, int dt, int64_t L, int64_t J, int64_t T, const FactorRef *f,
                     int nf, int R, void *out, int out_dt, int64_t out_tstride,
                     int64_t out_rstride, RowPad pad) override {
    RoctxRange roctx_("K1/K2/K8/K11 tensor scan");
    const int out32 = out_dt == F32 ? 1 : 0;
    if (dt == BF16)
      scan_bf16((const uint16_t *)V, L, J, T, f, nf, R, (double *)out, out_tstride, out_rstride, out32,
                pad);
    else if (dt == F32)
      scan_t<float>((const float *)V, L, J, T, f, nf, R, (double *)out, out_tstride, out_rstride,
                    out32, pad);
    else
      scan_t<double>((const double *)V, L, J, T, f, nf, R, (double *)out, out_tstride,
                     out_rstride, out32, pad);
  }
  // Tucker mode product keeping the mode in place. Small inputs (the second-level products of a
  // chain: tens of MB with at least a tile of contiguous rows) run as ONE batched thin GEMM on the
  // fp64 matrix cores instead of the streaming scan's pack + scan + slab-combine launches; everything
  // else is the scan.
  void ttm_keep(const void *X, int dt, int64_t L, int64_t J, int64_t T, const double *W, int64_t ldw,
                int Kc, double *out) override {
    const double bytes = (double)L * J * T * dtype_size(dt);
    if (L >= 16 && Kc <= 64 && bytes <= 64e6 && (double)L * J < 2e9 && T <= 65535 && J >= 16 &&
        (double)ldw * Kc < 4e9) {
      RoctxRange roctx_("K11 mode product (batched thin GEMM)");
      const int nt = Kc <= 16 ? 1 : (Kc <= 32 ? 2 : 4);
      route("ttm_keep.gemm nt=%d", nt);
      dim3 grid((unsigned)((L + 15) / 16), (unsigned)((Kc + 16 * nt - 1) / (16 * nt)), (unsigned)T);
      prof_begin(1, bytes);
      dispatch<1, 2, 4>(nt, [&](auto ntv) {
        auto launch = [&](auto ta) {
          using TA = decltype(ta);
          hipLaunchKernelGGL((k_mode_product_small<TA, ntv>), grid, dim3(512), 0, st_, (const TA *)X, (int)L,
                             (int)J, W, ldw, Kc, out);
        };
        if (dt == F32) launch(float());
        else launch(double());
      });
      prof_end();
      HIP_CHECK(hipGetLastError());
      return;
    }
    route("%s", "ttm_keep.scan");
    Ops::ttm_keep(X, dt, L, J, T, W, ldw, Kc, out);
  }
  bool ttm_lead_front(const void *X, int dt, int64_t J, int64_t S, int64_t T, const double *W, int64_t ldw,
                      int Kc, double *out) override {
    const double bytes = (double)J * S * T * dtype_size(dt);
    if (!(S >= 16 && J >= 16 && Kc <= 64 && bytes <= 64e6 && (double)J * S < 2e9 && T <= 65535 &&
          (double)ldw * Kc < 4e9)) {
      route("%s", "ttm_lead.refused");
      return false;
    }
    RoctxRange roctx_("K11 leading-mode product (batched thin GEMM)");
    const int nt = Kc <= 16 ? 1 : (Kc <= 32 ? 2 : 4);
    route("ttm_lead.gemm nt=%d", nt);
    dim3 grid((unsigned)((S + 15) / 16), (unsigned)((Kc + 16 * nt - 1) / (16 * nt)), (unsigned)T);
    prof_begin(1, bytes);
    dispatch<1, 2, 4>(nt, [&](auto ntv) {
      auto launch = [&](auto ta) {
        using TA = decltype(ta);
        hipLaunchKernelGGL((k_mode_product_lead<TA, ntv>), grid, dim3(512), 0, st_, (const TA *)X, (int)J, (int)S,
                           W, ldw, Kc, out);
      };
      if (dt == F32) launch(float());
      else launch(double());
    });
    prof_end();
    HIP_CHECK(hipGetLastError());
    return true;
  }
  // padded resident layout, see ops.h: a pitched copy (rows == 1) or a transposition whose
  // destination rows are padded
  void pad_layout(const void *src, int dt, int64_t rows, int64_t cols, int64_t blk, int64_t ld,
                  void *dst) override {
    if (cols % blk || ld < blk) throw std::runtime_error("ppals: pad_layout block inconsistent");
    const size_t esz = dtype_size(dt);
    HIP_CHECK(hipMemsetAsync(dst, 0, (size_t)ld * (cols / blk) * rows * esz, st_));
    if (rows == 1) {
      HIP_CHECK(hipMemcpy2DAsync(dst, (size_t)ld * esz, src, (size_t)blk * esz, (size_t)blk * esz,
                                 (size_t)(cols / blk), hipMemcpyDeviceToDevice, st_));
      return;
    }
    const int64_t nb = ((rows + 63) / 64) * ((cols + 63) / 64);
    if (nb > 0x7fffffff) throw std::runtime_error("ppals: transpose grid too large");
    if (dt == F32)
      hipLaunchKernelGGL(k_transpose_pad<float>, dim3((unsigned)nb), dim3(256), 0, st_,
                         (const float *)src, rows, cols, blk, ld, (float *)dst);
    else if (dt == BF16)
      hipLaunchKernelGGL(k_transpose_pad<bf16s>, dim3((unsigned)nb), dim3(256), 0, st_,
                         (const bf16s *)src, rows, cols, blk, ld, (bf16s *)dst);
    else
      hipLaunchKernelGGL(k_transpose_pad<double>, dim3((unsigned)nb), dim3(256), 0, st_,
                         (const double *)src, rows, cols, blk, ld, (double *)dst);
    HIP_CHECK(hipGetLastError());
  }

  // ------------------------------------------------------------------ mttv
  template <typename TX>
  void mttv_t(const TX *X, int64_t L, int64_t J, int64_t T, int R, const double *B, int64_t ldb,
              double *out, int64_t rs, int accumulate, const double *scale) {
    constexpr int VL = 16 / sizeof(TX);
    // one more workgroup prepares S, S^-1 of the mode update this contraction feeds (armed by the
    // engine: arm_gram_system) — they depend on the other modes' Grams only
    SysArgs sys;
    size_t lds = 0;
    int extra = 0;
    if (sys_armed_ && sys_R_ == R) {
      sys = sys_;
      extra = 1;
      lds = sizeof(double) * (2 * (size_t)R * (R + 1) + 64) + sizeof(int) * 64;
    }
    prof_begin(1, (double)L * J * T * R * sizeof(TX));
    if (L == 1) {
      int64_t nw = ((T + 3) / 4) * R;
      int g = grid_for(nw * 64, 256, 16384);
      route("mttv.%s.1 extra=%d", tname<TX>(), extra);
      hipLaunchKernelGGL(k_mttv_1<TX>, dim3(g + extra), dim3(256), lds, st_, X, J, T, R, B, ldb, out, rs,
                         accumulate, scale, sys);
    } else if (L % VL == 0 && L >= 16 * VL && ((uintptr_t)X & 15) == 0 &&
               ((L + 64 * VL - 1) / (64 * VL)) * T * R >= 1024) {
      // streaming regime: enough (l-tile, t, r) waves to fill the chip on their own
      int64_t nb = ((L + 64 * VL - 1) / (64 * VL)) * T * R;
      int g = (int)std::min<int64_t>(nb, 1 << 20);
      route("mttv.%s.vec extra=%d", tname<TX>(), extra);
      hipLaunchKernelGGL(k_mttv_vec<TX>, dim3(g + extra), dim3(64), lds, st_, X, L, J, T, R, B, ldb, out,
                         rs, accumulate, scale, sys);
    } else if (L < 64 && L * J <= 2048 && T * R >= 2048) {
      // a short plane per (t, r) and many of them: one wave each, no workgroup barrier (k_mttv_s)
      const int64_t nwaves = T * R;
      int g = (int)std::min<int64_t>((nwaves + 3) / 4, 16384);
      route("mttv.%s.s extra=%d", tname<TX>(), extra);
      hipLaunchKernelGGL(k_mttv_s<TX>, dim3(g + extra), dim3(256), lds, st_, X, (int)L, J, T, R, B, ldb, out,
                         rs, accumulate, scale, sys);
    } else {
      int64_t nb = ((L + 63) / 64) * T * R;
      // a long reduction over few row tiles (128 x 7200 x R: 20 workgroups): the j range is cut into
      // pieces, one workgroup each, and a second launch adds the partial sums in a fixed order
      int jsplit = 1;
      if (nb < 512 && J >= 1024) jsplit = (int)std::min<int64_t>((1024 + nb - 1) / nb, J / 64);
      if (jsplit > 1) {
        const int64_t jchunk = (J + jsplit - 1) / jsplit;
        jsplit = (int)((J + jchunk - 1) / jchunk);
        double *partial = (double *)ensure(ws_mttv_, ws_mttv_sz_, sizeof(double) * (size_t)jsplit * L * T * R);
        const int64_t nbs = nb * jsplit;
        int g = (int)std::min<int64_t>(nbs, 32768);
        route("mttv.%s.l4 jsplit=%d extra=%d", tname<TX>(), jsplit, extra);
        hipLaunchKernelGGL((k_mttv_l<TX, 4>), dim3(g + extra), dim3(256), lds, st_, X, L, J, T, R, B, ldb,
                           out, rs, accumulate, scale, sys, jsplit, jchunk, partial);
        hipLaunchKernelGGL(k_mttv_combine, dim3(grid_for(L * T * R, 256, 1024)), dim3(256), 0, st_, partial,
                           jsplit, L * T, R, out, rs, accumulate, scale);
      } else {
        int g = (int)std::min<int64_t>(nb, 32768);
        route("mttv.%s.%s jsplit=1 extra=%d", tname<TX>(), nb * 4 < 1024 ? "l16" : "l4", extra);
        if (nb * 4 < 1024)  // few blocks: split the j loop 16 ways instead of 4
          hipLaunchKernelGGL((k_mttv_l<TX, 16>), dim3(g + extra), dim3(1024), lds, st_, X, L, J, T, R, B,
                             ldb, out, rs, accumulate, scale, sys);
        else
          hipLaunchKernelGGL((k_mttv_l<TX, 4>), dim3(g + extra), dim3(256), lds, st_, X, L, J, T, R, B, ldb,
                             out, rs, accumulate, scale, sys);
      }
    }
    if (extra) {
      sys_ready_ = true;
      sys_armed_ = false;
    }
    prof_end();
    HIP_CHECK(hipGetLastError());
  }
  void mttv(const void *X, int xdt, int64_t L, int64_t J, int64_t T, const FactorRef *f, int nf,
            int R, double *out, int64_t out_rstride, int accumulate,
            const double *out_scale) override {
    RoctxRange roctx_("K3/K9 mttv (cached intermediate)");
    const double *B;
    int64_t ldb;
    if (nf == 1) {
      if (f[0].rows != J) throw std::runtime_error("ppals: mttv factor extent mismatch");
      B = f[0].ptr;
      ldb = f[0].ld;
    } else {
      double *kb = (double *)ensure(ws_krp_, ws_krp_sz_, sizeof(double) * J * R);
      krp(kb, f, nf, 0, R);
      B = kb;
      ldb = J;
    }
    if (xdt == F32)
      mttv_t<float>((const float *)X, L, J, T, R, B, ldb, out, out_rstride, accumulate, out_scale);
    else
      mttv_t<double>((const double *)X, L, J, T, R, B, ldb, out, out_rstride, accumulate,
                     out_scale);
  }
  void scale_update(double *dst, const double *scales, unsigned mask, int set_one) override {
    hipLaunchKernelGGL(k_scale_update, dim3(1), dim3(64), 0, st_, dst, scales, mask, set_one);
    HIP_CHECK(hipGetLastError());
  }
  void scale_update_many(double *dst, const double *scales, const unsigned *masks, unsigned active,
                         unsigned fresh) override {
    ScaleMasks sm;
    for (int k = 0; k < 32; k++) sm.m[k] = masks[k];
    hipLaunchKernelGGL(k_scale_update_many, dim3(1), dim3(64), 0, st_, dst, scales, sm, active,
                       fresh);
    HIP_CHECK(hipGetLastError());
  }
  const double *normalize_scales() override { return small(MAX_ORDER); }

  // ------------------------------------------------------------------ R x R side
  void gram(const double *W, int64_t rows, int64_t ld, int R, double *G) override {
    RoctxRange roctx_("K4 gram");
    int npairs = R * (R + 1) / 2;
    int g = std::min(64, (npairs + 15) / 16);
    hipLaunchKernelGGL(k_gram, dim3(g), dim3(1024), 0, st_, W, rows, ld, R, G);
    HIP_CHECK(hipGetLastError());
  }
  void gram_system(const double *Gall, int N, int mode, int R, double lambda, double *S,
                   double *Sinv) override {
    if (sys_ready_ && sys_.Gall == Gall && sys_.mode == mode && sys_.S == S && sys_.Sinv == Sinv &&
        sys_.lambda == lambda && sys_R_ == R) {  // prepared on the side of the last contraction
      sys_ready_ = false;
      route("%s", "gram_system.ready");
      return;
    }
    sys_ready_ = false;
    if (R > 64) {  // S, S^-1 out of global memory (kernels_small.hip.h, "rank above 64")
      double *work = (double *)ensure(ws_big_, ws_big_sz_, sizeof(double) * (size_t)R * R + 64);
      int *status = (int *)(work + (size_t)R * R);
      const size_t lds_gj = sizeof(double) * ((size_t)R * R + 2 * (size_t)R);
      const size_t RP = ((size_t)R + 15) & ~(size_t)15;
      const size_t LDm = RP + ((34 - (RP & 31)) & 31);
      const size_t lds_mf = sizeof(double) * (LDm * RP + 8 * RP);
      route("gram_system.%s", lds_mf <= 150 * 1024 && !gj_scalar_ ? "mfma" : lds_gj <= 150 * 1024 ? "lds" : "big");
      if (lds_mf <= 150 * 1024 && !gj_scalar_)   // block sweeps, trailing update on the fp64 matrix cores
        hipLaunchKernelGGL(k_gram_system_mfma, dim3(1), dim3(1024), lds_mf, st_, Gall, N, mode, R,
                           lambda, S, Sinv, status);
      else if (lds_gj <= 150 * 1024)
        hipLaunchKernelGGL(k_gram_system_lds, dim3(1), dim3(1024), lds_gj, st_, Gall, N, mode, R,
                           lambda, S, Sinv, status);
      else
        hipLaunchKernelGGL(k_gram_system_big, dim3(1), dim3(1024), 0, st_, Gall, N, mode, R, lambda,
                           S, Sinv, work, status);
      HIP_CHECK(hipGetLastError());
      // a non-positive pivot (S not positive definite: a rank above a mode extent, collinear
      // columns, a negative lambda) leaves NaNs in Sinv: take the reference's route instead, the
      // untruncated inverse through a full eigen- or singular value decomposition.
      // Up to 128 columns that route is two CONDITIONAL launches on the stream — the one-workgroup
      // one-sided Jacobi of S (S V = W = U Sigma) and V Sigma^-2 W^T, both returning at once unless
      // the elimination set its status word — so a mode update above 64 columns holds no host
      // synchronisation any more (round 6: four read-backs per sweep were 40 us of idle stream each,
      // and milliseconds each whenever the host's cores were busy). PPALS_FORCE_EIGINV=2 runs the two
      // launches ungated (tests).
      if (R <= kJacobiBigMax && force_eiginv_ != 1) {
        double *fb = (double *)ensure(ws_gsfb_, ws_gsfb_sz_, sizeof(double) * (3 * (size_t)R * R + R));
        double *Vt = fb, *Yz = Vt + (size_t)R * R, *Wc = Yz + (size_t)R * R, *wv = Wc + (size_t)R * R;
        const int *gate = force_eiginv_ == 2 ? nullptr : status;
        const size_t lds_j = sizeof(double) * ((size_t)R * (R + 1) + 256) + sizeof(int) * 256;
        hipLaunchKernelGGL(k_jacobi_onesided, dim3(1), dim3(1024), lds_j, st_, (const double *)S, R, Vt, Yz, wv,
                           (double *)nullptr, gate, Wc);
        hipLaunchKernelGGL(k_svd_inverse, dim3(grid_for((int64_t)R * R, 256)), dim3(256), 0, st_,
                           (const double *)Vt, (const double *)Wc, R, Sinv, gate);
        HIP_CHECK(hipGetLastError());
        return;
      }
      int bad = 0;
      route("%s", "gram_system.host_fallback");
      HIP_CHECK(hipMemcpyAsync(&bad, status, sizeof(int), hipMemcpyDeviceToHost, st_));
      HIP_CHECK(hipStreamSynchronize(st_));
      if (bad || force_eiginv_) {
        RocSolver &rs = rocsolver();
        double *D = (double *)ensure(ws_krp_, ws_krp_sz_, sizeof(double) * (2 * (size_t)R + 2));
        double *E = D + R;
        int *info = (int *)(E + R);
        HIP_CHECK(hipMemcpyAsync(work, S, sizeof(double) * (size_t)R * R, hipMemcpyDeviceToDevice, st_));
        if (rs.dsyevd(rs.handle, 211 /*evect_original*/, 121 /*fill_upper*/, R, work, R, D, E, info) != 0)
          throw std::runtime_error("ppals: rocsolver_dsyevd failed (R x R normal equations)");
        hipLaunchKernelGGL(k_eig_inverse, dim3(grid_for((int64_t)R * R, 256)), dim3(256), 0, st_, work,
                           D, R, Sinv);
        HIP_CHECK(hipGetLastError());
      }
      return;
    }
    size_t lds = sizeof(double) * (2 * (size_t)R * (R + 1) + 64) + sizeof(int) * 64;
    route("%s", "gram_system.wave");
    hipLaunchKernelGGL(k_gram_system, dim3(1), dim3(64), lds, st_, Gall, N, mode, R, lambda, S,
                       Sinv, force_jacobi_);
    HIP_CHECK(hipGetLastError());
  }
  void cp_mode_update_blocked(double *Gall, int N, int mode, int R, double lambda, const double *Mblk,
                              int64_t blk, int P, double *scratch, double *W, int64_t ldw, double *grad,
                              int64_t ldg, int64_t rows, double *gradsq, const double *Winit, int64_t ldi,
                              double *dW, int64_t ldd, double ratio, double *S, double *Sinv) override {
    // the staged fused launch reads the gathered blocks as they lie (one launch less per update of the
    // partitioned mode); anything else re-assembles them first
    const size_t lds = sizeof(double) * (32 + 2 * (size_t)R * R + 2 * (size_t)R * (R + 1) + 64) + sizeof(int) * 64;
    const size_t stage = 2 * sizeof(double) * (size_t)rows * R;
    if (R > 64 || force_jacobi_ || norm_armed_ || lds + stage > 150 * 1024 || blk * P != rows ||
        blk > 0x7fffffff) {
      route("%s", "update_blocked.unpack");
      Ops::cp_mode_update_blocked(Gall, N, mode, R, lambda, Mblk, blk, P, scratch, W, ldw, grad, ldg, rows,
                                  gradsq, Winit, ldi, dW, ldd, ratio, S, Sinv);
      return;
    }
    update_mblk_ = (int)blk;
    route("%s", "update_blocked.direct");
    cp_mode_update(Gall, N, mode, R, lambda, Mblk, rows, W, ldw, grad, ldg, rows, gradsq, Winit, ldi, dW,
                   ldd, ratio, S, Sinv, nullptr);
    update_mblk_ = 0;
  }
  int update_mblk_ = 0;
  // rows x R from which a mode update that does not fit the staged launch is row-parallel: the unstaged
  // one-workgroup launch costs 4 us + 4.5 us per 1000 entries (53 us at 1344 x 10, 333 us at 7200 x 10),
  // the row-parallel route five short launches (~30 us)
  static constexpr int64_t kUpdateRowParallelFrom = 6144;
  void cp_mode_update(double *Gall, int N, int mode, int R, double lambda, const double *M,
                      int64_t ldm, double *W, int64_t ldw, double *grad, int64_t ldg, int64_t rows,
                      double *gradsq, const double *Winit, int64_t ldi, double *dW, int64_t ldd,
                      double ratio, double *S, double *Sinv, double *dwsq) override {
    RoctxRange roctx_("K4-K6 mode update");
    if (R > 64) {  // unfused route: S / S^-1, row-parallel update, Gram refresh
      route("%s", "update.unfused why=R");
      Ops::cp_mode_update(Gall, N, mode, R, lambda, M, ldm, W, ldw, grad, ldg, rows, gradsq, Winit,
                          ldi, dW, ldd, ratio, S, Sinv, dwsq);
      return;
    }
    if (force_jacobi_) {  // A/B path: the three separate kernels with the Jacobi inverse
      route("%s", "update.unfused why=jacobi");
      Ops::cp_mode_update(Gall, N, mode, R, lambda, M, ldm, W, ldw, grad, ldg, rows, gradsq, Winit,
                          ldi, dW, ldd, ratio, S, Sinv, dwsq);
      return;
    }
    if (!Winit) dwsq = nullptr;
    size_t lds = sizeof(double) * (32 + 2 * (size_t)R * R + 2 * (size_t)R * (R + 1) + 64) +
                 sizeof(int) * 64;
    const size_t stage = 2 * sizeof(double) * (size_t)rows * R;
    // A long mode (7200 rows at R = 10: coil-100's last mode) does not fit the staged launch, and ONE
    // workgroup walking rows x R entries out of global memory takes 333 us there: the row-parallel
    // unfused route (S / S^-1, rows over many workgroups, Gram) takes a few short launches instead
    if (lds + stage > 150 * 1024 && (int64_t)rows * R > kUpdateRowParallelFrom && !norm_armed_ && !update_mblk_) {
      route("%s", "update.unfused why=rows");
      Ops::cp_mode_update(Gall, N, mode, R, lambda, M, ldm, W, ldw, grad, ldg, rows, gradsq, Winit, ldi, dW,
                          ldd, ratio, S, Sinv, dwsq);
      return;
    }
    // S / S^-1 prepared by the contraction launched before (arm_gram_system + pp_correct)?
    const int presolved = (sys_ready_ && sys_.Gall == Gall && sys_.mode == mode && sys_.S == S &&
                           sys_.Sinv == Sinv && S && sys_.lambda == lambda) ? 1 : 0;
    sys_ready_ = false;
    sys_armed_ = false;
    NormArgs nrm;
    if (norm_armed_) {
      if (!(norm_.on && norm_mode_ == mode && norm_G_ == Gall && ldw == rows))
        throw std::logic_error("ppals: armed Normalize does not match the mode update that followed");
      nrm = norm_;
      nrm.scales = small(MAX_ORDER);
      norm_armed_ = false;
    }
    if (lds + stage <= 150 * 1024) {
      route("update.staged presolved=%d norm=%d mblk=%d dwsq=%d", presolved, nrm.on ? 1 : 0, update_mblk_ ? 1 : 0,
            dwsq ? 1 : 0);
      hipLaunchKernelGGL((k_cp_mode_update<true, true>), dim3(1), dim3(1024), lds + stage, st_, Gall, N, mode,
                         R, lambda, M, ldm, W, ldw, grad, ldg, rows, gradsq, Winit, ldi, dW, ldd, ratio, S,
                         Sinv, dwsq, presolved, nrm, update_mblk_);
    } else {
      if (update_mblk_) throw std::logic_error("ppals: blocked mode update needs the staged launch");
      route("update.unstaged presolved=%d", presolved);
      hipLaunchKernelGGL((k_cp_mode_update<false, false>), dim3(1), dim3(1024), lds, st_, Gall, N, mode,
                         R, lambda, M, ldm, W, ldw, grad, ldg, rows, gradsq, Winit, ldi, dW, ldd, ratio,
                         S, Sinv, dwsq, presolved);
    }
    HIP_CHECK(hipGetLastError());
  }
  // The non-negative (HALS) mode update (kernels_nn.hip.h): rows over one-wave workgroups of 64, the
  // tiles' partial sums of grad^2 added by k_sum_partials, the Gram refresh by the gram op — three
  // short launches, each a fixed summation order.
  void cp_mode_update_nn(double *Gall, int N, int mode, int R, double lambda, const double *M, int64_t ldm,
                         double *W, int64_t ldw, double *grad, int64_t ldg, int64_t rows, double *gradsq,
                         double *S) override {
    RoctxRange roctx_("K4-K6 mode update (non-negative)");
    if (R > 64) throw Unsupported("ppals: the non-negative mode update supports R <= 64");
    if (sys_armed_ || sys_ready_ || norm_armed_)
      throw std::logic_error("ppals: armed S / Normalize in front of a non-negative mode update");
    if (rows <= 0) {
      HIP_CHECK(hipMemsetAsync(gradsq, 0, sizeof(double), st_));
      gram(W, rows, ldw, R, Gall + (size_t)mode * R * R);
      return;
    }
    const int64_t nb = (rows + 63) / 64;
    if (nb > (int64_t)1 << 30) throw std::runtime_error("ppals: mode too long for the non-negative update");
    double *part = (double *)ensure(ws_big2_, ws_big2_sz_, sizeof(double) * (size_t)nb);
    const size_t lds = sizeof(double) * ((size_t)R * R + 64 * (size_t)R);
    route("update_nn R=%d tiles=%lld", R, (long long)nb);
    hipLaunchKernelGGL(k_cp_update_nn, dim3((unsigned)nb), dim3(64), lds, st_, Gall, N, mode, R, lambda, M,
                       ldm, W, ldw, grad, ldg, rows, part, S, kNnFloor);
    hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(1024), 0, st_, part, (int)nb, gradsq);
    HIP_CHECK(hipGetLastError());
    gram(W, rows, ldw, R, Gall + (size_t)mode * R * R);
  }
  // The non-negative mode updates of all starts of a multi-start session in TWO launches whatever the
  // number of starts: the row kernel on a grid of (row tiles x starts), then one workgroup per start that
  // adds the start's tile sums and refreshes its Gram. Bracketed as cp_mode_update_batched is.
  void cp_mode_update_nn_batched(double *Gall, int N, int mode, int R, int nstarts, double lambda,
                                 const double *M, int64_t ldm, double *W, int64_t ldw, double *grad,
                                 int64_t ldg, int64_t rows, double *gradsq, double *S) override {
    RoctxRange roctx_("K4-K6 mode update (non-negative, batched over starts)");
    if (R > 64) throw Unsupported("ppals: the non-negative mode update supports R <= 64");
    if (nstarts < 1 || nstarts > 65535) throw std::runtime_error("ppals: number of starts out of range");
    if (sys_armed_ || sys_ready_ || norm_armed_)
      throw std::logic_error("ppals: armed S / Normalize in front of a non-negative mode update");
    if (rows <= 0) {
      Ops::cp_mode_update_nn_batched(Gall, N, mode, R, nstarts, lambda, M, ldm, W, ldw, grad, ldg, rows,
                                     gradsq, S);
      return;
    }
    const int64_t nb = (rows + 63) / 64;
    if (nb * nstarts > (int64_t)1 << 30)
      throw std::runtime_error("ppals: mode too long for the non-negative update");
    double *part = (double *)ensure(ws_big2_, ws_big2_sz_, sizeof(double) * (size_t)nb * nstarts);
    const size_t lds = sizeof(double) * ((size_t)R * R + 64 * (size_t)R);
    route("update_nn_batched R=%d tiles=%lld starts=%d", R, (long long)nb, nstarts);
    prof_begin(1, 0.0);
    hipLaunchKernelGGL(k_cp_update_nn, dim3((unsigned)nb, (unsigned)nstarts), dim3(64), lds, st_, Gall, N,
                       mode, R, lambda, M, ldm, W, ldw, grad, ldg, rows, part, S, kNnFloor);
    hipLaunchKernelGGL(k_cp_finish_nn_batched, dim3((unsigned)nstarts), dim3(1024), 0, st_, part, (int)nb,
                       gradsq, W, ldw, rows, R, N, mode, Gall);
    prof_end();
    HIP_CHECK(hipGetLastError());
  }
  // The mode updates of all starts of a multi-start session in ONE launch: a 1024-thread workgroup per
  // start (nstarts <= 32 of them on 256 CUs: every workgroup has a CU and its LDS to itself, none waits
  // for another). The same routes as cp_mode_update: the staged launch where M and W of ONE start fit
  // the LDS, the unstaged one for short long modes, start by start through the unfused routes otherwise.
  void cp_mode_update_batched(double *Gall, int N, int mode, int R, int nstarts, double lambda,
                              const double *M, int64_t ldm, double *W, int64_t ldw, double *grad,
                              int64_t ldg, int64_t rows, double *gradsq, double *S, double *Sinv) override {
    RoctxRange roctx_("K4-K6 mode update (batched over starts)");
    const size_t lds = sizeof(double) * (32 + 2 * (size_t)R * R + 2 * (size_t)R * (R + 1) + 64) +
                       sizeof(int) * 64;
    const size_t stage = 2 * sizeof(double) * (size_t)rows * R;
    const bool staged = lds + stage <= 150 * 1024;
    if (R > 64 || force_jacobi_ || nstarts < 1 || (double)rows * R >= 2.0e9 ||
        (!staged && (int64_t)rows * R > kUpdateRowParallelFrom)) {
      // (bracketed start by start: the profile's launch count shows which route a session took)
      route("%s", "update_batched.loop");
      for (int b = 0; b < nstarts; b++) {
        const size_t rr = (size_t)R * R;
        prof_begin(1, 0.0);
        cp_mode_update(Gall + b * N * rr, N, mode, R, lambda, M + (size_t)b * R * ldm, ldm,
                       W + (size_t)b * R * ldw, ldw, grad + (size_t)b * R * ldg, ldg, rows, gradsq + b, nullptr,
                       rows, nullptr, rows, 1.0, S ? S + b * rr : nullptr, Sinv ? Sinv + b * rr : nullptr,
                       nullptr);
        prof_end();
      }
      return;
    }
    if (norm_armed_) throw std::logic_error("ppals: armed Normalize in front of a batched mode update");
    sys_ready_ = false;
    sys_armed_ = false;
    prof_begin(1, 0.0);
    route("%s", staged ? "update_batched.staged" : "update_batched.unstaged");
    if (staged)
      hipLaunchKernelGGL((k_cp_mode_update_batched<true, true>), dim3((unsigned)nstarts), dim3(1024),
                         lds + stage, st_, Gall, N, mode, R, lambda, M, ldm, W, ldw, grad, ldg, rows, gradsq,
                         S, Sinv);
    else
      hipLaunchKernelGGL((k_cp_mode_update_batched<false, false>), dim3((unsigned)nstarts), dim3(1024), lds,
                         st_, Gall, N, mode, R, lambda, M, ldm, W, ldw, grad, ldg, rows, gradsq, S, Sinv);
    prof_end();
    HIP_CHECK(hipGetLastError());
  }
  // ---- rank-sweep sessions: the three ops above for starts of different ranks (StartTable) ----
  // what the table must hold before a kernel indexes by it (the engine builds it; checked all the same)
  static void check_table(const StartTable &t) {
    bool ok = t.nstarts >= 1 && t.nstarts <= kMaxStarts && t.col[0] == 0 && t.sq[0] == 0;
    for (int b = 0; ok && b < t.nstarts; b++)
      ok = t.rank(b) >= 1 && t.sq[b + 1] == t.sq[b] + t.rank(b) * t.rank(b);
    if (!ok) throw std::runtime_error("ppals: malformed table of starts");
  }
  // One launch, a 1024-thread workgroup per start, each with its own rank (k_cp_mode_update_ragged). The
  // routes of cp_mode_update_batched, decided ONCE per launch with the largest rank: its LDS sizes the
  // launch, and a launch is staged only if the largest start's M and W fit.
  void cp_mode_update_ragged(double *Gall, int N, int mode, const StartTable &t, double lambda, const double *M,
                             int64_t ldm, double *W, int64_t ldw, double *grad, int64_t ldg, int64_t rows,
                             double *gradsq, double *S, double *Sinv) override {
    RoctxRange roctx_("K4-K6 mode update (starts of different ranks)");
    check_table(t);
    const int R = t.max_rank();
    const size_t lds = sizeof(double) * (32 + 2 * (size_t)R * R + 2 * (size_t)R * (R + 1) + 64) +
                       sizeof(int) * 64;
    const size_t stage = 2 * sizeof(double) * (size_t)rows * R;
    const bool staged = lds + stage <= 150 * 1024;
    if (R > 64 || force_jacobi_ || (double)rows * R >= 2.0e9 ||
        (!staged && (int64_t)rows * R > kUpdateRowParallelFrom)) {
      route("%s", "update_ragged.loop");
      for (int b = 0; b < t.nstarts; b++) {
        const size_t c0 = (size_t)t.col[b];
        prof_begin(1, 0.0);
        cp_mode_update(Gall + (size_t)N * t.sq[b], N, mode, t.rank(b), lambda, M + c0 * ldm, ldm, W + c0 * ldw,
                       ldw, grad + c0 * ldg, ldg, rows, gradsq + b, nullptr, rows, nullptr, rows, 1.0,
                       S ? S + t.sq[b] : nullptr, Sinv ? Sinv + t.sq[b] : nullptr, nullptr);
        prof_end();
      }
      return;
    }
    if (norm_armed_) throw std::logic_error("ppals: armed Normalize in front of a batched mode update");
    sys_ready_ = false;
    sys_armed_ = false;
    prof_begin(1, 0.0);
    route("%s", staged ? "update_ragged.staged" : "update_ragged.unstaged");
    if (staged)
      hipLaunchKernelGGL((k_cp_mode_update_ragged<true, true>), dim3((unsigned)t.nstarts), dim3(1024),
                         lds + stage, st_, Gall, N, mode, t, lambda, M, ldm, W, ldw, grad, ldg, rows, gradsq, S,
                         Sinv);
    else
      hipLaunchKernelGGL((k_cp_mode_update_ragged<false, false>), dim3((unsigned)t.nstarts), dim3(1024), lds,
                         st_, Gall, N, mode, t, lambda, M, ldm, W, ldw, grad, ldg, rows, gradsq, S, Sinv);
    prof_end();
    HIP_CHECK(hipGetLastError());
  }
  // One launch for all modes and starts: a grid of (starts x modes x row tiles), each workgroup inverting
  // its start's Gram of its mode in LDS (k_cp_pinv_ragged). The LDS of the launch is sized for the largest rank.
  void cp_pinv_ragged(const double *Gall, int N, const StartTable &t, double *const *W, const int64_t *rows,
                      double *const *P, int *bad) override {
    RoctxRange roctx_("core consistency: pseudo-inverse factors");
    check_table(t);
    const int R = t.max_rank();
    if (R > kPinvMaxRank) throw Unsupported("ppals: the pseudo-inverse factors support ranks <= 64");
    if (N < 1 || N > MAX_ORDER) throw std::runtime_error("ppals: cp_pinv_ragged order out of range");
    PinvArgs a;
    int64_t maxrows = 1;
    for (int i = 0; i < MAX_ORDER; i++) {
      a.w[i] = i < N ? W[i] : nullptr;
      a.p[i] = i < N ? P[i] : nullptr;
      a.rows[i] = i < N ? rows[i] : 0;
      if (i < N) maxrows = std::max(maxrows, rows[i]);
    }
    const size_t lds = sizeof(double) * ((size_t)R * R + 2 * (size_t)R);
    const unsigned ntiles = (unsigned)std::min<int64_t>((maxrows + 255) / 256, 1024);
    route("pinv_ragged starts=%d rmax=%d tiles=%u", t.nstarts, R, ntiles);
    prof_begin(1, 0.0);
    hipLaunchKernelGGL(k_cp_pinv_ragged, dim3((unsigned)t.nstarts, (unsigned)N, ntiles), dim3(256), lds, st_, Gall,
                       N, t, a, bad);
    prof_end();
    HIP_CHECK(hipGetLastError());
  }
  void core_score(double *core, int R, int N, const int *bad, double *cc) override {
    RoctxRange roctx_("core consistency: score");
    int64_t n = 1, dstride = 0;
    for (int i = 0; i < N; i++) {
      dstride += n;
      n *= R;
    }
    prof_begin(1, 8.0 * (double)n);
    hipLaunchKernelGGL(k_core_score, dim3(1), dim3(1024), 0, st_, core, n, R, dstride, bad, cc);
    prof_end();
    HIP_CHECK(hipGetLastError());
  }
  // Two launches whatever N, the columns and the extents: k_fms_cross on one workgroup per (mode, slab of
  // row chunks), k_fms_finish on the partials. The slabs are a function of the extents alone.
  static void fms_args(int N, const CongruenceSide &a, const CongruenceSide &b, unsigned mask, FmsArgs &A) {
    if (N < 1 || N > MAX_ORDER) throw std::runtime_error("ppals: factor_congruence order out of range");
    if (a.cols < 1 || b.cols < 1 || a.cols > kCongruenceMaxCols || b.cols > kCongruenceMaxCols)
      throw Unsupported("ppals: the factor congruence supports 1 .. 128 columns a side");
    A = FmsArgs();
    A.N = N;
    A.Ca = a.cols;
    A.Cb = b.cols;
    A.mask = mask;
    A.same = a.cols == b.cols;
    int at = 0;
    for (int i = 0; i < N; i++) {
      if (a.rows[i] < 1 || b.rows[i] < 1 || a.ld[i] < a.rows[i] || b.ld[i] < b.rows[i])
        throw std::runtime_error("ppals: factor_congruence rows / leading dimension out of range");
      if (((mask >> i) & 1u) && a.rows[i] != b.rows[i])
        throw std::runtime_error("ppals: factor_congruence extents differ in a compared mode");
      A.a[i] = a.w[i];
      A.b[i] = b.w[i];
      A.lda[i] = a.ld[i];
      A.ldb[i] = b.ld[i];
      A.rows_a[i] = a.rows[i];
      A.rows_b[i] = b.rows[i];
      A.same = A.same && a.w[i] == b.w[i] && a.ld[i] == b.ld[i] && a.rows[i] == b.rows[i];
      const int64_t chunks = (std::max(a.rows[i], b.rows[i]) + FMS_CH - 1) / FMS_CH;
      const int64_t cps = (chunks + FMS_MAXSLAB - 1) / FMS_MAXSLAB;
      if (cps > 0x7fffffff / FMS_CH) throw std::runtime_error("ppals: factor_congruence extent too large");
      A.cps[i] = (int)cps;
      A.slab0[i] = at;
      at += (int)((chunks + cps - 1) / cps);
    }
    for (int i = N; i <= MAX_ORDER; i++) A.slab0[i] = at;
  }
  static int fms_pad(int c) { return 16 * ((c + 15) / 16); }
  size_t factor_congruence_work(int N, const CongruenceSide &a, const CongruenceSide &b) override {
    FmsArgs A;
    fms_args(N, a, b, 0u, A);
    return sizeof(double) * (size_t)A.slab0[N] * (size_t)fms_part_stride(fms_pad(a.cols), fms_pad(b.cols));
  }
  void factor_congruence(int N, const CongruenceSide &a, const CongruenceSide &b, unsigned mask, void *work,
                         double *Phi, double *wa, double *wb) override {
    RoctxRange roctx_("factor congruence");
    FmsArgs A;
    fms_args(N, a, b, mask, A);
    if (!work) throw std::runtime_error("ppals: factor_congruence without its work buffer");
    const int cap = fms_pad(a.cols), cbp = fms_pad(b.cols), nslab = A.slab0[N];
    const size_t lds = fms_lds_bytes(cap, cbp, A.same != 0);
    double bytes = 0;
    for (int i = 0; i < N; i++) bytes += 8.0 * ((double)a.rows[i] * a.cols + (A.same ? 0.0 : (double)b.rows[i] * b.cols));
    const double pbytes = 8.0 * (double)nslab * (double)fms_part_stride(cap, cbp);
    route("fms.cross slabs=%d ca=%d cb=%d same=%d", nslab, a.cols, b.cols, A.same);
    prof_begin(1, bytes + pbytes);
    hipLaunchKernelGGL(k_fms_cross, dim3((unsigned)nslab), dim3(256), lds, st_, A, (double *)work);
    prof_end();
    HIP_CHECK(hipGetLastError());
    const int64_t entries = (int64_t)a.cols * b.cols;
    const unsigned nfin = (unsigned)std::min<int64_t>((entries + 255) / 256, 64);
    prof_begin(1, pbytes + 8.0 * (double)entries);
    hipLaunchKernelGGL(k_fms_finish, dim3(nfin), dim3(256), 0, st_, A, (const double *)work, Phi, wa, wb);
    prof_end();
    HIP_CHECK(hipGetLastError());
  }
  // Two launches whatever the ranks: the row kernel on (row tiles x starts) with the LDS of the largest
  // rank, then a workgroup per start for its tile sums and its Gram. Bracketed as the batched one is.
  void cp_mode_update_nn_ragged(double *Gall, int N, int mode, const StartTable &t, double lambda,
                                const double *M, int64_t ldm, double *W, int64_t ldw, double *grad, int64_t ldg,
                                int64_t rows, double *gradsq, double *S) override {
    RoctxRange roctx_("K4-K6 mode update (non-negative, starts of different ranks)");
    check_table(t);
    const int R = t.max_rank();
    if (R > 64) throw Unsupported("ppals: the non-negative mode update supports R <= 64");
    if (sys_armed_ || sys_ready_ || norm_armed_)
      throw std::logic_error("ppals: armed S / Normalize in front of a non-negative mode update");
    if (rows <= 0) {
      Ops::cp_mode_update_nn_ragged(Gall, N, mode, t, lambda, M, ldm, W, ldw, grad, ldg, rows, gradsq, S);
      return;
    }
    const int64_t nb = (rows + 63) / 64;
    if (nb * t.nstarts > (int64_t)1 << 30)
      throw std::runtime_error("ppals: mode too long for the non-negative update");
    double *part = (double *)ensure(ws_big2_, ws_big2_sz_, sizeof(double) * (size_t)nb * t.nstarts);
    const size_t lds = sizeof(double) * ((size_t)R * R + 64 * (size_t)R);
    route("update_nn_ragged rmax=%d tiles=%lld starts=%d", R, (long long)nb, t.nstarts);
    prof_begin(1, 0.0);
    hipLaunchKernelGGL(k_cp_update_nn_ragged, dim3((unsigned)nb, (unsigned)t.nstarts), dim3(64), lds, st_, Gall, N,
                       mode, t, lambda, M, ldm, W, ldw, grad, ldg, rows, part, S, kNnFloor);
    hipLaunchKernelGGL(k_cp_finish_nn_ragged, dim3((unsigned)t.nstarts), dim3(1024), 0, st_, part, (int)nb,
                       gradsq, W, ldw, rows, t, N, mode, Gall);
    prof_end();
    HIP_CHECK(hipGetLastError());
  }
  // The orthonormal mode update (kernels_polar.hip.h) in THREE launches whatever the starts, ranks and rows:
  // a workgroup per start for T = (M^T M)^(-1/2) and the start's status, the row kernel on (row tiles x
  // starts) for grad, its tile sums and W = M T, then k_cp_finish_nn_ragged for the sums and the Grams. Each
  // launch is bracketed on its own, so the launch profile counts them. Scratch: T | tile sums | status.
  void cp_mode_update_ortho_ragged(double *Gall, int N, int mode, const StartTable &t, double lambda,
                                   const double *M, int64_t ldm, double *W, int64_t ldw, double *grad,
                                   int64_t ldg, int64_t rows, double *gradsq, double *S) override {
    RoctxRange roctx_("K4-K6 mode update (orthonormal)");
    check_table(t);
    const int R = t.max_rank();
    if (R > 64) throw Unsupported("ppals: the orthonormal mode update supports R <= 64");
    if (sys_armed_ || sys_ready_ || norm_armed_)
      throw std::logic_error("ppals: armed S / Normalize in front of an orthonormal mode update");
    if (rows <= 0) {
      Ops::cp_mode_update_ortho_ragged(Gall, N, mode, t, lambda, M, ldm, W, ldw, grad, ldg, rows, gradsq, S);
      return;
    }
    const int64_t nb = (rows + 63) / 64;
    if (nb * t.nstarts > (int64_t)1 << 30)
      throw std::runtime_error("ppals: mode too long for the orthonormal update");
    const size_t nT = (size_t)t.sq[t.nstarts], npart = (size_t)nb * t.nstarts;
    double *Tm = (double *)ensure(ws_big2_, ws_big2_sz_, sizeof(double) * (nT + npart) + sizeof(int) * kMaxStarts);
    double *part = Tm + nT;
    int *status = (int *)(part + npart);
    const size_t lds1 = sizeof(double) * (2 * (size_t)R * (R + 1) + 64 + 18) + sizeof(int) * 64;
    const size_t lds2 = sizeof(double) * ((size_t)R * R + 64 * (size_t)R);
    route("update_ortho R=%d starts=%d tiles=%d", R, t.nstarts, (int)nb);
    prof_begin(1, 0.0);
    hipLaunchKernelGGL(k_polar_factor, dim3((unsigned)t.nstarts), dim3(1024), lds1, st_, M, ldm, rows, t,
                       kOrthoMinRatio, Tm, status);
    prof_end();
    prof_begin(1, 0.0);
    hipLaunchKernelGGL(k_cp_update_ortho_ragged, dim3((unsigned)nb, (unsigned)t.nstarts), dim3(64), lds2, st_, Gall,
                       N, mode, t, lambda, M, ldm, W, ldw, grad, ldg, rows, part, S, Tm, status);
    prof_end();
    prof_begin(1, 0.0);
    hipLaunchKernelGGL(k_cp_finish_nn_ragged, dim3((unsigned)t.nstarts), dim3(1024), 0, st_, part, (int)nb,
                       gradsq, W, ldw, rows, t, N, mode, Gall);
    prof_end();
    HIP_CHECK(hipGetLastError());
  }
  // The shaped non-negative mode update (kernels_shape.hip.h) in THREE launches whatever the starts, ranks and
  // rows: the gradient on (row tiles x starts), a workgroup per start for the column loop, then
  // k_cp_finish_nn_ragged for the sums and the Grams. Each launch is bracketed on its own, so the launch profile
  // counts them. The column loop keeps its work arrays in LDS while S and shape_work_bytes(rows) fit in
  // kShapeLdsBytes (route tag "lds"), else in the scratch behind the tile sums ("global").
  void cp_mode_update_shape_ragged(double *Gall, int N, int mode, const StartTable &t, double lambda,
                                   const double *M, int64_t ldm, double *W, int64_t ldw, double *grad,
                                   int64_t ldg, int64_t rows, double *gradsq, double *S, int shape) override {
    RoctxRange roctx_("K4-K6 mode update (shaped non-negative)");
    check_table(t);
    const int R = t.max_rank();
    if (R > 64) throw Unsupported("ppals: the shaped mode update supports R <= 64");
    if (shape < kShapeUnimodal || shape > kShapeDecreasing)
      throw std::invalid_argument("ppals: a shaped mode update needs PPALS_SHAPE_UNIMODAL, _INCREASING or _DECREASING");
    if (sys_armed_ || sys_ready_ || norm_armed_)
      throw std::logic_error("ppals: armed S / Normalize in front of a shaped mode update");
    if (rows <= 0) {
      Ops::cp_mode_update_shape_ragged(Gall, N, mode, t, lambda, M, ldm, W, ldw, grad, ldg, rows, gradsq, S, shape);
      return;
    }
    const int64_t nb = (rows + 63) / 64;
    if (rows > (int64_t)1 << 30 || nb * t.nstarts > (int64_t)1 << 30)
      throw std::runtime_error("ppals: mode too long for the shaped update");
    const size_t lds1 = sizeof(double) * ((size_t)R * R + 64 * (size_t)R);
    const size_t sbytes = sizeof(double) * (size_t)R * R, wbytes = shape_work_bytes(rows);
    const bool in_lds = sbytes + wbytes <= kShapeLdsBytes;
    const size_t npart = (size_t)nb * t.nstarts, wstride = wbytes / sizeof(double);
    double *part = (double *)ensure(ws_big2_, ws_big2_sz_,
                                    sizeof(double) * npart + (in_lds ? 0 : wbytes * (size_t)t.nstarts));
    double *gwork = in_lds ? nullptr : part + npart;
    route("update_shape kind=%d R=%d starts=%d rows=%lld %s", shape, R, t.nstarts, (long long)rows,
          in_lds ? "lds" : "global");
    prof_begin(1, 0.0);
    hipLaunchKernelGGL(k_shape_grad, dim3((unsigned)nb, (unsigned)t.nstarts), dim3(64), lds1, st_, Gall, N, mode, t,
                       lambda, M, ldm, W, ldw, grad, ldg, rows, part, S);
    prof_end();
    prof_begin(1, 0.0);
    hipLaunchKernelGGL(k_shape_columns, dim3((unsigned)t.nstarts), dim3(1024), sbytes + (in_lds ? wbytes : 0), st_,
                       Gall, N, mode, t, lambda, M, ldm, W, ldw, rows, shape, kNnFloor, R, gwork, (int64_t)wstride);
    prof_end();
    prof_begin(1, 0.0);
    hipLaunchKernelGGL(k_cp_finish_nn_ragged, dim3((unsigned)t.nstarts), dim3(1024), 0, st_, part, (int)nb,
                       gradsq, W, ldw, rows, t, N, mode, Gall);
    prof_end();
    HIP_CHECK(hipGetLastError());
  }
  // one launch, a workgroup per start, every pair's sum that of k_gram
  void gram_ragged(const double *W, int64_t rows, int64_t ld, const StartTable &t, int N, int mode,
                   double *Gall) override {
    RoctxRange roctx_("K4 gram (starts of different ranks)");
    check_table(t);
    hipLaunchKernelGGL(k_gram_ragged, dim3((unsigned)t.nstarts), dim3(1024), 0, st_, W, rows, ld, t, N, mode,
                       Gall);
    HIP_CHECK(hipGetLastError());
  }
  // one launch, a workgroup per start (k_cp_hold_rows); a start that holds nothing out returns at once
  void cp_hold_rows(double *W, int64_t ldw, double *grad, int64_t ldg, double *scores, int64_t lds, int64_t rows,
                    const StartTable &t, const uint8_t *keep, unsigned holds, double *Gall, int N, int mode,
                    double *gradsq) override {
    RoctxRange roctx_("hold-out rows of the sample mode");
    check_table(t);
    if (rows <= 0 || ldw < rows || ldg < rows || lds < rows || mode < 0 || mode >= N || !keep)
      throw std::runtime_error("ppals: cp_hold_rows arguments out of range");
    if (t.nstarts < 32) holds &= (1u << t.nstarts) - 1u;
    if (!holds) return;
    route("hold_rows starts=%d holds=0x%x", t.nstarts, holds);
    prof_begin(1, 0.0);
    hipLaunchKernelGGL(k_cp_hold_rows, dim3((unsigned)t.nstarts), dim3(1024), 0, st_, W, ldw, grad, ldg, scores,
                       lds, rows, t, keep, holds, N, mode, Gall, gradsq);
    prof_end();
    HIP_CHECK(hipGetLastError());
  }
  bool arm_normalize(double *const *W, const int64_t *rows, int N, int R, double *Gall, int mode,
                     double *wsq, double *ms_dst, const unsigned *masks, unsigned active,
                     unsigned fresh) override {
    norm_armed_ = false;
    if (R > 64 || force_jacobi_ || N > MAX_ORDER) {
      route("%s", "arm_normalize.refused");
      return false;
    }
    int64_t tot = 0;
    for (int i = 0; i < N; i++) tot += rows[i] * R;
    const size_t lds = sizeof(double) * (32 + 2 * (size_t)R * R + 2 * (size_t)R * (R + 1) + 64) +
                       sizeof(int) * 64;
    if (tot > 65536 || lds + 2 * sizeof(double) * (size_t)rows[mode] * R > 150 * 1024) {
      route("%s", "arm_normalize.refused");
      return false;
    }
    norm_ = NormArgs();
    norm_.on = 1;
    for (int i = 0; i < N; i++) {
      norm_.w.p[i] = W[i];
      norm_.w.n[i] = rows[i] * R;
    }
    norm_.wsq = wsq;
    if (active && ms_dst && masks) {
      norm_.ms_dst = ms_dst;
      for (int k = 0; k < 32; k++) norm_.masks.m[k] = masks[k];
      norm_.active = active;
      norm_.fresh = fresh;
    }
    norm_mode_ = mode;
    norm_G_ = Gall;
    (void)small(MAX_ORDER);  // (allocated now: no workspace growth inside the armed launch)
    norm_armed_ = true;
    route("%s", "arm_normalize.taken");
    return true;
  }
  void arm_gram_system(const double *Gall, int N, int mode, int R, double lambda, double *S,
                       double *Sinv) override {
    sys_ready_ = false;
    sys_armed_ = false;
    if (force_jacobi_ || R > 32 || !S || !Sinv) return;
    sys_.Gall = Gall;
    sys_.N = N;
    sys_.mode = mode;
    sys_.lambda = lambda;
    sys_.S = S;
    sys_.Sinv = Sinv;
    sys_.force_jacobi = 0;
    sys_R_ = R;
    sys_armed_ = true;
  }
  void pp_correct(const double *M0, int64_t rows, int R, const PPTerm *terms, int nterms,
                  double *M) override {
    RoctxRange roctx_("K9 pp_correct");
    if (nterms > MAX_ORDER) throw std::runtime_error("ppals: too many PP correction terms");
    PPTerms tm;
    tm.n = nterms;
    for (int t = 0; t < nterms; t++) {
      tm.T[t] = terms[t].T;
      tm.dW[t] = terms[t].dW;
      tm.ny[t] = terms[t].ny;
      tm.lddw[t] = terms[t].lddw;
      tm.keep_first[t] = terms[t].keep_first;
    }
    dim3 grid((unsigned)((rows + 15) / 16), (unsigned)R);
    SysArgs sys;
    size_t lds = 0;
    if (sys_armed_ && sys_R_ == R) {  // one more column of blocks: its first block prepares S, S^-1
      sys = sys_;
      grid.x += 1;
      lds = sizeof(double) * (2 * (size_t)R * (R + 1) + 64) + sizeof(int) * 64;
    }
    route("pp_correct terms=%d extra=%d", nterms, sys.Gall ? 1 : 0);
    prof_begin(1, 0.0);
    hipLaunchKernelGGL(k_pp_correct, grid, dim3(256), lds, st_, M0, rows, R, tm, M, sys);
    prof_end();
    HIP_CHECK(hipGetLastError());
    if (sys.Gall) sys_ready_ = true;
    sys_armed_ = false;
  }
  void cp_update(const double *M, int64_t ldm, const double *Wold, int64_t ldw, double *Wnew,
                 int64_t ldn, double *grad, int64_t ldg, int64_t rows, int R, const double *S,
                 const double *Sinv, double *gradsq, const double *Winit, int64_t ldi, double *dW,
                 int64_t ldd, double ratio) override {
    if (rows <= 0) {  // a rank that owns no rows of this mode (row-block plan): nothing to launch
      route("%s", "cp_update.empty");
      HIP_CHECK(hipMemsetAsync(gradsq, 0, sizeof(double), st_));
      return;
    }
    if (R > 64 && ldg == rows && ldn == rows && (!Winit || ratio == 1.0) && rows * (int64_t)R < (1 << 30)) {
      // both products on the matrix cores (S and S^-1 are symmetric: they ARE their own
      // transposed operand): grad = W_old S - M, then W = M S^-1 (may alias W_old: stream order)
      route("cp_update.gemm tail=%d", Winit ? 1 : 0);
      gemm_nt(Wold, ldw, S, R, M, ldm, grad, ldg, (int)rows, R, R, 1.0, -1.0);
      sumsq(grad, rows * R, gradsq);
      gemm_nt(M, ldm, Sinv, R, nullptr, 0, Wnew, ldn, (int)rows, R, R, 1.0, 0.0);
      if (Winit) {  // SVD_solve_mod tail with ratio 1: dW = W - W_init
        if (ldi != rows || ldd != rows) throw std::runtime_error("ppals: cp_update expects packed factors");
        double *A[1] = {Wnew}, *B[1] = {const_cast<double *>(Winit)}, *D[1] = {dW};
        int64_t n[1] = {rows * R};
        diff_norms(A, B, n, 1, 1, D, 0, (double *)ensure(ws_big2_, ws_big2_sz_, 4 * sizeof(double)));
      }
      HIP_CHECK(hipGetLastError());
      return;
    }
    if (R > 64 || (int64_t)rows * R > kUpdateRowParallelFrom) {
      // several blocks update the rows: W_old is read from a scratch copy so that Wnew may alias it
      route("%s", "cp_update.rows");
      const int nb = (int)((rows + 63) / 64);
      double *wcopy = (double *)ensure(ws_big2_, ws_big2_sz_,
                                       sizeof(double) * ((size_t)rows * R + (size_t)nb));
      double *part = wcopy + (size_t)rows * R;
      HIP_CHECK(hipMemcpy2DAsync(wcopy, sizeof(double) * rows, Wold, sizeof(double) * ldw,
                                 sizeof(double) * rows, R, hipMemcpyDeviceToDevice, st_));
      hipLaunchKernelGGL(k_cp_update_big, dim3(nb), dim3(256), 0, st_, M, ldm, wcopy, rows, Wnew, ldn,
                         grad, ldg, rows, R, S, Sinv, part, Winit, ldi, dW, ldd, ratio);
      hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(1024), 0, st_, part, nb, gradsq);
      HIP_CHECK(hipGetLastError());
      return;
    }
    size_t lds = sizeof(double) * (32 + 2 * (size_t)R * R);
    route("%s", "cp_update.one");
    hipLaunchKernelGGL(k_cp_update, dim3(1), dim3(1024), lds, st_, M, ldm, Wold, ldw, Wnew, ldn,
                       grad, ldg, rows, R, S, Sinv, gradsq, Winit, ldi, dW, ldd, ratio);
    HIP_CHECK(hipGetLastError());
  }
  void normalize(double *const *W, const int64_t *rows, int N, int R, double *Gall) override {
    double *scales = small(MAX_ORDER);
    route("%s", "normalize.grid");
    hipLaunchKernelGGL(k_norm_scales, dim3(1), dim3(1024), 0, st_, Gall, N, R, scales);
    HIP_CHECK(hipGetLastError());
    PtrsN w;
    int64_t mx = 1;
    for (int i = 0; i < N; i++) {
      w.p[i] = W[i];
      w.n[i] = rows[i] * R;
      mx = std::max(mx, w.n[i]);
    }
    hipLaunchKernelGGL(k_scale_factors, dim3(grid_for(mx, 256, 64), N), dim3(256), 0, st_, w, N,
                       scales);
    HIP_CHECK(hipGetLastError());
  }
  void normalize_ms(double *const *W, const int64_t *rows, int N, int R, double *Gall,
                    double *ms_dst, const unsigned *masks, unsigned active, unsigned fresh,
                    double *wsq) override {
    RoctxRange roctx_("K7 normalize");
    int64_t tot = 0;
    for (int i = 0; i < N; i++) tot += rows[i] * R;
    if (tot > 65536) {  // big factors: the grid-wide scaling kernel pays off
      Ops::normalize_ms(W, rows, N, R, Gall, ms_dst, masks, active, fresh, wsq);
      return;
    }
    PtrsN w;
    for (int i = 0; i < N; i++) {
      w.p[i] = W[i];
      w.n[i] = rows[i] * R;
    }
    ScaleMasks sm;
    for (int k = 0; k < 32; k++) sm.m[k] = masks ? masks[k] : 0u;
    route("%s", "normalize.fused");
    hipLaunchKernelGGL(k_normalize_fused, dim3(1), dim3(1024), 0, st_, Gall, N, R, w,
                       small(MAX_ORDER), active ? ms_dst : nullptr, sm, active, fresh, wsq);
    HIP_CHECK(hipGetLastError());
  }
  void diff_norms(double *const *A, double *const *B, const int64_t *n, int N, int store_diff,
                  double *const *D, int update_prev, double *out) override {
    PtrsN a;
    for (int i = 0; i < N; i++) {
      a.p[i] = A[i];
      a.q[i] = B ? B[i] : nullptr;
      a.d[i] = D ? D[i] : nullptr;
      a.n[i] = n[i];
    }
    hipLaunchKernelGGL(k_diff_norms, dim3(N), dim3(1024), 0, st_, a, store_diff, update_prev, out);
    HIP_CHECK(hipGetLastError());
  }
  void pack_blocks(const double *nat, int64_t rows, int64_t ld, int R, int64_t blk, int P,
                   double *blocked) override {
    hipLaunchKernelGGL(k_pack_blocks, dim3(grid_for(blk * R * P, 256)), dim3(256), 0, st_, nat,
                       rows, ld, R, blk, P, blocked);
    HIP_CHECK(hipGetLastError());
  }
  void unpack_blocks(const double *blocked, int64_t rows, int64_t ld, int R, int64_t blk, int P,
                     double *nat) override {
    hipLaunchKernelGGL(k_unpack_blocks, dim3(grid_for(blk * R * P, 256)), dim3(256), 0, st_,
                       blocked, rows, ld, R, blk, P, nat);
    HIP_CHECK(hipGetLastError());
  }
  // K12/K13: Gram of the mode unfolding (fp64 accumulation), reduction split over grid.z slabs
  void unfold_gram(const void *X, int dt, int64_t L, int64_t J, int64_t T, double *G) override {
    RoctxRange roctx_("K12/K13 unfold gram");
    const int64_t C = L * T;
    if (dt == F64 && J >= 64 && J <= 8192 && C >= 16 && C <= 4096 &&
        (double)J * (double)C * 8.0 <= 64e6) {
      // the Gram of a HOOI leaf (a few hundred rows and columns): the latency-bound symmetric
      // product of the eigen-step (one 16 x 16 tile per workgroup, 8 waves split the columns) on
      // the unfolding with the mode in front — 8 us instead of 31 at cfg5
      const double *A = (const double *)X;
      if (L > 1) {
        double *Ym = (double *)ensure(ws_big2_, ws_big2_sz_, sizeof(double) * (size_t)J * C);
        transpose_batched(X, F64, L, J, T, Ym);
        A = Ym;
      }
      route("unfold_gram.sym transposed=%d lds=%d", L > 1 ? 1 : 0, (int)J >= sym_lds_min_ ? 1 : 0);
      prof_begin(1, (double)C * J * 8.0);
      sym_product(A, J, A, J, nullptr, 0, G, J, (int)J, (int)C, 1.0, 0.0);
      prof_end();
      HIP_CHECK(hipGetLastError());
      return;
    }
    if (dt == F32 && J >= 64 && C >= 4096 &&
        ((L == 1 && J % 4 == 0) || (L > 1 && L % 4 == 0))) {
      // K13 at size (the HOSVD Grams of the full tensor): the tiled SYRK, upper triangle only
      const int nt = (int)((J + 63) / 64);
      const int ntri = nt * (nt + 1) / 2;
      // (three workgroups per CU are resident — 134 registers, 40 KB of LDS —: the split is rounded DOWN
      // so that tiles x splits fit one round; rounded up, cfg5's 28 x 28 = 784 workgroups ran as 768 +
      // 16, i.e. two rounds: 1.10 ms per Gram)
      const int want = (int)std::min<int64_t>(std::max<int64_t>(1, ((int64_t)ncu_ * 3) / ntri),
                                              std::max<int64_t>(1, C / 1024));
      const KSplit ks = k_split(C, std::min(want, 512), 1, 32);
      double *dst = pass_dst(ks.nsplit, J * J, 1, 1, G, 0, 0, 0, RowPad()).p;
      route("unfold_gram.syrk nsplit=%d", ks.nsplit);
      prof_begin(1, (double)C * J * dtype_size(dt));
      hipLaunchKernelGGL(k_unfold_syrk_f32, dim3((unsigned)ntri, 1, (unsigned)ks.nsplit), dim3(256), 0, st_,
                         (const float *)X, L, J, T, ks.per, dst);
      prof_end();
      HIP_CHECK(hipGetLastError());
      slab_combine(ks.nsplit, dst, J * J, J * J, 1, G, 1, 0, 0);
      return;
    }
    const int tiles = (int)((J + 31) / 32);
    int want = 1;
    const int64_t target = (int64_t)ncu_ * 4;
    if ((int64_t)tiles * tiles < target) want = (int)std::min<int64_t>(
        (target + (int64_t)tiles * tiles - 1) / ((int64_t)tiles * tiles), std::max<int64_t>(1, C / 256));
    const KSplit ks = k_split(C, std::min(want, 1024), 1, 32);
    const int nsplit = ks.nsplit;
    const int64_t per = ks.per;
    double *dst = pass_dst(nsplit, J * J, 1, 1, G, 0, 0, 0, RowPad()).p;
    dim3 grid(tiles, tiles, nsplit);
    route("unfold_gram.%s.%s nsplit=%d", J >= 16 ? "mfma" : "valu", dt == F32 ? "f32" : "f64", nsplit);
    prof_begin(1, (double)C * J * dtype_size(dt));
    if (J >= 16) {  // matrix cores (K13); tiny modes: the VALU tile kernel
      if (dt == F32)
        hipLaunchKernelGGL(k_unfold_gram_mfma<float>, grid, dim3(256), 0, st_, (const float *)X, L, J,
                           T, per, dst);
      else
        hipLaunchKernelGGL(k_unfold_gram_mfma<double>, grid, dim3(256), 0, st_, (const double *)X, L,
                           J, T, per, dst);
    } else if (dt == F32)
      hipLaunchKernelGGL(k_unfold_gram<float>, grid, dim3(256), 0, st_, (const float *)X, L, J, T,
                         per, dst);
    else
      hipLaunchKernelGGL(k_unfold_gram<double>, grid, dim3(256), 0, st_, (const double *)X, L, J,
                         T, per, dst);
    prof_end();
    HIP_CHECK(hipGetLastError());
    slab_combine(nsplit, dst, J * J, J * J, 1, G, 1, 0, 0);
  }
  // Leading eigenvectors of the s x s Gram (the reference's MTM.svd(U,S,VT,rank),
  // als_Tucker.cxx:20,402). SURVEY.md §2.1 K12 allows the vendor symmetric eigensolver here:
  // rocSOLVER dsyevd, resolved with dlopen on first use (only Tucker sessions ever load it).
  void top_eigvecs(double *G, int64_t J, int rank, double *U) override {
    RoctxRange roctx_("K12 eig (full solver)");
    if (J <= 64) {  // small modes: in-LDS Jacobi, one block
      route("%s", "eig.full.lds_jacobi");
      launch_top_eig_small(G, (int)J, rank, U, nullptr);
      HIP_CHECK(hipGetLastError());
      return;
    }
    if (J <= kJacobiBigMax) {
      // 64 < J <= 128 (the small side of a tall unfolding at core ranks 70-100, a short mode): the
      // whole eigen-decomposition by the one-workgroup one-sided Jacobi, no vendor library
      route("%s", "eig.full.onesided_jacobi");
      double *w = (double *)ensure(ws_jac_, ws_jac_sz_, sizeof(double) * (2 * (size_t)J * J + 2 * J));
      double *Vt = w, *Y = Vt + J * J, *evd = Y + J * J, *D = evd + J;
      const size_t lds = sizeof(double) * ((size_t)J * (J + 1) + 256) + sizeof(int) * 256;
      hipLaunchKernelGGL(k_jacobi_onesided, dim3(1), dim3(1024), lds, st_, G, (int)J, Vt, Y, evd, (double *)nullptr);
      HIP_CHECK(hipMemcpyAsync(U, Y, sizeof(double) * J * rank, hipMemcpyDeviceToDevice, st_));
      // (eig_bootstrap reads the eigenvalues ASCENDING from the start of ws_krp_, as dsyevd leaves them)
      double *Dk = (double *)ensure(ws_krp_, ws_krp_sz_, sizeof(double) * (2 * J + 2));
      hipLaunchKernelGGL(k_reverse_copy, dim3(1), dim3(256), 0, st_, evd, (int)J, Dk);
      (void)D;
      HIP_CHECK(hipGetLastError());
      return;
    }
    route("%s", "eig.full.dsyevd");
    RocSolver &rs = rocsolver();
    double *D = (double *)ensure(ws_krp_, ws_krp_sz_, sizeof(double) * (2 * J + 2));
    double *E = D + J;
    int *info = (int *)(E + J);
    int rc = rs.dsyevd(rs.handle, 211 /*evect_original*/, 121 /*fill_upper*/, (int)J, G, (int)J, D,
                       E, info);
    if (rc != 0) throw std::runtime_error("ppals: rocsolver_dsyevd failed");
    hipLaunchKernelGGL(k_take_top, dim3(grid_for(J * rank, 256)), dim3(256), 0, st_, G, J, rank, U);
    HIP_CHECK(hipGetLastError());
  }
  static constexpr int kTailBlocks = 64;
  // the one read-back of a projector step (layout: kernels_eig.hip.h, kEigOff*)
  static_assert(kTailBlocks == 64, "residual shares: 64 words");
  static constexpr size_t kEE = (size_t)kEigEvMax * kEigEvMax;  // a (rank + wide)^2 scratch matrix
  static constexpr size_t kEigReadback = sizeof(double) * kEigChkDoubles;
  // ---- K12 inside a HOOI iteration: spectral projector by the scaled Newton-Schulz sign iteration
  // (kernels_eig.hip.h), warm-started per slot, verified by trace(P) == rank, else the full solver.
  struct EigState {
    int64_t J = 0;
    int rank = 0;
    bool valid = false;
    double lamR = 0, lamR1 = 0, rho = 0;  // rank-th / next eigenvalue, largest eigenvalue
    double rho_frob = 0;  // 1.0001 ||G - deflation - sigma I||_F of the last projector step (0: none)
    double head = 4.0;    // head room of the spectral-bound scale (projector_step, fused form)
    double dom_move = -1;  // sine between the dominant eigenvector of the last two steps (< 0: not measured)
    // lazy Rayleigh-Ritz (eig_lazy): the Jacobi of H runs on the second stream
    bool lazy = false;          // the session allows it for this slot
    bool lazy_pending = false;  // eigenvalues of the last step still to be read (evd)
    bool rot_pending = false;   // the caller has not applied Y yet
    int lazy_m = 0;
    bool lazy_strict = false;
    bool jacobi_launched = false;
    double *Hd = nullptr, *Yd = nullptr, *evd = nullptr;  // 64*64, 64*64, 64 (device)
    double *ev_pinned = nullptr;  // 64 doubles of pinned host memory the Jacobi writes directly
    hipEvent_t ev_h = nullptr, ev_done = nullptr;
    double *Q = nullptr;                  // previous basis (J x rank)
    double *Qn = nullptr;                 // spare buffer of the same size (the step's result lands here)
    double evh[kEigEvMax] = {0};          // eigenvalues of the last accepted step (descending)
    int fast = 0, full = 0;
    // deferred acceptance (eig_defer / eig_verify): the step's read-back lands in the slot's own
    // pinned block behind ev_chk; what the checks need from the time of the call is kept in `dp`
    bool defer = false;     // the session allows it for this slot
    int stable = 0;         // consecutive steps accepted at the first attempt, as scheduled
    bool deferred = false;  // a step is waiting for eig_verify
    double *chk_pinned = nullptr;
    hipEvent_t ev_chk = nullptr;
    double *GBd = nullptr, *chkd = nullptr;  // G*B (J x rank) and the checks' device block, the slot's own
    double *Gd = nullptr;                    // the slot's own Gram (eig_gram): the second stream reads it
    size_t GBd_elems = 0, Gd_elems = 0;
    struct {
      double sigma = 0, rho = 0, ell0 = 0;
      int m = 0, iters = 0, pow = 0;
    } dp;
    int n_deferred = 0, n_defer_failed = 0;
  };
  // The symmetric product C = alpha A Bt^T + beta D of the sign iteration (and of the leaf Grams),
  // by size: a few hundred rows are a latency problem — one 16 x 16 tile per workgroup, eight waves
  // splitting K — from sym_lds_min_ rows on (PPALS_SYM_LDS_MIN, 768: tools/nsprod_bench.hip,
  // profiles/r04d_nsprod_*.txt: 640 rows 18.6 vs 21.3 us, 896 rows 35.6 vs 30.8, 1344 rows 88.6 vs
  // 68.1) it is 2 J^3 flops — 32 x 32 tiles staged through LDS. sym_tiles() = workgroups = check-sum
  // partials per product.
  // (the GEMM kernels address their operands with 32-bit element offsets)
  static void gemm_offsets_fit(int64_t lda, int64_t ca, int64_t ldb, int64_t cb) {
    if ((double)lda * (double)ca >= 4.0e9 || (double)ldb * (double)cb >= 4.0e9)
      throw std::runtime_error("ppals: dense operand of the eigen-step beyond 2^32 elements");
  }
  unsigned sym_tiles(int M) const {
    const unsigned nt = (unsigned)((M + (M >= sym_lds_min_ ? 31 : 15)) / (M >= sym_lds_min_ ? 32 : 16));
    return nt * (nt + 1) / 2;
  }
  void sym_product(const double *A, int64_t lda, const double *Bt, int64_t ldb, const double *D, int64_t ldd,
                   double *C, int64_t ldc, int M, int K, double alpha, double beta, int chk_mode = 0,
                   double *chk_part = nullptr) {
    gemm_offsets_fit(lda, K, ldb, K);
    if (M >= sym_lds_min_)
      hipLaunchKernelGGL(k_dgemm_nt_sym_lds<32>, dim3(sym_tiles(M)), dim3(256), 0, st_, A, lda, Bt, ldb, D, ldd, C,
                         ldc, M, K, alpha, beta, chk_mode, chk_part);
    else
      hipLaunchKernelGGL(k_dgemm_nt_sym<8>, dim3(sym_tiles(M)), dim3(512), 0, st_, A, lda, Bt, ldb, D, ldd, C, ldc,
                         M, K, alpha, beta, chk_mode, chk_part);
  }
  void gemm_nt(const double *A, int64_t lda, const double *Bt, int64_t ldb, const double *D,
               int64_t ldd, double *C, int64_t ldc, int M, int N, int K, double alpha, double beta) {
    gemm_offsets_fit(lda, K, ldb, K);
    dim3 grid((unsigned)((M + 15) / 16), (unsigned)((N + 15) / 16));
    hipLaunchKernelGGL(k_dgemm_nx<false>, grid, dim3(256), 0, st_, A, lda, Bt, ldb, D, ldd, C, ldc, M,
                       N, K, alpha, beta);
  }
  // in-LDS eigen-decomposition of a small symmetric matrix (J <= 64) by one workgroup: a thread
  // per element when there are that many (two barriers per Jacobi round whatever the size)
  void launch_top_eig_small(const double *G, int J, int rank, double *U, double *evals) {
    // (a thread per element up to 15 waves, plus the wave that prepares the next round's angles)
    const int nthr = std::min(1024, std::max(192, (J * J + 63) / 64 * 64) + 64);
    hipLaunchKernelGGL(k_top_eig_small, dim3(1), dim3(nthr), top_eig_small_lds(J), st_, G, J, rank, U,
                       evals);
  }
  // the same with the second operand as it is (K x N, column-major): thin tails, no transposition
  void gemm_nn(const double *A, int64_t lda, const double *B, int64_t ldb, const double *D,
               int64_t ldd, double *C, int64_t ldc, int M, int N, int K, double alpha, double beta,
               const double *Qov = nullptr, int mov = 0, hipStream_t st = nullptr) {
    gemm_offsets_fit(lda, K, ldb, N);
    dim3 grid((unsigned)((M + 15) / 16), (unsigned)((N + 15) / 16));
    hipLaunchKernelGGL(k_dgemm_nx<true>, grid, dim3(256), 0, st ? st : st_, A, lda, B, ldb, D, ldd, C, ldc,
                       M, N, K, alpha, beta, Qov, mov);
  }
  // full solver + what the next call of the slot needs (rank-th and next eigenvalue, the basis)
  void eig_bootstrap(EigState &es, double *G, int64_t J, int rank, double *U) {
    // ||G||_F^2 = sum of squared eigenvalues: taken before dsyevd overwrites G
    top_eigvecs(G, J, rank, U);
    es.full++;
    if (J <= 64 || rank >= J || rank + 16 > kEigEvMax) {
      es.valid = false;
      return;
    }
    // dsyevd left the ascending eigenvalues in ws_krp_ (D)
    double lam[kEigEvMax + 1];
    const double *D = (const double *)ws_krp_;
    HIP_CHECK(hipMemcpyAsync(lam, D + (J - rank - 1), (rank + 1) * sizeof(double),
                             hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipStreamSynchronize(st_));
    es.lamR1 = lam[0];
    es.lamR = lam[1];
    for (int d = 0; d < rank; d++) es.evh[d] = lam[rank - d];  // descending
    es.rho = lam[rank];
    if (!es.Q || es.J != J || es.rank != rank) {
      if (es.Q) hipFree(es.Q);
      if (es.Qn) hipFree(es.Qn);
      HIP_CHECK(hipMalloc(&es.Q, sizeof(double) * J * rank));
      HIP_CHECK(hipMalloc(&es.Qn, sizeof(double) * J * rank));
    }
    es.J = J;
    es.rank = rank;
    HIP_CHECK(hipMemcpyAsync(es.Q, U, sizeof(double) * J * rank, hipMemcpyDeviceToDevice, st_));
    es.rho_frob = 0;  // the next projector step reads its norm once
    es.head = 4.0;
    es.valid = es.lamR > 0 && es.lamR1 >= 0 && es.lamR > es.lamR1 * (1 + 1e-9);
  }
  // Z (J x r) -> orthonormal columns, Cholesky QR twice (status 2 of a pass = "far from
  // orthonormal" is no failure here: the second pass repairs it); returns the buffer holding the
  // result. npass = 1: for a Z that is close to orthonormal already — the caller must treat ANY
  // non-zero status as a failure then.
  double *chol_qr2(double *cur, double *nxt, int64_t J, int r, double *C, int *status,
                   int npass = 2) {
    if (r > 64) {
      // more columns than the one-wave Cholesky holds (core ranks above 48, test_ALS.cxx:366-379):
      // block Gram-Schmidt, 64 columns at a time, in place — its own read-back says whether it held
      route("chol_qr2.blocks r=%d", r);
      const int st[2] = {orthonormalize(cur, J, r) ? 0 : 1, 0};
      HIP_CHECK(hipMemcpyAsync(status, st, sizeof(int) * std::min(npass, 2), hipMemcpyHostToDevice, st_));
      HIP_CHECK(hipStreamSynchronize(st_));
      return cur;
    }
    // R^-1 by ONE elimination of [C | I] on a whole workgroup (k_chol_m: two pivots per barrier, all
    // 2 r^2 elements of a step in parallel) instead of the one-wave Cholesky + column-wise substitution
    // (k_chol_rinv: 175 us a call at 64 columns, 1.8 ms of a time-lapse HOOI sweep; round 6)
    const size_t lds_m = sizeof(double) * (4 * (size_t)r * r + r + 8);
    double *Minv = (double *)ensure(ws_cholm_, ws_cholm_sz_, sizeof(double) * 64 * 64);
    for (int pass = 0; pass < npass; pass++) {
      hipLaunchKernelGGL(k_tn_small, dim3((r * r + 15) / 16), dim3(1024), 0, st_, cur, cur, J, r, C);
      hipLaunchKernelGGL(k_chol_m, dim3(1), dim3(k_chol_threads(r)), lds_m, st_, cur, (const double *)nullptr, J, r, 0,
                         (const double *)C, Minv, status + pass);
      hipLaunchKernelGGL(k_right_mult, dim3(grid_for(J * r, 256)), dim3(256),
                         sizeof(double) * r * r, st_, cur, J, r, Minv, nxt);
      std::swap(cur, nxt);
    }
    return cur;
  }
  // block Gram-Schmidt with re-orthogonalisation: 64 columns at a time are cleared of the columns
  // before them (twice) and made orthonormal by Cholesky QR (twice)
  bool orthonormalize(double *U, int64_t rows, int r) override {
    if (r <= 0) return true;
    if (r > 2048) throw std::runtime_error("ppals: orthonormalize supports at most 2048 columns");
    const int nblk = (r + 63) / 64;
    route("orthonormalize nblk=%d", nblk);
    double *w = (double *)ensure(ws_orth_, ws_orth_sz_,
                                 sizeof(double) * ((size_t)rows * 64 + 64 * 64 + (size_t)r * 64) +
                                     sizeof(int) * 2 * 64);
    double *tmp = w, *C = tmp + (size_t)rows * 64, *T = C + 64 * 64;
    int *status = (int *)(T + (size_t)r * 64);
    HIP_CHECK(hipMemsetAsync(status, 0, sizeof(int) * 2 * nblk, st_));
    for (int b = 0; b < nblk; b++) {
      const int b0 = b * 64, rb = std::min(64, r - b0);
      double *Zb = U + (size_t)rows * b0;
      for (int pass = 0; pass < 2 && b0 > 0; pass++) {
        hipLaunchKernelGGL(k_tn_rect, dim3((b0 * rb + 15) / 16), dim3(1024), 0, st_, U, b0, Zb, rb,
                           rows, T);
        hipLaunchKernelGGL(k_sub_mult, dim3(grid_for(rows * rb, 256)), dim3(256), 0, st_, Zb, rows,
                           rb, U, b0, T);
      }
      double *res = chol_qr2(Zb, tmp, rows, rb, C, status + 2 * b);  // two passes: ends in Zb
      if (res != Zb) throw std::logic_error("ppals: orthonormalize buffer parity");
    }
    int hs[2 * 32];
    HIP_CHECK(hipMemcpyAsync(hs, status, sizeof(int) * 2 * nblk, hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipStreamSynchronize(st_));
    for (int b = 0; b < nblk; b++)  // first pass: 2 = "far from orthonormal" is what the second is for
      if (hs[2 * b] == 1 || hs[2 * b + 1] != 0) return false;
    return true;
  }
  // Rayleigh-Ritz of G on the orthonormal basis B (J x r): U = eigenvectors sorted descending,
  // ev (device) = eigenvalues; GB/H/Yr/Bt scratch. Leaves G*U in GU when GU != nullptr.
  void rayleigh_ritz(const double *G, const double *B, int64_t J, int r, double *Bt, double *GB,
                     double *H, double *Yr, double *U, double *ev, double *GU) {
    transpose2d(B, F64, J, r, Bt);
    gemm_nt(G, J, Bt, r, nullptr, 0, GB, J, (int)J, r, (int)J, 1.0, 0.0);
    if (r > 64) {
      // above the in-LDS two-sided Jacobi: H = B^T (G B) and the products with Y on the matrix
      // cores, the eigen-decomposition of H by the one-workgroup one-sided Jacobi (r <= 128)
      if (r > kJacobiBigMax) throw std::runtime_error("ppals: Rayleigh-Ritz supports at most 128 columns");
      gemm_nn(Bt, r, GB, J, nullptr, 0, H, r, r, r, (int)J, 1.0, 0.0);
      double *Vt = (double *)ensure(ws_jac_, ws_jac_sz_, sizeof(double) * (size_t)r * r);
      const size_t lds = sizeof(double) * ((size_t)r * (r + 1) + 256) + sizeof(int) * 256;
      hipLaunchKernelGGL(k_jacobi_onesided, dim3(1), dim3(1024), lds, st_, H, r, Vt, Yr, ev, (double *)nullptr);
      gemm_nn(B, J, Yr, r, nullptr, 0, U, J, (int)J, r, r, 1.0, 0.0);
      if (GU) gemm_nn(GB, J, Yr, r, nullptr, 0, GU, J, (int)J, r, r, 1.0, 0.0);
      return;
    }
    hipLaunchKernelGGL(k_tn_small, dim3((r * r + 15) / 16), dim3(1024), 0, st_, B, GB, J, r, H);
    launch_top_eig_small(H, r, r, Yr, ev);
    hipLaunchKernelGGL(k_right_mult, dim3(grid_for(J * r, 256)), dim3(256),
                       sizeof(double) * r * r, st_, B, J, r, Yr, U);
    if (GU)
      hipLaunchKernelGGL(k_right_mult, dim3(grid_for(J * r, 256)), dim3(256),
                         sizeof(double) * r * r, st_, GB, J, r, Yr, GU);
  }
  // Small modes (16 <= J <= 64: the in-LDS Jacobi, 1 ms at J = 50 from a cold start — 15 % of an
  // order-6 s = 50 HOOI sweep): the Jacobi runs on H = Q^T G Q with Q the slot's previous
  // eigenvector matrix. G changes little from sweep to sweep, so H is nearly diagonal and the
  // cyclic Jacobi (quadratically convergent) needs 2-3 sweeps instead of ~8; the result Q Y is
  // the same eigen-decomposition, with no assumption about gaps. Every 64th call starts cold
  // (the product Q Y accumulates rounding in its orthogonality).
  struct SmallEig {
    int64_t J = 0;
    double *Q = nullptr;  // J x J, ranked descending
    bool valid = false;
    int age = 0;
  };
  std::map<int, SmallEig> eig_small_;  // by slot (session base + mode, see eig_session_new)
  void top_eigvecs_small_warm(double *G, int64_t J, int rank, double *U, int slot) {
    SmallEig &sm = eig_small_[slot];
    const int Ji = (int)J;
    const size_t nJJ = (size_t)J * J;
    if (sm.J != J) {
      if (sm.Q) hipFree(sm.Q);
      HIP_CHECK(hipMalloc(&sm.Q, sizeof(double) * nJJ));
      sm.J = J;
      sm.valid = false;
    }
    if (!sm.valid || ++sm.age >= 64) {
      route("%s", "eig.small cold=1");
      launch_top_eig_small(G, Ji, Ji, sm.Q, nullptr);
      sm.valid = true;
      sm.age = 0;
    } else {
      route("%s", "eig.small cold=0");
      double *w = (double *)ensure(ws_eig_, ws_eig_sz_, sizeof(double) * 5 * nJJ);
      double *Qt = w, *C1 = Qt + nJJ, *H = C1 + nJJ, *Y = H + nJJ, *Qn = Y + nJJ;
      transpose2d(sm.Q, F64, J, J, Qt);
      gemm_nt(G, J, Qt, J, nullptr, 0, C1, J, Ji, Ji, Ji, 1.0, 0.0);  // G Q
      hipLaunchKernelGGL(k_tn_small, dim3((Ji * Ji + 15) / 16), dim3(1024), 0, st_, sm.Q, C1, J, Ji, H);
      launch_top_eig_small(H, Ji, Ji, Y, nullptr);
      hipLaunchKernelGGL(k_right_mult, dim3(grid_for(J * J, 256)), dim3(256), sizeof(double) * nJJ, st_,
                         sm.Q, J, Ji, Y, Qn);
      HIP_CHECK(hipMemcpyAsync(sm.Q, Qn, sizeof(double) * nJJ, hipMemcpyDeviceToDevice, st_));
    }
    HIP_CHECK(hipMemcpyAsync(U, sm.Q, sizeof(double) * J * rank, hipMemcpyDeviceToDevice, st_));
    HIP_CHECK(hipGetLastError());
  }
  void top_eigvecs_warm(double *G, int64_t J, int rank, double *U, int slot) override {
    RoctxRange roctx_("K12 eig (projector route)");
    if (J >= 16 && J <= 64 && rank <= J && slot >= 0 && eig_fast_) {
      top_eigvecs_small_warm(G, J, rank, U, slot);
      return;
    }
    // (up to core rank 112: rank + 16 columns of a wide tail / cold start must fit kEigEvMax)
    if (J <= 64 || rank + 16 > kEigEvMax || rank + 16 >= J || slot < 0 || !eig_fast_) {
      route("eig.warm.direct why=%s", J <= 64 ? "J" : rank + 16 > kEigEvMax ? "rank_max" : rank + 16 >= J ? "rank_J"
                                                    : slot < 0 ? "slot" : "fast");
      top_eigvecs(G, J, rank, U);
      return;
    }
    EigState &es = eig_state_[slot];
    resolve_lazy(es);
    es.rot_pending = false;  // (whatever rotation was owed belonged to the factor this call replaces)
    if (es.valid && (es.J != J || es.rank != rank)) es.valid = false;
    if (es.valid && projector_step(es, G, J, rank, U, slot, false)) return;
    if (es.valid) {  // the spectral bound may have been outrun: once more on the measured norm
      route("%s", "eig.warm.frob_retry");
      eig_frob_once_ = true;
      const bool ok = projector_step(es, G, J, rank, U, slot, false);
      eig_frob_once_ = false;
      if (ok) {
        es.head = 8.0;
        return;
      }
    }
    // nothing known about this matrix (first call of the slot, a shift that no longer separates
    // the wanted eigenvalues): a few steps of block subspace iteration place the shift, the same
    // projector step — checked against machine precision, not against an estimated gap — delivers
    // the eigenpairs; the full solver remains the fallback of the fallback
    if (eig_cold_) {
      const bool ritz_ok = cold_ritz_state(es, G, J, rank, slot);
      route("eig.cold.ritz ok=%d", ritz_ok ? 1 : 0);
      if (ritz_ok) {
        // (long modes: thin products instead of ~46 products of J^3; kColdSubspaceFrom: where a J^3
        // product, 7.4 us at J = 400, stops being cheap against a step of thin products + Rayleigh-Ritz)
        if (J >= cold_subspace_from_ && cold_subspace(es, G, J, rank, U, slot)) {
          route("%s", "eig.cold.subspace");
          return;
        }
        if (projector_step(es, G, J, rank, U, slot, true)) return;
      }
      // a flat spectrum around the cut (the Gram of a noise tensor: the HOSVD initialisation), where
      // Ritz values cannot place the shift: place it by COUNTING eigenvalues with the sign iteration
      if (cold_ok_ && cold_bisect(es, G, J, rank, U, slot)) {
        route("%s", "eig.cold.bisect");
        return;
      }
    }
    route("%s", "eig.warm.bootstrap");
    es.valid = false;
    if (eig_debug_)
      fprintf(stderr, "[ppals eig] slot %d J %lld rank %d: full solver (%s)\n", slot, (long long)J, rank,
              J <= kJacobiBigMax ? "one-sided Jacobi, one workgroup" : "dsyevd");
    eig_bootstrap(es, G, J, rank, U);
  }
  // Warm-start state belongs to the SESSION that made it: a session draws a block of 64 slots
  // here and gives it back when it ends, so sessions that alternate on one context (or the thin
  // c x c route and its s x s fallback inside one factor update, which use different slots of the
  // block) never see each other's bases, gaps or eigenvalue scales.
  void free_lazy(EigState &es) {
    if (st2_) hipStreamSynchronize(st2_);  // (nothing on the second stream reads the slot's buffers any more)
    if (es.Hd) hipFree(es.Hd);
    if (es.Yd) hipFree(es.Yd);
    if (es.evd) hipFree(es.evd);
    if (es.ev_pinned) hipHostFree(es.ev_pinned);
    es.ev_pinned = nullptr;
    if (es.chk_pinned) hipHostFree(es.chk_pinned);
    es.chk_pinned = nullptr;
    if (es.ev_chk) hipEventDestroy(es.ev_chk);
    es.ev_chk = nullptr;
    if (es.GBd) hipFree(es.GBd);
    if (es.chkd) hipFree(es.chkd);
    if (es.Gd) hipFree(es.Gd);
    es.GBd = es.chkd = es.Gd = nullptr;
    es.GBd_elems = es.Gd_elems = 0;
    if (es.ev_h) hipEventDestroy(es.ev_h);
    if (es.ev_done) hipEventDestroy(es.ev_done);
    es.Hd = es.Yd = es.evd = nullptr;
    es.ev_h = es.ev_done = nullptr;
  }
  // second stream, events and the slot's buffers: set up when a session ASKS for lazy steps (its
  // set-up), not inside the first timed sweep
  void lazy_prepare(EigState &es) {
    if (!st2_) HIP_CHECK(hipStreamCreateWithFlags(&st2_, hipStreamNonBlocking));
    if (!handover_) {
      // (zero BEFORE any stream can wait on it: a recycled allocation may hold a larger sequence number)
      HIP_CHECK(hipMalloc(&handover_, 16));
      HIP_CHECK(hipMemset(handover_, 0, 16));
      HIP_CHECK(hipDeviceSynchronize());
      // A runtime without stream memory operations, or one on which a value stored by a KERNEL is not
      // seen by the waiting stream, gets the event hand-over instead. The probe is the real thing once:
      // a one-workgroup kernel on the sweep's stream publishes 1, the second stream waits for it and
      // records an event, which must arrive within a deadline. If it does not, the second stream is
      // released from the host and the flag is never waited on again.
      if (handover_ok_) {
        hipEvent_t probe = nullptr;
        bool ok = hipEventCreateWithFlags(&probe, hipEventDisableTiming) == hipSuccess;
        ok = ok && hipStreamWaitValue64(st2_, handover_, 1, hipStreamWaitValueGte, 0xFFFFFFFFFFFFFFFFull) == hipSuccess;
        if (ok) {
          ok = hipEventRecord(probe, st2_) == hipSuccess;
          hipLaunchKernelGGL(k_handover_probe, dim3(1), dim3(64), 0, st_, handover_, 1ull);
          ok = ok && hipGetLastError() == hipSuccess;
          const auto t0 = std::chrono::steady_clock::now();
          bool arrived = false;
          while (ok && !arrived) {
            const hipError_t q = hipEventQuery(probe);
            if (q == hipSuccess) arrived = true;
            else if (q != hipErrorNotReady) ok = false;
            else if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(500)) break;
          }
          if (!arrived) {
            // release the waiting stream whatever went wrong (the wait is queued already)
            const unsigned long long one = 1;
            (void)hipMemcpy(handover_, &one, sizeof one, hipMemcpyHostToDevice);
            (void)hipStreamSynchronize(st2_);
            ok = false;
          }
        }
        if (probe) hipEventDestroy(probe);
        (void)hipGetLastError();
        if (!ok) handover_ok_ = false;
        handover_seq_ = 1;  // (sequence numbers go on from the probe's)
      }
    }
    if (!es.Hd) {
      HIP_CHECK(hipMalloc(&es.Hd, sizeof(double) * 64 * 64));
      HIP_CHECK(hipMalloc(&es.Yd, sizeof(double) * 64 * 64));
      HIP_CHECK(hipMalloc(&es.evd, sizeof(double) * 64));
      HIP_CHECK(hipHostMalloc(&es.ev_pinned, sizeof(double) * 64, hipHostMallocDefault));
      HIP_CHECK(hipEventCreateWithFlags(&es.ev_h, hipEventDisableTiming));
      HIP_CHECK(hipEventCreateWithFlags(&es.ev_done, hipEventDisableTiming));
      HIP_CHECK(hipHostMalloc(&es.chk_pinned, kEigReadback, hipHostMallocDefault));
      HIP_CHECK(hipEventCreateWithFlags(&es.ev_chk, hipEventDisableTiming));
      HIP_CHECK(hipMalloc(&es.chkd, kEigReadback));
    }
  }
  void eig_lazy(int slot, bool on) override {
    if (slot < 0) return;
    EigState &es = eig_state_[slot];
    es.lazy = on;
    if (es.lazy) lazy_prepare(es);
  }
  void eig_defer(int slot, bool on) override {
    if (slot < 0) return;
    eig_state_[slot].defer = on && eig_defer_ok_;
  }
  // The slot's own Gram buffer. A deferred step leaves G B, H = B^T G B and the residual to the
  // second stream, which reads G long after the sweep's stream has moved on to the next mode — so
  // the Gram of a deferring slot must not live in the caller's shared workspace. Whatever the
  // second stream still owes this slot is waited for here (the wait resolve_lazy() would do a
  // moment later), before the caller overwrites the buffer.
  double *eig_gram(int slot, int64_t J) override {
    if (slot < 0 || J > 4096) return nullptr;
    auto it = eig_state_.find(slot);
    if (it == eig_state_.end() || !it->second.defer || !it->second.lazy) return nullptr;
    EigState &es = it->second;
    if (es.jacobi_launched) HIP_CHECK(hipEventSynchronize(es.ev_done));
    if (es.Gd_elems < (size_t)(J * J)) {
      if (es.Gd) HIP_CHECK(hipFree(es.Gd));
      HIP_CHECK(hipMalloc(&es.Gd, sizeof(double) * (size_t)(J * J)));
      es.Gd_elems = (size_t)(J * J);
    }
    return es.Gd;
  }
  // What decides whether a projector step's result is accepted, from its one read-back `hc`
  // (chk[16] | evW[64] | status[8 ints] | lamD[64] | per-workgroup residual shares, already summed
  // into hc[4]) and the quantities the step was scheduled with.
  struct StepCheck {
    bool converged = false, good = false;
    double cnt = 0, res = 0, rho_now = 0, gap_now = 0, res_tol = 0;
  };
  StepCheck check_step(const double *hc, int64_t J, int rank, double sigma, double rho, bool strict,
                       bool fused_tail, bool fused_scale, bool lazy_used) const {
    StepCheck c;
    const double *evn = hc + 16;
    const int *hs = (const int *)(hc + kEigOffStatus);
    c.cnt = 0.5 * (hc[1] + (double)J);
    c.res = std::sqrt(hc[4]);
    c.rho_now = fused_scale ? rho : 1.0001 * std::sqrt(hc[8]);
    // (fused tail: hc[0] is ||E||_F^2 of the iterate BEFORE the last step, E = X^2 - I; the step
    // squares it — E_new = (3 E^2 + E^3) / 4 — so ||E_new||_F <= ||E||_F^2 = hc[0])
    c.converged = fused_tail ? hc[0] <= 1e-10 * std::sqrt((double)J) : hc[0] <= 1e-20 * (double)J;
    // accepted when the eigenpair residual is at the level the full solver reaches: 1e-9 of the
    // gap (projector error <= 1e-9), or the rounding floor eps * lambda_1 of any method
    // (from THIS step's quantities only: trace(P) == rank says that exactly `rank` eigenvalues
    // lie above this step's shift, so the gap below the rank-th one is at least its distance to
    // the shift; the slot's previous gap / eigenvalue scale only scheduled the iteration)
    // (lazy tail: the Jacobi has not run yet — Gershgorin bounds of H's spectrum stand in for
    // the smallest / largest eigenvalue of the subspace, and the residual is the subspace's)
    const double ev_lo = lazy_used ? hc[5] : evn[rank - 1], ev_hi = lazy_used ? hc[6] : evn[0];
    c.gap_now = std::max(0.0, ev_lo - sigma);
    c.res_tol = (strict ? 1e-13 * ev_hi : std::max(1e-9 * c.gap_now, 1e-14 * ev_hi)) * std::sqrt((double)rank);
    const bool chol_ok = hs[0] == 0;
    c.good = c.converged && std::fabs(c.cnt - rank) < 1e-6 && chol_ok && hs[2] != 1 && hs[3] == 0 &&
             c.res <= c.res_tol && std::isfinite(c.rho_now);
    return c;
  }
  bool eig_deferred(int slot) override {
    auto it = eig_state_.find(slot);
    return it != eig_state_.end() && it->second.deferred;
  }
  int eig_verify(int slot, bool discard) override {
    auto it = eig_state_.find(slot);
    if (it == eig_state_.end() || !it->second.deferred) {
      route("%s", "eig.verify idle");
      return -1;
    }
    EigState &es = it->second;
    es.deferred = false;
    HIP_CHECK(hipEventSynchronize(es.ev_chk));
    double *hc = es.chk_pinned;
    {
      const double *rp = hc + kEigOffResp;
      double r2 = 0;
      for (int b2 = 0; b2 < kTailBlocks; b2++) r2 += rp[b2];
      hc[4] = r2;
    }
    const StepCheck c = check_step(hc, es.J, es.rank, es.dp.sigma, es.dp.rho, false, true, true, true);
    bool ok = c.good && !discard;
    if (ok && eig_defer_fail_ > 0 && ++eig_defer_count_ % eig_defer_fail_ == 0) ok = false;  // (tests)
    if (eig_debug_) {
      const int *hs = (const int *)(hc + kEigOffStatus);
      fprintf(stderr, "[ppals eig] slot %d J %lld rank %d: lamR %.6e lamR1 %.6e deflated %d rho %.3e "
                      "(now %.3e) ell0 %.2e iters %d | ||X^2-I||^2 %.3e count %.6f residual %.3e "
                      "(gap %.3e) dominant vector moved %.1e after %d power steps chol %d%d%d%d -> %s (fast %d full %d)\n",
              slot, (long long)es.J, es.rank, es.lamR, es.lamR1, es.dp.m, es.dp.rho, c.rho_now, es.dp.ell0,
              es.dp.iters, hc[0], c.cnt, c.res, c.gap_now, es.dp.m == 1 ? std::sqrt(std::max(0.0, hc[9])) : 0.0, es.dp.pow,
              hs[0], hs[1], hs[2], hs[3],
              ok ? "accepted (deferred check)" : (discard ? "dropped (its input was withdrawn)"
                                                          : "NOT accepted (deferred check): the caller repeats the step"),
              es.fast, es.full);
    }
    if (ok) {
      // the eigenvalues arrive with the second stream's Jacobi: resolve_lazy() turns them into
      // the slot's state when the slot is used next; the caller holds the basis, Y is owed to it
      es.lazy_pending = true;
      es.rot_pending = true;
      es.lazy_m = es.dp.m;
      es.lazy_strict = false;
      es.rho_frob = c.rho_now;
      es.dom_move = es.dp.m == 1 ? std::sqrt(std::max(0.0, hc[9])) : -1.0;
      es.fast++;
      es.stable++;
      route("%s", "eig.verify accepted");
      return 0;
    }
    route("eig.verify %s", discard ? "discarded" : "rejected");
    std::swap(es.Q, es.Qn);  // (the step had put its basis in front)
    es.stable = 0;
    es.dom_move = -1;
    es.n_defer_failed++;
    return 1;
  }
  const double *eig_pending_rotation(int slot) override {
    auto it = eig_state_.find(slot);
    if (it == eig_state_.end() || !it->second.rot_pending) return nullptr;
    HIP_CHECK(hipEventSynchronize(it->second.ev_done));
    // (the rotation is read by launches on the main stream: order them behind the Jacobi)
    HIP_CHECK(hipStreamWaitEvent(st_, it->second.ev_done, 0));
    return it->second.Yd;
  }
  void eig_rotation_done(int slot) override {
    auto it = eig_state_.find(slot);
    if (it != eig_state_.end()) it->second.rot_pending = false;
  }
  // the eigenvalues a lazy step left on the second stream become the slot's state (what the
  // accepted branch of projector_step does at once when the Jacobi runs inside the step)
  void resolve_lazy(EigState &es) {
    if (!es.lazy_pending) return;
    es.lazy_pending = false;
    double evn[kEigEvMax];
    // (the Jacobi wrote them into pinned host memory itself: waiting for ITS event is all it takes —
    // a copy would queue behind the other slots' Jacobis on the second stream, or drain the main one)
    HIP_CHECK(hipEventSynchronize(es.ev_done));
    es.jacobi_launched = false;  // (nothing of this slot is in flight on the second stream any more)
    for (int d = 0; d < es.rank; d++) evn[d] = es.ev_pinned[d];
    const int rank = es.rank, m = es.lazy_m;
    bool sane = true;
    for (int d = 0; d < rank; d++) sane = sane && std::isfinite(evn[d]);
    if (!sane) {
      es.valid = false;
      return;
    }
    const int mi = std::min(m, rank - 1);
    const double growth = es.evh[mi] > 0 ? evn[mi] / es.evh[mi] : 2.0;
    es.head = std::min(8.0, std::max(1.25, 1.25 * growth * growth));
    for (int d = 0; d < rank; d++) es.evh[d] = evn[d];
    const double shift = evn[rank - 1] - es.lamR;
    es.lamR = evn[rank - 1];
    es.lamR1 = std::min(std::max(0.0, es.lamR1 + shift), es.lamR);
    if (es.lazy_strict) es.lamR1 = std::min(es.lamR1, es.lamR * (1 - 1e-6));
    if (!(es.lamR > es.lamR1 * (1 + 1e-9))) es.valid = false;
  }
  int eig_session_new() override {
    eig_next_base_ += 64;
    return eig_next_base_;
  }
  void eig_session_free(int base) override {
    hipStreamSynchronize(st_);
    for (auto it = eig_state_.begin(); it != eig_state_.end();)
      if (it->first >= base && it->first < base + 64) {
        if (it->second.Q) hipFree(it->second.Q);
        if (it->second.Qn) hipFree(it->second.Qn);
        free_lazy(it->second);
        it = eig_state_.erase(it);
      } else {
        ++it;
      }
    for (auto it = eig_small_.begin(); it != eig_small_.end();)
      if (it->first >= base && it->first < base + 64) {
        if (it->second.Q) hipFree(it->second.Q);
        it = eig_small_.erase(it);
      } else {
        ++it;
      }
  }

  // The tail of a projector step in six launches, none of them a lone workgroup with the rows in
  // The tail of a projector step in seven launches, everything that touches the J rows multi-
  // workgroup: Z = (Omega + X Omega) / 2 | C = Z^T Z and t = Q_D^T Z | M with [Q_D | Z] M
  // orthonormal (one workgroup, cols x cols) | B = [Q_D | Z] M | G B | H = B^T G B | every
  // workgroup diagonalises H itself (block Jacobi in LDS) and forms its rows of U = B Y and of the
  // residual. `rounds` = 2 repeats the Gram / Cholesky / product on B (a basis far from
  // orthonormal: cold starts, wide tails).
  void fused_tail_launches(const double *G, const double *X, int64_t J, int cols, int rank,
                           const double *Omega, const double *QD, int m, double *Z, double *Z2,
                           double *GZ, double *C, double *H, double *Uout, double *evW, double *chk,
                           int *status, const double *pe2, const double *ptr_, int np, int rounds = 1,
                           double *Uout2 = nullptr, EigState *lazy = nullptr, double *host_chk = nullptr) {
    const int Ji = (int)J;
    const int nblk = (int)std::min<int64_t>(kTailBlocks, (J + 31) / 32);
    const int rows_per = (int)((J + nblk - 1) / nblk);
    const bool deferred = lazy && host_chk && rounds == 1 && m <= 1 && cols <= kSeriesMax;
    if (deferred) {
      // The tail of a DEFERRED step (kernels_eig.hip.h, k_tn_gram / k_rmult_chol). On the sweep's
      // stream only what the next mode waits for: Z' = [q_D | P Omega_rest], its Gram, B = Z' R^-1
      // straight into the caller's buffer — three launches. Everything the CHECKS read (G B,
      // H = B^T G B, the subspace residual, the Jacobi of H) is formed from B on the second stream,
      // in the slot's own buffers, from the slot's own copy of the Gram (eig_gram); a Gram in the
      // caller's workspace is multiplied on the sweep's stream first.
      EigState &es = *lazy;
      lazy_prepare(es);
      if (es.GBd_elems < (size_t)J * cols) {
        if (es.GBd) HIP_CHECK(hipFree(es.GBd));
        HIP_CHECK(hipMalloc(&es.GBd, sizeof(double) * (size_t)J * cols));
        es.GBd_elems = (size_t)J * cols;
      }
      double *C1 = C;
      const bool own_gram = G == es.Gd;
      gemm_nn(X, J, Omega, J, Omega, J, Z, J, Ji, cols, Ji, 0.5, 0.5, QD, m);  // Z' = [q_D | P Omega_rest]
      // (a Jacobi of this slot that is still in flight — a step that was not accepted — must be through
      // with the slot's buffers before they are written again)
      if (es.jacobi_launched) HIP_CHECK(hipStreamWaitEvent(st_, es.ev_done, 0));
      hipLaunchKernelGGL(k_tn_gram, dim3((cols * cols + 15) / 16 + 1), dim3(1024), 0, st_, Z, J, cols, C1, pe2, ptr_,
                         np, chk, es.chkd);
      // The second stream takes over from the kernel itself when it reads the slot's own Gram: the
      // last workgroup of k_rmult_chol publishes a sequence number, the second stream waits for the
      // value — no marker packet on the sweep's stream (an event record + wait costs it 6-8 us per
      // step: profiles/r04c_cfg5_timeline_deferred_checks.txt, tools/waitvalue_bench.hip).
      const bool by_flag = own_gram && handover_ok_ && handover_;
      const unsigned long long seq = by_flag ? ++handover_seq_ : 0;
      const int rb = kRmultRows;
      hipLaunchKernelGGL(k_rmult_chol, dim3((unsigned)((J + rb - 1) / rb)), dim3(rmult_chol_threads(cols)),
                         rmult_chol_lds(cols), st_, Z, J, cols, m,
                         C1, Uout, status, chk,
                         es.chkd, by_flag ? (unsigned *)(handover_ + 1) : (unsigned *)nullptr,
                         by_flag ? handover_ : (unsigned long long *)nullptr, seq);
      // (a launch that failed never publishes its number: nothing may be queued behind it)
      if (const hipError_t le = hipGetLastError(); le != hipSuccess) {
        if (by_flag) --handover_seq_;
        throw std::runtime_error(std::string("ppals: k_rmult_chol launch failed: ") + hipGetErrorString(le));
      }
      if (!own_gram) gemm_nn(G, J, Uout, J, nullptr, 0, es.GBd, J, Ji, cols, Ji, 1.0, 0.0);
      es.jacobi_launched = true;
      if (by_flag) {
        HIP_CHECK(hipStreamWaitValue64(st2_, handover_, seq, hipStreamWaitValueGte, 0xFFFFFFFFFFFFFFFFull));
      } else {
        // (measured, round 4: making this event the completion signal of the launch above —
        // hipExtLaunchKernelGGL's stop event — instead of a marker packet leaves 30 us of idle main
        // stream behind it instead of 6-8: profiles/r04v_ext_launch_event.txt)
        HIP_CHECK(hipEventRecord(es.ev_h, st_));
        HIP_CHECK(hipStreamWaitEvent(st2_, es.ev_h, 0));
      }
      if (own_gram) gemm_nn(G, J, Uout, J, nullptr, 0, es.GBd, J, Ji, cols, Ji, 1.0, 0.0, nullptr, 0, st2_);
      hipLaunchKernelGGL(k_tn_small, dim3((cols * cols + 15) / 16), dim3(1024), 0, st2_, Uout, es.GBd, J, cols,
                         es.Hd, (double *)nullptr);
      hipLaunchKernelGGL(k_sub_residual, dim3(nblk), dim3(256), sizeof(double) * ((size_t)cols * cols + 17 + 128),
                         st2_, Uout, es.GBd, J, cols, es.Hd, rows_per, (const double *)nullptr,
                         (const double *)nullptr, -1, (double *)nullptr, Uout2, es.chkd, es.chkd + kEigOffResp,
                         host_chk);
      HIP_CHECK(hipEventRecord(es.ev_chk, st2_));
      const int nthr_j = std::min(1024, std::max(192, (cols * cols / 2 + 63) / 64 * 64) + 64);
      hipLaunchKernelGGL(k_rr_small, dim3(1), dim3(nthr_j), top_eig_small_lds(cols) + sizeof(int) * 64, st2_,
                         es.Hd, cols, es.Yd, es.evd, es.ev_pinned);
      HIP_CHECK(hipEventRecord(es.ev_done, st2_));
      return;
    }
    gemm_nn(X, J, Omega, J, Omega, J, Z, J, Ji, cols, Ji, 0.5, 0.5);
    double *src = Z, *dst = Z2;
    for (int rd = 0; rd < rounds; rd++) {
      const int mm = rd == 0 ? m : 0;  // (the deflated columns are in place after the first round)
      hipLaunchKernelGGL(k_tn_two, dim3((cols * cols + mm * cols + 15) / 16), dim3(1024), 0, st_, src, QD,
                         J, cols, mm, C);
      const int nn = cols - mm;
      const size_t lds_c = sizeof(double) * (4 * (size_t)nn * nn + (size_t)std::max(mm, 1) * cols + 8);
      // (M goes into H's area, which is free until the Gram of G B)
      hipLaunchKernelGGL(k_chol_m, dim3(1), dim3(k_chol_threads(nn)), lds_c, st_, src, QD, J, cols, mm, C, H,
                         status + rd);
      gemm_nn(src, J, H, cols, nullptr, 0, dst, J, Ji, cols, cols, 1.0, 0.0);
      std::swap(src, dst);
    }
    double *B = src;  // (rounds == 1: Z2, rounds == 2: Z)
    double *GB = GZ;
    gemm_nn(G, J, B, J, nullptr, 0, GB, J, Ji, cols, Ji, 1.0, 0.0);
    double *Hd2 = nullptr;
    if (lazy) {
      // (the Jacobi on the second stream works on its own copy of H — the workspace copy is
      // overwritten by the next step — which the Gram kernel writes beside H; a Jacobi of this slot
      // that is still in flight — a step that was not accepted — must be through with the buffers
      // first)
      EigState &es = *lazy;
      lazy_prepare(es);
      if (es.jacobi_launched) HIP_CHECK(hipStreamWaitEvent(st_, es.ev_done, 0));
      Hd2 = es.Hd;
    }
    hipLaunchKernelGGL(k_tn_small, dim3((cols * cols + 15) / 16), dim3(1024), 0, st_, B, GB, J, cols, H, Hd2);
    double *resp = chk + kEigOffResp;
    if (lazy) {
      // the basis itself goes out, checked as a subspace; the Jacobi of H moves to the second stream
      EigState &es = *lazy;
      es.jacobi_launched = true;
      HIP_CHECK(hipEventRecord(es.ev_h, st_));
      HIP_CHECK(hipStreamWaitEvent(st2_, es.ev_h, 0));
      const int nthr_j = std::min(1024, std::max(192, (cols * cols / 2 + 63) / 64 * 64) + 64);
      hipLaunchKernelGGL(k_rr_small, dim3(1), dim3(nthr_j), top_eig_small_lds(cols) + sizeof(int) * 64, st2_,
                         es.Hd, cols, es.Yd, es.evd, es.ev_pinned);
      HIP_CHECK(hipEventRecord(es.ev_done, st2_));
      hipLaunchKernelGGL(k_sub_residual, dim3(nblk), dim3(256),
                         sizeof(double) * ((size_t)cols * cols + 17 + 128), st_, B, GB, J, cols, H, rows_per,
                         pe2, ptr_, np, Uout, Uout2, chk, resp);
      return;
    }
    // (two elements of H per thread + the wave that prepares the next Jacobi round's angles)
    const int nthr_rr = std::min(1024, std::max(192, (cols * cols / 2 + 63) / 64 * 64) + 64);
    hipLaunchKernelGGL(k_rr_apply, dim3(nblk), dim3(nthr_rr), top_eig_small_lds(cols) + sizeof(int) * 64, st_, B,
                       GB, J, cols, rank, H, rows_per, pe2, ptr_, np, Uout, Uout2, evW, chk, resp);
  }
  // The tail of a projector step by plain launches, for any number of columns up to kEigEvMax
  // (PPALS_EIG_FUSED=0, block deflation, and every step of a core rank above 48: rank + 16 columns
  // no longer fit the one-workgroup kernels of the fused tail): Z = (Omega + X Omega) / 2 | the
  // deflated directions projected out and put in front | orthonormal basis (Cholesky QR, block
  // Gram-Schmidt above 64 columns) | Rayleigh-Ritz | residual of the leading `rank` pairs -> chk[4].
  void plain_tail(const double *G, const double *X, int64_t J, int cols, int rank, const double *Omega,
                  const double *QD, int m, double *Ot, double *Z, double *Z2, double *GZ, double *Ut, double *GU,
                  double *C, double *H, double *Yr, double *Uout, double *evW, double *chk, int *status,
                  int npass) {
    const int Ji = (int)J;
    transpose2d(Omega, F64, J, cols, Ot);  // Omega^T (cols x J): coalesced B operand
    gemm_nt(X, J, Ot, cols, Omega, J, Z, J, Ji, cols, Ji, 0.5, 0.5);
    if (m > 0) {
      double *Zr = Z + (size_t)J * m;
      const int nz = cols - m;
      for (int pass = 0; pass < 2; pass++) {
        hipLaunchKernelGGL(k_tn_rect, dim3((m * nz + 15) / 16), dim3(1024), 0, st_, QD, m, Zr, nz, J, H);
        hipLaunchKernelGGL(k_sub_mult, dim3(grid_for((int64_t)J * nz, 256)), dim3(256), 0, st_, Zr, J, nz, QD,
                           m, H);
      }
      HIP_CHECK(hipMemcpyAsync(Z, QD, sizeof(double) * J * m, hipMemcpyDeviceToDevice, st_));
    }
    // (P Omega is within a HOOI sweep's change of orthonormal: one pass, verified by status;
    // the unit vectors of the wide tail are not: two)
    double *B = chol_qr2(Z, Z2, J, cols, C, status, npass);
    rayleigh_ritz(G, B, J, cols, Ut, GZ, H, Yr, Uout, evW, GU);
    hipLaunchKernelGGL(k_eig_residual, dim3(1), dim3(1024), 0, st_, GU, Uout, evW, J, rank, chk + 4);
  }
  // One projector step from the state of the slot; false: not accepted (the caller falls back).
  // strict: the state is a rough estimate (cold start) — accept only residuals at the rounding
  // floor eps * lambda_1, whatever the estimated gap says.
  bool projector_step(EigState &es, double *G, int64_t J, int rank, double *U, int slot, bool strict) {
    // The whole step is enqueued without a read-back: what the host needs in order to schedule it
    // (where the gap lies, the scale of the shifted matrix) it knows from the previous call of the
    // slot, and everything that decides whether the result is accepted (||X^2 - I||, trace(P),
    // Cholesky pivots, eigenpair residual) is read once, at the end, together with the new
    // eigenvalues and the norm the next call will schedule with.
    const int Ji = (int)J;
    const size_t nJJ = (size_t)J * J, nJR = (size_t)J * rank;
    // (column buffers with room for kWide extra columns: the "wide tail" below)
    constexpr int kWide = 16;
    const size_t nJW = (size_t)J * (rank + kWide);
    double *w = (double *)ensure(ws_eig_, ws_eig_sz_,
                                 sizeof(double) * (3 * nJJ + 10 * nJW + 4 * kEE + 512));
    double *X = w, *Xn = X + nJJ, *Y = Xn + nJJ;
    double *Ot = Y + nJJ, *Z = Ot + nJW, *Z2 = Z + nJW, *GZ = Z2 + nJW, *Ut = GZ + nJW,
           *GU = Ut + nJW, *QD = GU + nJW, *QD2 = QD + nJW, *Om = QD2 + nJW, *Uw = Om + nJW;
    const size_t nJR_end = 10 * nJW;  // (columns of the workspace behind Y)
    // the tail of the workspace is what the one read-back fetches in a single copy:
    //   chk[16] (0,1: sign check, 4: residual, 8: ||.||_F^2) | evW[64] | status[8 ints] | lamD[64]
    double *C = Ot + nJR_end, *H = C + kEE, *Yr = H + kEE, *chk = Yr + kEE,
           *evW = chk + 16;
    int *status = (int *)(chk + kEigOffStatus);
    double *lamD = chk + kEigOffLamD;
    constexpr size_t kReadback = kEigReadback;
    double sigma = 0.5 * (es.lamR + es.lamR1);
    if (eig_sigma_scale_ > 0) sigma = eig_sigma_scale_ * es.lamR1;  // tests: a shift that is too low
    // ---- dominant eigenpairs (a relative gap >= 20 above the rest of the wanted ones): refined
    // to machine precision by a few block power steps from the previous basis, then deflated —
    // the sign iteration amplifies rounding by (spectral radius / gap), and a tensor with a mean
    // component has lambda_1 ~ 1e6 x the rest
    int m = 0;
    double ratio = 1.0;
    for (int d = 1; d < rank; d++)
      if (es.evh[d] > 0 && es.evh[d - 1] / es.evh[d] >= 20.0) {
        m = d;
        ratio = es.evh[d] / es.evh[d - 1];
      }
    double tau = 0;
    // the step's status words: cleared by the kernel that sets up the iteration (k_ns_prepare /
    // k_deflate_shift) unless block deflation writes some of them before that (m > 1)
    int *zero8 = m <= 1 ? status : nullptr;
    if (!zero8) HIP_CHECK(hipMemsetAsync(status, 0, 8 * sizeof(int), st_));
    // Fused form of a warm step (PPALS_EIG_FUSED=0: the round-2 launch sequence, kept for A/B and as
    // the route of block deflation / cold starts): the scale of the iteration comes from what the
    // slot knows about the spectrum instead of a Frobenius norm measured on the device (G is a Gram
    // matrix: every eigenvalue of G - sigma I lies in [-sigma, lambda_max - sigma], so
    // max(sigma, lambda_next - sigma) bounds the spectral radius of the deflated, shifted matrix —
    // an order of magnitude below its Frobenius norm for a flat bulk of a few hundred eigenvalues,
    // i.e. 2-3 iterations fewer). Head room (EigState::head): 25 % in steady state, the square of
    // the growth the slot's leading eigenvalue showed over its last step otherwise, 4 x right after a
    // cold start (the first HOOI sweeps move the spectrum by factors); beyond it the iteration still
    // converges up to sqrt(3) x, after which an eigenvalue is folded to the wrong side, the count
    // comes out short and the step is repeated on the measured Frobenius norm (top_eigvecs_warm).
    const bool fused_scale = !strict && m <= 1 && eig_sigma_scale_ <= 0 && !eig_frob_once_;
    const double *pow_y = nullptr, *pow_p = nullptr;
    int pow_n = 0, pow_steps = 0;
    if (m == 1) {
      // one dominant eigenpair (a tensor with a mean component): power steps on one vector. The
      // previous vector is off by at most ~1e-2 (one HOOI sweep); each step gains `ratio`. The
      // Rayleigh quotient left by the last step is that of its input: second order in its error.
      // (k steps leave an error of 1e-2 * ratio^k in the vector and its square in the quotient: the
      // target 1e-14 needs ratio^k <= 1e-12 — two steps at the 1e-6 of a tensor with a mean component,
      // where counting from 1e-14 itself took three; a vector that was further off shows in the
      // residual of the step, which is then repeated cold)
      // (round 4: the 1e-2 is an assumption only until the slot has MEASURED how far its dominant vector
      // moved from one step to the next — k_ns_prepare leaves the sine in the step's check block —: the
      // next step starts from 8 x that, so a converging HOOI run drops from three launches to two)
      double start = 1e-2;
      if (es.dom_move >= 0) start = std::min(1e-2, std::max(1e-8, 8.0 * es.dom_move));
      const int nsteps = std::min(14, std::max(2, (int)std::ceil(std::log(1e-14 / start) / std::log(ratio))));
      pow_steps = nsteps;
      const int nb = (int)((J + 7) / 8);
      double *pw = (double *)ensure(ws_pow_, ws_pow_sz_, sizeof(double) * 4 * (size_t)nb);
      double *pbuf[2] = {pw, pw + 2 * (size_t)nb};
      double *ybuf[2] = {QD2, Z2};  // (Z2 is free until the Cholesky QR of the projected basis)
      const double *src = es.Q;
      const double *pin = nullptr;
      for (int it = 0; it < nsteps; it++) {
        hipLaunchKernelGGL(k_power_mv, dim3(nb), dim3(256), 0, st_, G, J, src, pin, nb, ybuf[it & 1],
                           pbuf[it & 1]);
        src = ybuf[it & 1];
        pin = pbuf[it & 1];
      }
      pow_y = src;
      pow_p = pin;
      pow_n = nb;
      tau = es.lamR * 1.5 + 1e-300;
      if (!fused_scale)
        hipLaunchKernelGGL(k_power_finish, dim3(1), dim3(256), 0, st_, src, J, pin, nb, QD, lamD);
    } else if (m > 0) {
      const int nsteps = std::min(14, std::max(3, (int)std::ceil(std::log(1e-18) / std::log(ratio))));
      HIP_CHECK(hipMemcpyAsync(QD, es.Q, sizeof(double) * J * m, hipMemcpyDeviceToDevice, st_));
      double *cur = QD;
      for (int it = 0; it < nsteps; it++) {
        double *other = (cur == QD) ? QD2 : QD;
        transpose2d(cur, F64, J, m, Ot);
        gemm_nt(G, J, Ot, m, nullptr, 0, Z, J, Ji, m, Ji, 1.0, 0.0);
        double *res = chol_qr2(Z, other, J, m, C, status + 2);  // ends in Z (two passes)
        if (res != cur) HIP_CHECK(hipMemcpyAsync(cur, res, sizeof(double) * J * m,
                                                 hipMemcpyDeviceToDevice, st_));
      }
      rayleigh_ritz(G, cur, J, m, Ot, Z, H, Yr, Z2, lamD, nullptr);
      HIP_CHECK(hipMemcpyAsync(QD, Z2, sizeof(double) * J * m, hipMemcpyDeviceToDevice, st_));
      tau = es.lamR * 1.5 + 1e-300;  // still above sigma: they keep counting as "wanted"
    }
    // X = (G - deflation - sigma I) / rho, rho = its Frobenius norm >= every |eigenvalue| (safe:
    // an eigenvalue of the scaled matrix beyond 1 would be folded back by the scaled iteration).
    // The norm stays on the device; the host schedules the iteration with the norm of the slot's
    // previous call (the matrices of consecutive HOOI sweeps differ by a few per cent at most, and
    // an under-estimated lower bound `ell` only costs a fraction of an iteration).
    const int gdef = grid_for(nJJ, 256, 1024);
    double *part = (double *)ensure(ws_part_, ws_part_sz_, sizeof(double) * (gdef + 1));
    double *fro2_d = chk + 8;
    double rho = es.rho_frob;
    if (fused_scale) {
      const double next = m < rank ? es.evh[m] : 0.0;  // largest eigenvalue that is not deflated
      rho = es.head * std::max(sigma, next - sigma);
      if (!(rho > 0) || !std::isfinite(rho)) return false;
      hipLaunchKernelGGL(k_ns_prepare, dim3(gdef), dim3(256), 0, st_, G, J, pow_y, pow_p, pow_n, m, tau,
                         sigma, 1.0 / rho, X, QD, lamD, zero8, m == 1 ? (const double *)es.Q : (const double *)nullptr,
                         m == 1 ? chk + 9 : (double *)nullptr);
    } else {
      hipLaunchKernelGGL(k_deflate_shift, dim3(gdef), dim3(256), 0, st_, G, J, QD, m, lamD, tau, sigma,
                         X, part, zero8);
      hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(1024), 0, st_, part, gdef, fro2_d);
      if (!(rho > 0)) {  // first projector step of the slot: read the norm
        double fro2 = 0;
        HIP_CHECK(hipMemcpyAsync(&fro2, fro2_d, sizeof(double), hipMemcpyDeviceToHost, st_));
        HIP_CHECK(hipStreamSynchronize(st_));
        rho = 1.0001 * std::sqrt(fro2);
        if (!(rho > 0) || !std::isfinite(rho)) return false;
      }
      hipLaunchKernelGGL(k_scale_by_frob, dim3(grid_for(nJJ, 256)), dim3(256), 0, st_, X, (int64_t)nJJ,
                         fro2_d);
    }
    // (strict = cold start: the distance of the shift to the nearest eigenvalue is unknown — the
    // Ritz values around it are rough — so a small lower bound is assumed: a few iterations more)
    double ell0 = 0.9 * 0.5 * std::min(es.lamR - sigma, sigma - es.lamR1) / rho;
    if (strict) ell0 = std::min(ell0, 2e-5);
    double ell = std::max(ell0, eig_sigma_scale_ > 0 ? 1e-4 : 1e-14);
    int iters = 0;
    const unsigned ntri = sym_tiles(Ji);
    // fused tail: the check sums ride on the LAST step's two products (per-tile partial sums of
    // ||X_prev^2 - I||_F^2 and of trace(X_new), added up by the tail's last kernel)
    const bool fused_tail = m <= 1 && rank + kWide <= 64;
    // (the step's tag of the route log: what scheduled it and how it ended)
    auto tag = [&](bool wide, bool lazy, bool defer, bool ok) {
      route("eig.projector m=%d strict=%d fused_scale=%d fused_tail=%d wide=%d lazy=%d defer_now=%d ok=%d",
            std::min(m, 2), strict ? 1 : 0, fused_scale ? 1 : 0, fused_tail ? 1 : 0, wide ? 1 : 0, lazy ? 1 : 0,
            defer ? 1 : 0, ok ? 1 : 0);
    };
    double *pe2 = (double *)ensure(ws_part2_, ws_part2_sz_, sizeof(double) * (2 * (size_t)ntri + 2 * 256 + 2));
    double *ptr_ = pe2 + ntri;
    auto ns_step = [&](double mu, bool last = false) {
      // Y = X^2, X <- X (a I + b X^2): symmetric products, stored symmetric bit for bit
      sym_product(X, J, X, J, nullptr, 0, Y, J, Ji, Ji, 1.0, 0.0, last ? 1 : 0, pe2);
      sym_product(X, J, Y, J, X, J, Xn, J, Ji, Ji, -0.5 * mu * mu * mu, 1.5 * mu, last ? 2 : 0, ptr_);
      std::swap(X, Xn);
      iters++;
    };
    while (1.0 - ell > 1e-3 && iters < 80) {
      const double mu = std::sqrt(3.0 / (1.0 + ell + ell * ell));
      ns_step(mu);
      ell = 0.5 * mu * ell * (3.0 - mu * mu * ell * ell);
    }
    ns_step(1.0);
    ns_step(1.0, fused_tail);
    for (int attempt = 0;; attempt++) {
      // ---- check of the sign iteration: ||X^2 - I||_F^2 and trace(X) (-> chk[0], chk[1])
      if (!fused_tail) {
        sym_product(X, J, X, J, nullptr, 0, Y, J, Ji, Ji, 1.0, 0.0);
        const int gc = 256;
        double *pc = ptr_ + ntri;
        hipLaunchKernelGGL(k_sign_check, dim3(gc), dim3(256), 0, st_, Y, X, J, pc);
        hipLaunchKernelGGL(k_sum_pairs, dim3(1), dim3(256), 0, st_, pc, gc, chk);
      }
      // ---- Z = P * Omega = (Omega + X Omega) / 2 with the previous basis, Cholesky-QR twice, then
      // Rayleigh-Ritz inside the subspace: the eigenvectors one by one, sorted descending
      // (the deflated directions come from the power iteration, accurate to machine precision: the
      // projector of the DEFLATED matrix carries them only to eps * lambda_1 / gap. So the basis is
      // [Q_D | (I - Q_D Q_D^T) P Omega_rest].)
      // `tail(cols, Omega, Uout)`: basis of `cols` columns = P applied to Omega (J x cols), Cholesky
      // QR, Rayleigh-Ritz on cols x cols; the leading `rank` eigenvectors land in Uout (ld J), their
      // residual in chk[4], all `cols` eigenvalues in evW; then the one read-back of the step
      bool lazy_used = false;
      // deferred acceptance: a slot whose last steps went through as scheduled hands out the basis
      // without waiting for its checks (Ops::eig_defer / eig_verify)
      const bool defer_now = attempt == 0 && es.lazy && es.defer && es.stable >= 2 && fused_tail &&
                             fused_scale && !strict && !eig_frob_once_;
      auto tail = [&](int cols, const double *Omega, double *Uout, int npass) {
        if (fused_tail) {
          // (the leading eigenvectors also go to the slot's spare basis buffer: accepted = a swap)
          const bool lazy_now = es.lazy && cols == rank && Uout == U && npass == 1;
          lazy_used = lazy_now;
          fused_tail_launches(G, X, J, cols, rank, Omega, QD, m, Z, Z2, GZ, C, H, Uout, evW, chk, status,
                              pe2, ptr_, (int)ntri, npass, Uout == U ? es.Qn : nullptr,
                              lazy_now ? &es : nullptr, (defer_now && lazy_now) ? es.chk_pinned : nullptr);
          if (defer_now && lazy_now) {
            // no wait and no copy: the checks are finished on the second stream, whose kernel writes
            // them into the slot's pinned block (ev_chk); eig_verify() reads them when the caller
            // comes back to the slot
            HIP_CHECK(hipGetLastError());
            return;
          }
          if (!eig_host_) HIP_CHECK(hipHostMalloc(&eig_host_, kReadback, hipHostMallocDefault));
          HIP_CHECK(hipMemcpyAsync(eig_host_, chk, kReadback, hipMemcpyDeviceToHost, st_));
          HIP_CHECK(hipStreamSynchronize(st_));
          HIP_CHECK(hipGetLastError());
          {  // the residual's per-workgroup shares are added up here
            double *hcw = (double *)eig_host_;
            const double *rp = hcw + kEigOffResp;
            double r2 = 0;
            for (int b2 = 0; b2 < kTailBlocks; b2++) r2 += rp[b2];
            hcw[4] = r2;
          }
          return;
        }
        plain_tail(G, X, J, cols, rank, Omega, QD, m, Ot, Z, Z2, GZ, Ut, GU, C, H, Yr, Uout, evW, chk, status,
                   npass);
        if (!eig_host_) HIP_CHECK(hipHostMalloc(&eig_host_, kReadback, hipHostMallocDefault));
        HIP_CHECK(hipMemcpyAsync(eig_host_, chk, kReadback, hipMemcpyDeviceToHost, st_));
        HIP_CHECK(hipStreamSynchronize(st_));
        HIP_CHECK(hipGetLastError());
      };
      tail(rank, es.Q, U, 1);
      if (defer_now && lazy_used) {
        es.deferred = true;
        es.n_deferred++;
        es.dp.sigma = sigma;
        es.dp.rho = rho;
        es.dp.ell0 = ell0;
        es.dp.m = m;
        es.dp.iters = iters;
        es.dp.pow = pow_steps;
        std::swap(es.Q, es.Qn);  // (eig_verify swaps back when the step is not accepted)
        tag(false, true, true, true);
        return true;
      }
      const double *hc = (const double *)eig_host_, *evn = hc + 16;
      const int *hs = (const int *)(hc + kEigOffStatus);
      const StepCheck sc = check_step(hc, J, rank, sigma, rho, strict, fused_tail, fused_scale, lazy_used);
      const double cnt = sc.cnt, res = sc.res, rho_now = sc.rho_now, gap_now = sc.gap_now, res_tol = sc.res_tol;
      const bool converged = sc.converged, good = sc.good;
      if (eig_debug_)
        fprintf(stderr, "[ppals eig] slot %d J %lld rank %d: lamR %.6e lamR1 %.6e deflated %d rho %.3e "
                        "(now %.3e) ell0 %.2e iters %d | ||X^2-I||^2 %.3e count %.6f residual %.3e "
                        "(gap %.3e) chol %d%d%d%d -> %s (fast %d full %d)\n",
                slot, (long long)J, rank, es.lamR, es.lamR1, m, rho, rho_now, ell0, iters, hc[0], cnt,
                res, gap_now, hs[0], hs[1], hs[2], hs[3],
                good ? "accepted" : (converged ? "not accepted as it is" : "more steps"), es.fast, es.full);
      es.stable = (good && attempt == 0) ? es.stable + 1 : 0;
      if (good && lazy_used) {
        // the eigenvalues arrive with the second stream's Jacobi: resolve_lazy() turns them into
        // the slot's state when the slot is used next; U holds the basis, Y is owed to the caller
        es.lazy_pending = true;
        es.rot_pending = true;
        es.lazy_m = m;
        es.lazy_strict = strict;
        es.rho_frob = rho_now;
        es.dom_move = (m == 1 && fused_scale) ? std::sqrt(std::max(0.0, hc[9])) : -1.0;
        std::swap(es.Q, es.Qn);
        es.fast++;
        tag(false, true, false, true);
        return true;
      }
      if (lazy_used) {
        // not accepted: the Jacobi on the second stream is of no use (its buffers are the slot's own)
        lazy_used = false;
      }
      if (!good) es.dom_move = -1;
      if (good) {
        {
          const int mi = std::min(m, rank - 1);
          const double growth = es.evh[mi] > 0 ? evn[mi] / es.evh[mi] : 2.0;
          es.head = std::min(8.0, std::max(1.25, 1.25 * growth * growth));
        }
        for (int d = 0; d < rank; d++) es.evh[d] = evn[d];
        const double shift = evn[rank - 1] - es.lamR;
        es.lamR = evn[rank - 1];
        es.lamR1 = std::min(std::max(0.0, es.lamR1 + shift), es.lamR);
        es.rho_frob = rho_now;
        es.dom_move = (m == 1 && fused_scale) ? std::sqrt(std::max(0.0, hc[9])) : -1.0;
        if (strict) es.lamR1 = std::min(es.lamR1, es.lamR * (1 - 1e-6));  // (a rough estimate)
        if (!(es.lamR > es.lamR1 * (1 + 1e-9))) es.valid = false;  // next call: full solver
        if (fused_tail)
          std::swap(es.Q, es.Qn);
        else
          HIP_CHECK(hipMemcpyAsync(es.Q, U, sizeof(double) * nJR, hipMemcpyDeviceToDevice, st_));
        es.fast++;
        tag(false, false, false, true);
        return true;
      }
      const int cwide = (int)std::lround(cnt);
      if (converged && std::fabs(cnt - cwide) < 1e-6 && cwide > rank && cwide <= rank + kWide &&
          cwide <= kEigEvMax && cwide < Ji && hs[2] != 1 && hs[3] == 0 && std::isfinite(rho_now)) {
        // The shift fell a few eigenvalues too low: P projects onto an invariant subspace of
        // cwide > rank dimensions — still exact. Rayleigh-Ritz on a basis of THAT many columns
        // (the previous basis plus P applied to a few unit vectors) yields its eigenpairs one by
        // one, the leading `rank` of them are the answer, and the next one is the new estimate of
        // the eigenvalue below the cut. A 0.2 ms tail instead of the 9 ms full solver.
        HIP_CHECK(hipMemcpyAsync(Om, es.Q, sizeof(double) * nJR, hipMemcpyDeviceToDevice, st_));
        HIP_CHECK(hipMemsetAsync(Om + nJR, 0, sizeof(double) * J * (cwide - rank), st_));
        hipLaunchKernelGGL(k_set_unit_cols, dim3(1), dim3(64), 0, st_, Om + nJR, J, cwide - rank);
        HIP_CHECK(hipMemsetAsync(status, 0, 2 * sizeof(int), st_));
        tail(cwide, Om, Uw, 2);
        const double resw = std::sqrt(hc[4]);
        const bool goodw = hs[0] != 1 && hs[1] == 0 && resw <= res_tol &&
                           evn[rank - 1] > evn[rank] * (1 + 1e-9);
        if (eig_debug_)
          fprintf(stderr, "[ppals eig]   wide tail with %d columns: residual %.3e chol %d%d -> %s\n",
                  cwide, resw, hs[0], hs[1], goodw ? "accepted" : "full solver");
        if (goodw) {
          HIP_CHECK(hipMemcpyAsync(U, Uw, sizeof(double) * nJR, hipMemcpyDeviceToDevice, st_));
          es.head = 4.0;  // (the estimates were off by several eigenvalues: the spectrum is moving)
          for (int d = 0; d < rank; d++) es.evh[d] = evn[d];
          es.lamR = evn[rank - 1];
          es.lamR1 = std::max(0.0, evn[rank]);
          es.rho_frob = rho_now;
          HIP_CHECK(hipMemcpyAsync(es.Q, U, sizeof(double) * nJR, hipMemcpyDeviceToDevice, st_));
          es.fast++;
          tag(true, false, false, true);
          return true;
        }
        tag(true, false, false, false);
        return false;
      }
      if (converged || attempt >= (strict ? 4 : 2)) break;
      // the gap was narrower than estimated: a few more steps, then the tail again
      if (strict) {
        ns_step(1.0);
        ns_step(1.0);
      }
      ns_step(1.0);
      ns_step(1.0, fused_tail);
      HIP_CHECK(hipMemsetAsync(status, 0, 2 * sizeof(int), st_));  // (the Cholesky QR of the tail)
    }
    // sigma does not separate `rank` eigenvalues, a lost direction, no convergence
    tag(false, false, false, false);
    return false;
  }
  // Cold start of a slot: q steps of block subspace iteration from a pseudo-random block of
  // rank + 16 columns, Rayleigh-Ritz — rough Ritz pairs (lower bounds of the eigenvalues). They
  // become the slot's state with a deliberately LOW estimate of the eigenvalue below the cut, so
  // that the shift of the projector step has at least `rank` eigenvalues above it; a few more are
  // what its wide tail is for. false: the Ritz values do not resolve the neighbourhood of the cut
  // (a flat spectrum) or the block lost rank — the caller goes to the full solver.
  bool cold_ritz_state(EigState &es, double *G, int64_t J, int rank, int slot) {
    cold_ok_ = false;
    const int b = std::min(kEigEvMax, rank + 16);
    if (b >= J || rank + 4 >= b) return false;
    const int Ji = (int)J;
    const size_t nJB = (size_t)J * b;
    double *w = (double *)ensure(ws_cold_, ws_cold_sz_, sizeof(double) * (5 * nJB + 3 * kEE + kEigEvMax + 64));
    double *Z = w, *Z2 = Z + nJB, *Zt = Z2 + nJB, *GB = Zt + nJB, *Uo = GB + nJB;
    double *C = Uo + nJB, *H = C + kEE, *Yr = H + kEE, *ev = Yr + kEE;
    int *status = (int *)(ev + kEigEvMax);
    HIP_CHECK(hipMemsetAsync(status, 0, 4 * sizeof(int), st_));
    hipLaunchKernelGGL(k_fill_hash, dim3(grid_for((int64_t)nJB, 256)), dim3(256), 0, st_, Z, (int64_t)nJB,
                       (uint64_t)(0x5eed + slot));
    double *cur = Z, *oth = Z2;
    for (int it = 0; it < 4; it++) {
      gemm_nn(G, J, cur, J, nullptr, 0, oth, J, Ji, b, Ji, 1.0, 0.0);  // G * block
      if (b <= 64) {
        // Cholesky QR twice: Gram (one wave per entry) | M = R^-1 by one workgroup | thin product
        double *src = oth, *dst = cur;
        for (int pass = 0; pass < 2; pass++) {
          hipLaunchKernelGGL(k_tn_two, dim3((b * b + 15) / 16), dim3(1024), 0, st_, src, (const double *)nullptr,
                             J, b, 0, C);
          hipLaunchKernelGGL(k_chol_m, dim3(1), dim3(k_chol_threads(b)), sizeof(double) * (4 * (size_t)b * b + b + 8), st_,
                             src, (const double *)nullptr, J, b, 0, C, H, status + pass);
          gemm_nn(src, J, H, b, nullptr, 0, dst, J, Ji, b, b, 1.0, 0.0);
          std::swap(src, dst);
        }
        // (two passes: the result is back in `oth`)
      } else {
        double *res = chol_qr2(oth, cur, J, b, C, status);  // two passes: ends in `oth`
        if (res != oth) return false;
      }
      std::swap(cur, oth);
    }
    rayleigh_ritz(G, cur, J, b, Zt, GB, H, Yr, Uo, ev, nullptr);
    double th[kEigEvMax];
    int hs[4];
    HIP_CHECK(hipMemcpyAsync(th, ev, sizeof(double) * b, hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipMemcpyAsync(hs, status, sizeof(int) * 4, hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipStreamSynchronize(st_));
    HIP_CHECK(hipGetLastError());
    const int below = std::min(b - 1, rank + 4);  // index of the estimate placed under the cut
    const bool sane = hs[0] != 1 && hs[1] == 0 && th[rank - 1] > 0 && th[below] >= 0;
    const bool ok = sane && th[rank - 1] > th[below] * 1.02;
    // (kept for cold_bisect: the Ritz block is a generic basis, its Ritz values are lower bounds)
    cold_ok_ = sane;
    cold_b_ = b;
    cold_Uo_ = Uo;
    for (int d = 0; d < b; d++) cold_th_[d] = th[d];
    if (eig_debug_)
      fprintf(stderr, "[ppals eig] slot %d J %lld rank %d: cold start, Ritz values %.4e .. %.4e | %.4e "
                      "(index %d) -> %s\n", slot, (long long)J, rank, th[0], th[rank - 1], th[below],
              below, ok ? "projector step" : "full solver");
    if (!ok) return false;
    if (!es.Q || es.J != J || es.rank != rank) {
      if (es.Q) hipFree(es.Q);
      if (es.Qn) hipFree(es.Qn);
      HIP_CHECK(hipMalloc(&es.Q, sizeof(double) * J * rank));
      HIP_CHECK(hipMalloc(&es.Qn, sizeof(double) * J * rank));
    }
    es.J = J;
    es.rank = rank;
    HIP_CHECK(hipMemcpyAsync(es.Q, Uo, sizeof(double) * J * rank, hipMemcpyDeviceToDevice, st_));
    for (int d = 0; d < rank; d++) es.evh[d] = th[d];
    es.lamR = th[rank - 1];
    es.lamR1 = th[below];
    es.rho = th[0];
    es.rho_frob = 0;
    es.head = 4.0;
    es.valid = true;
    return true;
  }

  // Cold start of a LONG mode by block subspace iteration with Rayleigh-Ritz in every step (round 6).
  // The projector route costs ~46 products of J^3 from cold — 8.9 ms each at J = 7200, the image mode of
  // coil-100 (test_ALS.cxx:296-299): 408 of the 516 ms of that HOSVD — to deliver `rank` vectors;
  // a step here costs two THIN products (G times J x (rank + 16)) and a Rayleigh-Ritz on rank + 16
  // columns. From the Ritz pairs (U, theta) of cold_ritz_state: B = orth(G U theta^-1) — scaled column
  // by column, so the block stays near orthonormal whatever the spread of the spectrum (a mean
  // component 1e6 above the rest included) —, Rayleigh-Ritz on B, residual of the leading `rank` pairs;
  // accepted at the bar of every other cold start (residual <= 1e-13 lambda_1 sqrt(rank), the strict
  // projector step's and cold_bisect's: a cold start has no previous gap to lean on, and the op-level
  // tests hold all cold routes to that one bar). The iteration converges like
  // (lambda_{rank+17} / lambda_rank)^k: where the residual shows that this will not get there within
  // the budget — 40 steps, each two thin products, still a fraction of ONE J^3 product per step on a
  // long mode —, false: the caller goes on to the projector.
  bool cold_subspace(EigState &es, double *G, int64_t J, int rank, double *U, int slot) {
    const int b = cold_b_, Ji = (int)J;
    if (b <= rank || !cold_Uo_) return false;
    const size_t nJB = (size_t)J * b;
    double *w = (double *)ensure(ws_cold_, ws_cold_sz_, sizeof(double) * (5 * nJB + 3 * kEE + kEigEvMax + 64));
    double *Z = w, *Z2 = Z + nJB, *Zt = Z2 + nJB, *GB = Zt + nJB, *Uo = GB + nJB;
    double *C = Uo + nJB, *H = C + kEE, *Yr = H + kEE, *ev = Yr + kEE;
    int *status = (int *)(ev + kEigEvMax);
    if (Uo != cold_Uo_) return false;  // (the workspace moved: nothing to continue from)
    double *w2 = (double *)ensure(ws_cold2_, ws_cold2_sz_, sizeof(double) * (nJB + 16));
    double *GU = w2, *res_d = GU + nJB;
    constexpr int kMaxIt = 40;
    double th[kEigEvMax], res_prev = 0;
    for (int it = 0; it < kMaxIt; it++) {
      gemm_nn(G, J, Uo, J, nullptr, 0, Z, J, Ji, b, Ji, 1.0, 0.0);  // G * (Ritz vectors)
      hipLaunchKernelGGL(k_scale_cols_inv, dim3(grid_for((int64_t)nJB, 256)), dim3(256), 0, st_, Z, J, b,
                         (const double *)ev);
      HIP_CHECK(hipMemsetAsync(status, 0, 4 * sizeof(int), st_));
      double *B = chol_qr2(Z, Z2, J, b, C, status);
      rayleigh_ritz(G, B, J, b, Zt, GB, H, Yr, Uo, ev, GU);
      hipLaunchKernelGGL(k_eig_residual, dim3(1), dim3(1024), 0, st_, GU, Uo, ev, J, rank, res_d);
      double res2 = 0;
      int hs[4];
      HIP_CHECK(hipMemcpyAsync(th, ev, sizeof(double) * b, hipMemcpyDeviceToHost, st_));
      HIP_CHECK(hipMemcpyAsync(&res2, res_d, sizeof(double), hipMemcpyDeviceToHost, st_));
      HIP_CHECK(hipMemcpyAsync(hs, status, sizeof(int) * 4, hipMemcpyDeviceToHost, st_));
      HIP_CHECK(hipStreamSynchronize(st_));
      HIP_CHECK(hipGetLastError());
      const double res = std::sqrt(res2);
      const bool sane = hs[0] != 1 && hs[1] == 0 && std::isfinite(res) && th[rank - 1] > 0 && th[rank] >= 0;
      const double gap = sane ? th[rank - 1] - th[rank] : 0.0;
      const double tol = 1e-13 * th[0] * std::sqrt((double)rank);
      if (eig_debug_)
        fprintf(stderr, "[ppals eig] slot %d J %lld rank %d: cold subspace step %d, Ritz %.4e .. %.4e | %.4e, "
                        "residual %.3e (bar %.3e)\n", slot, (long long)J, rank, it, th[0], th[rank - 1], th[rank],
                res, tol);
      if (!sane) return false;
      if (gap > 0 && res <= tol) {
        const int below = std::min(b - 1, rank + 4);
        if (!es.Q || es.J != J || es.rank != rank) {
          if (es.Q) hipFree(es.Q);
          if (es.Qn) hipFree(es.Qn);
          HIP_CHECK(hipMalloc(&es.Q, sizeof(double) * J * rank));
          HIP_CHECK(hipMalloc(&es.Qn, sizeof(double) * J * rank));
        }
        es.J = J;
        es.rank = rank;
        HIP_CHECK(hipMemcpyAsync(es.Q, Uo, sizeof(double) * J * rank, hipMemcpyDeviceToDevice, st_));
        HIP_CHECK(hipMemcpyAsync(U, Uo, sizeof(double) * J * rank, hipMemcpyDeviceToDevice, st_));
        for (int d = 0; d < rank; d++) es.evh[d] = th[d];
        es.lamR = th[rank - 1];
        es.lamR1 = th[below];
        es.rho = th[0];
        es.rho_frob = 0;
        es.head = 4.0;
        es.valid = es.lamR > es.lamR1 * (1 + 1e-9);
        es.fast++;
        n_cold_subspace_++;
        return true;
      }
      // the residual of a linearly converging iteration: where will it be when the budget ends?
      if (it >= 2 && res_prev > 0) {
        const double f = res / res_prev;
        if (!(f < 0.97) || res * std::pow(f, kMaxIt - 1 - it) > tol) return false;
      }
      res_prev = res;
    }
    return false;
  }
  int64_t n_cold_subspace_ = 0;
  void *ws_cold2_ = nullptr;
  size_t ws_cold2_sz_ = 0;
  void *ws_cholm_ = nullptr;
  size_t ws_cholm_sz_ = 0;
  void *ws_gsfb_ = nullptr;
  size_t ws_gsfb_sz_ = 0;

  // Cold start by eigenvalue counting. trace(sign(G - sigma I)) says how many eigenvalues lie above
  // sigma — exactly, whatever the spectrum looks like — so the shift is placed by a few trials of
  // the sign iteration instead of by Ritz values: a bracket [lo, hi] with count(lo) >= rank (the
  // rank-th Ritz value is a lower bound of the rank-th eigenvalue) and count(hi) < rank, then
  // interpolation on count^(2/3) (the edge law of a bulk spectrum) until rank <= count <=
  // rank + kWide. The projector of that trial is exact for an invariant subspace of `count`
  // dimensions; Rayleigh-Ritz on P applied to the Ritz block delivers its eigenpairs one by one and
  // the leading `rank` are the answer (the same tail as a warm step's "wide tail"). A trial costs
  // ~0.25 ms (28 products of J^3), the full solver 9 ms at J = 400. One dominant eigenpair (a mean
  // component) is refined by power steps and deflated; anything this cannot handle returns false.
  bool cold_bisect(EigState &es, double *G, int64_t J, int rank, double *U, int slot) {
    constexpr int kWide = 16;
    const int Ji = (int)J, b = cold_b_;
    const size_t nJJ = (size_t)J * J, nJR = (size_t)J * rank, nJW = (size_t)J * (rank + kWide);
    if (rank + kWide > b || rank + kWide >= Ji) return false;
    const bool big = rank + kWide > 64;  // (the counting is the same; the tail is made of plain launches)
    const double *th = cold_th_;
    int m = 0;
    for (int d = 1; d < rank; d++)
      if (th[d] > 0 && th[d - 1] / th[d] >= 20.0) m = d;
    if (m > 1) return false;
    const unsigned ntri = sym_tiles(Ji);
    double *w = (double *)ensure(ws_eig_, ws_eig_sz_,
                                 sizeof(double) * (3 * nJJ + 10 * nJW + 4 * kEE + 512));
    double *X = w, *Xn = X + nJJ, *Y = Xn + nJJ;
    double *Z = Y + nJJ, *Z2 = Z + nJW, *GZ = Z2 + nJW, *QD = GZ + nJW, *y0 = QD + nJW, *y1 = y0 + nJW,
           *Uw = y1 + nJW, *Ot = Uw + nJW, *Ut = Ot + nJW, *GU = Ut + nJW;
    double *Cw = Y + nJJ + 10 * nJW, *Hw = Cw + kEE;
    double *chk = Y + nJJ + 10 * nJW + 3 * kEE, *evW = chk + 16;
    int *status = (int *)(chk + kEigOffStatus);
    double *lamD = chk + kEigOffLamD;
    constexpr size_t kReadback = kEigReadback;
    double *pe2 = (double *)ensure(ws_part2_, ws_part2_sz_, sizeof(double) * (2 * (size_t)ntri + 2 * 256 + 2));
    double *ptr_ = pe2 + ntri;
    if (!eig_host_) HIP_CHECK(hipHostMalloc(&eig_host_, kReadback, hipHostMallocDefault));
    // the Ritz block lives in ws_cold_, which nothing below touches
    const double *Om = cold_Uo_;
    const double *pow_y = nullptr, *pow_p = nullptr;
    int pow_n = 0;
    if (m == 1) {
      const int nb = (int)((J + 7) / 8);
      double *pw = (double *)ensure(ws_pow_, ws_pow_sz_, sizeof(double) * 4 * (size_t)nb);
      double *pbuf[2] = {pw, pw + 2 * (size_t)nb};
      double *ybuf[2] = {y0, y1};
      const double *src = Om, *pin = nullptr;
      for (int it = 0; it < 4; it++) {
        hipLaunchKernelGGL(k_power_mv, dim3(nb), dim3(256), 0, st_, G, J, src, pin, nb, ybuf[it & 1],
                           pbuf[it & 1]);
        src = ybuf[it & 1];
        pin = pbuf[it & 1];
      }
      pow_y = src;
      pow_p = pin;
      pow_n = nb;
    }
    const double next_ub = 1.5 * th[m];  // generous bound of the largest eigenvalue left in place
    int trials = 0, products = 0;
    // one trial: X = sign((G - deflation - sigma I) / rho), returns count and convergence
    auto trial = [&](double sigma, double *count, bool *conv) {
      const double rho = 1.25 * std::max(sigma, next_ub - sigma);
      const int gdef = grid_for(nJJ, 256, 1024);
      hipLaunchKernelGGL(k_ns_prepare, dim3(gdef), dim3(256), 0, st_, G, J, pow_y, pow_p, pow_n, m,
                         2.0 * sigma, sigma, 1.0 / rho, X, QD, lamD);
      auto ns_step = [&](double mu, bool last) {
        sym_product(X, J, X, J, nullptr, 0, Y, J, Ji, Ji, 1.0, 0.0, last ? 1 : 0, pe2);
        sym_product(X, J, Y, J, X, J, Xn, J, Ji, Ji, -0.5 * mu * mu * mu, 1.5 * mu, last ? 2 : 0, ptr_);
        std::swap(X, Xn);
        products += 2;
      };
      double ell = 1e-5;  // assumed distance of the shift to the nearest eigenvalue (scaled)
      int it = 0;
      while (1.0 - ell > 1e-3 && it++ < 80) {
        const double mu = std::sqrt(3.0 / (1.0 + ell + ell * ell));
        ns_step(mu, false);
        ell = 0.5 * mu * ell * (3.0 - mu * mu * ell * ell);
      }
      ns_step(1.0, false);
      for (int attempt = 0;; attempt++) {
        ns_step(1.0, true);
        hipLaunchKernelGGL(k_chk_sums, dim3(1), dim3(256), 0, st_, pe2, ptr_, (int)ntri, chk);
        HIP_CHECK(hipMemcpyAsync(eig_host_, chk, 2 * sizeof(double), hipMemcpyDeviceToHost, st_));
        HIP_CHECK(hipStreamSynchronize(st_));
        const double *hc = (const double *)eig_host_;
        *conv = hc[0] <= 1e-10 * std::sqrt((double)J);
        *count = 0.5 * (hc[1] + (double)J);
        if (*conv || attempt >= 3) break;
        ns_step(1.0, false);  // the shift sits closer to an eigenvalue than assumed: more steps
        ns_step(1.0, false);
        ns_step(1.0, false);
      }
      trials++;
      if (eig_debug_)
        fprintf(stderr, "[ppals eig] slot %d   count trial %d: sigma %.8e -> count %.4f (%s)\n", slot,
                trials, sigma, *count, *conv ? "converged" : "NOT converged");
    };
    double lo = th[rank - 1], hi = 1.08 * th[m], c_lo = -1, c_hi = -1;
    double cnt = 0;
    bool conv = false;
    // upper end of the bracket: fewer than `rank` eigenvalues above it
    for (int k = 0; k < 6; k++) {
      trial(hi, &cnt, &conv);
      if (conv && std::lround(cnt) < rank) {
        c_hi = (double)std::lround(cnt);
        break;
      }
      if (conv && std::lround(cnt) <= rank + kWide) break;  // landed inside the window already
      if (conv) lo = hi, c_lo = (double)std::lround(cnt);
      hi *= conv ? 1.08 : 1.0003;
    }
    double sigma = hi;
    auto in_window = [&]() { return conv && std::lround(cnt) >= rank && std::lround(cnt) <= rank + kWide; };
    if (!in_window()) {
      if (c_hi < 0) return false;
      if (c_lo < 0) {  // count at the Ritz lower bound
        trial(lo, &cnt, &conv);
        if (!conv) {
          lo *= 0.9997;
          trial(lo, &cnt, &conv);
        }
        if (!conv) return false;
        c_lo = (double)std::lround(cnt);
        sigma = lo;
      }
      const double target = rank + kWide / 2;
      for (int k = 0; k < 12 && !in_window(); k++) {
        if (c_lo < rank) return false;  // the Ritz value was no lower bound: give up
        // N(sigma)^(2/3) is close to linear below a spectral edge; plain bisection every third trial
        const double tl = std::pow(c_lo, 2.0 / 3.0), thh = std::pow(std::max(c_hi, 0.0), 2.0 / 3.0),
                     tt = std::pow(target, 2.0 / 3.0);
        double f = (k % 3 == 2) ? 0.5 : (tl - tt) / std::max(tl - thh, 1e-300);
        f = std::min(0.95, std::max(0.05, f));
        sigma = lo + f * (hi - lo);
        trial(sigma, &cnt, &conv);
        if (!conv) {  // on top of an eigenvalue: nudge
          sigma = lo + std::min(0.97, f + 0.02) * (hi - lo);
          trial(sigma, &cnt, &conv);
          if (!conv) return false;
        }
        const long c = std::lround(cnt);
        if (c > rank + kWide) {
          lo = sigma;
          c_lo = (double)c;
        } else if (c < rank) {
          hi = sigma;
          c_hi = (double)c;
        }
      }
      if (!in_window()) return false;
    }
    const int cols = (int)std::lround(cnt);
    if (std::fabs(cnt - cols) > 1e-6) return false;
    // ---- the tail on `cols` columns: P applied to the Ritz block (a generic basis), two Cholesky-QR
    // passes, Rayleigh-Ritz; the deflated eigenvector takes the place of the first column
    HIP_CHECK(hipMemsetAsync(status, 0, 8 * sizeof(int), st_));
    if (big) {
      HIP_CHECK(hipMemsetAsync(chk + kEigOffResp, 0, sizeof(double) * kTailBlocks, st_));
      plain_tail(G, X, J, cols, rank, Om, QD, m, Ot, Z, Z2, GZ, Ut, GU, Cw, Hw, Hw + kEE, Uw, evW, chk, status, 2);
    } else {
      fused_tail_launches(G, X, J, cols, rank, Om, QD, m, Z, Z2, GZ, Cw, Hw, Uw, evW, chk, status, pe2, ptr_,
                          (int)ntri, 2);
    }
    HIP_CHECK(hipMemcpyAsync(eig_host_, chk, kReadback, hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipStreamSynchronize(st_));
    HIP_CHECK(hipGetLastError());
    if (!big) {  // (the fused tail leaves per-workgroup shares of the residual; the plain one the sum)
      double *hcw = (double *)eig_host_;
      const double *rp = hcw + kEigOffResp;
      double r2 = 0;
      for (int b2 = 0; b2 < kTailBlocks; b2++) r2 += rp[b2];
      hcw[4] = r2;
    }
    const double *hc = (const double *)eig_host_, *evn = hc + 16;
    const int *hs = (const int *)(hc + kEigOffStatus);
    const double res = std::sqrt(hc[4]);
    const double res_tol = 1e-13 * evn[0] * std::sqrt((double)rank);
    const bool good = hs[0] != 1 && hs[1] == 0 && res <= res_tol && std::isfinite(res) &&
                      (cols == rank || evn[rank - 1] > evn[rank] * (1 + 1e-12));
    if (eig_debug_)
      fprintf(stderr, "[ppals eig] slot %d J %lld rank %d: cold start by counting, %d trials (%d products), "
                      "sigma %.8e count %d, residual %.3e (tol %.3e) chol %d%d -> %s\n",
              slot, (long long)J, rank, trials, products, sigma, cols, res, res_tol, hs[0], hs[1],
              good ? "accepted" : "full solver");
    if (!good) return false;
    HIP_CHECK(hipMemcpyAsync(U, Uw, sizeof(double) * nJR, hipMemcpyDeviceToDevice, st_));
    if (!es.Q || es.J != J || es.rank != rank) {
      if (es.Q) hipFree(es.Q);
      if (es.Qn) hipFree(es.Qn);
      HIP_CHECK(hipMalloc(&es.Q, sizeof(double) * J * rank));
      HIP_CHECK(hipMalloc(&es.Qn, sizeof(double) * J * rank));
    }
    es.J = J;
    es.rank = rank;
    HIP_CHECK(hipMemcpyAsync(es.Q, Uw, sizeof(double) * nJR, hipMemcpyDeviceToDevice, st_));
    for (int d = 0; d < rank; d++) es.evh[d] = evn[d];
    es.lamR = evn[rank - 1];
    es.lamR1 = cols > rank ? std::max(0.0, evn[rank]) : std::min(sigma, es.lamR * (1 - 1e-6));
    es.rho = evn[0];
    es.rho_frob = 0;
    es.head = 4.0;
    es.valid = es.lamR > es.lamR1 * (1 + 1e-9);
    es.fast++;
    return true;
  }
  bool cold_ok_ = false;
  int64_t cold_subspace_from_ = 2048;  // PPALS_COLD_SUBSPACE_FROM (tests: lower it to exercise the route)
  int cold_b_ = 0;
  const double *cold_Uo_ = nullptr;
  double cold_th_[kEigEvMax] = {0};
  double frob_shifted(const double *G, int64_t J, double sigma) {
    const int g = grid_for(J * J, 256, 1024);
    double *part = (double *)ensure(ws_part_, ws_part_sz_, sizeof(double) * (g + 1));
    hipLaunchKernelGGL(k_frob_shifted, dim3(g), dim3(256), 0, st_, G, J, sigma, part);
    hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(1024), 0, st_, part, g, part + g);
    double h = 0;
    HIP_CHECK(hipMemcpyAsync(&h, part + g, sizeof(double), hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipStreamSynchronize(st_));
    return std::sqrt(h);
  }
  void sign_align(double *W, const double *Wref, int64_t rows, int r) override {
    hipLaunchKernelGGL(k_sign_align, dim3((r + 3) / 4), dim3(256), 0, st_, W, Wref, rows, r);
    HIP_CHECK(hipGetLastError());
  }
  void add_inplace(double *dst, const double *src, int64_t n) override {
    hipLaunchKernelGGL(k_add_inplace, dim3(grid_for(n, 256)), dim3(256), 0, st_, dst, src, n);
    HIP_CHECK(hipGetLastError());
  }
  void rows_times_small(const double *A, int64_t rows, int K, const double *B, int C,
                        const double *D, double *out) override {
    if ((size_t)K * C * sizeof(double) > 60 * 1024)
      throw std::runtime_error("ppals: rows_times_small: the small operand does not fit LDS");
    double *dst = out;
    if (out == A) dst = (double *)ensure(ws_big2_, ws_big2_sz_, sizeof(double) * (size_t)rows * C);
    route("rows_times_small copy=%d", dst != out ? 1 : 0);
    hipLaunchKernelGGL(k_rows_times_small, dim3(grid_for(rows * C, 256)), dim3(256),
                       sizeof(double) * (size_t)K * C, st_, A, rows, K, B, C, D, dst);
    HIP_CHECK(hipGetLastError());
    if (dst != out)
      HIP_CHECK(hipMemcpyAsync(out, dst, sizeof(double) * rows * C, hipMemcpyDeviceToDevice, st_));
  }
  void lowrank_accumulate(void *X, int xdt, int64_t n, int R, const double *T, int r,
                          const double *VT) override {
    const size_t lds = sizeof(double) * (size_t)r * R;
    if (xdt == F32)
      hipLaunchKernelGGL(k_lowrank_accumulate<float>, dim3(grid_for(n, 256)), dim3(256), lds, st_,
                         (float *)X, n, R, T, r, VT);
    else
      hipLaunchKernelGGL(k_lowrank_accumulate<double>, dim3(grid_for(n, 256)), dim3(256), lds, st_,
                         (double *)X, n, R, T, r, VT);
    HIP_CHECK(hipGetLastError());
  }
  void sumsq(const double *x, int64_t n, double *out) override {
    int g = grid_for(n, 256, 1024);
    double *part = (double *)ensure(ws_part_, ws_part_sz_, sizeof(double) * g);
    hipLaunchKernelGGL(k_sumsq, dim3(g), dim3(256), 0, st_, x, n, part);
    hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(1024), 0, st_, part, g, out);
    HIP_CHECK(hipGetLastError());
  }

  // ------------------------------------------------------------------ stopwatch (ops.h)
  int timer_begin() override {
    int h = -1;
    for (size_t q = 0; q < timers_.size(); q++)
      if (!timers_[q].busy) h = (int)q;
    if (h < 0) {
      if (timers_.size() >= 64) return -1;
      Timer t;
      if (hipEventCreate(&t.a) != hipSuccess) return -1;
      if (hipEventCreate(&t.b) != hipSuccess) {
        hipEventDestroy(t.a);
        return -1;
      }
      timers_.push_back(t);
      h = (int)timers_.size() - 1;
    }
    timers_[h].busy = true;
    timers_[h].ended = false;
    if (hipEventRecord(timers_[h].a, st_) != hipSuccess) {
      timers_[h].busy = false;
      return -1;
    }
    return h;
  }
  void timer_end(int h) override {
    if (h < 0 || h >= (int)timers_.size() || !timers_[h].busy) return;
    timers_[h].ended = hipEventRecord(timers_[h].b, st_) == hipSuccess;
  }
  double timer_read(int h) override {
    if (h < 0 || h >= (int)timers_.size() || !timers_[h].busy) return -1.0;
    Timer &t = timers_[h];
    t.busy = false;
    float ms = 0;
    if (!t.ended || hipEventSynchronize(t.b) != hipSuccess ||
        hipEventElapsedTime(&ms, t.a, t.b) != hipSuccess)
      return -1.0;
    return 1e-3 * (double)ms;
  }

  // ------------------------------------------------------------------ profiling
  void profile_enable(int level) override { profiling_ = level; }
  void profile_collect() override {
    HIP_CHECK(hipStreamSynchronize(st_));
    for (size_t i = 0; i < nev_; i++) {
      float ms = 0;
      if (hipEventElapsedTime(&ms, events_[i].a, events_[i].b) == hipSuccess) {
        prof[events_[i].slot].launches += 1;
        prof[events_[i].slot].ms += ms;
        prof[events_[i].slot].bytes += events_[i].bytes;
      }
    }
    nev_ = 0;
  }

 private:
  struct RocSolver {
    void *handle = nullptr;
    int (*dsyevd)(void *, int, int, int, double *, int, double *, double *, int *) = nullptr;
  };
  RocSolver &rocsolver() {
    if (rs_.handle) return rs_;
    EigLibs &l = eig_libs();  // loads on first use unless hip_preload_eigensolver() ran earlier
    auto create = (int (*)(void **))dlsym(l.blas, "rocblas_create_handle");
    auto set_stream = (int (*)(void *, hipStream_t))dlsym(l.blas, "rocblas_set_stream");
    *(void **)(&rs_.dsyevd) = dlsym(l.solver, "rocsolver_dsyevd");
    if (!create || !set_stream || !rs_.dsyevd)
      throw std::runtime_error("ppals: rocSOLVER symbols missing");
    if (create(&rs_.handle) != 0 || set_stream(rs_.handle, st_) != 0)
      throw std::runtime_error("ppals: rocblas handle creation failed");
    return rs_;
  }
  RocSolver rs_;
  struct Timer {
    hipEvent_t a = nullptr, b = nullptr;
    bool busy = false, ended = false;
  };
  std::vector<Timer> timers_;
  struct Ev {
    hipEvent_t a, b;
    int slot;
    double bytes;
  };
  void prof_begin(int slot, double bytes) {
    cur_ = -1;
    if (profiling_ < 1 + slot) return;  // level 1: tensor scans only, level 2: every timed slot
    if (nev_ == events_.size()) {
      if (events_.size() >= 16384) return;
      Ev e;
      if (hipEventCreate(&e.a) != hipSuccess || hipEventCreate(&e.b) != hipSuccess) return;
      events_.push_back(e);
    }
    cur_ = (int)nev_++;
    events_[cur_].slot = slot;
    events_[cur_].bytes = bytes;
    hipEventRecord(events_[cur_].a, st_);
  }
  void prof_end() {
    if (cur_ >= 0) hipEventRecord(events_[cur_].b, st_);
    cur_ = -1;
  }
  // grow-only workspace; regrowth synchronises (only happens while shapes are first seen)
  void *ensure(void *&p, size_t &sz, size_t need) {
    if (need > sz) {
      if (p) {
        HIP_CHECK(hipStreamSynchronize(st_));
        HIP_CHECK(hipFree(p));
      }
      size_t n = need + need / 4 + 256;
      HIP_CHECK(hipMalloc(&p, n));
      sz = n;
    }
    return p;
  }
  double *small(int n) { return (double *)ensure(ws_small_, ws_small_sz_, sizeof(double) * n); }
  // one tag of the route log (ops.h); nothing is formatted while no log is attached
  template <typename... A>
  void route(const char *fmt, A... a) {
    if (!route_log) return;
    char buf[160];
    snprintf(buf, sizeof(buf), fmt, a...);
    route_log->emplace_back(buf);
  }
  template <typename T>
  static constexpr const char *tname() {
    return sizeof(T) == 8 ? "f64" : "f32";
  }
  template <typename T>
  static constexpr const char *sname() {  // the storage type of a tensor, bf16 included
    return std::is_same<T, bf16s>::value ? "bf16" : tname<T>();
  }

  // Where a pass of nsplit k-splits writes its ncols x M result (T batches): the output o itself, or
  // for nsplit > 1 the fp64 slab [split][batch][ncols][M] that slab_combine sums into o. A padded
  // layout's rows are compacted by whichever kernel stores to o: the pass, or the combine.
  struct PassDst {
    double *p;
    int out32;
    int64_t nstride, split_stride, batch_stride, row_ld, row_valid;
  };
  PassDst pass_dst(int nsplit, int64_t M, int64_t T, int ncols, double *o, int out32, int64_t out_rstride,
                   int64_t out_tstride, RowPad pad) {
    if (nsplit == 1) return {o, out32, out_rstride, 0, out_tstride, pad.ld, pad.valid};
    double *slab = (double *)ensure(ws_slab_, ws_slab_sz_, sizeof(double) * nsplit * ncols * M * T);
    return {slab, 0, M, (int64_t)ncols * M * T, (int64_t)ncols * M, 0, 0};
  }
  // k_slab_reduce: the sum of the nsplit partial results in the slab, into out (nothing to do for one split)
  void slab_combine(int nsplit, const double *slab, int64_t split_stride, int64_t M, int ncols, double *out,
                    int64_t out_mstride, int64_t out_rstride, int out32, RowPad pad = RowPad(), int64_t T = 1,
                    int64_t slab_bstride = 0, int64_t out_bstride = 0) {
    if (nsplit == 1) return;
    hipLaunchKernelGGL(k_slab_reduce, dim3(grid_for(M * ncols, 256), (unsigned)T), dim3(256), 0, st_, slab, nsplit,
                       split_stride, M, ncols, out, out_mstride, out_rstride, out32, pad.ld, pad.valid, slab_bstride,
                       out_bstride);
    HIP_CHECK(hipGetLastError());
  }
  // A result too large for the 256 MB Infinity Cache is stored non-temporally: the stream of
  // ordinary stores costs the scan 0.2 ms per 320 MB (cfg2) next to its 6.4 GB of reads, the
  // non-temporal one 0.1 ms (tools/place6_bench, profiles/r03q_place6_nt.txt: 1.09-1.10 ms
  // against 1.19-1.20 ms per launch for the same source and result buffers), and what reads
  // the result next streams it from HBM either way. Not on every pair of buffers, though: in one
  // process (r03q_place6_nt_same_process.txt) 1.21 -> 1.06 ms for some, +1 % for others — so
  // the engine's online placement choice tries both kinds for the first-level intermediate
  // (scan_store_mode); this rule is for every other large result. A k-split pass writes the slab.
  static constexpr double kNtMinBytes = 192.0 * 1048576.0;
  bool nt_store(int nsplit, double result_bytes) const {
    return nsplit == 1 && (scan_nt_mode_ < 0 ? result_bytes >= kNtMinBytes : scan_nt_mode_ == 1);
  }
  // resident workgroups per CU of a kernel, asked of the runtime once and kept in `cached`
  // (`fallback` when the runtime has no answer)
  static int occupancy(int &cached, const void *kernel, int block, size_t lds, int fallback) {
    if (cached == 0) {
      int nb = 0;
      const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, block, lds);
      if (e != hipSuccess) (void)hipGetLastError();
      cached = (e == hipSuccess && nb > 0) ? nb : fallback;
    }
    return cached;
  }

  int dev_ = 0, ncu_ = 256, force_jacobi_ = 0, persist_mult_ = 40;
  int eig_debug_ = 0;
  SysArgs sys_;             // arm_gram_system: the system the next contraction prepares on the side
  int sys_R_ = 0;
  bool sys_armed_ = false, sys_ready_ = false;
  NormArgs norm_;           // arm_normalize: folded into the next cp_mode_update
  int norm_mode_ = -1;
  const double *norm_G_ = nullptr;
  bool norm_armed_ = false;
  bool eig_frob_once_ = false;
  void *ws_jac_ = nullptr;  // rotation product of the one-sided Jacobi (r x r)
  size_t ws_jac_sz_ = 0;
  int sym_lds_min_ = 768;   // PPALS_SYM_LDS_MIN: rows from which the symmetric product is LDS-tiled
  int eig_defer_ok_ = 1;    // PPALS_EIG_DEFER=0: every projector step waits for its own checks
  bool handover_ok_ = true;                 // second stream released by a value the kernel stores (else: events)
  unsigned long long *handover_ = nullptr;  // [0] the sequence number published last, [1] workgroup counter
  unsigned long long handover_seq_ = 0;
  int eig_defer_fail_ = 0;  // PPALS_EIG_DEFER_FAIL=n (tests): every n-th deferred check is reported as failed
  int eig_defer_count_ = 0;
  int eig_cold_ = 1;  // PPALS_EIG_FAST=2: cold starts go straight to the full solver (A/B, tests)
  void *ws_cold_ = nullptr;
  size_t ws_cold_sz_ = 0;
  double eig_sigma_scale_ = 0;  // PPALS_EIG_SIGMA_SCALE=f: shift = f * (estimate of the next eigenvalue) (tests)
  int force_eiginv_ = 0;  // PPALS_FORCE_EIGINV=1: R > 64 always inverts S through dsyevd (tests)
  int eig_fast_ = 1;  // PPALS_EIG_FAST=0: always the full eigensolver (A/B, tests)
  std::map<int, EigState> eig_state_;  // by slot
  int eig_next_base_ = 0;
  void *eig_host_ = nullptr;  // pinned: the read-back of a projector step
  void *ws_eig_ = nullptr, *ws_orth_ = nullptr, *ws_pow_ = nullptr, *ws_part2_ = nullptr;
  size_t ws_eig_sz_ = 0, ws_orth_sz_ = 0, ws_pow_sz_ = 0, ws_part2_sz_ = 0;
  hipStream_t st_ = nullptr;
  hipStream_t st2_ = nullptr;  // the Jacobi of a lazy eigen-step (created on first use)
  void *ws_mttv_ = nullptr;  // partial sums of a j-split k_mttv_l
  void *ws_mv_ = nullptr;    // offset tables of model_to_view
  size_t ws_mv_sz_ = 0;
  void *ws_hist_ = nullptr;  // the global histogram of model_absres_hist
  size_t ws_hist_sz_ = 0;
  size_t ws_mttv_sz_ = 0;
  void *ws_pack_ = nullptr, *ws_slab_ = nullptr, *ws_krp_ = nullptr, *ws_part_ = nullptr,
       *ws_small_ = nullptr, *ws_big_ = nullptr, *ws_big2_ = nullptr;
  size_t ws_pack_sz_ = 0, ws_slab_sz_ = 0, ws_krp_sz_ = 0, ws_part_sz_ = 0, ws_small_sz_ = 0,
         ws_big_sz_ = 0, ws_big2_sz_ = 0;
  int profiling_ = 0;
  int scan_slot_ = 0;  // profile slot of the scans (scan_profile_slot)
  std::vector<Ev> events_;
  size_t nev_ = 0;
  int cur_ = -1;
};

Ops *make_hip_ops(int device) { return new HipOps(device); }
void hip_preload_eigensolver() { (void)eig_libs(); }

}  // namespace ppals
