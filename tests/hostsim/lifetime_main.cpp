// lifetime_main.cpp — TEST INFRASTRUCTURE: who owns the device memory when an allocation fails.
//
// One scenario through the C ABI on the host stand-in ops (host_ops.cpp), built once from seeded inputs, takes
// every grow-only buffer of the two engines at least once: an ordinary CP session (both schedules, a PP phase, a
// low-rank-update step, the diagnostics), a multi-start session of ranks {2, 3} (sweeps, hold-out, factor match scores) and a Tucker session (HOSVD, sweeps,
// a PP phase), all on one 9 x 8 x 7 fp32 tensor. It runs unarmed first: every call must succeed. Then the k-th
// allocation is made to fail, k = 1, 2, ...: the scenario stops at the first call that reports an error,
// everything created so far is destroyed, and k + 1 follows, until a k whose failure never came.
//
// This program is linked against the AddressSanitizer + UBSan build of the library and carries the sanitizer
// runtime itself; a double free, a use after free, a leak or undefined behaviour anywhere ends it with a
// report and a non-zero status. On its own account it checks that every failing call returned a PPALS_ERR_*
// code with the injected message, and that EVERY call site of the scenario was the failing one for some k (a
// site that allocates nothing at this shape does not belong here: the loop could end early and hide the rest).
//
// Calls that only set the scene and allocate nothing (ppals_tensor_fill_uniform, the two set_factors, set_schedule)
// are booked under the call site they prepare. ppals_cp_leverages comes first of the three diagnostics: behind the
// other two it would find every buffer it uses already there.
// Left out: ppals_cp_export_model_device and ppals_cp_impute_device. The stand-in has no device views (ops.h) and
// refuses both with PPALS_ERR_UNSUPPORTED before anything is allocated, whatever the shape, so their operand
// buffers (xq_ / xp_) are not reached from here.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ppals.h"

extern "C" {
void hostsim_fail_alloc_after(long k);
long hostsim_fail_alloc_countdown(void);
}

namespace {

const int64_t kLens[3] = {9, 8, 7};
const int kR = 3;
const int kMultiRanks[2] = {2, 3};
const int kTuckerRanks[3] = {2, 2, 2};
const char *const kInjected = "injected allocation failure";

enum Site {
  CTX_TENSOR_CREATE,
  CP_CREATE,
  CP_SWEEPS_MSDT,
  CP_SWEEPS_DT,
  CP_PP,
  CP_ALS_LR,
  CP_LEVERAGES,
  CP_CORE_CONSISTENCY,
  CP_SLICE_RESIDUALS,
  MULTI_CREATE,
  MULTI_SWEEPS,
  MULTI_SET_HOLDOUT,
  MULTI_FMS,
  TUCKER_CREATE,
  TUCKER_HOSVD,
  TUCKER_SWEEPS,
  TUCKER_PP,
  NSITES
};
const char *const kSiteName[NSITES] = {
    "ppals_tensor_create",       "ppals_cp_create",           "ppals_cp_sweeps_dt (MSDT)",  "ppals_cp_sweeps_dt (DT)",
    "ppals_cp_pp",               "ppals_cpd_als_lr",          "ppals_cp_leverages",         "ppals_cp_core_consistency",
    "ppals_cp_slice_residuals",  "ppals_cp_multi_create_ranks", "ppals_cp_multi_sweeps",    "ppals_cp_multi_set_holdout",
    "ppals_cp_multi_fms",        "ppals_tucker_create",       "ppals_tucker_hosvd",         "ppals_tucker_sweeps_dt",
    "ppals_tucker_pp"};

struct Inputs {
  std::vector<double> W, Wmulti;
  std::vector<uint8_t> keep;
  Inputs() {
    const int64_t rows = kLens[0] + kLens[1] + kLens[2];
    W.resize((size_t)rows * kR);
    ppals_fill_uniform_host(W.data(), (int64_t)W.size(), 11, 0, 0.1, 1.0);
    Wmulti.resize((size_t)rows * (kMultiRanks[0] + kMultiRanks[1]));
    ppals_fill_uniform_host(Wmulti.data(), (int64_t)Wmulti.size(), 12, 0, 0.1, 1.0);
    keep.assign((size_t)2 * kLens[0], 1);  // start 0 holds row 1 of mode 0 out, start 1 row 4
    keep[1] = 0;
    keep[(size_t)kLens[0] + 4] = 0;
  }
};

struct Handles {
  ppals_ctx *ctx = nullptr;
  ppals_tensor *V = nullptr;
  ppals_cp *cp = nullptr;
  ppals_cp_multi *multi = nullptr;
  ppals_tucker *tk = nullptr;
  void destroy() {  // in reverse order of creation
    ppals_tucker_destroy(tk);
    ppals_cp_multi_destroy(multi);
    ppals_cp_destroy(cp);
    ppals_tensor_destroy(V);
    ppals_ctx_destroy(ctx);
    *this = Handles();
  }
};

ppals_cp_opts driver_opts() {
  ppals_cp_opts o;
  std::memset(&o, 0, sizeof(o));
  o.tol = 1e-14;
  o.timelimit = 1e3;
  o.maxiter = 4;  // (one exact sweep, then one PP phase: the operators are built once)
  o.lambda = 1e-8;
  o.resprint = 1;
  o.tol_init = 1e9;  // (every dW counts as small: the first exact sweep already hands over to PP)
  o.ratio_step = 1.0;
  o.update_percentage = 1.0;
  return o;
}

struct Outcome {
  int site = -1;  // the failing call, -1: none
  int rc = 0;
  bool fired_there = false;  // the injected failure came inside that call
  std::string message;
};

// the scenario up to its first failing call; `h` keeps whatever was created
Outcome run_scenario(const Inputs &in, Handles &h) {
  Outcome out;
  const ppals_cp_opts o = driver_opts();
  double buf[1024];
  double sweeps = 0;
  int iters = 0;
  int64_t n = 0;
#define STEP(site_id, call)                                                \
  do {                                                                     \
    const long before = hostsim_fail_alloc_countdown();                    \
    const int rc_ = (call);                                                \
    if (rc_ < 0) {                                                         \
      out.site = (site_id);                                                \
      out.rc = rc_;                                                        \
      out.fired_there = before > 0 && hostsim_fail_alloc_countdown() == 0; \
      out.message = ppals_last_error();                                    \
      return out;                                                          \
    }                                                                      \
  } while (0)
  // (no device is asked for: the stand-in's context allocates nothing)
  if (ppals_ctx_create(&h.ctx, 0) != PPALS_OK) {
    out.site = CTX_TENSOR_CREATE, out.rc = PPALS_ERR_NO_DEVICE, out.message = ppals_last_error();
    return out;
  }
  STEP(CTX_TENSOR_CREATE, ppals_tensor_create(h.ctx, 3, kLens, PPALS_F32, &h.V));
  STEP(CTX_TENSOR_CREATE, ppals_tensor_fill_uniform(h.V, 7, 0.0, 1.0));
  STEP(CP_CREATE, ppals_cp_create(h.ctx, h.V, kR, &h.cp));
  STEP(CP_CREATE, ppals_cp_set_factors(h.cp, in.W.data(), nullptr));
  STEP(CP_SWEEPS_MSDT, ppals_cp_sweeps_dt(h.cp, 2, 1e-8));
  STEP(CP_SWEEPS_DT, ppals_cp_set_schedule(h.cp, PPALS_SCHEDULE_DT));
  STEP(CP_SWEEPS_DT, ppals_cp_sweeps_dt(h.cp, 2, 1e-8));
  STEP(CP_SWEEPS_DT, ppals_cp_set_schedule(h.cp, PPALS_SCHEDULE_MSDT));
  STEP(CP_PP, ppals_cp_pp(h.cp, &o, &iters));
  STEP(CP_ALS_LR, ppals_cpd_als_lr(h.cp, PPALS_OPT_MSDT_LR, 1, 0, &o, &sweeps, &iters));
  STEP(CP_LEVERAGES, ppals_cp_leverages(h.cp, buf));
  STEP(CP_CORE_CONSISTENCY, ppals_cp_core_consistency(h.cp, buf, nullptr, &n));
  STEP(CP_SLICE_RESIDUALS, ppals_cp_slice_residuals(h.cp, buf, nullptr));
  STEP(MULTI_CREATE, ppals_cp_multi_create_ranks(h.ctx, h.V, 2, kMultiRanks, &h.multi));
  STEP(MULTI_CREATE, ppals_cp_multi_set_factors(h.multi, -1, in.Wmulti.data(), nullptr));
  STEP(MULTI_SWEEPS, ppals_cp_multi_sweeps(h.multi, 2, 1e-8));
  STEP(MULTI_SET_HOLDOUT, ppals_cp_multi_set_holdout(h.multi, 0, in.keep.data()));
  STEP(MULTI_FMS, ppals_cp_multi_fms(h.multi, -1, 0, buf));
  STEP(TUCKER_CREATE, ppals_tucker_create(h.ctx, h.V, kTuckerRanks, &h.tk));
  STEP(TUCKER_HOSVD, ppals_tucker_hosvd(h.tk));
  STEP(TUCKER_SWEEPS, ppals_tucker_sweeps_dt(h.tk, 2));
  STEP(TUCKER_PP, ppals_tucker_pp(h.tk, &o, &iters));
#undef STEP
  return out;
}

}  // namespace

int main() {
  const Inputs in;
  Handles h;
  hostsim_fail_alloc_after(0);
  Outcome base = run_scenario(in, h);
  h.destroy();
  if (base.site >= 0) {
    std::fprintf(stderr, "unarmed: %s returned %d: %s\n", kSiteName[base.site], base.rc, base.message.c_str());
    return 1;
  }
  long failed_at[NSITES] = {0};
  long visited = 0, survived = 0;
  int bad = 0;
  for (long k = 1;; k++) {
    hostsim_fail_alloc_after(k);
    const Outcome r = run_scenario(in, h);
    const bool fired = hostsim_fail_alloc_countdown() == 0;
    hostsim_fail_alloc_after(0);
    h.destroy();
    if (r.site < 0 && !fired) break;  // the scenario has fewer than k allocations
    visited++;
    if (r.site < 0) {  // an optional buffer (Ops::try_alloc): the session does without it
      survived++;
      continue;
    }
    failed_at[r.site]++;
    const bool code_ok = r.rc <= PPALS_ERR_NO_DEVICE && r.rc >= PPALS_ERR_UNSUPPORTED;
    if (!r.fired_there || !code_ok || r.message.find(kInjected) == std::string::npos) {
      std::fprintf(stderr, "k = %ld: %s returned %d (failure injected in this call: %s): %s\n", k, kSiteName[r.site],
                   r.rc, r.fired_there ? "yes" : "no", r.message.c_str());
      bad++;
    }
  }
  for (int s = 0; s < NSITES; s++) {
    std::printf("%-32s failed at %ld positions\n", kSiteName[s], failed_at[s]);
    if (failed_at[s] == 0) {
      std::fprintf(stderr, "%s was never the failing call\n", kSiteName[s]);
      bad++;
    }
  }
  std::printf("allocation positions visited: %ld (%ld of them optional buffers the sessions did without)\n", visited,
              survived);
  return bad ? 1 : 0;
}
