// ppals_api.cpp — the C ABI declared in include/ppals.h: thin, exception-free glue between plain
// pointers/sizes and the engine. The backend (device ops + communicator) comes from backend.h:
// libppals.so links the HIP/RCCL backend; there is no other backend in the product.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <set>
#include <string>
#include <vector>

#include "../../include/ppals.h"
#include "backend.h"
#include "preload_policy.h"
#include "engine.h"
#include "assignment.h"
#include "tucker.h"

using namespace ppals;

static thread_local std::string g_err;

struct ppals_ctx {
  Ops *ops = nullptr;
  Comm *comm = nullptr;
  SelfComm self;
  Comm &c() { return comm ? *comm : self; }
  // Live children. A caller should destroy sessions, then tensors, then the context; a garbage-
  // collected binding (or an exception on the way out) may not. ppals_ctx_destroy therefore tears
  // down whatever is still alive itself and leaves the orphaned handles DEAD (eng / data null):
  // destroying them later is a no-op, using them an error — never a use-after-free of the device.
  std::set<ppals_cp *> cps;
  std::set<ppals_cp_multi *> multis;
  std::set<ppals_tucker *> tks;
  std::set<ppals_tensor *> tensors;
  std::set<struct ppals_parafac2 *> p2s;
};
struct ppals_tensor {
  ppals_ctx *ctx;
  TensorDesc d;
  DeviceBuffer data;        // owns d.data (empty in a dead handle)
  uint64_t generation = 1;  // bumped by every fill / upload; sessions rebuild what they derived
  uint64_t prep_epoch = 0;  // bumped by center / shift / scale / rescale (TensorDesc::prep_epoch)
};
struct ppals_cp {
  ppals_ctx *ctx;
  CpEngine *eng;
};
struct ppals_cp_multi {
  ppals_ctx *ctx;
  CpEngine *eng;  // nstarts * R columns, start-major (engine.h)
};
struct ppals_tucker {
  ppals_ctx *ctx;
  TuckerEngine *eng;
};
// PARAFAC2: the owner of the compressed tensor Y (R x J x K), of the rank-R session on it and of the
// projections. Y and cp are ordinary handles of the context (it leaves them dead like any other when it goes
// first); the device buffers are this object's.
struct ppals_parafac2 {
  ppals_ctx *ctx;
  int64_t I, J, K;
  int R;
  ppals_tensor *Y;
  ppals_cp *cp;
  DeviceBuffer P, Q, T, out;  // I x R x K twice, R x R x K, 3 doubles
  DeviceBuffer status;        // K ints
  // slices of unequal length (ppals_parafac2_create_ragged): I is 0, slice k has rows[k] rows, roff is their
  // prefix sum (K + 1 entries, roff[K] = N), P and Q hold R N doubles with P_k at R roff[k]
  bool ragged = false;
  std::vector<int64_t> rows, roff;
  int64_t tiles = 0;             // sum of ceil(rows[k] / 64)
  DeviceBuffer tab;              // rows[K] | roff[K] (int64), then tile0[K] | tile_slice[tiles] (int)
  DeviceBuffer xv;               // the view of the last step: offsets[K] | col_strides[K] (int64)
  std::vector<int64_t> xv_host;  // what xv holds (empty before the first step)
};

#define API_BEGIN try {
#define API_END(code)                     \
  }                                       \
  catch (const ppals::Unsupported &e) {   \
    g_err = e.what();                     \
    return PPALS_ERR_UNSUPPORTED;         \
  }                                       \
  catch (const std::exception &e) {       \
    g_err = e.what();                     \
    return code;                          \
  }                                       \
  catch (...) {                           \
    g_err = "ppals: unknown exception";   \
    return code;                          \
  }

static int fail(int code, const char *msg) {
  g_err = msg;
  return code;
}
static int fail_fn(int code, const char *fn, const char *what) {
  g_err = std::string(fn) + ": " + what;
  return code;
}

extern "C" {

const char *ppals_last_error(void) { return g_err.c_str(); }
const char *ppals_version(void) { return backend_name(); }

int ppals_preload_eigensolver(void) {
  API_BEGIN
  backend_preload_eigensolver();
  return PPALS_OK;
  API_END(PPALS_ERR_UNSUPPORTED)
}
int ppals_ctx_create(ppals_ctx **out, int device) {
  if (!out) return fail(PPALS_ERR_ARG, "ppals_ctx_create: out is NULL");
  *out = nullptr;
  API_BEGIN
  std::unique_ptr<ppals_ctx> c(new ppals_ctx);
  c->ops = backend_make_ops(device);  // throws when no HIP device: there is no CPU fallback
  *out = c.release();
  return PPALS_OK;
  API_END(PPALS_ERR_NO_DEVICE)
}
static void p2_free_buffers(ppals_parafac2 *p) {
  for (DeviceBuffer *b : {&p->P, &p->Q, &p->T, &p->out, &p->status, &p->tab, &p->xv}) {
    try {
      b->reset();
    } catch (...) {
    }
  }
}
void ppals_ctx_destroy(ppals_ctx *ctx) {
  if (!ctx) return;
  for (ppals_parafac2 *p : ctx->p2s) {  // (its session and tensor are in the sets below)
    p2_free_buffers(p);
    p->ctx = nullptr;
  }
  for (ppals_cp *s : ctx->cps) {
    delete s->eng;
    s->eng = nullptr;
    s->ctx = nullptr;
  }
  for (ppals_cp_multi *s : ctx->multis) {
    delete s->eng;
    s->eng = nullptr;
    s->ctx = nullptr;
  }
  for (ppals_tucker *s : ctx->tks) {
    delete s->eng;
    s->eng = nullptr;
    s->ctx = nullptr;
  }
  for (ppals_tensor *t : ctx->tensors) {
    try {
      t->data.reset();
    } catch (...) {
    }
    t->d.data = nullptr;
    t->ctx = nullptr;
  }
  delete ctx->comm;
  delete ctx->ops;
  delete ctx;
}
int ppals_get_unique_id(void *out128) {
  API_BEGIN
  backend_unique_id(out128);
  return PPALS_OK;
  API_END(PPALS_ERR_COMM)
}
int ppals_ctx_init_comm(ppals_ctx *ctx, int rank, int nranks, const void *uid) {
  if (!ctx) return fail(PPALS_ERR_ARG, "ctx is NULL");
  API_BEGIN
  if (nranks < 1 || rank < 0 || rank >= nranks) return fail(PPALS_ERR_ARG, "bad rank / nranks");
  // one rank needs no communicator; PPALS_FORCE_COMM=1 (tests) still builds a real one
  if (nranks == 1 && !force_comm_path()) return PPALS_OK;
  ctx->comm = backend_make_comm(ctx->ops, rank, nranks, uid);
  return PPALS_OK;
  API_END(PPALS_ERR_COMM)
}
int ppals_ctx_rank(const ppals_ctx *ctx) { return ctx && ctx->comm ? ctx->comm->rank() : 0; }
int ppals_ctx_nranks(const ppals_ctx *ctx) { return ctx && ctx->comm ? ctx->comm->size() : 1; }
int ppals_ctx_sync(ppals_ctx *ctx) {
  API_BEGIN
  ctx->ops->sync();
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_profile_enable(ppals_ctx *ctx, int on) {
  API_BEGIN
  ctx->ops->profile_enable(on < 0 ? 0 : on);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_profile_read(ppals_ctx *ctx, int which, int64_t *launches, double *total_ms,
                       double *algo_bytes) {
  if (which < 0 || which > 1) return fail(PPALS_ERR_ARG, "which must be 0 or 1");
  API_BEGIN
  ctx->ops->profile_collect();
  if (launches) *launches = ctx->ops->prof[which].launches;
  if (total_ms) *total_ms = ctx->ops->prof[which].ms;
  if (algo_bytes) *algo_bytes = ctx->ops->prof[which].bytes;
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_profile_reset(ppals_ctx *ctx) {
  API_BEGIN
  ctx->ops->profile_collect();
  ctx->ops->prof[0] = ProfileSlot();
  ctx->ops->prof[1] = ProfileSlot();
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}

// ------------------------------------------------------------------ tensor
int ppals_tensor_create(ppals_ctx *ctx, int order, const int64_t *global_lens, int dtype,
                        ppals_tensor **out) {
  if (!ctx || !global_lens || !out) return fail(PPALS_ERR_ARG, "NULL argument");
  if (dtype != PPALS_F32 && dtype != PPALS_F64 && dtype != PPALS_BF16) return fail(PPALS_ERR_ARG, "bad dtype");
  API_BEGIN
  std::unique_ptr<ppals_tensor> t(new ppals_tensor);
  t->ctx = ctx;
  std::string err;
  if (tensor_create(*ctx->ops, ctx->c(), order, global_lens, dtype, &t->d, &err) != 0) {
    g_err = "ppals_tensor_create: " + err;
    return PPALS_ERR_ARG;
  }
  t->data = DeviceBuffer(*ctx->ops, t->d.data, (size_t)t->d.nloc * dtype_size(dtype));
  t->d.generation = &t->generation;
  t->d.prep_epoch = &t->prep_epoch;
  ctx->tensors.insert(t.get());
  *out = t.release();
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
void ppals_tensor_destroy(ppals_tensor *t) {
  if (!t) return;
  if (t->ctx) {
    try {
      t->data.reset();
    } catch (...) {
    }
    t->ctx->tensors.erase(t);
  }
  delete t;
}
int ppals_tensor_local_rows(const ppals_tensor *t, int64_t *lo, int64_t *n) {
  if (!t || !t->ctx) return fail(PPALS_ERR_ARG, "NULL tensor");
  if (lo) *lo = t->d.row0;
  if (n) *n = t->d.llens[0];
  return PPALS_OK;
}
int ppals_tensor_fill_cp(ppals_tensor *t, int R, const double *Wtrue_flat) {
  if (!t || !t->ctx || !Wtrue_flat || R <= 0) return fail(PPALS_ERR_ARG, "bad argument");
  API_BEGIN
  t->generation++;
  tensor_fill_cp(*t->ctx->ops, t->d, R, Wtrue_flat);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_tensor_fill_uniform(ppals_tensor *t, uint64_t seed, double lo, double hi) {
  if (!t || !t->ctx) return fail(PPALS_ERR_ARG, "NULL tensor");
  API_BEGIN
  t->generation++;
  tensor_fill_uniform(*t->ctx->ops, t->d, seed, lo, hi);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_tensor_fill_laplacian(ppals_tensor *t, int ndigits, int s) {
  if (!t || !t->ctx || ndigits < 2 || ndigits % 2 || s < 1) return fail(PPALS_ERR_ARG, "bad argument");
  API_BEGIN
  double total = 1, want = 1;
  for (int i = 0; i < t->d.order; i++) total *= (double)t->d.glens[i];
  for (int i = 0; i < ndigits; i++) want *= s;
  if (total != want) return fail(PPALS_ERR_ARG, "tensor extents do not hold size^dim elements");
  t->generation++;
  tensor_fill_laplacian(*t->ctx->ops, t->d, ndigits, s);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_tensor_fill_collinear(ppals_tensor *t, int R, double col_min, double col_max,
                                double ratio_noise, uint64_t seed) {
  if (!t || !t->ctx || R <= 0) return fail(PPALS_ERR_ARG, "bad argument (rank must be positive)");
  API_BEGIN
  t->generation++;
  tensor_fill_collinear(*t->ctx->ops, t->ctx->c(), t->d, R, col_min, col_max, ratio_noise, seed);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_collinear_factors(int order, const int64_t *lens, int R, double col_min, double col_max,
                            uint64_t seed, double *Wflat) {
  if (!lens || !Wflat || order < 1 || R <= 0) return fail(PPALS_ERR_ARG, "bad argument");
  API_BEGIN
  collinear_factors(lens, order, R, col_min, col_max, seed, Wflat);
  return PPALS_OK;
  API_END(PPALS_ERR_ARG)
}
int ppals_tensor_upload(ppals_tensor *t, const double *host_full) {
  if (!t || !t->ctx || !host_full) return fail(PPALS_ERR_ARG, "NULL argument");
  API_BEGIN
  t->generation++;
  tensor_upload(*t->ctx->ops, t->d, host_full);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_tensor_download(ppals_tensor *t, double *host_full) {
  if (!t || !t->ctx || !host_full) return fail(PPALS_ERR_ARG, "NULL argument");
  API_BEGIN
  tensor_download(*t->ctx->ops, t->d, host_full);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_tensor_norm(ppals_tensor *t, double *out) {
  if (!t || !t->ctx || !out) return fail(PPALS_ERR_ARG, "NULL argument");
  API_BEGIN
  *out = tensor_norm(*t->ctx->ops, t->ctx->c(), t->d);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}

// ------------------------------------------------------------------ preprocessing in place
// the checks all five calls share; nothing is launched, allocated or bumped before every check has passed
static int prep_check(ppals_tensor *t, int mode, const char *fn) {
  if (!t || !t->ctx) return fail_fn(PPALS_ERR_ARG, fn, "NULL tensor or a dead handle");
  if (mode < 0 || mode >= t->d.order)
    return fail_fn(PPALS_ERR_ARG, fn, ("mode " + std::to_string(mode) + " is outside [0, " +
                                       std::to_string(t->d.order) + ")").c_str());
  if (t->ctx->c().size() > 1)
    return fail_fn(PPALS_ERR_UNSUPPORTED, fn,
                   "a context of more than one rank is not supported (centring across the sharded mode needs a "
                   "collective of the size of the offsets)");
  return PPALS_OK;
}
// the contents change in place: sessions rebuild what they derived, Tucker sessions also forget their history
static void prep_bump(ppals_tensor *t) {
  t->generation++;
  t->prep_epoch++;
}
// an offsets buffer in device memory: the checks of the device views on L*T doubles at ptr
static int prep_check_device(ppals_ctx *ctx, const char *fn, const void *ptr, int64_t count) {
  Ops::PtrInfo info;
  std::string err;
  bool known = false;
  try {
    known = ctx->ops->device_ptr_info(ptr, &info, &err);
  } catch (const ppals::Unsupported &e) {  // a back end without device views
    return fail_fn(PPALS_ERR_UNSUPPORTED, fn, e.what());
  }
  if (!known || !info.is_device)
    return fail_fn(PPALS_ERR_ARG, fn,
                   ("the offsets pointer is not device memory of the context's device (" +
                    (err.empty() ? std::string("host, pinned host or managed memory") : err) +
                    "); a torch tensor must live on that device, and torch must be imported before libppals is "
                    "loaded so that both share one HIP runtime").c_str());
  if ((uintptr_t)ptr % sizeof(double))
    return fail_fn(PPALS_ERR_ARG, fn, "the offsets pointer is not aligned to 8 bytes");
  if (!dv_in_allocation((uint64_t)(uintptr_t)ptr, count * (int64_t)sizeof(double), info.base, info.size))
    return fail_fn(PPALS_ERR_ARG, fn,
                   ("the offsets span " + std::to_string(count * (int64_t)sizeof(double)) +
                    " bytes from the pointer, past the end of its allocation (" + std::to_string(info.size) +
                    " bytes, the pointer at offset " + std::to_string((uint64_t)(uintptr_t)ptr - info.base) + ")").c_str());
  return PPALS_OK;
}
int ppals_tensor_center(ppals_tensor *t, int mode, double *offsets, int where, void *stream) {
  static const char *fn = "ppals_tensor_center";
  API_BEGIN
  int rc = prep_check(t, mode, fn);
  if (rc != PPALS_OK) return rc;
  Ops &ops = *t->ctx->ops;
  if (!offsets) {
    prep_bump(t);
    tensor_center(ops, t->d, mode, nullptr);
    return PPALS_OK;
  }
  if (where != PPALS_HOST && where != PPALS_DEVICE) return fail_fn(PPALS_ERR_ARG, fn, "where must be PPALS_HOST or PPALS_DEVICE");
  const PrepShape s = prep_shape(t->d, mode);
  if (where == PPALS_DEVICE) {
    rc = prep_check_device(t->ctx, fn, offsets, s.L * s.T);
    if (rc != PPALS_OK) return rc;
    prep_bump(t);
    ops.join_stream(stream);
    tensor_center(ops, t->d, mode, offsets);
    ops.release_stream(stream);
    return PPALS_OK;
  }
  DeviceBuffer tmp(ops, sizeof(double) * s.L * s.T);
  prep_bump(t);
  tensor_center(ops, t->d, mode, tmp.as<double>());
  ops.d2h(offsets, tmp.as<double>(), sizeof(double) * s.L * s.T);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_tensor_shift(ppals_tensor *t, int mode, const double *offsets, int where, double alpha, void *stream) {
  static const char *fn = "ppals_tensor_shift";
  API_BEGIN
  int rc = prep_check(t, mode, fn);
  if (rc != PPALS_OK) return rc;
  if (!offsets) return fail_fn(PPALS_ERR_ARG, fn, "offsets is NULL");
  if (where != PPALS_HOST && where != PPALS_DEVICE) return fail_fn(PPALS_ERR_ARG, fn, "where must be PPALS_HOST or PPALS_DEVICE");
  if (!std::isfinite(alpha)) return fail_fn(PPALS_ERR_ARG, fn, "alpha is not finite");
  Ops &ops = *t->ctx->ops;
  const PrepShape s = prep_shape(t->d, mode);
  if (where == PPALS_DEVICE) {
    rc = prep_check_device(t->ctx, fn, offsets, s.L * s.T);
    if (rc != PPALS_OK) return rc;
    prep_bump(t);
    ops.join_stream(stream);
    tensor_shift(ops, t->d, mode, offsets, alpha);
    ops.release_stream(stream);
    return PPALS_OK;
  }
  DeviceBuffer tmp(ops, sizeof(double) * s.L * s.T);
  ops.h2d(tmp.as<double>(), offsets, sizeof(double) * s.L * s.T);
  prep_bump(t);
  tensor_shift(ops, t->d, mode, tmp.as<double>(), alpha);
  tmp.reset();  // (waits for the launch: the host buffer has been consumed long before)
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_tensor_slice_sumsq(ppals_tensor *t, int mode, double *ss) {
  static const char *fn = "ppals_tensor_slice_sumsq";
  API_BEGIN
  const int rc = prep_check(t, mode, fn);
  if (rc != PPALS_OK) return rc;
  if (!ss) return fail_fn(PPALS_ERR_ARG, fn, "ss is NULL");
  tensor_slice_sumsq(*t->ctx->ops, t->d, mode, ss);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_tensor_scale(ppals_tensor *t, int mode, double *scales) {
  static const char *fn = "ppals_tensor_scale";
  API_BEGIN
  const int rc = prep_check(t, mode, fn);
  if (rc != PPALS_OK) return rc;
  prep_bump(t);
  tensor_scale(*t->ctx->ops, t->d, mode, scales);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_tensor_rescale(ppals_tensor *t, int mode, const double *factors) {
  static const char *fn = "ppals_tensor_rescale";
  API_BEGIN
  const int rc = prep_check(t, mode, fn);
  if (rc != PPALS_OK) return rc;
  if (!factors) return fail_fn(PPALS_ERR_ARG, fn, "factors is NULL");
  for (int64_t x = 0; x < t->d.llens[mode]; x++)
    if (!std::isfinite(factors[x]))
      return fail_fn(PPALS_ERR_ARG, fn, ("factors[" + std::to_string(x) + "] is not finite").c_str());
  prep_bump(t);
  tensor_rescale(*t->ctx->ops, t->d, mode, factors);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}

// ------------------------------------------------------------------ N-PLS regression
// (the tensor is only read: nothing is bumped; the checks of the handle, the mode and the ranks are prep_check's)
struct ppals_npls {
  NplsModel m;
};
static int npls_check_finite(const double *a, int64_t n, const char *fn, const char *name) {
  for (int64_t i = 0; i < n; i++)
    if (!std::isfinite(a[i]))
      return fail_fn(PPALS_ERR_ARG, fn, (std::string(name) + "[" + std::to_string(i) + "] is not finite").c_str());
  return PPALS_OK;
}
int ppals_tensor_contract_mode(ppals_tensor *t, int mode, const double *U, int C, double *Z) {
  static const char *fn = "ppals_tensor_contract_mode";
  API_BEGIN
  const int rc = prep_check(t, mode, fn);
  if (rc != PPALS_OK) return rc;
  if (!U || !Z) return fail_fn(PPALS_ERR_ARG, fn, "U or Z is NULL");
  if (C < 1) return fail_fn(PPALS_ERR_ARG, fn, "C must be at least 1");
  tensor_contract_mode(*t->ctx->ops, t->d, mode, U, C, Z);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_tensor_slice_inner(ppals_tensor *t, int mode, const double *W, int C, double *S) {
  static const char *fn = "ppals_tensor_slice_inner";
  API_BEGIN
  const int rc = prep_check(t, mode, fn);
  if (rc != PPALS_OK) return rc;
  if (!W || !S) return fail_fn(PPALS_ERR_ARG, fn, "W or S is NULL");
  if (C < 1) return fail_fn(PPALS_ERR_ARG, fn, "C must be at least 1");
  tensor_slice_inner(*t->ctx->ops, t->d, mode, W, C, S);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_tensor_contract_columns(ppals_tensor *t, int mode, const double *U, int C, double *Z) {
  static const char *fn = "ppals_tensor_contract_columns";
  API_BEGIN
  const int rc = prep_check(t, mode, fn);
  if (rc != PPALS_OK) return rc;
  if (!U || !Z) return fail_fn(PPALS_ERR_ARG, fn, "U or Z is NULL");
  if (C < 1) return fail_fn(PPALS_ERR_ARG, fn, "C must be at least 1");
  tensor_contract_columns(*t->ctx->ops, t->d, mode, U, C, Z);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_tensor_slice_inner_columns(ppals_tensor *t, int mode, const double *W, int C, double *S) {
  static const char *fn = "ppals_tensor_slice_inner_columns";
  API_BEGIN
  const int rc = prep_check(t, mode, fn);
  if (rc != PPALS_OK) return rc;
  if (!W || !S) return fail_fn(PPALS_ERR_ARG, fn, "W or S is NULL");
  if (C < 1) return fail_fn(PPALS_ERR_ARG, fn, "C must be at least 1");
  tensor_slice_inner_columns(*t->ctx->ops, t->d, mode, W, C, S);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
// the options of a fit or a cross-validation, checked; opts == NULL: the defaults
static int npls_take_opts(const ppals_npls_opts *opts, const char *fn, NplsOpts *o) {
  if (!opts) return PPALS_OK;
  o->hopm_tol = opts->hopm_tol;
  o->hopm_max = opts->hopm_max;
  o->inner_tol = opts->inner_tol;
  o->inner_max = opts->inner_max;
  if (!(o->hopm_tol >= 0) || !(o->inner_tol >= 0)) return fail_fn(PPALS_ERR_ARG, fn, "a tolerance is negative or NaN");
  if (o->hopm_max < 1 || o->inner_max < 1) return fail_fn(PPALS_ERR_ARG, fn, "hopm_max and inner_max must be at least 1");
  return PPALS_OK;
}
int ppals_npls_crossval(ppals_tensor *X, int mode, const double *Y, int M, int F, const int32_t *segment, int S,
                        int center, const ppals_npls_opts *opts, double *Ycv, double *press, int *fitted, int *status,
                        int64_t *x_passes) {
  static const char *fn = "ppals_npls_crossval";
  API_BEGIN
  int rc = prep_check(X, mode, fn);
  if (rc != PPALS_OK) return rc;
  if (!Y || !segment || !Ycv) return fail_fn(PPALS_ERR_ARG, fn, "Y, segment or Ycv is NULL");
  if (X->d.order < 2) return fail_fn(PPALS_ERR_ARG, fn, "the tensor must have at least two modes");
  if (M < 1) return fail_fn(PPALS_ERR_ARG, fn, "M must be at least 1");
  if (F < 1) return fail_fn(PPALS_ERR_ARG, fn, "F must be at least 1");
  if (center != 0 && center != 1) return fail_fn(PPALS_ERR_ARG, fn, "center must be 0 or 1");
  const int64_t I = X->d.llens[mode];
  if (S < 2 || S > I)
    return fail_fn(PPALS_ERR_ARG, fn, ("S = " + std::to_string(S) + " is outside [2, " + std::to_string(I) +
                                       "], the number of samples").c_str());
  std::vector<int64_t> count((size_t)S, 0);
  for (int64_t i = 0; i < I; i++) {
    if (segment[i] < 0 || segment[i] >= S)
      return fail_fn(PPALS_ERR_ARG, fn, ("segment[" + std::to_string(i) + "] = " + std::to_string(segment[i]) +
                                         " is outside [0, " + std::to_string(S) + ")").c_str());
    count[(size_t)segment[i]]++;
  }
  int64_t largest = 0;
  for (int g = 0; g < S; g++) {
    if (!count[(size_t)g]) return fail_fn(PPALS_ERR_ARG, fn, ("segment " + std::to_string(g) + " is empty").c_str());
    largest = std::max(largest, count[(size_t)g]);
  }
  if (F > I - largest - center)
    return fail_fn(PPALS_ERR_ARG, fn, ("F = " + std::to_string(F) + " is larger than " + std::to_string(I - largest - center) +
                                       ", the smallest training set" + (center ? " less one for the mean" : "")).c_str());
  NplsOpts o;
  rc = npls_take_opts(opts, fn, &o);
  if (rc != PPALS_OK) return rc;
  rc = npls_check_finite(Y, I * M, fn, "Y");
  if (rc != PPALS_OK) return rc;
  npls_crossval(*X->ctx->ops, X->d, mode, Y, M, F, segment, S, center, o, Ycv, press, fitted, status, x_passes);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_npls_fit(ppals_tensor *X, int mode, const double *Y, int M, int F, const ppals_npls_opts *opts,
                   ppals_npls **out) {
  static const char *fn = "ppals_npls_fit";
  if (out) *out = nullptr;
  API_BEGIN
  int rc = prep_check(X, mode, fn);
  if (rc != PPALS_OK) return rc;
  if (!Y || !out) return fail_fn(PPALS_ERR_ARG, fn, "Y or out is NULL");
  if (X->d.order < 2) return fail_fn(PPALS_ERR_ARG, fn, "the tensor must have at least two modes");
  if (M < 1) return fail_fn(PPALS_ERR_ARG, fn, "M must be at least 1");
  const int64_t I = X->d.llens[mode];
  if (F < 1 || F > I)
    return fail_fn(PPALS_ERR_ARG, fn, ("F = " + std::to_string(F) + " is outside [1, " + std::to_string(I) +
                                       "], the number of samples").c_str());
  NplsOpts o;
  rc = npls_take_opts(opts, fn, &o);
  if (rc != PPALS_OK) return rc;
  rc = npls_check_finite(Y, I * M, fn, "Y");
  if (rc != PPALS_OK) return rc;
  std::unique_ptr<ppals_npls> m(new ppals_npls);
  npls_fit(*X->ctx->ops, X->d, mode, Y, M, F, o, &m->m);
  *out = m.release();
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
void ppals_npls_destroy(ppals_npls *m) { delete m; }
int ppals_npls_dims(const ppals_npls *m, int *order, int *mode, int64_t *lens, int *M, int *wanted, int *fitted) {
  if (!m) return fail_fn(PPALS_ERR_ARG, "ppals_npls_dims", "NULL model");
  if (order) *order = m->m.order;
  if (mode) *mode = m->m.mode;
  if (lens)
    for (int i = 0; i < m->m.order; i++) lens[i] = m->m.lens[i];
  if (M) *M = m->m.M;
  if (wanted) *wanted = m->m.F;
  if (fitted) *fitted = m->m.nf;
  return PPALS_OK;
}
int ppals_npls_get(const ppals_npls *m, int what, double *out, int64_t *n) {
  static const char *fn = "ppals_npls_get";
  if (!m) return fail_fn(PPALS_ERR_ARG, fn, "NULL model");
  API_BEGIN
  const NplsModel &d = m->m;
  std::vector<double> st;
  const std::vector<double> *src = nullptr;
  switch (what) {
    case PPALS_NPLS_T: src = &d.T; break;
    case PPALS_NPLS_U: src = &d.U; break;
    case PPALS_NPLS_Q: src = &d.Q; break;
    case PPALS_NPLS_B: src = &d.B; break;
    case PPALS_NPLS_SSX: src = &d.ssx; break;
    case PPALS_NPLS_SSY: src = &d.ssy; break;
    case PPALS_NPLS_STATUS:
      st.assign(d.status.begin(), d.status.end());
      src = &st;
      break;
    default:
      if (what >= PPALS_NPLS_W && what < PPALS_NPLS_W + d.order - 1) src = &d.W[(size_t)(what - PPALS_NPLS_W)];
  }
  if (!src) return fail_fn(PPALS_ERR_ARG, fn, ("there is no array " + std::to_string(what)).c_str());
  if (n) *n = (int64_t)src->size();
  if (out && !src->empty()) std::memcpy(out, src->data(), sizeof(double) * src->size());
  return PPALS_OK;
  API_END(PPALS_ERR_ARG)
}
int ppals_npls_predict(const ppals_npls *m, ppals_tensor *Xnew, int ncomp, double *Yhat, double *Tnew) {
  static const char *fn = "ppals_npls_predict";
  API_BEGIN
  if (!m) return fail_fn(PPALS_ERR_ARG, fn, "NULL model");
  const int rc = prep_check(Xnew, m->m.mode, fn);  // (the mode is the model's: in range whenever the orders agree)
  if (rc != PPALS_OK && (!Xnew || !Xnew->ctx || Xnew->d.order == m->m.order)) return rc;
  if (Xnew->d.order != m->m.order)
    return fail_fn(PPALS_ERR_ARG, fn, ("the tensor has " + std::to_string(Xnew->d.order) + " modes, the model " +
                                       std::to_string(m->m.order)).c_str());
  for (int i = 0; i < m->m.order; i++)
    if (i != m->m.mode && Xnew->d.llens[i] != m->m.lens[i])
      return fail_fn(PPALS_ERR_ARG, fn, ("mode " + std::to_string(i) + " has extent " + std::to_string(Xnew->d.llens[i]) +
                                         ", the model's has " + std::to_string(m->m.lens[i])).c_str());
  if (ncomp < 1 || ncomp > m->m.nf)
    return fail_fn(PPALS_ERR_ARG, fn, ("ncomp = " + std::to_string(ncomp) + " is outside [1, " +
                                       std::to_string(m->m.nf) + "], the components fitted").c_str());
  if (!Yhat) return fail_fn(PPALS_ERR_ARG, fn, "Yhat is NULL");
  npls_predict(*Xnew->ctx->ops, m->m, Xnew->d, ncomp, Yhat, Tnew);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}

// ------------------------------------------------------------------ device views
// every check of ppals_tensor_check_device_view; on success *a holds the resolved view
// (`what` names the entry point in the messages; the model exports check their views here too)
// (the half that asks the runtime about the pointer, after dv_check_args has resolved *a)
static int check_view_ptr(ppals_ctx *ctx, const char *what, const void *ptr, const ViewArgs *a) {
  std::string err;
  Ops::PtrInfo info;
  if (!ctx->ops->device_ptr_info(ptr, &info, &err) || !info.is_device) {
    g_err = std::string(what) + "the pointer is not device memory of the context's device (" +
            (err.empty() ? "host, pinned host or managed memory" : err) +
            "); a torch tensor must live on that device, and torch must be imported before "
            "libppals is loaded so that both share one HIP runtime";
    return PPALS_ERR_ARG;
  }
  if (!dv_in_allocation((uint64_t)(uintptr_t)ptr, a->span, info.base, info.size)) {
    g_err = std::string(what) + "the view spans " + std::to_string(a->span) +
            " bytes from the pointer, past the end of its allocation (" + std::to_string(info.size) +
            " bytes, the pointer at offset " + std::to_string((uint64_t)(uintptr_t)ptr - info.base) + ")";
    return PPALS_ERR_ARG;
  }
  return PPALS_OK;
}
static int check_desc_view(ppals_ctx *ctx, const TensorDesc &d, const char *what, int dir,
                           const void *ptr, int dtype, const int64_t *box_lo, const int64_t *box_len,
                           const int64_t *strides, ViewArgs *a, bool mask = false) {
  std::string err;
  if (!dv_check_args(dir, d.order, d.glens, dtype, box_lo, box_len, strides, a, &err, mask)) {
    g_err = what + err;
    return PPALS_ERR_ARG;
  }
  return check_view_ptr(ctx, what, ptr, a);
}
static int check_view(ppals_tensor *t, int dir, const void *ptr, int dtype, const int64_t *box_lo,
                      const int64_t *box_len, const int64_t *strides, ViewArgs *a) {
  if (!t || !t->ctx || !ptr) return fail(PPALS_ERR_ARG, "NULL tensor or pointer");
  return check_desc_view(t->ctx, t->d,
                         dir == DV_EXPORT ? "ppals_tensor_export_device: " : "ppals_tensor_import_device: ",
                         dir, ptr, dtype, box_lo, box_len, strides, a);
}
static int copy_device_view(ppals_tensor *t, int dir, void *ptr, int dtype, const int64_t *box_lo,
                            const int64_t *box_len, const int64_t *strides, void *stream) {
  ViewArgs a;
  const int rc = check_view(t, dir, ptr, dtype, box_lo, box_len, strides, &a);
  if (rc != PPALS_OK) return rc;
  const ViewPlan p = dv_plan(a, t->d.glens, t->d.row0, t->d.llens[0]);
  if (dir == DV_IMPORT) t->generation++;
  if (p.kind != DV_EMPTY) t->ctx->ops->copy_view(p, dir, ptr, dtype, t->d.data, t->d.dtype, stream);
  return PPALS_OK;
}
int ppals_tensor_check_device_view(ppals_tensor *t, int direction, const void *ptr, int dtype,
                                   const int64_t *box_lo, const int64_t *box_len,
                                   const int64_t *strides) {
  API_BEGIN
  ViewArgs a;
  return check_view(t, direction, ptr, dtype, box_lo, box_len, strides, &a);
  API_END(PPALS_ERR_HIP)
}
int ppals_tensor_import_device(ppals_tensor *t, const void *src, int src_dtype, const int64_t *box_lo,
                               const int64_t *box_len, const int64_t *strides, void *stream) {
  API_BEGIN
  return copy_device_view(t, DV_IMPORT, const_cast<void *>(src), src_dtype, box_lo, box_len,
                          strides, stream);
  API_END(PPALS_ERR_HIP)
}
int ppals_tensor_export_device(ppals_tensor *t, void *dst, int dst_dtype, const int64_t *box_lo,
                               const int64_t *box_len, const int64_t *strides, void *stream) {
  API_BEGIN
  return copy_device_view(t, DV_EXPORT, dst, dst_dtype, box_lo, box_len, strides, stream);
  API_END(PPALS_ERR_HIP)
}

static inline uint64_t sm64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
void ppals_fill_uniform_host(double *out, int64_t n, uint64_t seed, uint64_t offset, double lo,
                             double hi) {
  const uint64_t s = sm64(seed);
  for (int64_t i = 0; i < n; i++) {
    uint64_t h = sm64(s ^ (offset + (uint64_t)i));
    out[i] = lo + (hi - lo) * ((double)(h >> 11) * (1.0 / 9007199254740992.0));
  }
}

// ------------------------------------------------------------------ CP
int ppals_cp_create(ppals_ctx *ctx, ppals_tensor *V, int R, ppals_cp **out) {
  if (!ctx || !V || !out) return fail(PPALS_ERR_ARG, "NULL argument");
  if (R <= 0) return fail(PPALS_ERR_ARG, "rank must be positive");
  API_BEGIN
  std::unique_ptr<ppals_cp> s(new ppals_cp);
  s->ctx = ctx;
  s->eng = new CpEngine(*ctx->ops, ctx->c(), V->d, R);
  ctx->cps.insert(s.get());
  *out = s.release();
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
void ppals_cp_destroy(ppals_cp *s) {
  if (!s) return;
  delete s->eng;
  if (s->ctx) s->ctx->cps.erase(s);
  delete s;
}
static_assert(PPALS_NN_FLOOR == ppals::kNnFloor, "the ABI's floor is the one the update applies");
int ppals_cp_set_factors(ppals_cp *s, const double *Wflat, const double *gradWflat) {
  if (!s || !s->eng || !Wflat) return fail(PPALS_ERR_ARG, "NULL argument");
  API_BEGIN
  if (s->eng->nonneg_modes()) {  // Wflat is on the host: looked at here, before anything is uploaded
    const bool all = s->eng->nonneg();
    size_t at = 0;
    for (int i = 0; i < s->eng->order(); i++) {  // (the NONNEG modes' blocks)
      const size_t n = (size_t)s->eng->tensor().glens[i] * s->eng->rank_r();
      if (s->eng->mode_kind(i) == ppals::kModeNonneg)
        for (size_t e = at; e < at + n; e++)
          if (!(Wflat[e] >= 0) || !std::isfinite(Wflat[e]))
            return fail(PPALS_ERR_ARG,
                        all ? "ppals_cp_set_factors: a non-negative session takes finite factors >= 0"
                            : "ppals_cp_set_factors: a non-negative mode takes a finite factor >= 0");
      at += n;
    }
  }
  s->eng->set_factors(Wflat, gradWflat);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_cp_get_factors(ppals_cp *s, double *Wflat, double *gradWflat) {
  if (!s || !s->eng) return fail(PPALS_ERR_ARG, "NULL argument");
  API_BEGIN
  s->eng->get_factors(Wflat, gradWflat);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_cp_set_schedule(ppals_cp *s, int schedule) {
  if (!s || !s->eng) return fail(PPALS_ERR_ARG, "NULL session");
  if (schedule != PPALS_SCHEDULE_DT && schedule != PPALS_SCHEDULE_MSDT)
    return fail(PPALS_ERR_ARG, "schedule must be PPALS_SCHEDULE_DT or PPALS_SCHEDULE_MSDT");
  API_BEGIN
  s->eng->set_schedule(schedule);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_cp_get_schedule(const ppals_cp *s) { return s && s->eng ? s->eng->schedule() : PPALS_ERR_ARG; }
int ppals_cp_set_nonneg(ppals_cp *s, int on) {
  if (!s || !s->eng) return fail(PPALS_ERR_ARG, "NULL session");
  API_BEGIN
  const bool was = s->eng->nonneg();
  int before[ppals::MAX_ORDER];  // (all FREE unless ppals_cp_set_mode_constraints was used)
  for (int i = 0; i < s->eng->order(); i++) before[i] = s->eng->mode_kind(i);
  s->eng->set_nonneg(on != 0);
  if (on && !was && !s->eng->factors_nonneg()) {
    s->eng->restore_mode_kinds(before);
    return fail(PPALS_ERR_ARG, "ppals_cp_set_nonneg: the session's factors have a negative or non-finite entry");
  }
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_cp_get_nonneg(const ppals_cp *s) { return s && s->eng ? (s->eng->nonneg() ? 1 : 0) : PPALS_ERR_ARG; }
static_assert(PPALS_ORTHO_MIN_RATIO == ppals::kOrthoMinRatio, "the ABI's ratio is the one the update applies");
static_assert(PPALS_MODE_FREE == ppals::kModeFree && PPALS_MODE_NONNEG == ppals::kModeNonneg &&
                  PPALS_MODE_FIXED == ppals::kModeFixed && PPALS_MODE_ORTHO == ppals::kModeOrtho,
              "the ABI's kinds are the engine's");
// (both kinds of session: everything is refused before the engine changes anything)
static int set_mode_constraints(CpEngine *e, const int *kinds, const char *fn, const char *whose) {
  if (!e) return fail_fn(PPALS_ERR_ARG, fn, "NULL session");
  if (!kinds) return fail_fn(PPALS_ERR_ARG, fn, "kinds is NULL");
  API_BEGIN
  std::string why;
  if (const int rc = e->check_mode_kinds(kinds, &why))
    return fail_fn(rc == 2 ? PPALS_ERR_UNSUPPORTED : PPALS_ERR_ARG, fn, why.c_str());
  unsigned look = 0;  // modes that become NONNEG: their factors are looked at, as ppals_cp_set_nonneg does
  for (int i = 0; i < e->order(); i++)
    if (kinds[i] == PPALS_MODE_NONNEG && e->mode_kind(i) != ppals::kModeNonneg) look |= 1u << i;
  if (look && !e->factors_nonneg(look))
    return fail_fn(PPALS_ERR_ARG, fn,
                   (std::string(whose) + " of a mode that becomes non-negative have a negative or non-finite entry")
                       .c_str());
  e->set_mode_kinds(kinds);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
static int get_mode_constraints(const CpEngine *e, int *kinds, const char *fn) {
  if (!e) return fail_fn(PPALS_ERR_ARG, fn, "NULL session");
  if (!kinds) return fail_fn(PPALS_ERR_ARG, fn, "kinds is NULL");
  for (int i = 0; i < e->order(); i++) kinds[i] = e->mode_kind(i);
  return PPALS_OK;
}
int ppals_cp_set_mode_constraints(ppals_cp *s, const int *kinds) {
  return set_mode_constraints(s ? s->eng : nullptr, kinds, "ppals_cp_set_mode_constraints", "the session's factors");
}
int ppals_cp_get_mode_constraints(const ppals_cp *s, int *kinds) {
  return get_mode_constraints(s ? s->eng : nullptr, kinds, "ppals_cp_get_mode_constraints");
}
static_assert(PPALS_SHAPE_NONE == ppals::kShapeNone && PPALS_SHAPE_UNIMODAL == ppals::kShapeUnimodal &&
                  PPALS_SHAPE_INCREASING == ppals::kShapeIncreasing && PPALS_SHAPE_DECREASING == ppals::kShapeDecreasing,
              "the ABI's shapes are the engine's");
// (both kinds of session: everything is refused before the engine changes anything)
static int set_mode_shapes(CpEngine *e, const int *shapes, const char *fn) {
  if (!e) return fail_fn(PPALS_ERR_ARG, fn, "NULL session");
  if (!shapes) return fail_fn(PPALS_ERR_ARG, fn, "shapes is NULL");
  API_BEGIN
  std::string why;
  if (const int rc = e->check_mode_shapes(shapes, &why))
    return fail_fn(rc == 2 ? PPALS_ERR_UNSUPPORTED : PPALS_ERR_ARG, fn, why.c_str());
  e->set_mode_shapes(shapes);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
static int get_mode_shapes(const CpEngine *e, int *shapes, const char *fn) {
  if (!e) return fail_fn(PPALS_ERR_ARG, fn, "NULL session");
  if (!shapes) return fail_fn(PPALS_ERR_ARG, fn, "shapes is NULL");
  for (int i = 0; i < e->order(); i++) shapes[i] = e->mode_shape(i);
  return PPALS_OK;
}
int ppals_cp_set_mode_shapes(ppals_cp *s, const int *shapes) {
  return set_mode_shapes(s ? s->eng : nullptr, shapes, "ppals_cp_set_mode_shapes");
}
int ppals_cp_get_mode_shapes(const ppals_cp *s, int *shapes) {
  return get_mode_shapes(s ? s->eng : nullptr, shapes, "ppals_cp_get_mode_shapes");
}
int ppals_cp_placement_report(const ppals_cp *s, char *buf, int cap) {
  if (!s || !s->eng || !buf || cap <= 0) return fail(PPALS_ERR_ARG, "NULL argument");
  API_BEGIN
  const std::string r = s->eng->placement_report();
  if ((int)r.size() + 1 > cap) return fail(PPALS_ERR_ARG, "buffer too small");
  std::memcpy(buf, r.c_str(), r.size() + 1);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_cp_pp_build_stats(ppals_cp *s, int mode, int64_t *builds, double *seconds) {
  if (!s || !s->eng) return fail(PPALS_ERR_ARG, "NULL argument");
  API_BEGIN
  s->eng->pp_build_stats(mode, builds, seconds);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_cp_sweeps_dt(ppals_cp *s, int n, double lambda) {
  if (!s || !s->eng) return fail(PPALS_ERR_ARG, "NULL argument");
  API_BEGIN
  for (int i = 0; i < n; i++) s->eng->sweep_dt(lambda);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_cp_gradnorm(ppals_cp *s, double *out) {
  if (!s || !s->eng || !out) return fail(PPALS_ERR_ARG, "NULL argument");
  API_BEGIN
  *out = s->eng->gradnorm();
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_cp_residual(ppals_cp *s, double *out) {
  if (!s || !s->eng || !out) return fail(PPALS_ERR_ARG, "NULL argument");
  API_BEGIN
  *out = s->eng->residual();
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
// the model exports: every check of ppals_tensor_export_device and of `what`, nothing launched
static int check_model_view(ppals_ctx *ctx, const TensorDesc &d, const char *what, int kind, void *dst,
                            int dst_dtype, const int64_t *box_lo, const int64_t *box_len,
                            const int64_t *strides, ViewArgs *a) {
  if (!dst) return fail(PPALS_ERR_ARG, "NULL pointer");
  if (kind != PPALS_MODEL && kind != PPALS_RESIDUAL) {
    g_err = std::string(what) + "`what` must be PPALS_MODEL (0) or PPALS_RESIDUAL (1)";
    return PPALS_ERR_ARG;
  }
  return check_desc_view(ctx, d, what, DV_EXPORT, dst, dst_dtype, box_lo, box_len, strides, a);
}
int ppals_cp_export_model_device(ppals_cp *s, int what, void *dst, int dst_dtype, const int64_t *box_lo,
                                 const int64_t *box_len, const int64_t *strides, void *stream) {
  if (!s || !s->eng) return fail(PPALS_ERR_ARG, "NULL session");
  API_BEGIN
  ViewArgs a;
  const int rc = check_model_view(s->ctx, s->eng->tensor(), "ppals_cp_export_model_device: ", what, dst,
                                  dst_dtype, box_lo, box_len, strides, &a);
  if (rc != PPALS_OK) return rc;
  s->eng->export_model(a, dst, what == PPALS_RESIDUAL, stream);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_tucker_export_model_device(ppals_tucker *s, int what, void *dst, int dst_dtype,
                                     const int64_t *box_lo, const int64_t *box_len,
                                     const int64_t *strides, void *stream) {
  if (!s || !s->eng) return fail(PPALS_ERR_ARG, "NULL session");
  API_BEGIN
  ViewArgs a;
  const int rc = check_model_view(s->ctx, s->eng->tensor(), "ppals_tucker_export_model_device: ", what,
                                  dst, dst_dtype, box_lo, box_len, strides, &a);
  if (rc != PPALS_OK) return rc;
  s->eng->export_model(a, dst, what == PPALS_RESIDUAL, stream);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
// the mask of an imputation: every check ppals_tensor_check_device_view makes of an import source, for a
// view of PPALS_U8 (a type the tensor import itself goes on refusing)
static int check_mask_view(ppals_ctx *ctx, const TensorDesc &d, const char *what, const void *mask,
                           const int64_t *box_lo, const int64_t *box_len, const int64_t *strides,
                           ViewArgs *a) {
  if (!mask) {
    g_err = std::string(what) + "the mask pointer is NULL";
    return PPALS_ERR_ARG;
  }
  return check_desc_view(ctx, d, what, DV_IMPORT, mask, DV_U8, box_lo, box_len, strides, a, true);
}
int ppals_cp_impute_device(ppals_cp *s, const void *mask, const int64_t *box_lo, const int64_t *box_len,
                           const int64_t *strides, void *stream, double *observed_sq) {
  if (!s || !s->eng || !s->ctx) return fail(PPALS_ERR_ARG, "NULL session");
  API_BEGIN
  ViewArgs a;
  const int rc = check_mask_view(s->ctx, s->eng->tensor(), "ppals_cp_impute_device: ", mask, box_lo, box_len,
                                 strides, &a);
  if (rc != PPALS_OK) return rc;
  s->eng->impute(a, mask, stream, observed_sq);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_tucker_impute_device(ppals_tucker *s, const void *mask, const int64_t *box_lo,
                               const int64_t *box_len, const int64_t *strides, void *stream,
                               double *observed_sq) {
  if (!s || !s->eng || !s->ctx) return fail(PPALS_ERR_ARG, "NULL session");
  API_BEGIN
  ViewArgs a;
  const int rc = check_mask_view(s->ctx, s->eng->tensor(), "ppals_tucker_impute_device: ", mask, box_lo,
                                 box_len, strides, &a);
  if (rc != PPALS_OK) return rc;
  s->eng->impute(a, mask, stream, observed_sq);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_tree_node(ppals_cp *s, const char *key, double *out, int64_t *n) {
  if (!s || !s->eng || !key) return fail(PPALS_ERR_ARG, "NULL argument");
  API_BEGIN
  int64_t c = s->eng->tree_node(key, out);
  if (c < 0) return fail(PPALS_ERR_ARG, "ppals_tree_node: not a node of the dimension tree");
  if (n) *n = c;
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_mttkrp(ppals_cp *s, int mode, double *M) {
  if (!s || !s->eng || !M) return fail(PPALS_ERR_ARG, "NULL argument");
  if (mode < 0 || mode >= s->eng->order()) return fail(PPALS_ERR_ARG, "mode out of range");
  API_BEGIN
  s->eng->mttkrp(mode, M);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_pp_operator(ppals_cp *s, const char *contracted, double *out, int64_t *n) {
  if (!s || !s->eng || !contracted) return fail(PPALS_ERR_ARG, "NULL argument");
  API_BEGIN
  int64_t c = s->eng->pp_operator(contracted, out);
  if (c < 0) return fail(PPALS_ERR_ARG, "ppals_pp_operator: bad mode string");
  if (n) *n = c;
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_cp_gram_system(ppals_cp *s, int mode, double lambda, double *S, double *Sinv) {
  if (!s || !s->eng || !S || !Sinv) return fail(PPALS_ERR_ARG, "NULL argument");
  if (mode < 0 || mode >= s->eng->order()) return fail(PPALS_ERR_ARG, "mode out of range");
  API_BEGIN
  s->eng->gram_system(mode, lambda, S, Sinv);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}

static CpOpts to_opts(const ppals_cp_opts *o) {
  CpOpts c;
  c.tol = o->tol;
  c.timelimit = o->timelimit;
  c.maxiter = o->maxiter;
  c.lambda = o->lambda;
  c.resprint = o->resprint > 0 ? o->resprint : 10;
  c.bench = o->bench;
  c.tol_init = o->tol_init;
  c.ratio_step = o->ratio_step;
  if (o->csv_path) c.csv_path = o->csv_path;
  c.csv_append = o->csv_append != 0;
  c.verbose = o->verbose != 0;
  c.update_percentage = o->update_percentage;
  return c;
}
int ppals_cp_dt(ppals_cp *s, const ppals_cp_opts *o, int *iters) {
  if (!s || !s->eng || !o) return fail(PPALS_ERR_ARG, "NULL argument");
  API_BEGIN
  return s->eng->run_dt(to_opts(o), iters);
  API_END(PPALS_ERR_HIP)
}
// (an all-NONNEG session keeps the engine's own message)
static bool mixed_constraints(const CpEngine *e) { return e->any_nonfree() && !e->nonneg(); }
int ppals_cp_pp(ppals_cp *s, const ppals_cp_opts *o, int *iters) {
  if (!s || !s->eng || !o) return fail(PPALS_ERR_ARG, "NULL argument");
  if (mixed_constraints(s->eng))
    return fail_fn(PPALS_ERR_UNSUPPORTED, "ppals_cp_pp",
                   "a session with constrained modes has no pairwise-perturbation driver");
  API_BEGIN
  return s->eng->run_pp(to_opts(o), iters);
  API_END(PPALS_ERR_HIP)
}

int ppals_cp_pp_partupdate(ppals_cp *s, const ppals_cp_opts *o, int *iters) {
  if (!s || !s->eng || !o) return fail(PPALS_ERR_ARG, "NULL argument");
  if (mixed_constraints(s->eng))
    return fail_fn(PPALS_ERR_UNSUPPORTED, "ppals_cp_pp_partupdate",
                   "a session with constrained modes has no pairwise-perturbation driver");
  API_BEGIN
  return s->eng->run_pp_partupdate(to_opts(o), iters);
  API_END(PPALS_ERR_HIP)
}
int ppals_cpd_als(ppals_cp *s, int optimizer, const ppals_cp_opts *o, double *sweeps, int *iters) {
  if (!s || !s->eng || !o) return fail(PPALS_ERR_ARG, "NULL argument");
  if (optimizer < PPALS_OPT_SIMPLE || optimizer > PPALS_OPT_MSDT)
    return fail(PPALS_ERR_ARG, "optimizer must be PPALS_OPT_SIMPLE, PPALS_OPT_DT or PPALS_OPT_MSDT");
  API_BEGIN
  return s->eng->run_class(optimizer, to_opts(o), sweeps, iters);
  API_END(PPALS_ERR_HIP)
}

int ppals_cpd_als_lr(ppals_cp *s, int optimizer, int update_rank, int randomsvd,
                     const ppals_cp_opts *o, double *sweeps, int *iters) {
  if (!s || !s->eng || !o) return fail(PPALS_ERR_ARG, "NULL argument");
  if (optimizer != PPALS_OPT_DT_LR && optimizer != PPALS_OPT_MSDT_LR)
    return fail(PPALS_ERR_ARG, "optimizer must be PPALS_OPT_DT_LR or PPALS_OPT_MSDT_LR");
  if (update_rank < 1 || update_rank > s->eng->rank_r())
    return fail(PPALS_ERR_ARG, "update_rank must be in [1, R]");
  if (randomsvd < 0 || randomsvd > 1) return fail(PPALS_ERR_ARG, "randomsvd must be 0 or 1");
  if (mixed_constraints(s->eng))
    return fail_fn(PPALS_ERR_UNSUPPORTED, "ppals_cpd_als_lr",
                   "a session with constrained modes has no low-rank-update optimizer");
  API_BEGIN
  CpOpts c = to_opts(o);
  c.update_rank = update_rank;
  c.randomsvd = randomsvd;
  return s->eng->run_class(optimizer, c, sweeps, iters);
  API_END(PPALS_ERR_HIP)
}

int ppals_cp_em(ppals_cp *s, const void *mask, const int64_t *box_lo, const int64_t *box_len,
                const int64_t *strides, void *stream, const ppals_cp_opts *o, int inner_sweeps,
                int *iters, double *observed_res) {
  API_BEGIN
  if (!o) return fail(PPALS_ERR_ARG, "ppals_cp_em: NULL options");
  if (inner_sweeps < 1) return fail(PPALS_ERR_ARG, "ppals_cp_em: inner_sweeps must be at least 1");
  if (o->maxiter < 0) return fail(PPALS_ERR_ARG, "ppals_cp_em: maxiter must not be negative");
  if (!s || !s->eng || !s->ctx) return fail(PPALS_ERR_ARG, "NULL session");
  ViewArgs a;
  const int rc = check_mask_view(s->ctx, s->eng->tensor(), "ppals_cp_em: ", mask, box_lo, box_len, strides, &a);
  if (rc != PPALS_OK) return rc;
  return s->eng->run_em(a, mask, stream, to_opts(o), inner_sweeps, iters, observed_res);
  API_END(PPALS_ERR_HIP)
}

// the two views of a weighted step: every check ppals_tensor_check_device_view makes of an import source,
// the arithmetic of both views (and what the session itself refuses) ahead of the pointer queries
// (weights_optional: the Huber step and the residual quantile take weights == NULL for h = 1 everywhere, and
// `w` is then left alone; `refusal`: what the session refuses for this entry point, or nullptr)
static int check_wls_views(ppals_cp *s, const char *fn, const void *data, const void *weights, int dtype,
                           const int64_t *box_lo, const int64_t *box_len, const int64_t *data_strides,
                           const int64_t *weight_strides, ViewArgs *a, ViewArgs *w, bool weights_optional = false,
                           const char *refusal = nullptr, bool own_refusal = false) {
  if (!data) return fail_fn(PPALS_ERR_ARG, fn, "the data pointer is NULL");
  if (!weights && !weights_optional) return fail_fn(PPALS_ERR_ARG, fn, "the weights pointer is NULL");
  if (dtype != PPALS_F32 && dtype != PPALS_F64)
    return fail_fn(PPALS_ERR_ARG, fn, "bad dtype of the data and weights views (PPALS_F32 or PPALS_F64)");
  const TensorDesc &d = s->eng->tensor();
  std::string err;
  if (!dv_check_args(DV_IMPORT, d.order, d.glens, dtype, box_lo, box_len, data_strides, a, &err))
    return fail_fn(PPALS_ERR_ARG, fn, ("the data view: " + err).c_str());
  if (weights && !dv_check_args(DV_IMPORT, d.order, d.glens, dtype, box_lo, box_len, weight_strides, w, &err))
    return fail_fn(PPALS_ERR_ARG, fn, ("the weights view: " + err).c_str());
  if (const char *why = own_refusal ? refusal : s->eng->wls_refusal()) return fail_fn(PPALS_ERR_UNSUPPORTED, fn, why);
  const std::string pre = std::string(fn) + ": ";
  if (const int rc = check_view_ptr(s->ctx, (pre + "the data view: ").c_str(), data, a)) return rc;
  return weights ? check_view_ptr(s->ctx, (pre + "the weights view: ").c_str(), weights, w) : PPALS_OK;
}
int ppals_cp_wls_device(ppals_cp *s, const void *data, const void *weights, int dtype, const int64_t *box_lo,
                        const int64_t *box_len, const int64_t *data_strides, const int64_t *weight_strides,
                        void *stream, double *weighted_sq) {
  if (!s || !s->eng || !s->ctx) return fail(PPALS_ERR_ARG, "NULL session");
  API_BEGIN
  ViewArgs a, w;
  const int rc = check_wls_views(s, "ppals_cp_wls_device", data, weights, dtype, box_lo, box_len, data_strides,
                                 weight_strides, &a, &w);
  if (rc != PPALS_OK) return rc;
  s->eng->wls_step(a, data, w, weights, stream, weighted_sq);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_cp_wls(ppals_cp *s, const void *data, const void *weights, int dtype, const int64_t *box_lo,
                 const int64_t *box_len, const int64_t *data_strides, const int64_t *weight_strides, void *stream,
                 const ppals_cp_opts *o, int inner_sweeps, double rel_change, int *iters, double *weighted_res) {
  API_BEGIN
  if (!o) return fail(PPALS_ERR_ARG, "ppals_cp_wls: NULL options");
  if (inner_sweeps < 1) return fail(PPALS_ERR_ARG, "ppals_cp_wls: inner_sweeps must be at least 1");
  if (!(rel_change >= 0)) return fail(PPALS_ERR_ARG, "ppals_cp_wls: rel_change must not be negative");
  if (o->maxiter < 0) return fail(PPALS_ERR_ARG, "ppals_cp_wls: maxiter must not be negative");
  if (!s || !s->eng || !s->ctx) return fail(PPALS_ERR_ARG, "NULL session");
  ViewArgs a, w;
  const int rc = check_wls_views(s, "ppals_cp_wls", data, weights, dtype, box_lo, box_len, data_strides,
                                 weight_strides, &a, &w);
  if (rc != PPALS_OK) return rc;
  return s->eng->run_wls(a, data, w, weights, stream, to_opts(o), inner_sweeps, rel_change, iters, weighted_res);
  API_END(PPALS_ERR_HIP)
}

// ------------------------------------------------------------------ robust CP (Huber)
int ppals_cp_huber_device(ppals_cp *s, const void *data, const void *weights, int dtype, const int64_t *box_lo,
                          const int64_t *box_len, const int64_t *data_strides, const int64_t *weight_strides,
                          double c, void *stream, double *huber_loss, int64_t *clipped) {
  if (!s || !s->eng || !s->ctx) return fail(PPALS_ERR_ARG, "NULL session");
  API_BEGIN
  if (!(c > 0)) return fail(PPALS_ERR_ARG, "ppals_cp_huber_device: c must be positive (+inf: no clipping)");
  ViewArgs a, w;
  const int rc = check_wls_views(s, "ppals_cp_huber_device", data, weights, dtype, box_lo, box_len, data_strides,
                                 weight_strides, &a, &w, true);
  if (rc != PPALS_OK) return rc;
  s->eng->huber_step(a, data, weights ? &w : nullptr, weights, stream, c, huber_loss, clipped);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_cp_robust(ppals_cp *s, const void *data, const void *weights, int dtype, const int64_t *box_lo,
                    const int64_t *box_len, const int64_t *data_strides, const int64_t *weight_strides, void *stream,
                    double c, const ppals_cp_opts *o, int inner_sweeps, double rel_change, int *iters,
                    double *robust_res) {
  API_BEGIN
  if (!o) return fail(PPALS_ERR_ARG, "ppals_cp_robust: NULL options");
  if (inner_sweeps < 1) return fail(PPALS_ERR_ARG, "ppals_cp_robust: inner_sweeps must be at least 1");
  if (!(rel_change >= 0)) return fail(PPALS_ERR_ARG, "ppals_cp_robust: rel_change must not be negative");
  if (o->maxiter < 0) return fail(PPALS_ERR_ARG, "ppals_cp_robust: maxiter must not be negative");
  if (!(c > 0)) return fail(PPALS_ERR_ARG, "ppals_cp_robust: c must be positive (+inf: no clipping)");
  if (!s || !s->eng || !s->ctx) return fail(PPALS_ERR_ARG, "NULL session");
  ViewArgs a, w;
  const int rc = check_wls_views(s, "ppals_cp_robust", data, weights, dtype, box_lo, box_len, data_strides,
                                 weight_strides, &a, &w, true);
  if (rc != PPALS_OK) return rc;
  return s->eng->run_robust(a, data, weights ? &w : nullptr, weights, stream, c, to_opts(o), inner_sweeps, rel_change,
                            iters, robust_res);
  API_END(PPALS_ERR_HIP)
}
int ppals_cp_abs_residual_quantile(ppals_cp *s, const void *data, const void *weights, int dtype,
                                   const int64_t *box_lo, const int64_t *box_len, const int64_t *data_strides,
                                   const int64_t *weight_strides, void *stream, double p, double *value,
                                   int64_t *count) {
  if (!s || !s->eng || !s->ctx) return fail(PPALS_ERR_ARG, "NULL session");
  API_BEGIN
  if (!(p >= 0 && p <= 1)) return fail(PPALS_ERR_ARG, "ppals_cp_abs_residual_quantile: p must lie in [0, 1]");
  if (!value) return fail(PPALS_ERR_ARG, "ppals_cp_abs_residual_quantile: NULL value");
  ViewArgs a, w;
  const int rc = check_wls_views(s, "ppals_cp_abs_residual_quantile", data, weights, dtype, box_lo, box_len,
                                 data_strides, weight_strides, &a, &w, true, s->eng->quantile_refusal(), true);
  if (rc != PPALS_OK) return rc;
  s->eng->abs_residual_quantile(a, data, weights ? &w : nullptr, weights, stream, p, value, count);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}

// ------------------------------------------------------------------ PARAFAC2
// the refusals both kinds of object share, after the extents: dtype, BF16, more than one rank
static int p2_check_create(ppals_ctx *ctx, const char *fn, int storage_dtype) {
  if (storage_dtype != PPALS_F32 && storage_dtype != PPALS_F64 && storage_dtype != PPALS_BF16)
    return fail_fn(PPALS_ERR_ARG, fn, "bad storage dtype");
  if (storage_dtype == PPALS_BF16)
    return fail_fn(PPALS_ERR_UNSUPPORTED, fn,
                   "BF16 storage is not supported: the loss identity needs Y = P^T X to a rounding well below the "
                   "residual it is compared with");
  if (ctx->c().size() > 1)
    return fail_fn(PPALS_ERR_UNSUPPORTED, fn,
                   "a context of more than one rank is not supported (the compressed tensor's leading mode is the "
                   "rank R and cannot be sharded usefully)");
  return PPALS_OK;
}
// Y, the inner session and its initial factors; on failure nothing is left behind
static int p2_create_inner(ppals_ctx *ctx, ppals_parafac2 *p, int storage_dtype) {
  const int R = p->R;
  const int64_t J = p->J, K = p->K;
  const int64_t lens[3] = {R, J, K};
  int rc = ppals_tensor_create(ctx, 3, lens, storage_dtype, &p->Y);
  if (rc == PPALS_OK) {
    ctx->ops->zero(p->Y->d.data, (size_t)p->Y->d.nloc * dtype_size(p->Y->d.dtype));
    rc = ppals_cp_create(ctx, p->Y, R, &p->cp);
  }
  if (rc == PPALS_OK) {  // B = I_R, A = the uniform generator's block of mode 1, C = 1
    std::vector<double> W((size_t)R * (R + J + K), 0.0);
    for (int r = 0; r < R; r++) W[(size_t)r * (R + 1)] = 1.0;
    ppals_fill_uniform_host(W.data() + (size_t)R * R, J * R, 1, 0, 0.0, 1.0);
    std::fill(W.begin() + (size_t)R * (R + J), W.end(), 1.0);
    rc = ppals_cp_set_factors(p->cp, W.data(), nullptr);
  }
  if (rc != PPALS_OK) {
    ppals_cp_destroy(p->cp);
    ppals_tensor_destroy(p->Y);
  }
  return rc;
}
// the buffers every object has but P and Q: T, out, status (zeroed)
static void p2_alloc_small(ppals_ctx *ctx, ppals_parafac2 *q) {
  q->T = DeviceBuffer(*ctx->ops, sizeof(double) * (size_t)q->R * q->R * q->K);
  q->out = DeviceBuffer(*ctx->ops, sizeof(double) * 3);
  q->status = DeviceBuffer(*ctx->ops, sizeof(int) * (size_t)q->K);
  ctx->ops->zero(q->status.get(), sizeof(int) * (size_t)q->K);
}
// the ragged step's description but for the view and `out`
static void p2_ragged_desc(ppals_parafac2 *p, Ops::Parafac2Ragged *out) {
  Ops::Parafac2Ragged s;
  s.J = p->J, s.K = p->K, s.R = p->R, s.tiles = p->tiles;
  s.rows = p->tab.as<int64_t>(), s.roff = s.rows + p->K;
  s.tile0 = (const int *)(s.roff + p->K), s.tile_slice = s.tile0 + p->K;
  s.xoff = p->xv.as<int64_t>(), s.xcs = s.xoff + p->K;
  s.Q = p->Q.as<double>(), s.P = p->P.as<double>(), s.T = p->T.as<double>(), s.status = p->status.as<int>();
  s.min_ratio = PPALS_ORTHO_MIN_RATIO;
  s.Y = p->Y->d.data, s.dt = p->Y->d.dtype;
  *out = s;
}
int ppals_parafac2_create(ppals_ctx *ctx, int64_t I, int64_t J, int64_t K, int R, int storage_dtype,
                          ppals_parafac2 **out) {
  const char *fn = "ppals_parafac2_create";
  if (!ctx || !out) return fail_fn(PPALS_ERR_ARG, fn, "NULL argument");
  *out = nullptr;
  if (I < 1 || J < 1 || K < 1) return fail_fn(PPALS_ERR_ARG, fn, "the extents I, J, K must be positive");
  if (R < 2 || R > 64) return fail_fn(PPALS_ERR_ARG, fn, "the rank must lie in [2, 64]");
  if (R > I || R > J) return fail_fn(PPALS_ERR_ARG, fn, "the rank must not exceed min(I, J)");
  if (const int rc = p2_check_create(ctx, fn, storage_dtype)) return rc;
  API_BEGIN
  ctx->ops->parafac2_check();  // a back end without device views refuses here, nothing allocated
  std::unique_ptr<ppals_parafac2> p(new ppals_parafac2());
  p->ctx = ctx;
  p->I = I, p->J = J, p->K = K, p->R = R;
  if (const int rc = p2_create_inner(ctx, p.get(), storage_dtype)) return rc;
  ctx->p2s.insert(p.get());  // from here on ppals_parafac2_destroy undoes everything
  ppals_parafac2 *q = p.release();
  try {
    const size_t n = sizeof(double) * (size_t)I * R * K;
    q->P = DeviceBuffer(*ctx->ops, n);
    q->Q = DeviceBuffer(*ctx->ops, n);
    p2_alloc_small(ctx, q);
    ctx->ops->parafac2_init(q->P.as<double>(), I, R, K);
  } catch (...) {
    ppals_parafac2_destroy(q);
    throw;
  }
  *out = q;
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_parafac2_create_ragged(ppals_ctx *ctx, int64_t K, const int64_t *rows, int64_t J, int R, int storage_dtype,
                                 ppals_parafac2 **out) {
  const char *fn = "ppals_parafac2_create_ragged";
  if (!ctx || !out) return fail_fn(PPALS_ERR_ARG, fn, "NULL argument");
  *out = nullptr;
  if (!rows) return fail_fn(PPALS_ERR_ARG, fn, "rows is NULL");
  if (K < 1 || J < 1) return fail_fn(PPALS_ERR_ARG, fn, "the number of slices K and the extent J must be positive");
  if (R < 2 || R > 64) return fail_fn(PPALS_ERR_ARG, fn, "the rank must lie in [2, 64]");
  if (R > J) return fail_fn(PPALS_ERR_ARG, fn, "the rank must not exceed J");
  int64_t N = 0, tiles = 0, bytes = 0;
  for (int64_t k = 0; k < K; k++) {
    if (rows[k] < R)
      return fail_fn(PPALS_ERR_ARG, fn,
                     ("slice " + std::to_string(k) + " has " + std::to_string(rows[k]) +
                      " rows, fewer than the rank " + std::to_string(R))
                         .c_str());
    if (!dv_add(N, rows[k], &N)) return fail_fn(PPALS_ERR_ARG, fn, "the total number of rows overflows int64");
    tiles += (rows[k] - 1) / 64 + 1;  // (at most N: no overflow)
  }
  if (!dv_mul(N, (int64_t)sizeof(double) * R, &bytes))
    return fail_fn(PPALS_ERR_ARG, fn, "the projections' size overflows int64");
  if (tiles > 0x7fffffff) return fail_fn(PPALS_ERR_ARG, fn, "too many row tiles (the sum of ceil(rows[k] / 64))");
  if (const int rc = p2_check_create(ctx, fn, storage_dtype)) return rc;
  API_BEGIN
  ctx->ops->parafac2_check();  // a back end without device views refuses here, nothing allocated
  std::unique_ptr<ppals_parafac2> p(new ppals_parafac2());
  p->ctx = ctx;
  p->I = 0, p->J = J, p->K = K, p->R = R;
  p->ragged = true;
  p->tiles = tiles;
  p->rows.assign(rows, rows + K);
  p->roff.assign((size_t)K + 1, 0);
  // the device tables as one host image: rows | roff (int64), tile0 | tile_slice (int)
  std::vector<int64_t> img((size_t)(2 * K) + (size_t)((K + tiles + 1) / 2), 0);
  int *tile0 = (int *)(img.data() + 2 * K), *tile_slice = tile0 + K;
  int t = 0;
  for (int64_t k = 0; k < K; k++) {
    p->roff[(size_t)k + 1] = p->roff[(size_t)k] + rows[k];
    img[(size_t)k] = rows[k], img[(size_t)(K + k)] = p->roff[(size_t)k];
    tile0[k] = t;
    for (int64_t i = 0; i < rows[k]; i += 64) tile_slice[t++] = (int)k;
  }
  if (const int rc = p2_create_inner(ctx, p.get(), storage_dtype)) return rc;
  ctx->p2s.insert(p.get());  // from here on ppals_parafac2_destroy undoes everything
  ppals_parafac2 *q = p.release();
  try {
    q->P = DeviceBuffer(*ctx->ops, (size_t)bytes);
    q->Q = DeviceBuffer(*ctx->ops, (size_t)bytes);
    p2_alloc_small(ctx, q);
    q->tab = DeviceBuffer(*ctx->ops, sizeof(int64_t) * img.size());
    q->xv = DeviceBuffer(*ctx->ops, sizeof(int64_t) * 2 * (size_t)K);
    ctx->ops->h2d(q->tab.get(), img.data(), sizeof(int64_t) * img.size());
    Ops::Parafac2Ragged d;
    p2_ragged_desc(q, &d);
    ctx->ops->parafac2_init_ragged(d);
  } catch (...) {
    ppals_parafac2_destroy(q);
    throw;
  }
  *out = q;
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_parafac2_rows(ppals_parafac2 *p, int64_t *rows, int64_t *total) {
  if (!p || !p->ctx || !rows) return fail(PPALS_ERR_ARG, "ppals_parafac2_rows: NULL argument or dead handle");
  for (int64_t k = 0; k < p->K; k++) rows[k] = p->ragged ? p->rows[(size_t)k] : p->I;
  if (total) *total = p->ragged ? p->roff[(size_t)p->K] : p->I * p->K;
  return PPALS_OK;
}
void ppals_parafac2_destroy(ppals_parafac2 *p) {
  if (!p) return;
  if (p->ctx) {
    p2_free_buffers(p);
    p->ctx->p2s.erase(p);
  }
  ppals_cp_destroy(p->cp);  // (dead handles when the context went first: then these only delete them)
  ppals_tensor_destroy(p->Y);
  delete p;
}
ppals_cp *ppals_parafac2_cp(ppals_parafac2 *p) { return p && p->ctx ? p->cp : nullptr; }
ppals_tensor *ppals_parafac2_tensor(ppals_parafac2 *p) { return p && p->ctx ? p->Y : nullptr; }

// every check of a step, nothing launched or allocated: on success *st is ready but for `out`
static int p2_check_step(ppals_parafac2 *p, const char *fn, const void *data, int dtype, const int64_t *strides,
                         Ops::Parafac2Step *st) {
  if (!p || !p->ctx || !p->cp || !p->cp->eng) return fail_fn(PPALS_ERR_ARG, fn, "NULL or dead handle");
  if (p->ragged)
    return fail_fn(PPALS_ERR_ARG, fn,
                   "the object holds slices of unequal length (ppals_parafac2_create_ragged): use "
                   "ppals_parafac2_step_ragged_device / ppals_parafac2_run_ragged");
  if (!data) return fail_fn(PPALS_ERR_ARG, fn, "the data pointer is NULL");
  if (dtype != PPALS_F32 && dtype != PPALS_F64)
    return fail_fn(PPALS_ERR_ARG, fn, "bad dtype of the data view (PPALS_F32 or PPALS_F64)");
  if (p->cp->eng->mode_kind(0) != ppals::kModeFree)
    return fail_fn(PPALS_ERR_ARG, fn, "mode 0 of the inner session (B) must stay PPALS_MODE_FREE");
  const int64_t lens[3] = {p->I, p->J, p->K};
  ViewArgs a;
  std::string err;
  if (!dv_check_args(DV_IMPORT, 3, lens, dtype, nullptr, nullptr, strides, &a, &err))
    return fail_fn(PPALS_ERR_ARG, fn, ("the data view: " + err).c_str());
  if (a.stride[0] != 1 || !dv_no_self_overlap(3, a.len, a.stride))
    return fail_fn(PPALS_ERR_UNSUPPORTED, fn,
                   "the data view needs a unit stride in mode 0 and slices that do not overlap: permute the tensor "
                   "so that the shifting mode comes first and make it contiguous");
  if ((uintptr_t)data % (uintptr_t)a.esize)
    return fail_fn(PPALS_ERR_ARG, fn, "the data pointer is not aligned to its element size");
  const int rc = check_view_ptr(p->ctx, (std::string(fn) + ": the data view: ").c_str(), data, &a);
  if (rc != PPALS_OK) return rc;
  const CpEngine &e = *p->cp->eng;
  st->I = p->I, st->J = p->J, st->K = p->K, st->R = p->R;
  st->X = data, st->vdt = dtype, st->s1 = a.stride[1], st->s2 = a.stride[2];
  st->B = e.factor_device(0), st->A = e.factor_device(1), st->C = e.factor_device(2);
  st->Q = p->Q.as<double>(), st->P = p->P.as<double>(), st->T = p->T.as<double>(), st->status = p->status.as<int>();
  st->min_ratio = PPALS_ORTHO_MIN_RATIO;
  st->Y = p->Y->d.data, st->dt = p->Y->d.dtype;
  return PPALS_OK;
}
static void p2_step(ppals_parafac2 *p, Ops::Parafac2Step st, void *stream, double *lost_sq, int *failed) {
  const bool want = lost_sq || failed;
  st.out = want ? p->out.as<double>() : nullptr;
  p->Y->generation++;  // the contents change with these launches: the session rebuilds what it derived
  p->ctx->ops->parafac2_step(st, stream);
  if (!want) return;
  double o[3];
  p->ctx->ops->d2h(o, p->out.as<double>(), sizeof(o));
  if (lost_sq) *lost_sq = o[0] - o[1];
  if (failed) *failed = (int)o[2];
}
int ppals_parafac2_step_device(ppals_parafac2 *p, const void *data, int dtype, const int64_t *strides, void *stream,
                               double *lost_sq, int *failed) {
  API_BEGIN
  Ops::Parafac2Step st;
  const int rc = p2_check_step(p, "ppals_parafac2_step_device", data, dtype, strides, &st);
  if (rc != PPALS_OK) return rc;
  p2_step(p, st, stream, lost_sq, failed);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_parafac2_run(ppals_parafac2 *p, const void *data, int dtype, const int64_t *strides, void *stream,
                       const ppals_cp_opts *o, int inner_sweeps, double rel_change, int *iters, double *res) {
  API_BEGIN
  if (!o) return fail(PPALS_ERR_ARG, "ppals_parafac2_run: NULL options");
  if (inner_sweeps < 1) return fail(PPALS_ERR_ARG, "ppals_parafac2_run: inner_sweeps must be at least 1");
  if (!(rel_change >= 0)) return fail(PPALS_ERR_ARG, "ppals_parafac2_run: rel_change must not be negative");
  if (o->maxiter < 0) return fail(PPALS_ERR_ARG, "ppals_parafac2_run: maxiter must not be negative");
  Ops::Parafac2Step st;
  const int rc = p2_check_step(p, "ppals_parafac2_run", data, dtype, strides, &st);
  if (rc != PPALS_OK) return rc;
  CpEngine *e = p->cp->eng;
  // the quantity looked at: lost_sq + the inner residual^2 after the step (one pass over the small Y)
  return e->run_steps(
      [&](double *sq) {
        double lost = 0;
        p2_step(p, st, stream, sq ? &lost : nullptr, nullptr);
        if (sq) {
          const double r = e->residual();
          *sq = std::max(lost, 0.0) + r * r;
        }
      },
      to_opts(o), inner_sweeps, rel_change, iters, res);
  API_END(PPALS_ERR_HIP)
}
// every check of a ragged step, nothing launched, copied or allocated: on success *xv holds the resolved view
// (offsets | column strides) and *st is ready but for `out`
static int p2_check_step_ragged(ppals_parafac2 *p, const char *fn, const void *data, int dtype,
                                const int64_t *offsets, const int64_t *col_strides, Ops::Parafac2Ragged *st,
                                std::vector<int64_t> *xv) {
  if (!p || !p->ctx || !p->cp || !p->cp->eng) return fail_fn(PPALS_ERR_ARG, fn, "NULL or dead handle");
  if (!p->ragged)
    return fail_fn(PPALS_ERR_ARG, fn,
                   "the object holds slices of one length (ppals_parafac2_create): use ppals_parafac2_step_device / "
                   "ppals_parafac2_run");
  if (!data) return fail_fn(PPALS_ERR_ARG, fn, "the data pointer is NULL");
  if (dtype != PPALS_F32 && dtype != PPALS_F64)
    return fail_fn(PPALS_ERR_ARG, fn, "bad dtype of the data view (PPALS_F32 or PPALS_F64)");
  if (p->cp->eng->mode_kind(0) != ppals::kModeFree)
    return fail_fn(PPALS_ERR_ARG, fn, "mode 0 of the inner session (B) must stay PPALS_MODE_FREE");
  const int64_t K = p->K, J = p->J;
  xv->resize(2 * (size_t)K);
  int64_t lo = INT64_MAX, hi = 0;  // the first and the last element any slice reads
  for (int64_t k = 0; k < K; k++) {
    const int64_t rows = p->rows[(size_t)k];
    int64_t off, cs = col_strides ? col_strides[k] : rows, last;
    if (offsets)
      off = offsets[k];
    else if (!dv_mul(J, p->roff[(size_t)k], &off))
      return fail_fn(PPALS_ERR_ARG, fn, "the packed offsets overflow int64");
    if (off < 0) return fail_fn(PPALS_ERR_ARG, fn, ("offsets[" + std::to_string(k) + "] is negative").c_str());
    if (cs < rows)
      return fail_fn(PPALS_ERR_ARG, fn,
                     ("col_strides[" + std::to_string(k) + "] = " + std::to_string(cs) + " is less than the slice's " +
                      std::to_string(rows) + " rows")
                         .c_str());
    if (!dv_mul(cs, J - 1, &last) || !dv_add(last, rows - 1, &last) || !dv_add(last, off, &last))
      return fail_fn(PPALS_ERR_ARG, fn, "the data view's span overflows int64");
    lo = std::min(lo, off), hi = std::max(hi, last);
    (*xv)[(size_t)k] = off, (*xv)[(size_t)(K + k)] = cs;
  }
  ViewArgs a;  // the union of the slices' spans as one view of hi - lo + 1 elements from data + lo
  a.order = 1, a.dtype = dtype, a.esize = dv_elem_size(dtype);
  a.lo[0] = 0, a.len[0] = hi - lo + 1, a.stride[0] = 1;
  int64_t lo_bytes;
  if (!dv_mul(a.len[0], a.esize, &a.span) || !dv_mul(lo, a.esize, &lo_bytes))
    return fail_fn(PPALS_ERR_ARG, fn, "the data view's byte span overflows int64");
  if ((uintptr_t)data % (uintptr_t)a.esize)
    return fail_fn(PPALS_ERR_ARG, fn, "the data pointer is not aligned to its element size");
  const int rc =
      check_view_ptr(p->ctx, (std::string(fn) + ": the data view: ").c_str(), (const char *)data + lo_bytes, &a);
  if (rc != PPALS_OK) return rc;
  const CpEngine &e = *p->cp->eng;
  p2_ragged_desc(p, st);
  st->X = data, st->vdt = dtype;
  st->B = e.factor_device(0), st->A = e.factor_device(1), st->C = e.factor_device(2);
  return PPALS_OK;
}
// the view's tables travel only when they differ from the last step's (h2d is ordered behind that step)
static void p2_step_ragged(ppals_parafac2 *p, Ops::Parafac2Ragged st, const std::vector<int64_t> &xv, void *stream,
                           double *lost_sq, int *failed) {
  if (xv != p->xv_host) {
    p->xv_host.clear();  // (a failed copy leaves nothing believed)
    p->ctx->ops->h2d(p->xv.get(), xv.data(), sizeof(int64_t) * xv.size());
    p->xv_host = xv;
  }
  const bool want = lost_sq || failed;
  st.out = want ? p->out.as<double>() : nullptr;
  p->Y->generation++;  // the contents change with these launches: the session rebuilds what it derived
  p->ctx->ops->parafac2_step_ragged(st, stream);
  if (!want) return;
  double o[3];
  p->ctx->ops->d2h(o, p->out.as<double>(), sizeof(o));
  if (lost_sq) *lost_sq = o[0] - o[1];
  if (failed) *failed = (int)o[2];
}
int ppals_parafac2_step_ragged_device(ppals_parafac2 *p, const void *data, int dtype, const int64_t *offsets,
                                      const int64_t *col_strides, void *stream, double *lost_sq, int *failed) {
  API_BEGIN
  Ops::Parafac2Ragged st;
  std::vector<int64_t> xv;
  const int rc = p2_check_step_ragged(p, "ppals_parafac2_step_ragged_device", data, dtype, offsets, col_strides, &st, &xv);
  if (rc != PPALS_OK) return rc;
  p2_step_ragged(p, st, xv, stream, lost_sq, failed);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_parafac2_run_ragged(ppals_parafac2 *p, const void *data, int dtype, const int64_t *offsets,
                              const int64_t *col_strides, void *stream, const ppals_cp_opts *o, int inner_sweeps,
                              double rel_change, int *iters, double *res) {
  API_BEGIN
  if (!o) return fail(PPALS_ERR_ARG, "ppals_parafac2_run_ragged: NULL options");
  if (inner_sweeps < 1) return fail(PPALS_ERR_ARG, "ppals_parafac2_run_ragged: inner_sweeps must be at least 1");
  if (!(rel_change >= 0)) return fail(PPALS_ERR_ARG, "ppals_parafac2_run_ragged: rel_change must not be negative");
  if (o->maxiter < 0) return fail(PPALS_ERR_ARG, "ppals_parafac2_run_ragged: maxiter must not be negative");
  Ops::Parafac2Ragged st;
  std::vector<int64_t> xv;
  const int rc = p2_check_step_ragged(p, "ppals_parafac2_run_ragged", data, dtype, offsets, col_strides, &st, &xv);
  if (rc != PPALS_OK) return rc;
  CpEngine *e = p->cp->eng;
  return e->run_steps(
      [&](double *sq) {
        double lost = 0;
        p2_step_ragged(p, st, xv, stream, sq ? &lost : nullptr, nullptr);
        if (sq) {
          const double r = e->residual();
          *sq = std::max(lost, 0.0) + r * r;
        }
      },
      to_opts(o), inner_sweeps, rel_change, iters, res);
  API_END(PPALS_ERR_HIP)
}
int ppals_parafac2_projections(ppals_parafac2 *p, double *P_host) {
  if (!p || !p->ctx || !P_host) return fail(PPALS_ERR_ARG, "ppals_parafac2_projections: NULL argument or dead handle");
  API_BEGIN
  const size_t n = p->ragged ? (size_t)p->roff[(size_t)p->K] * p->R : (size_t)p->I * p->R * p->K;
  p->ctx->ops->d2h(P_host, p->P.as<double>(), sizeof(double) * n);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_parafac2_projections_device(ppals_parafac2 *p, const double **P) {
  if (!p || !p->ctx || !P) return fail(PPALS_ERR_ARG, "ppals_parafac2_projections_device: NULL argument or dead handle");
  *P = p->P.as<double>();
  return PPALS_OK;
}

// ------------------------------------------------------------------ multi-start CP
int ppals_cp_multi_create(ppals_ctx *ctx, ppals_tensor *V, int R, int nstarts, ppals_cp_multi **out) {
  if (!ctx || !V || !out) return fail(PPALS_ERR_ARG, "NULL argument");
  *out = nullptr;
  if (V->ctx != ctx || !V->d.data) return fail(PPALS_ERR_ARG, "the tensor belongs to another context");
  if (R <= 0) return fail(PPALS_ERR_ARG, "rank must be positive");
  if (nstarts < 1 || nstarts > PPALS_MULTI_MAX_STARTS)
    return fail(PPALS_ERR_ARG, "nstarts must be in [1, 32]");
  if ((int64_t)R * nstarts > PPALS_MULTI_MAX_COLUMNS)
    return fail(PPALS_ERR_ARG, "R * nstarts must not exceed 128");
  if (ctx->c().size() > 1)
    return fail(PPALS_ERR_UNSUPPORTED, "a multi-start session runs on one rank (sharded multi-start is not implemented)");
  API_BEGIN
  std::unique_ptr<ppals_cp_multi> s(new ppals_cp_multi);
  s->ctx = ctx;
  s->eng = new CpEngine(*ctx->ops, ctx->c(), V->d, R, nstarts, true);
  ctx->multis.insert(s.get());
  *out = s.release();
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_cp_multi_create_ranks(ppals_ctx *ctx, ppals_tensor *V, int nstarts, const int *ranks,
                                ppals_cp_multi **out) {
  if (!ctx || !V || !out) return fail(PPALS_ERR_ARG, "NULL argument");
  *out = nullptr;
  if (!ranks) return fail(PPALS_ERR_ARG, "ppals_cp_multi_create_ranks: ranks is NULL");
  if (V->ctx != ctx || !V->d.data) return fail(PPALS_ERR_ARG, "the tensor belongs to another context");
  if (nstarts < 1 || nstarts > PPALS_MULTI_MAX_STARTS)
    return fail(PPALS_ERR_ARG, "nstarts must be in [1, 32]");
  int64_t total = 0;
  for (int b = 0; b < nstarts; b++) {
    if (ranks[b] <= 0) return fail(PPALS_ERR_ARG, "ppals_cp_multi_create_ranks: every rank must be positive");
    total += ranks[b];
  }
  if (total > PPALS_MULTI_MAX_COLUMNS)
    return fail(PPALS_ERR_ARG, "ppals_cp_multi_create_ranks: the ranks must not add up to more than 128");
  if (ctx->c().size() > 1)
    return fail(PPALS_ERR_UNSUPPORTED, "a multi-start session runs on one rank (sharded multi-start is not implemented)");
  API_BEGIN
  std::unique_ptr<ppals_cp_multi> s(new ppals_cp_multi);
  s->ctx = ctx;
  s->eng = new CpEngine(*ctx->ops, ctx->c(), V->d, 0, nstarts, true, ranks);
  ctx->multis.insert(s.get());
  *out = s.release();
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_cp_multi_ranks(const ppals_cp_multi *s, int *nstarts, int *ranks) {
  if (!s || !s->eng || !nstarts) return fail(PPALS_ERR_ARG, "NULL argument");
  *nstarts = s->eng->nstarts();
  if (ranks)
    for (int b = 0; b < s->eng->nstarts(); b++) ranks[b] = s->eng->start_rank(b);
  return PPALS_OK;
}
void ppals_cp_multi_destroy(ppals_cp_multi *s) {
  if (!s) return;
  delete s->eng;
  if (s->ctx) s->ctx->multis.erase(s);
  delete s;
}
static int check_start(const ppals_cp_multi *s, int start, bool all_ok) {
  if (!s || !s->eng) return fail(PPALS_ERR_ARG, "NULL session");
  if (start >= s->eng->nstarts() || start < (all_ok ? -1 : 0))
    return fail(PPALS_ERR_ARG, all_ok ? "start must be in [0, nstarts) or -1" : "start must be in [0, nstarts)");
  return PPALS_OK;
}
int ppals_cp_multi_set_factors(ppals_cp_multi *s, int start, const double *Wflat, const double *gradWflat) {
  if (int rc = check_start(s, start, true)) return rc;
  if (!Wflat) return fail(PPALS_ERR_ARG, "NULL argument");
  API_BEGIN
  if (s->eng->nonneg_modes()) {  // Wflat is on the host: looked at here, before anything is uploaded
    const bool all = s->eng->nonneg();
    size_t at = 0;  // (the blocks of the starts, each of its own length; of those the NONNEG modes' blocks)
    for (int b = start < 0 ? 0 : start; b < (start < 0 ? s->eng->nstarts() : start + 1); b++)
      for (int i = 0; i < s->eng->order(); i++) {
        const size_t n = (size_t)s->eng->tensor().glens[i] * (size_t)s->eng->start_rank(b);
        if (s->eng->mode_kind(i) == ppals::kModeNonneg)
          for (size_t e = at; e < at + n; e++)
            if (!(Wflat[e] >= 0) || !std::isfinite(Wflat[e]))
              return fail(PPALS_ERR_ARG,
                          all ? "ppals_cp_multi_set_factors: a non-negative session takes finite factors >= 0"
                              : "ppals_cp_multi_set_factors: a non-negative mode takes a finite factor >= 0");
        at += n;
      }
  }
  s->eng->set_factors_start(start, Wflat, gradWflat);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_cp_multi_get_factors(ppals_cp_multi *s, int start, double *Wflat, double *gradWflat) {
  if (int rc = check_start(s, start, true)) return rc;
  API_BEGIN
  s->eng->get_factors_start(start, Wflat, gradWflat);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_cp_multi_set_schedule(ppals_cp_multi *s, int schedule) {
  if (!s || !s->eng) return fail(PPALS_ERR_ARG, "NULL session");
  if (schedule != PPALS_SCHEDULE_DT && schedule != PPALS_SCHEDULE_MSDT)
    return fail(PPALS_ERR_ARG, "schedule must be PPALS_SCHEDULE_DT or PPALS_SCHEDULE_MSDT");
  API_BEGIN
  s->eng->set_schedule(schedule);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_cp_multi_sweeps(ppals_cp_multi *s, int n, double lambda) {
  if (!s || !s->eng) return fail(PPALS_ERR_ARG, "NULL session");
  if (n < 0) return fail(PPALS_ERR_ARG, "the number of sweeps must not be negative");
  API_BEGIN
  for (int i = 0; i < n; i++) s->eng->update_modes(0, s->eng->order(), lambda);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_cp_multi_set_nonneg(ppals_cp_multi *s, int on) {
  if (!s || !s->eng) return fail(PPALS_ERR_ARG, "NULL session");
  API_BEGIN
  const bool was = s->eng->nonneg();
  int before[ppals::MAX_ORDER];  // (all FREE unless ppals_cp_multi_set_mode_constraints was used)
  for (int i = 0; i < s->eng->order(); i++) before[i] = s->eng->mode_kind(i);
  s->eng->set_nonneg(on != 0);
  if (on && !was && !s->eng->factors_nonneg()) {
    s->eng->restore_mode_kinds(before);
    return fail(PPALS_ERR_ARG, "ppals_cp_multi_set_nonneg: a start's factors have a negative or non-finite entry");
  }
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_cp_multi_set_mode_constraints(ppals_cp_multi *s, const int *kinds) {
  return set_mode_constraints(s ? s->eng : nullptr, kinds, "ppals_cp_multi_set_mode_constraints",
                              "a start's factors");
}
int ppals_cp_multi_get_mode_constraints(const ppals_cp_multi *s, int *kinds) {
  return get_mode_constraints(s ? s->eng : nullptr, kinds, "ppals_cp_multi_get_mode_constraints");
}
int ppals_cp_multi_set_mode_shapes(ppals_cp_multi *s, const int *shapes) {
  return set_mode_shapes(s ? s->eng : nullptr, shapes, "ppals_cp_multi_set_mode_shapes");
}
int ppals_cp_multi_get_mode_shapes(const ppals_cp_multi *s, int *shapes) {
  return get_mode_shapes(s ? s->eng : nullptr, shapes, "ppals_cp_multi_get_mode_shapes");
}
int ppals_cp_multi_get_nonneg(const ppals_cp_multi *s) {
  return s && s->eng ? (s->eng->nonneg() ? 1 : 0) : PPALS_ERR_ARG;
}
int ppals_cp_multi_residuals(ppals_cp_multi *s, double *out) {
  if (!s || !s->eng || !out) return fail(PPALS_ERR_ARG, "NULL argument");
  API_BEGIN
  s->eng->residuals(out);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_cp_multi_gradnorms(ppals_cp_multi *s, double *out) {
  if (!s || !s->eng || !out) return fail(PPALS_ERR_ARG, "NULL argument");
  API_BEGIN
  s->eng->gradnorms(out);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_cp_multi_run(ppals_cp_multi *s, const ppals_cp_opts *o, int *sweeps, int *best) {
  if (!s || !s->eng || !o) return fail(PPALS_ERR_ARG, "NULL argument");
  if (o->maxiter < 0) return fail(PPALS_ERR_ARG, "maxiter must not be negative");
  API_BEGIN
  return s->eng->run_multi(to_opts(o), sweeps, best);
  API_END(PPALS_ERR_HIP)
}
int ppals_cp_multi_take(ppals_cp_multi *s, int start, ppals_cp *dst) {
  if (int rc = check_start(s, start, false)) return rc;
  if (!dst || !dst->eng) return fail(PPALS_ERR_ARG, "NULL destination session");
  if (dst->ctx != s->ctx) return fail(PPALS_ERR_ARG, "the destination session belongs to another context");
  if (dst->eng->tensor().data != s->eng->tensor().data)
    return fail(PPALS_ERR_ARG, "the destination session is on another tensor");
  if (dst->eng->rank_r() != s->eng->start_rank(start)) {
    char msg[128];
    std::snprintf(msg, sizeof(msg), "ppals_cp_multi_take: the destination session has rank %d, the start rank %d",
                  dst->eng->rank_r(), s->eng->start_rank(start));
    return fail(PPALS_ERR_ARG, msg);
  }
  // (a destination that is NONNEG in every mode keeps the engine's own message)
  if (!dst->eng->nonneg() && !dst->eng->takes_nonneg_from(*s->eng))
    return fail_fn(PPALS_ERR_UNSUPPORTED, "ppals_cp_multi_take",
                   "the destination is non-negative in a mode where the multi-start session is not");
  API_BEGIN
  dst->eng->take_from(*s->eng, start);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}

// ------------------------------------------------------------------ hold-out rows per start
int ppals_cp_multi_set_holdout(ppals_cp_multi *s, int mode, const uint8_t *keep) {
  const char *fn = "ppals_cp_multi_set_holdout";
  if (!s || !s->eng) return fail_fn(PPALS_ERR_ARG, fn, "NULL session");
  if (keep) {  // (the table is on the host: looked at here, before anything is allocated or launched)
    if (mode < 0 || mode >= s->eng->order()) return fail_fn(PPALS_ERR_ARG, fn, "mode must be in [0, N)");
    if (s->eng->mode_kind(mode) == ppals::kModeFixed || s->eng->mode_kind(mode) == ppals::kModeOrtho)
      return fail_fn(PPALS_ERR_UNSUPPORTED, fn, "the hold-out mode cannot be fixed or orthonormal");
    if (s->eng->mode_shape(mode) != ppals::kShapeNone)
      return fail_fn(PPALS_ERR_UNSUPPORTED, fn, "the hold-out mode cannot have a shape");
    const int64_t n = s->eng->mode_extent(mode);
    for (int b = 0; b < s->eng->nstarts(); b++) {
      bool any = false;
      for (int64_t x = 0; x < n && !any; x++) any = keep[(size_t)b * n + x] != 0;
      if (!any) return fail_fn(PPALS_ERR_ARG, fn, "every start must keep at least one row");
    }
  }
  API_BEGIN
  s->eng->set_holdout(mode, keep);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_cp_multi_get_holdout(const ppals_cp_multi *s, int *mode, uint8_t *keep) {
  const char *fn = "ppals_cp_multi_get_holdout";
  if (!s || !s->eng) return fail_fn(PPALS_ERR_ARG, fn, "NULL session");
  if (!mode) return fail_fn(PPALS_ERR_ARG, fn, "mode is NULL");
  *mode = s->eng->holdout_mode();
  if (keep && *mode >= 0) std::memcpy(keep, s->eng->holdout_keep().data(), s->eng->holdout_keep().size());
  return PPALS_OK;
}
int ppals_cp_multi_heldout_scores(ppals_cp_multi *s, int start, double *scores) {
  const char *fn = "ppals_cp_multi_heldout_scores";
  if (!s || !s->eng) return fail_fn(PPALS_ERR_ARG, fn, "NULL session");
  if (start < 0 || start >= s->eng->nstarts()) return fail_fn(PPALS_ERR_ARG, fn, "start must be in [0, nstarts)");
  if (!scores) return fail_fn(PPALS_ERR_ARG, fn, "scores is NULL");
  if (s->eng->holdout_mode() < 0) return fail_fn(PPALS_ERR_ARG, fn, "the session has no hold-out");
  API_BEGIN
  s->eng->heldout_scores(start, scores);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_cp_multi_take_predicted(ppals_cp_multi *s, int start, ppals_cp *dst) {
  const char *fn = "ppals_cp_multi_take_predicted";
  if (!s || !s->eng) return fail_fn(PPALS_ERR_ARG, fn, "NULL session");
  if (start < 0 || start >= s->eng->nstarts()) return fail_fn(PPALS_ERR_ARG, fn, "start must be in [0, nstarts)");
  if (!dst || !dst->eng) return fail_fn(PPALS_ERR_ARG, fn, "NULL destination session");
  if (s->eng->holdout_mode() < 0) return fail_fn(PPALS_ERR_ARG, fn, "the session has no hold-out");
  if (dst->ctx != s->ctx) return fail_fn(PPALS_ERR_ARG, fn, "the destination session belongs to another context");
  if (dst->eng->tensor().data != s->eng->tensor().data)
    return fail_fn(PPALS_ERR_ARG, fn, "the destination session is on another tensor");
  if (dst->eng->rank_r() != s->eng->start_rank(start)) {
    char msg[128];
    std::snprintf(msg, sizeof(msg), "the destination session has rank %d, the start rank %d", dst->eng->rank_r(),
                  s->eng->start_rank(start));
    return fail_fn(PPALS_ERR_ARG, fn, msg);
  }
  if (!dst->eng->takes_nonneg_from(*s->eng))
    return fail_fn(PPALS_ERR_UNSUPPORTED, fn,
                   "a non-negative session does not take an unconstrained multi-start's factors");
  API_BEGIN
  dst->eng->take_predicted_from(*s->eng, start);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}

// ------------------------------------------------------------------ core consistency
// the refusals the three entry points share, before anything is launched: more than one rank, a core above
// the cap, a rank above the LDS elimination's (starts [b0, b1) of the session)
static int check_core_consistency(ppals_ctx *ctx, const CpEngine &e, int b0, int b1, const char *fn) {
  char msg[192];
  if (ctx->c().size() > 1) {
    std::snprintf(msg, sizeof(msg), "%s: the core consistency runs on one rank (no sharded form)", fn);
    return fail(PPALS_ERR_UNSUPPORTED, msg);
  }
  if (e.order() < 2) {
    std::snprintf(msg, sizeof(msg), "%s: the tensor must have order >= 2", fn);
    return fail(PPALS_ERR_UNSUPPORTED, msg);
  }
  for (int b = b0; b < b1; b++) {
    if (e.core_entries(b) > CpEngine::kCoreMaxEntries) {
      std::snprintf(msg, sizeof(msg), "%s: the core of a rank-%d model of order %d has more than 2^24 entries",
                    fn, e.start_rank(b), e.order());
      return fail(PPALS_ERR_UNSUPPORTED, msg);
    }
    if (e.start_rank(b) > Ops::kPinvMaxRank) {
      std::snprintf(msg, sizeof(msg), "%s: rank %d is above 64, the largest the pseudo-inverse factors take",
                    fn, e.start_rank(b));
      return fail(PPALS_ERR_UNSUPPORTED, msg);
    }
  }
  return PPALS_OK;
}
int ppals_cp_core_consistency(ppals_cp *s, double *cc, double *core, int64_t *n) {
  if (!s || !s->eng) return fail(PPALS_ERR_ARG, "ppals_cp_core_consistency: NULL session");
  if (!cc) return fail(PPALS_ERR_ARG, "ppals_cp_core_consistency: cc is NULL");
  if (int rc = check_core_consistency(s->ctx, *s->eng, 0, 1, "ppals_cp_core_consistency")) return rc;
  API_BEGIN
  if (n) *n = s->eng->core_entries(0);
  s->eng->core_consistency(-1, cc, core);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_cp_multi_core_consistency(ppals_cp_multi *s, double *cc) {
  if (!s || !s->eng) return fail(PPALS_ERR_ARG, "ppals_cp_multi_core_consistency: NULL session");
  if (!cc) return fail(PPALS_ERR_ARG, "ppals_cp_multi_core_consistency: cc is NULL");
  if (int rc = check_core_consistency(s->ctx, *s->eng, 0, s->eng->nstarts(), "ppals_cp_multi_core_consistency"))
    return rc;
  API_BEGIN
  s->eng->core_consistency(-1, cc, nullptr);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_cp_multi_core(ppals_cp_multi *s, int start, double *core, int64_t *n) {
  if (!s || !s->eng) return fail(PPALS_ERR_ARG, "ppals_cp_multi_core: NULL session");
  if (start < 0 || start >= s->eng->nstarts())
    return fail(PPALS_ERR_ARG, "ppals_cp_multi_core: start must be in [0, nstarts)");
  if (!core && !n) return fail(PPALS_ERR_ARG, "ppals_cp_multi_core: core and n are both NULL");
  if (int rc = check_core_consistency(s->ctx, *s->eng, start, start + 1, "ppals_cp_multi_core")) return rc;
  API_BEGIN
  if (n) *n = s->eng->core_entries(start);
  if (!core) return PPALS_OK;  // the size query
  double cc = 0;
  s->eng->core_consistency(start, &cc, core);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}

// ------------------------------------------------------------------ factor match score
int ppals_match_columns(const double *score, int ra, int rb, int ld, int *perm, double *sum) {
  if (!score) return fail(PPALS_ERR_ARG, "ppals_match_columns: score is NULL");
  if (ra < 1 || rb < 1) return fail(PPALS_ERR_ARG, "ppals_match_columns: ra and rb must be >= 1");
  if (ld < ra) return fail(PPALS_ERR_ARG, "ppals_match_columns: ld must be >= ra");
  API_BEGIN
  if (!match_columns(score, ra, rb, ld, perm, sum))
    return fail(PPALS_ERR_ARG, "ppals_match_columns: score has an entry that is not finite");
  return PPALS_OK;
  API_END(PPALS_ERR_ARG)
}
// the refusals the congruence / fms entry points share, before anything is launched
static int check_congruence(ppals_ctx *ca, const CpEngine *a, ppals_ctx *cb, const CpEngine *b, int skip_mode,
                            int flags, const char *fn) {
  char msg[224];
  if (!a || !b) {
    std::snprintf(msg, sizeof(msg), "%s: NULL session", fn);
    return fail(PPALS_ERR_ARG, msg);
  }
  if (ca != cb) {
    std::snprintf(msg, sizeof(msg), "%s: the sessions belong to different contexts", fn);
    return fail(PPALS_ERR_ARG, msg);
  }
  if (a->order() != b->order()) {
    std::snprintf(msg, sizeof(msg), "%s: the sessions differ in order (%d and %d)", fn, a->order(), b->order());
    return fail(PPALS_ERR_ARG, msg);
  }
  if (skip_mode < -1 || skip_mode >= a->order()) {
    std::snprintf(msg, sizeof(msg), "%s: skip_mode %d is outside [-1, %d)", fn, skip_mode, a->order());
    return fail(PPALS_ERR_ARG, msg);
  }
  if (flags & ~PPALS_FMS_WEIGHTS) {
    std::snprintf(msg, sizeof(msg), "%s: unknown flag bits 0x%x", fn, (unsigned)(flags & ~PPALS_FMS_WEIGHTS));
    return fail(PPALS_ERR_ARG, msg);
  }
  for (int i = 0; i < a->order(); i++)
    if (i != skip_mode && a->mode_extent(i) != b->mode_extent(i)) {
      std::snprintf(msg, sizeof(msg), "%s: mode %d has extent %lld in the first session and %lld in the second",
                    fn, i, (long long)a->mode_extent(i), (long long)b->mode_extent(i));
      return fail(PPALS_ERR_ARG, msg);
    }
  if (ca->c().size() > 1) {
    std::snprintf(msg, sizeof(msg), "%s: the factor match score runs on one rank (no sharded form)", fn);
    return fail(PPALS_ERR_UNSUPPORTED, msg);
  }
  if (a->rank_r() > Ops::kCongruenceMaxCols || b->rank_r() > Ops::kCongruenceMaxCols) {
    std::snprintf(msg, sizeof(msg), "%s: a session of more than 128 columns", fn);
    return fail(PPALS_ERR_UNSUPPORTED, msg);
  }
  return PPALS_OK;
}
static int congruence_call(ppals_ctx *ca, CpEngine *a, ppals_ctx *cb, CpEngine *b, int skip_mode, double *Phi,
                           int64_t *n, const char *fn) {
  if (int rc = check_congruence(ca, a, cb, b, skip_mode, 0, fn)) return rc;
  if (!Phi && !n) {
    g_err = std::string(fn) + ": Phi and n are both NULL";
    return PPALS_ERR_ARG;
  }
  API_BEGIN
  const int64_t total = (int64_t)a->rank_r() * b->rank_r();
  if (n) *n = total;
  if (!Phi) return PPALS_OK;  // the size query
  std::vector<double> h;
  a->congruence(*b, skip_mode, h);
  std::memcpy(Phi, h.data(), sizeof(double) * (size_t)total);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_cp_congruence(ppals_cp *a, ppals_cp *b, int skip_mode, double *Phi, int64_t *n) {
  return congruence_call(a ? a->ctx : nullptr, a ? a->eng : nullptr, b ? b->ctx : nullptr, b ? b->eng : nullptr,
                         skip_mode, Phi, n, "ppals_cp_congruence");
}
int ppals_cp_multi_congruence(ppals_cp_multi *s, ppals_cp_multi *other, int skip_mode, double *Phi, int64_t *n) {
  if (!other) other = s;
  return congruence_call(s ? s->ctx : nullptr, s ? s->eng : nullptr, other ? other->ctx : nullptr,
                         other ? other->eng : nullptr, skip_mode, Phi, n, "ppals_cp_multi_congruence");
}
int ppals_cp_fms(ppals_cp *a, ppals_cp *b, int skip_mode, int flags, double *fms, int *perm) {
  if (int rc = check_congruence(a ? a->ctx : nullptr, a ? a->eng : nullptr, b ? b->ctx : nullptr,
                                b ? b->eng : nullptr, skip_mode, flags, "ppals_cp_fms"))
    return rc;
  if (!fms) return fail(PPALS_ERR_ARG, "ppals_cp_fms: fms is NULL");
  API_BEGIN
  a->eng->fms_pairs(*b->eng, skip_mode, (flags & PPALS_FMS_WEIGHTS) != 0, false, fms, perm);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_cp_multi_fms(ppals_cp_multi *s, int skip_mode, int flags, double *fms) {
  if (int rc = check_congruence(s ? s->ctx : nullptr, s ? s->eng : nullptr, s ? s->ctx : nullptr,
                                s ? s->eng : nullptr, skip_mode, flags, "ppals_cp_multi_fms"))
    return rc;
  if (!fms) return fail(PPALS_ERR_ARG, "ppals_cp_multi_fms: fms is NULL");
  API_BEGIN
  s->eng->fms_pairs(*s->eng, skip_mode, (flags & PPALS_FMS_WEIGHTS) != 0, true, fms, nullptr);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_cp_multi_fms_between(ppals_cp_multi *a, ppals_cp_multi *b, int skip_mode, int flags, double *fms) {
  if (int rc = check_congruence(a ? a->ctx : nullptr, a ? a->eng : nullptr, b ? b->ctx : nullptr,
                                b ? b->eng : nullptr, skip_mode, flags, "ppals_cp_multi_fms_between"))
    return rc;
  if (!fms) return fail(PPALS_ERR_ARG, "ppals_cp_multi_fms_between: fms is NULL");
  if (a->eng->nstarts() != b->eng->nstarts()) {
    char msg[160];
    std::snprintf(msg, sizeof(msg), "ppals_cp_multi_fms_between: the sessions have %d and %d starts",
                  a->eng->nstarts(), b->eng->nstarts());
    return fail(PPALS_ERR_ARG, msg);
  }
  API_BEGIN
  a->eng->fms_pairs(*b->eng, skip_mode, (flags & PPALS_FMS_WEIGHTS) != 0, false, fms, nullptr);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}

// ------------------------------------------------------------------ influence plot
// the refusals of the two calls, before anything is launched or allocated
static int check_influence(ppals_cp *s, const void *out, const char *fn, const char *outname, bool pinv) {
  char msg[192];
  if (!s || !s->eng) {
    std::snprintf(msg, sizeof(msg), "%s: NULL session", fn);
    return fail(PPALS_ERR_ARG, msg);
  }
  if (!out) {
    std::snprintf(msg, sizeof(msg), "%s: %s is NULL", fn, outname);
    return fail(PPALS_ERR_ARG, msg);
  }
  if (s->ctx->c().size() > 1) {
    std::snprintf(msg, sizeof(msg), "%s: the influence plot runs on one rank (no sharded form)", fn);
    return fail(PPALS_ERR_UNSUPPORTED, msg);
  }
  if (pinv && s->eng->rank_r() > Ops::kPinvMaxRank) {
    std::snprintf(msg, sizeof(msg), "%s: rank %d is above 64, the largest the pseudo-inverse factors take", fn,
                  s->eng->rank_r());
    return fail(PPALS_ERR_UNSUPPORTED, msg);
  }
  return PPALS_OK;
}
int ppals_cp_slice_residuals(ppals_cp *s, double *ss, double *total) {
  if (int rc = check_influence(s, ss, "ppals_cp_slice_residuals", "ss", false)) return rc;
  API_BEGIN
  s->eng->slice_residuals(ss, total);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_cp_leverages(ppals_cp *s, double *lev) {
  if (int rc = check_influence(s, lev, "ppals_cp_leverages", "lev", true)) return rc;
  API_BEGIN
  s->eng->leverages(lev);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}

// ------------------------------------------------------------------ Tucker
int ppals_tucker_create(ppals_ctx *ctx, ppals_tensor *V, const int *ranks, ppals_tucker **out) {
  if (!ctx || !V || !ranks || !out) return fail(PPALS_ERR_ARG, "NULL argument");
  if (V->d.dtype == PPALS_BF16)
    return fail(PPALS_ERR_UNSUPPORTED,
                "ppals_tucker_create: Tucker / HOSVD do not take a bf16 tensor (store it as F32 or F64)");
  API_BEGIN
  std::unique_ptr<ppals_tucker> s(new ppals_tucker);
  s->ctx = ctx;
  s->eng = new TuckerEngine(*ctx->ops, ctx->c(), V->d, ranks);
  ctx->tks.insert(s.get());
  *out = s.release();
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
void ppals_tucker_destroy(ppals_tucker *s) {
  if (!s) return;
  delete s->eng;
  if (s->ctx) s->ctx->tks.erase(s);
  delete s;
}
int ppals_tucker_set_factors(ppals_tucker *s, const double *Wflat) {
  if (!s || !s->eng || !Wflat) return fail(PPALS_ERR_ARG, "NULL argument");
  API_BEGIN
  s->eng->set_factors(Wflat);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_tucker_set_core(ppals_tucker *s, const double *core) {
  if (!s || !s->eng) return fail(PPALS_ERR_ARG, "NULL argument");
  API_BEGIN
  s->eng->set_core(core);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_tucker_get_factors(ppals_tucker *s, double *Wflat, double *core) {
  if (!s || !s->eng) return fail(PPALS_ERR_ARG, "NULL argument");
  API_BEGIN
  s->eng->get_factors(Wflat, core);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_tucker_hosvd(ppals_tucker *s) {
  if (!s || !s->eng) return fail(PPALS_ERR_ARG, "NULL argument");
  API_BEGIN
  s->eng->hosvd();
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_tucker_ttmc(ppals_tucker *s, int skip, double *Y, int64_t *n) {
  if (!s || !s->eng) return fail(PPALS_ERR_ARG, "NULL argument");
  API_BEGIN
  int64_t c = s->eng->ttmc(skip, Y);
  if (n) *n = c;
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_tucker_sweeps_dt(ppals_tucker *s, int n) {
  if (!s || !s->eng) return fail(PPALS_ERR_ARG, "NULL argument");
  API_BEGIN
  for (int i = 0; i < n; i++) s->eng->sweep_dt();
  s->eng->settle();
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_tucker_dt(ppals_tucker *s, const ppals_cp_opts *o, int *iters) {
  if (!s || !s->eng || !o) return fail(PPALS_ERR_ARG, "NULL argument");
  API_BEGIN
  return s->eng->run_dt(to_opts(o), iters);
  API_END(PPALS_ERR_HIP)
}

int ppals_tucker_em(ppals_tucker *s, const void *mask, const int64_t *box_lo, const int64_t *box_len,
                    const int64_t *strides, void *stream, const ppals_cp_opts *o, int inner_sweeps,
                    int *iters, double *observed_res) {
  API_BEGIN
  if (!o) return fail(PPALS_ERR_ARG, "ppals_tucker_em: NULL options");
  if (inner_sweeps < 1) return fail(PPALS_ERR_ARG, "ppals_tucker_em: inner_sweeps must be at least 1");
  if (o->maxiter < 0) return fail(PPALS_ERR_ARG, "ppals_tucker_em: maxiter must not be negative");
  if (!s || !s->eng || !s->ctx) return fail(PPALS_ERR_ARG, "NULL session");
  ViewArgs a;
  const int rc = check_mask_view(s->ctx, s->eng->tensor(), "ppals_tucker_em: ", mask, box_lo, box_len, strides,
                                 &a);
  if (rc != PPALS_OK) return rc;
  return s->eng->run_em(a, mask, stream, to_opts(o), inner_sweeps, iters, observed_res);
  API_END(PPALS_ERR_HIP)
}

int ppals_tucker_pp(ppals_tucker *s, const ppals_cp_opts *o, int *iters) {
  if (!s || !s->eng || !o) return fail(PPALS_ERR_ARG, "NULL argument");
  API_BEGIN
  return s->eng->run_pp(to_opts(o), iters);
  API_END(PPALS_ERR_HIP)
}

// ------------------------------------------------------------------ Tucker: residual and influence plot
// the refusals of the three calls, before anything is launched or allocated (one_rank: the two diagnostics)
static int check_tucker_influence(ppals_tucker *s, const void *out, const char *fn, const char *outname,
                                  bool one_rank) {
  char msg[192];
  if (!s || !s->eng) {
    std::snprintf(msg, sizeof(msg), "%s: NULL session", fn);
    return fail(PPALS_ERR_ARG, msg);
  }
  if (!out) {
    std::snprintf(msg, sizeof(msg), "%s: %s is NULL", fn, outname);
    return fail(PPALS_ERR_ARG, msg);
  }
  if (one_rank && s->ctx->c().size() > 1) {
    std::snprintf(msg, sizeof(msg), "%s: the influence plot runs on one rank (no sharded form)", fn);
    return fail(PPALS_ERR_UNSUPPORTED, msg);
  }
  return PPALS_OK;
}
int ppals_tucker_residual(ppals_tucker *s, double *out) {
  if (int rc = check_tucker_influence(s, out, "ppals_tucker_residual", "out", false)) return rc;
  API_BEGIN
  *out = s->eng->residual_now();
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_tucker_slice_residuals(ppals_tucker *s, double *ss, double *total) {
  if (int rc = check_tucker_influence(s, ss, "ppals_tucker_slice_residuals", "ss", true)) return rc;
  API_BEGIN
  s->eng->slice_residuals(ss, total);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}
int ppals_tucker_leverages(ppals_tucker *s, double *lev) {
  if (int rc = check_tucker_influence(s, lev, "ppals_tucker_leverages", "lev", true)) return rc;
  API_BEGIN
  s->eng->leverages(lev);
  return PPALS_OK;
  API_END(PPALS_ERR_HIP)
}

}  // extern "C"
