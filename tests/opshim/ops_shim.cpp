// ops_shim.cpp — TEST INFRASTRUCTURE: a C surface over ppals::Ops for the op-level tests of the
// contraction kernels (tests/contraction_cases.py), of the mode-update side (tests/update_cases.py),
// of the Tucker eigen side (tests/tucker_ops_cases.py), of the tensor streams (tests/stream_cases.py)
// and of the multi-start, constraint and diagnostic ops (tests/multistart_ops_cases.py). One source, two libraries: linked against the product's libppals.so it
// reaches the HIP kernels as compiled there, linked against the host stand-in it reaches HostOps. No
// HIP code and no HIP calls here: every device action goes through the Ops.
// Every function returns 0, or -1 after an exception whose text shim_error() then returns (the
// launchers' own refusals — "padded rows inconsistent" — arrive that way).
#include <cstring>
#include <exception>
#include <string>
#include <vector>

#include "backend.h"

using namespace ppals;

namespace {
struct Shim {
  Ops *ops = nullptr;
  std::vector<std::string> log;
  std::string err, joined;
};
std::string g_create_err;

template <typename F>
int guarded(Shim *s, F &&f) {
  try {
    s->ops->bind();
    f();
    return 0;
  } catch (const std::exception &e) {
    s->err = e.what();
  } catch (...) {
    s->err = "unknown exception";
  }
  return -1;
}
std::vector<FactorRef> factors(const double *const *ptr, const int64_t *rows, const int64_t *ld, int nf) {
  std::vector<FactorRef> f((size_t)nf);
  for (int i = 0; i < nf; i++) f[i] = FactorRef{ptr[i], rows[i], ld[i]};
  return f;
}
}  // namespace

extern "C" {
const char *shim_backend() { return backend_name(); }
void *shim_create(int device) {
  Shim *s = new Shim;
  try {
    s->ops = backend_make_ops(device);
    return s;
  } catch (const std::exception &e) {
    g_create_err = e.what();
  } catch (...) {
    g_create_err = "unknown exception";
  }
  delete s;
  return nullptr;
}
const char *shim_create_error() { return g_create_err.c_str(); }
void shim_destroy(void *h) {
  Shim *s = (Shim *)h;
  if (!s) return;
  try {
    delete s->ops;
  } catch (...) {
  }
  delete s;
}
const char *shim_error(void *h) { return ((Shim *)h)->err.c_str(); }

int shim_alloc(void *h, size_t bytes, void **out) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { *out = s->ops->alloc(bytes); });
}
int shim_free(void *h, void *p) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { s->ops->free(p); });
}
int shim_h2d(void *h, void *dst, const void *src, size_t bytes) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { s->ops->h2d(dst, src, bytes); });
}
int shim_d2h(void *h, void *dst, const void *src, size_t bytes) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { s->ops->d2h(dst, src, bytes); });
}
int shim_sync(void *h) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { s->ops->sync(); });
}
int shim_scan_store_mode(void *h, int mode) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { s->ops->scan_store_mode(mode); });
}

int shim_scan_contract(void *h, const void *V, int dt, int64_t L, int64_t J, int64_t T, const double *const *fptr,
                       const int64_t *frows, const int64_t *fld, int nf, int R, void *out, int out_dt,
                       int64_t out_tstride, int64_t out_rstride, int64_t pad_ld, int64_t pad_valid) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] {
    const std::vector<FactorRef> f = factors(fptr, frows, fld, nf);
    RowPad pad;
    pad.ld = pad_ld;
    pad.valid = pad_valid;
    s->ops->scan_contract(V, dt, L, J, T, f.data(), nf, R, out, out_dt, out_tstride, out_rstride, pad);
  });
}
int shim_mttv(void *h, const void *X, int xdt, int64_t L, int64_t J, int64_t T, const double *const *fptr,
              const int64_t *frows, const int64_t *fld, int nf, int R, double *out, int64_t out_rstride,
              int accumulate, const double *out_scale) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] {
    const std::vector<FactorRef> f = factors(fptr, frows, fld, nf);
    s->ops->mttv(X, xdt, L, J, T, f.data(), nf, R, out, out_rstride, accumulate, out_scale);
  });
}
int shim_ttm_keep(void *h, const void *X, int dt, int64_t L, int64_t J, int64_t T, const double *W, int64_t ldw,
                  int Kc, double *out) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { s->ops->ttm_keep(X, dt, L, J, T, W, ldw, Kc, out); });
}
int shim_ttm_lead_front(void *h, const void *X, int dt, int64_t J, int64_t S, int64_t T, const double *W,
                        int64_t ldw, int Kc, double *out, int *taken) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { *taken = s->ops->ttm_lead_front(X, dt, J, S, T, W, ldw, Kc, out) ? 1 : 0; });
}
int shim_pp_correct(void *h, const double *M0, int64_t rows, int R, const double *const *T, const int64_t *ny,
                    const int *keep_first, const double *const *dW, const int64_t *lddw, int nterms, double *M) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] {
    std::vector<PPTerm> tm((size_t)nterms);
    for (int t = 0; t < nterms; t++) tm[t] = PPTerm{T[t], ny[t], keep_first[t], dW[t], lddw[t]};
    s->ops->pp_correct(M0, rows, R, tm.data(), nterms, M);
  });
}
int shim_arm_gram_system(void *h, const double *Gall, int N, int mode, int R, double lambda, double *S,
                         double *Sinv) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { s->ops->arm_gram_system(Gall, N, mode, R, lambda, S, Sinv); });
}

// ---- the mode-update, Normalize and factor-side ops (tests/update_cases.py) ----
int shim_gram(void *h, const double *W, int64_t rows, int64_t ld, int R, double *G) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { s->ops->gram(W, rows, ld, R, G); });
}
int shim_gram_batched(void *h, const double *W, int64_t rows, int64_t ld, int R, int nstarts, double *G,
                      int64_t gstride) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { s->ops->gram_batched(W, rows, ld, R, nstarts, G, gstride); });
}
int shim_gram_system(void *h, const double *Gall, int N, int mode, int R, double lambda, double *S, double *Sinv) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { s->ops->gram_system(Gall, N, mode, R, lambda, S, Sinv); });
}
int shim_cp_update(void *h, const double *M, int64_t ldm, const double *Wold, int64_t ldw, double *Wnew, int64_t ldn,
                   double *grad, int64_t ldg, int64_t rows, int R, const double *S, const double *Sinv, double *gradsq,
                   const double *Winit, int64_t ldi, double *dW, int64_t ldd, double ratio) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] {
    s->ops->cp_update(M, ldm, Wold, ldw, Wnew, ldn, grad, ldg, rows, R, S, Sinv, gradsq, Winit, ldi, dW, ldd, ratio);
  });
}
int shim_cp_mode_update(void *h, double *Gall, int N, int mode, int R, double lambda, const double *M, int64_t ldm,
                        double *W, int64_t ldw, double *grad, int64_t ldg, int64_t rows, double *gradsq,
                        const double *Winit, int64_t ldi, double *dW, int64_t ldd, double ratio, double *S,
                        double *Sinv, double *dwsq) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] {
    s->ops->cp_mode_update(Gall, N, mode, R, lambda, M, ldm, W, ldw, grad, ldg, rows, gradsq, Winit, ldi, dW, ldd,
                           ratio, S, Sinv, dwsq);
  });
}
int shim_cp_mode_update_batched(void *h, double *Gall, int N, int mode, int R, int nstarts, double lambda,
                                const double *M, int64_t ldm, double *W, int64_t ldw, double *grad, int64_t ldg,
                                int64_t rows, double *gradsq, double *S, double *Sinv) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] {
    s->ops->cp_mode_update_batched(Gall, N, mode, R, nstarts, lambda, M, ldm, W, ldw, grad, ldg, rows, gradsq, S,
                                   Sinv);
  });
}
int shim_cp_mode_update_blocked(void *h, double *Gall, int N, int mode, int R, double lambda, const double *Mblk,
                                int64_t blk, int P, double *scratch, double *W, int64_t ldw, double *grad,
                                int64_t ldg, int64_t rows, double *gradsq, const double *Winit, int64_t ldi,
                                double *dW, int64_t ldd, double ratio, double *S, double *Sinv) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] {
    s->ops->cp_mode_update_blocked(Gall, N, mode, R, lambda, Mblk, blk, P, scratch, W, ldw, grad, ldg, rows, gradsq,
                                   Winit, ldi, dW, ldd, ratio, S, Sinv);
  });
}
int shim_arm_normalize(void *h, double *const *W, const int64_t *rows, int N, int R, double *Gall, int mode,
                       double *wsq, double *ms_dst, const unsigned *masks, unsigned active, unsigned fresh,
                       int *taken) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] {
    *taken = s->ops->arm_normalize(W, rows, N, R, Gall, mode, wsq, ms_dst, masks, active, fresh) ? 1 : 0;
  });
}
int shim_normalize(void *h, double *const *W, const int64_t *rows, int N, int R, double *Gall) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { s->ops->normalize(W, rows, N, R, Gall); });
}
int shim_normalize_ms(void *h, double *const *W, const int64_t *rows, int N, int R, double *Gall, double *ms_dst,
                      const unsigned *masks, unsigned active, unsigned fresh, double *wsq) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { s->ops->normalize_ms(W, rows, N, R, Gall, ms_dst, masks, active, fresh, wsq); });
}
int shim_normalize_scales(void *h, const double **out) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { *out = s->ops->normalize_scales(); });
}
int shim_diff_norms(void *h, double *const *A, double *const *B, const int64_t *n, int N, int store_diff,
                    double *const *D, int update_prev, double *out) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { s->ops->diff_norms(A, B, n, N, store_diff, D, update_prev, out); });
}
int shim_pack_blocks(void *h, const double *nat, int64_t rows, int64_t ld, int R, int64_t blk, int P,
                     double *blocked) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { s->ops->pack_blocks(nat, rows, ld, R, blk, P, blocked); });
}
int shim_unpack_blocks(void *h, const double *blocked, int64_t rows, int64_t ld, int R, int64_t blk, int P,
                       double *nat) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { s->ops->unpack_blocks(blocked, rows, ld, R, blk, P, nat); });
}
int shim_sumsq(void *h, const double *x, int64_t n, double *out) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { s->ops->sumsq(x, n, out); });
}
int shim_scale_update(void *h, double *dst, const double *scales, unsigned mask, int set_one) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { s->ops->scale_update(dst, scales, mask, set_one); });
}
int shim_scale_update_many(void *h, double *dst, const double *scales, const unsigned *masks, unsigned active,
                           unsigned fresh) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { s->ops->scale_update_many(dst, scales, masks, active, fresh); });
}

// ---- the Tucker eigen side and the low-rank factor ops (tests/tucker_ops_cases.py) ----
int shim_d2d(void *h, void *dst, const void *src, size_t bytes) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { s->ops->d2d(dst, src, bytes); });
}
int shim_unfold_gram(void *h, const void *X, int dt, int64_t L, int64_t J, int64_t T, double *G) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { s->ops->unfold_gram(X, dt, L, J, T, G); });
}
int shim_top_eigvecs(void *h, double *G, int64_t J, int rank, double *U) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { s->ops->top_eigvecs(G, J, rank, U); });
}
int shim_top_eigvecs_warm(void *h, double *G, int64_t J, int rank, double *U, int slot) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { s->ops->top_eigvecs_warm(G, J, rank, U, slot); });
}
int shim_eig_lazy(void *h, int slot, int on) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { s->ops->eig_lazy(slot, on != 0); });
}
int shim_eig_defer(void *h, int slot, int on) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { s->ops->eig_defer(slot, on != 0); });
}
int shim_eig_gram(void *h, int slot, int64_t J, double **out) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { *out = s->ops->eig_gram(slot, J); });
}
int shim_eig_deferred(void *h, int slot, int *out) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { *out = s->ops->eig_deferred(slot) ? 1 : 0; });
}
int shim_eig_verify(void *h, int slot, int discard, int *out) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { *out = s->ops->eig_verify(slot, discard != 0); });
}
int shim_eig_pending_rotation(void *h, int slot, const double **out) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { *out = s->ops->eig_pending_rotation(slot); });
}
int shim_eig_rotation_done(void *h, int slot) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { s->ops->eig_rotation_done(slot); });
}
int shim_eig_session_new(void *h, int *out) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { *out = s->ops->eig_session_new(); });
}
int shim_eig_session_free(void *h, int base) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { s->ops->eig_session_free(base); });
}
int shim_orthonormalize(void *h, double *U, int64_t rows, int r, int *ok) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { *ok = s->ops->orthonormalize(U, rows, r) ? 1 : 0; });
}
int shim_sign_align(void *h, double *W, const double *Wref, int64_t rows, int r) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { s->ops->sign_align(W, Wref, rows, r); });
}
int shim_rows_times_small(void *h, const double *A, int64_t rows, int K, const double *B, int C, const double *D,
                          double *out) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { s->ops->rows_times_small(A, rows, K, B, C, D, out); });
}
int shim_lowrank_accumulate(void *h, void *X, int xdt, int64_t n, int R, const double *T, int r, const double *VT) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { s->ops->lowrank_accumulate(X, xdt, n, R, T, r, VT); });
}
int shim_add_inplace(void *h, double *dst, const double *src, int64_t n) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { s->ops->add_inplace(dst, src, n); });
}
int shim_transpose2d(void *h, const void *src, int dt, int64_t rows, int64_t cols, void *dst) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { s->ops->transpose2d(src, dt, rows, cols, dst); });
}
int shim_transpose_batched(void *h, const void *src, int dt, int64_t rows, int64_t cols, int64_t batch, void *dst) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { s->ops->transpose_batched(src, dt, rows, cols, batch, dst); });
}

// ---- the tensor streams: generation, residual, layouts and shards (tests/stream_cases.py) ----
int shim_fill_uniform(void *h, void *V, int dt, int64_t l0, int64_t g0, int64_t row0, int64_t rest, uint64_t seed,
                      double lo, double hi) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { s->ops->fill_uniform(V, dt, l0, g0, row0, rest, seed, lo, hi); });
}
int shim_fill_laplacian(void *h, void *V, int dt, int64_t l0, int64_t g0, int64_t row0, int64_t rest, int ndigits,
                        int sdim) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { s->ops->fill_laplacian(V, dt, l0, g0, row0, rest, ndigits, sdim); });
}
int shim_add_uniform_noise(void *h, void *V, int dt, int64_t l0, int64_t g0, int64_t row0, int64_t rest,
                           uint64_t seed, double lo, double hi, double alpha) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { s->ops->add_uniform_noise(V, dt, l0, g0, row0, rest, seed, lo, hi, alpha); });
}
int shim_uniform_sumsq(void *h, int64_t l0, int64_t g0, int64_t row0, int64_t rest, uint64_t seed, double lo,
                       double hi, double *out) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { s->ops->uniform_sumsq(l0, g0, row0, rest, seed, lo, hi, out); });
}
int shim_fill_rank(void *h, void *V, int dt, int64_t M, int64_t K, const double *Q, const double *P, int R) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { s->ops->fill_rank(V, dt, M, K, Q, P, R); });
}
int shim_residual_sq(void *h, const void *V, int dt, int64_t M, int64_t K, const double *Q, const double *P, int R,
                     double *out) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { s->ops->residual_sq(V, dt, M, K, Q, P, R, out); });
}
// host_full: HOST memory, the full tensor (g0 x rest doubles)
int shim_upload_shard(void *h, void *V, int dt, const double *host_full, int64_t l0, int64_t g0, int64_t row0,
                      int64_t rest) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { s->ops->upload_shard(V, dt, host_full, l0, g0, row0, rest); });
}
int shim_download_shard(void *h, const void *V, int dt, double *host_full, int64_t l0, int64_t g0, int64_t row0,
                        int64_t rest) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { s->ops->download_shard(V, dt, host_full, l0, g0, row0, rest); });
}
int shim_pad_layout(void *h, const void *src, int dt, int64_t rows, int64_t cols, int64_t blk, int64_t ld,
                    void *dst) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { s->ops->pad_layout(src, dt, rows, cols, blk, ld, dst); });
}
int shim_unpack_shards(void *h, const void *stage, int dt, int64_t s0, int64_t rest, int64_t blk, int P,
                       int64_t chunk_bytes, void *full) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { s->ops->unpack_shards(stage, dt, s0, rest, blk, P, chunk_bytes, full); });
}
int shim_krp(void *h, double *out, const double *const *fptr, const int64_t *frows, const int64_t *fld, int nf,
             int col0, int ncols) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] {
    const std::vector<FactorRef> f = factors(fptr, frows, fld, nf);
    s->ops->krp(out, f.data(), nf, col0, ncols);
  });
}

// ---- the multi-start, constraint and diagnostic ops (tests/multistart_ops_cases.py) ----
// A StartTable crosses as (nstarts, col, sq) and is copied in AS GIVEN (col / sq hold min(max(nstarts, 0), 32)
// + 1 entries), so that a malformed table reaches the launcher's own check.
namespace {
StartTable table(int nstarts, const int *col, const int *sq) {
  StartTable t;
  t.nstarts = nstarts;
  const int n = nstarts < 0 ? 0 : nstarts > kMaxStarts ? kMaxStarts : nstarts;
  for (int b = 0; b <= n; b++) {
    t.col[b] = col[b];
    t.sq[b] = sq[b];
  }
  return t;
}
Ops::CongruenceSide side(const double *const *w, const int64_t *ld, const int64_t *rows, int cols, int N) {
  Ops::CongruenceSide s;
  for (int i = 0; i < MAX_ORDER; i++) {
    s.w[i] = i < N ? w[i] : nullptr;
    s.ld[i] = i < N ? ld[i] : 0;
    s.rows[i] = i < N ? rows[i] : 0;
  }
  s.cols = cols;
  return s;
}
}  // namespace
int shim_cp_mode_update_ragged(void *h, double *Gall, int N, int mode, int nstarts, const int *col, const int *sq,
                               double lambda, const double *M, int64_t ldm, double *W, int64_t ldw, double *grad,
                               int64_t ldg, int64_t rows, double *gradsq, double *S, double *Sinv) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] {
    s->ops->cp_mode_update_ragged(Gall, N, mode, table(nstarts, col, sq), lambda, M, ldm, W, ldw, grad, ldg, rows,
                                  gradsq, S, Sinv);
  });
}
int shim_gram_ragged(void *h, const double *W, int64_t rows, int64_t ld, int nstarts, const int *col, const int *sq,
                     int N, int mode, double *Gall) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { s->ops->gram_ragged(W, rows, ld, table(nstarts, col, sq), N, mode, Gall); });
}
int shim_cp_mode_update_nn(void *h, double *Gall, int N, int mode, int R, double lambda, const double *M, int64_t ldm,
                           double *W, int64_t ldw, double *grad, int64_t ldg, int64_t rows, double *gradsq,
                           double *S) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] {
    s->ops->cp_mode_update_nn(Gall, N, mode, R, lambda, M, ldm, W, ldw, grad, ldg, rows, gradsq, S);
  });
}
int shim_cp_mode_update_nn_batched(void *h, double *Gall, int N, int mode, int R, int nstarts, double lambda,
                                   const double *M, int64_t ldm, double *W, int64_t ldw, double *grad, int64_t ldg,
                                   int64_t rows, double *gradsq, double *S) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] {
    s->ops->cp_mode_update_nn_batched(Gall, N, mode, R, nstarts, lambda, M, ldm, W, ldw, grad, ldg, rows, gradsq, S);
  });
}
int shim_cp_mode_update_nn_ragged(void *h, double *Gall, int N, int mode, int nstarts, const int *col, const int *sq,
                                  double lambda, const double *M, int64_t ldm, double *W, int64_t ldw, double *grad,
                                  int64_t ldg, int64_t rows, double *gradsq, double *S) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] {
    s->ops->cp_mode_update_nn_ragged(Gall, N, mode, table(nstarts, col, sq), lambda, M, ldm, W, ldw, grad, ldg, rows,
                                     gradsq, S);
  });
}
int shim_cp_hold_rows(void *h, double *W, int64_t ldw, double *grad, int64_t ldg, double *scores, int64_t lds,
                      int64_t rows, int nstarts, const int *col, const int *sq, const uint8_t *keep, unsigned holds,
                      double *Gall, int N, int mode, double *gradsq) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] {
    s->ops->cp_hold_rows(W, ldw, grad, ldg, scores, lds, rows, table(nstarts, col, sq), keep, holds, Gall, N, mode,
                         gradsq);
  });
}
int shim_cp_pinv_ragged(void *h, const double *Gall, int N, int nstarts, const int *col, const int *sq,
                        double *const *W, const int64_t *rows, double *const *P, int *bad) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { s->ops->cp_pinv_ragged(Gall, N, table(nstarts, col, sq), W, rows, P, bad); });
}
int shim_core_score(void *h, double *core, int R, int N, const int *bad, double *cc) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { s->ops->core_score(core, R, N, bad, cc); });
}
int shim_factor_congruence_work(void *h, int N, const double *const *aw, const int64_t *ald, const int64_t *arows,
                                int acols, const double *const *bw, const int64_t *bld, const int64_t *brows,
                                int bcols, int64_t *bytes) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] {
    *bytes = (int64_t)s->ops->factor_congruence_work(N, side(aw, ald, arows, acols, N), side(bw, bld, brows, bcols, N));
  });
}
int shim_factor_congruence(void *h, int N, const double *const *aw, const int64_t *ald, const int64_t *arows,
                           int acols, const double *const *bw, const int64_t *bld, const int64_t *brows, int bcols,
                           unsigned mask, void *work, double *Phi, double *wa, double *wb) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] {
    s->ops->factor_congruence(N, side(aw, ald, arows, acols, N), side(bw, bld, brows, bcols, N), mask, work, Phi, wa,
                              wb);
  });
}
int shim_row_dots(void *h, const double *P, const double *W, int64_t rows, int R, int64_t ld, double *out) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { s->ops->row_dots(P, W, rows, R, ld, out); });
}
int shim_fold_slice_sums(void *h, const double *src, const int64_t *lens, int n, double *out) {
  Shim *s = (Shim *)h;
  return guarded(s, [&] { s->ops->fold_slice_sums(src, lens, n, out); });
}

// the route log (ops.h): attach (on != 0) or detach, read as one newline-joined string, clear
void shim_route_attach(void *h, int on) {
  Shim *s = (Shim *)h;
  s->ops->route_log = on ? &s->log : nullptr;
}
const char *shim_route_read(void *h) {
  Shim *s = (Shim *)h;
  s->joined.clear();
  for (const std::string &t : s->log) {
    if (!s->joined.empty()) s->joined += '\n';
    s->joined += t;
  }
  return s->joined.c_str();
}
void shim_route_clear(void *h) { ((Shim *)h)->log.clear(); }
}
