// engine.cpp — host control flow of the CP ALS sweep engine (dimension tree + pairwise
// perturbation) over abstract device ops. Mirrors the reference's orchestration:
//   Construct_Dimension_Tree  common.cxx:225-270     -> build_tree
//   mttkrp_map_DT             common.cxx:20-133      -> compute_node (fused per node, no s^(N-1)R
//                                                       intermediate, no copy of V)
//   alsCP_DT                  als_CP.cxx:127-320     -> run_dt / sweep_dt
//   Build_mttkrp_map          als_CP.cxx:352-409     -> pp_get
//   alsCP_DT_sub / PP_sub     als_CP.cxx:418-833     -> dt_sub / pp_sub
//   alsCP_PP                  als_CP.cxx:1082-1137   -> run_pp
//   alsCP_PP_partupdate       als_CP.cxx:852-1207    -> run_pp_partupdate
//   CPD<dtype,Optimizer>::als src/CP.cxx:100-186     -> run_class / update_modes
// Default sweep schedule: the multi-sweep dimension tree (MSDT) of the reference's class API
// (src/optimizer/cp_msdt_optimizer.cxx:172-207): ONE first-level contraction V x_r W_r is reused
// for the next N-1 mode updates, so an exact sweep costs N/(N-1) tensor scans instead of 2 — the
// very same ALS iterates (same update order, same normal equations), 1.5x fewer tensor bytes at
// N = 4. ppals_cp_set_schedule(0) selects the two-first-level-node tree of alsCP_DT instead.
// Multi-GPU: V is block-partitioned along mode 0; factors are replicated; each
// mode update combines the s x R partial MTTKRP rows over the communicator — one all-reduce plus
// the redundant fused update for small messages, reduce-scatter / row-block solve / all-gather
// otherwise (mode_update).
#include "engine.h"
#include "assignment.h"
#include "run_report.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <limits>
#include <stdexcept>

namespace ppals {

// ============================================================================ tensor helpers
int tensor_create(Ops &ops, Comm &comm, int order, const int64_t *glens, int dtype,
                  TensorDesc *out, std::string *err) {
  if (order < 2 || order > MAX_ORDER) {
    *err = "tensor order must be in [2, 8]";
    return -1;
  }
  if (!ops.supports_storage(dtype))
    throw Unsupported(dtype == BF16 ? "ppals: this back end cannot store a bf16 tensor"
                                    : "ppals: this back end cannot store this tensor type");
  TensorDesc t;
  t.order = order;
  t.dtype = dtype;
  int64_t rest = 1;
  for (int i = 0; i < order; i++) {
    if (glens[i] <= 0) {
      *err = "tensor extents must be positive";
      return -1;
    }
    t.glens[i] = glens[i];
    t.llens[i] = glens[i];
    if (i > 0) rest *= glens[i];
  }
  const int P = comm.size();
  const int64_t blk = block_rows(glens[0], P);
  t.row0 = blk * comm.rank();
  t.llens[0] = std::max<int64_t>(0, std::min(blk, glens[0] - t.row0));
  if (blk * (P - 1) >= glens[0]) {
    // decided from global quantities only, so EVERY rank returns the error (no rank is left
    // waiting in a collective): with row blocks of ceil(s0/P) the last rank would own no rows
    *err = "leading mode too short for this many ranks (the last rank would own no rows)";
    return -1;
  }
  t.nloc = t.llens[0] * rest;
  t.data = ops.alloc((size_t)t.nloc * dtype_size(dtype));
  *out = t;
  return 0;
}

static int64_t rest_of(const TensorDesc &V) {
  int64_t r = 1;
  for (int i = 1; i < V.order; i++) r *= V.glens[i];
  return r;
}

// device Khatri-Rao operands of the two halves of the mode set: Q over modes [0,h), P over [h,N)
static void split_krp(Ops &ops, const TensorDesc &V, int R, double *const *W, double *Q, double *P,
                      int64_t *M, int64_t *K) {
  const int N = V.order, h = N / 2;
  FactorRef fq[MAX_ORDER], fp[MAX_ORDER];
  int64_t m = 1, k = 1;
  for (int i = 0; i < h; i++) {
    fq[i].ptr = W[i] + (i == 0 ? V.row0 : 0);
    fq[i].rows = V.llens[i];
    fq[i].ld = V.glens[i];
    m *= V.llens[i];
  }
  for (int i = h; i < N; i++) {
    fp[i - h].ptr = W[i];
    fp[i - h].rows = V.glens[i];
    fp[i - h].ld = V.glens[i];
    k *= V.glens[i];
  }
  ops.krp(Q, fq, h, 0, R);
  ops.krp(P, fp, N - h, 0, R);
  *M = m;
  *K = k;
}
static void split_sizes(const TensorDesc &V, int64_t *M, int64_t *K) {
  const int N = V.order, h = N / 2;
  int64_t m = 1, k = 1;
  for (int i = 0; i < h; i++) m *= V.llens[i];
  for (int i = h; i < N; i++) k *= V.glens[i];
  *M = m;
  *K = k;
}

// `-tensor r` (test_ALS.cxx:275-286): V = [[W_true]], built on the device
void tensor_fill_cp(Ops &ops, const TensorDesc &V, int R, const double *Wtrue_flat) {
  const int N = V.order;
  DeviceBufferTable W;
  W.resize(N);
  const double *src = Wtrue_flat;
  for (int i = 0; i < N; i++) {
    size_t n = (size_t)V.glens[i] * R;
    W.alloc(ops, i, n * sizeof(double));
    ops.h2d(W[i], src, n * sizeof(double));
    src += n;
  }
  int64_t M, K;
  split_sizes(V, &M, &K);
  DeviceBuffer Q(ops, sizeof(double) * M * R), Pm(ops, sizeof(double) * K * R);
  split_krp(ops, V, R, W.data(), Q.as<double>(), Pm.as<double>(), &M, &K);
  ops.fill_rank(V.data, V.dtype, M, K, Q.as<double>(), Pm.as<double>(), R);
  ops.sync();
}
void tensor_fill_uniform(Ops &ops, const TensorDesc &V, uint64_t seed, double lo, double hi) {
  ops.fill_uniform(V.data, V.dtype, V.llens[0], V.glens[0], V.row0, rest_of(V), seed, lo, hi);
  ops.sync();
}
void tensor_upload(Ops &ops, const TensorDesc &V, const double *host_full) {
  ops.upload_shard(V.data, V.dtype, host_full, V.llens[0], V.glens[0], V.row0, rest_of(V));
}
void tensor_download(Ops &ops, const TensorDesc &V, double *host_full) {
  ops.download_shard(V.data, V.dtype, host_full, V.llens[0], V.glens[0], V.row0, rest_of(V));
}
void tensor_fill_laplacian(Ops &ops, const TensorDesc &V, int ndigits, int s) {
  ops.fill_laplacian(V.data, V.dtype, V.llens[0], V.glens[0], V.row0, rest_of(V), ndigits, s);
  ops.sync();
}

// host-side counter RNG identical to the device / oracle generator
static inline uint64_t sm64_host(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
static inline double u01_host(uint64_t seed, uint64_t idx) {
  uint64_t h = sm64_host(sm64_host(seed) ^ idx);
  return (double)(h >> 11) * (1.0 / 9007199254740992.0);
}

// Gen_collinearity (common.cxx:361-423): per mode j, the rank-i vector is re-drawn until its
// collinearity with every earlier vector of that mode lies in [col_min, col_max]; component i is
// weighted lambda_i = 0.2 + 0.6/R*(i+1) (folded into the mode-0 factor here).
void collinear_factors(const int64_t *lens, int N, int R, double col_min, double col_max,
                       uint64_t seed, double *Wflat) {
  double *W = Wflat;
  for (int j = 0; j < N; j++) {
    const int64_t s = lens[j];
    uint64_t draw = 0;
    for (int i = 0; i < R; i++) {
      double *vi = W + s * i;
      for (int attempt = 0; attempt < 100000; attempt++) {
        const uint64_t sd = seed + 7919ull * (uint64_t)j + 104729ull * (draw++);
        for (int64_t e = 0; e < s; e++) vi[e] = u01_host(sd, (uint64_t)e);
        bool ok = true;
        for (int k = 0; k < i && ok; k++) {
          const double *vk = W + s * k;
          double ip = 0, n1 = 0, n2 = 0;
          for (int64_t e = 0; e < s; e++) {
            ip += vi[e] * vk[e];
            n1 += vi[e] * vi[e];
            n2 += vk[e] * vk[e];
          }
          const double col = ip / (std::sqrt(n1) * std::sqrt(n2));
          if (col < col_min || col > col_max) ok = false;
        }
        if (ok) break;
      }
    }
    W += s * R;
  }
  for (int i = 0; i < R; i++) {
    const double lambda_ = 0.2 + 0.6 / R * (i + 1);
    for (int64_t e = 0; e < lens[0]; e++) Wflat[e + lens[0] * i] *= lambda_;
  }
}

void tensor_fill_collinear(Ops &ops, Comm &comm, const TensorDesc &V, int R, double col_min,
                           double col_max, double ratio_noise, uint64_t seed) {
  size_t tot = 0;
  for (int i = 0; i < V.order; i++) tot += (size_t)V.glens[i] * R;
  std::vector<double> W(tot);
  collinear_factors(V.glens, V.order, R, col_min, col_max, seed, W.data());
  tensor_fill_cp(ops, V, R, W.data());
  // V += ratio_noise * ||V|| / ||noise|| * noise, noise ~ U(-1,1)   (test_ALS.cxx:259-264)
  const double vnorm = tensor_norm(ops, comm, V);
  DeviceBuffer dbuf(ops, sizeof(double));
  double *d = dbuf.as<double>();
  const uint64_t nseed = seed + 0x5eedull;
  ops.uniform_sumsq(V.llens[0], V.glens[0], V.row0, rest_of(V), nseed, -1.0, 1.0, d);
  if (comm.size() > 1) comm.allreduce_sum(d, 1);
  double nsq = 0;
  ops.d2h(&nsq, d, sizeof(double));
  const double alpha = ratio_noise * vnorm / std::sqrt(nsq);
  ops.add_uniform_noise(V.data, V.dtype, V.llens[0], V.glens[0], V.row0, rest_of(V), nseed, -1.0,
                        1.0, alpha);
  ops.sync();
}

double tensor_norm(Ops &ops, Comm &comm, const TensorDesc &V) {
  int64_t M, K;
  split_sizes(V, &M, &K);
  DeviceBuffer dbuf(ops, sizeof(double));
  double *d = dbuf.as<double>();
  ops.residual_sq(V.data, V.dtype, M, K, nullptr, nullptr, 0, d);
  if (comm.size() > 1) comm.allreduce_sum(d, 1);
  double h = 0;
  ops.d2h(&h, d, sizeof(double));
  return std::sqrt(h);
}

PrepShape prep_shape(const TensorDesc &V, int mode) {
  PrepShape s;
  for (int i = 0; i < mode; i++) s.L *= V.llens[i];
  s.J = V.llens[mode];
  for (int i = mode + 1; i < V.order; i++) s.T *= V.llens[i];
  return s;
}
void tensor_center(Ops &ops, const TensorDesc &V, int mode, double *offsets_dev) {
  const PrepShape s = prep_shape(V, mode);
  ops.center_fibres(V.data, V.dtype, s.L, s.J, s.T, offsets_dev);
}
void tensor_shift(Ops &ops, const TensorDesc &V, int mode, const double *offsets_dev, double alpha) {
  const PrepShape s = prep_shape(V, mode);
  ops.shift_fibres(V.data, V.dtype, s.L, s.J, s.T, offsets_dev, alpha);
}
void tensor_slice_sumsq(Ops &ops, const TensorDesc &V, int mode, double *ss_host) {
  const PrepShape s = prep_shape(V, mode);
  DeviceBuffer dbuf(ops, sizeof(double) * s.J);
  double *d = dbuf.as<double>();
  ops.slice_sumsq(V.data, V.dtype, s.L, s.J, s.T, d);
  ops.d2h(ss_host, d, sizeof(double) * s.J);
}
void tensor_rescale(Ops &ops, const TensorDesc &V, int mode, const double *factors_host) {
  const PrepShape s = prep_shape(V, mode);
  DeviceBuffer dbuf(ops, sizeof(double) * s.J);
  double *d = dbuf.as<double>();
  ops.h2d(d, factors_host, sizeof(double) * s.J);
  ops.scale_slices(V.data, V.dtype, s.L, s.J, s.T, d);  // (the buffer's release waits for the launch)
}
void tensor_scale(Ops &ops, const TensorDesc &V, int mode, double *rms_host) {
  const PrepShape s = prep_shape(V, mode);
  std::vector<double> ss((size_t)s.J), f((size_t)s.J);
  tensor_slice_sumsq(ops, V, mode, ss.data());
  const double n = (double)s.L * (double)s.T;
  for (int64_t x = 0; x < s.J; x++) {
    const double rms = std::sqrt(ss[(size_t)x] / n);
    if (rms_host) rms_host[x] = rms;
    f[(size_t)x] = rms > 0 && rms <= std::numeric_limits<double>::max() ? 1.0 / rms : 1.0;
  }
  tensor_rescale(ops, V, mode, f.data());
}

// ============================================================================ N-PLS
namespace {
// a device array of n doubles for the length of a call
DeviceBuffer doubles(Ops &ops, int64_t n) {
  return DeviceBuffer(ops, sizeof(double) * (size_t)std::max<int64_t>(n, 1));
}
double dotn(const double *a, const double *b, int64_t n) {
  double s = 0;
  for (int64_t i = 0; i < n; i++) s += a[i] * b[i];
  return s;
}
// A x = b, A n x n column-major (destroyed), partial pivoting; a zero pivot gives x = 0 for that unknown
void solve_small(std::vector<double> &A, std::vector<double> &b, int n) {
  for (int k = 0; k < n; k++) {
    int p = k;
    for (int i = k + 1; i < n; i++)
      if (std::fabs(A[i + (size_t)n * k]) > std::fabs(A[p + (size_t)n * k])) p = i;
    if (p != k) {
      for (int j = 0; j < n; j++) std::swap(A[k + (size_t)n * j], A[p + (size_t)n * j]);
      std::swap(b[k], b[p]);
    }
    const double d = A[k + (size_t)n * k];
    if (d == 0) continue;
    for (int i = k + 1; i < n; i++) {
      const double m = A[i + (size_t)n * k] / d;
      if (m == 0) continue;
      for (int j = k; j < n; j++) A[i + (size_t)n * j] -= m * A[k + (size_t)n * j];
      b[i] -= m * b[k];
    }
  }
  for (int k = n - 1; k >= 0; k--) {
    double s = b[k];
    for (int j = k + 1; j < n; j++) s -= A[k + (size_t)n * j] * b[j];
    const double d = A[k + (size_t)n * k];
    b[k] = d == 0 ? 0.0 : s / d;
  }
}
// the modes off the sample mode: their extents, and where each one's vector starts in a component's weights
struct NplsDims {
  int K = 0;
  int64_t ext[MAX_ORDER], off[MAX_ORDER], sum = 0, LT = 1;
  NplsDims(int order, const int64_t *lens, int mode) {
    for (int i = 0; i < order; i++)
      if (i != mode) {
        ext[K] = lens[i];
        off[K] = sum;
        sum += lens[i];
        LT *= lens[i];
        K++;
      }
  }
};
// A = the outer product of the K vectors at wdev + off[k], leaving out mode `skip` (-1: none)
void npls_outer(Ops &ops, const NplsDims &d, const double *wdev, int skip, double *A) {
  int64_t ext[MAX_ORDER], n = 1;
  const double *w[MAX_ORDER];
  int K = 0;
  for (int k = 0; k < d.K; k++)
    if (k != skip) {
      ext[K] = d.ext[k];
      w[K] = wdev + d.off[k];
      n *= d.ext[k];
      K++;
    }
  ops.zero(A, sizeof(double) * (size_t)n);
  ops.npls_outer_axpy(A, ext, K, w, 1.0);
}
// v = Z contracted with the vectors at wdev over every mode but k (ext[k] doubles on the host); scratch: LT doubles
void npls_mode_product(Ops &ops, const NplsDims &d, const double *Z, const double *wdev, int k, double *scratch,
                       double *dS, double *v) {
  int64_t L = 1, T = 1;
  for (int j = 0; j < k; j++) L *= d.ext[j];
  for (int j = k + 1; j < d.K; j++) T *= d.ext[j];
  npls_outer(ops, d, wdev, k, scratch);
  ops.npls_slice_inner(Z, F64, L, d.ext[k], T, scratch, 1, dS);
  ops.d2h(v, dS, sizeof(double) * (size_t)d.ext[k]);
}
bool normalise(double *v, int64_t n) {
  const double nrm = std::sqrt(dotn(v, v, n));
  if (!(nrm > 0) || !std::isfinite(nrm)) return false;
  for (int64_t i = 0; i < n; i++) v[i] /= nrm;
  return true;
}
// The best rank-one approximation of Z (order K, LT doubles on the device) by alternating power iterations, started
// from the fibres through the entry of largest magnitude. w: d.sum doubles on the host, wdev: the same on the
// device (left holding w). false: Z is zero or not finite. *capped: hopm_max rounds ran without settling.
bool npls_rank_one(Ops &ops, const NplsDims &d, const double *Z, const NplsOpts &o, double *w, double *wdev,
                   double *scratch, double *dS, double *dE, bool *capped) {
  *capped = false;
  double top[2];
  ops.npls_argmax(Z, d.LT, dS);
  ops.d2h(top, dS, sizeof(top));
  if (!(top[0] > 0) || !std::isfinite(top[0])) return false;
  if (d.K == 1) {  // ordinary PLS: w = Z / |Z|
    ops.d2h(w, Z, sizeof(double) * (size_t)d.ext[0]);
    if (!normalise(w, d.ext[0])) return false;
    ops.h2d(wdev, w, sizeof(double) * (size_t)d.sum);
    return true;
  }
  {  // the start: unit vectors at the position of the largest entry pick its fibres
    std::vector<double> e((size_t)d.sum, 0.0);
    int64_t rem = (int64_t)top[1];
    for (int k = 0; k < d.K; k++) {
      e[(size_t)(d.off[k] + rem % d.ext[k])] = 1.0;
      rem /= d.ext[k];
    }
    ops.h2d(dE, e.data(), sizeof(double) * e.size());
    for (int k = 0; k < d.K; k++) {
      npls_mode_product(ops, d, Z, dE, k, scratch, dS, w + d.off[k]);
      if (!normalise(w + d.off[k], d.ext[k])) return false;
    }
    ops.h2d(wdev, w, sizeof(double) * (size_t)d.sum);
  }
  std::vector<double> v;
  bool settled = false;
  for (int round = 0; round < o.hopm_max && !settled; round++) {
    double moved = 0;
    for (int k = 0; k < d.K; k++) {
      v.resize((size_t)d.ext[k]);
      npls_mode_product(ops, d, Z, wdev, k, scratch, dS, v.data());
      if (!normalise(v.data(), d.ext[k])) return false;
      for (int64_t i = 0; i < d.ext[k]; i++) {
        moved = std::max(moved, std::fabs(v[(size_t)i] - w[d.off[k] + i]));
        w[d.off[k] + i] = v[(size_t)i];
      }
      ops.h2d(wdev + d.off[k], v.data(), sizeof(double) * v.size());
    }
    settled = moved <= o.hopm_tol;
  }
  *capped = !settled;
  // signs: the entry of largest magnitude of every vector but the last positive; the last one, updated last, has
  // <Z, W> > 0 with the others as they were and takes their flips
  double sg = 1.0;
  for (int k = 0; k + 1 < d.K; k++) {
    int64_t p = 0;
    for (int64_t i = 1; i < d.ext[k]; i++)
      if (std::fabs(w[d.off[k] + i]) > std::fabs(w[d.off[k] + p])) p = i;
    if (w[d.off[k] + p] < 0) {
      for (int64_t i = 0; i < d.ext[k]; i++) w[d.off[k] + i] = -w[d.off[k] + i];
      sg = -sg;
    }
  }
  if (sg < 0)
    for (int64_t i = 0; i < d.ext[d.K - 1]; i++) w[d.off[d.K - 1] + i] = -w[d.off[d.K - 1] + i];
  ops.h2d(wdev, w, sizeof(double) * (size_t)d.sum);
  return true;
}
// <W_g, W_h> = prod_k w_g^(k) . w_h^(k); wall: component g at g * d.sum
double npls_ww(const NplsDims &d, const double *wall, int g, int h) {
  double p = 1.0;
  for (int k = 0; k < d.K; k++) p *= dotn(wall + g * d.sum + d.off[k], wall + h * d.sum + d.off[k], d.ext[k]);
  return p;
}
}  // namespace

void tensor_contract_mode(Ops &ops, const TensorDesc &V, int mode, const double *U_host, int C, double *Z_host) {
  const PrepShape s = prep_shape(V, mode);
  DeviceBuffer U = doubles(ops, s.J * C), Z = doubles(ops, s.L * s.T * C);
  ops.h2d(U.as<double>(), U_host, sizeof(double) * (size_t)(s.J * C));
  ops.npls_contract(V.data, V.dtype, s.L, s.J, s.T, U.as<double>(), C, Z.as<double>());
  ops.d2h(Z_host, Z.as<double>(), sizeof(double) * (size_t)(s.L * s.T * C));
}
void tensor_slice_inner(Ops &ops, const TensorDesc &V, int mode, const double *W_host, int C, double *S_host) {
  const PrepShape s = prep_shape(V, mode);
  DeviceBuffer W = doubles(ops, s.L * s.T * C), S = doubles(ops, s.J * C);
  ops.h2d(W.as<double>(), W_host, sizeof(double) * (size_t)(s.L * s.T * C));
  ops.npls_slice_inner(V.data, V.dtype, s.L, s.J, s.T, W.as<double>(), C, S.as<double>());
  ops.d2h(S_host, S.as<double>(), sizeof(double) * (size_t)(s.J * C));
}

void npls_fit(Ops &ops, const TensorDesc &X, int mode, const double *Y, int M, int F, const NplsOpts &o,
              NplsModel *out) {
  const PrepShape s = prep_shape(X, mode);
  const int64_t I = s.J;
  const NplsDims d(X.order, X.llens, mode);
  const int64_t LT = d.LT;
  NplsModel m;
  m.order = X.order;
  m.mode = mode;
  m.M = M;
  m.F = F;
  for (int i = 0; i < X.order; i++) m.lens[i] = X.llens[i];
  std::vector<double> T((size_t)I * F, 0.0), S((size_t)I * F, 0.0), Uy((size_t)I * F, 0.0), Q((size_t)M * F, 0.0);
  std::vector<double> B((size_t)F * F, 0.0), wall((size_t)d.sum * F, 0.0), Yres(Y, Y + (size_t)I * M), q((size_t)M), qn((size_t)M);
  const double normY2 = dotn(Y, Y, I * M);
  double normX2 = 0;
  {
    std::vector<double> ss((size_t)I);
    tensor_slice_sumsq(ops, X, mode, ss.data());
    for (int64_t i = 0; i < I; i++) normX2 += ss[(size_t)i];
  }
  DeviceBuffer dY = doubles(ops, I * M), dZm = doubles(ops, LT * M), dZ = doubles(ops, LT), dW = doubles(ops, LT);
  DeviceBuffer dwall = doubles(ops, d.sum * F), dE = doubles(ops, d.sum), dq = doubles(ops, M);
  DeviceBuffer dS = doubles(ops, std::max<int64_t>(std::max<int64_t>(I, M), std::max<int64_t>(d.sum, 2)));
  int f = 0;
  for (; f < F; f++) {
    // 1. Z_m of the deflated tensor, without deflating
    ops.h2d(dY.as<double>(), Yres.data(), sizeof(double) * Yres.size());
    ops.npls_contract(X.data, X.dtype, s.L, I, s.T, dY.as<double>(), M, dZm.as<double>());
    for (int g = 0; g < f; g++)
      for (int c = 0; c < M; c++) {
        const double coef = dotn(&T[(size_t)I * g], &Yres[(size_t)I * c], I);
        const double *w[MAX_ORDER];
        for (int k = 0; k < d.K; k++) w[k] = dwall.as<double>() + g * d.sum + d.off[k];
        if (coef != 0) ops.npls_outer_axpy(dZm.as<double>() + LT * c, d.ext, d.K, w, -coef);
      }
    // 2. q = e_m*, the column of Y_res with the largest sum of squares
    int best = 0;
    double bestss = -1;
    for (int c = 0; c < M; c++) {
      const double ss = dotn(&Yres[(size_t)I * c], &Yres[(size_t)I * c], I);
      if (ss > bestss) {
        bestss = ss;
        best = c;
      }
    }
    std::fill(q.begin(), q.end(), 0.0);
    q[(size_t)best] = 1.0;
    double *w = &wall[(size_t)d.sum * f], *wdev = dwall.as<double>() + d.sum * f;
    int status = 0;
    bool ok = true;
    for (int round = 0;; round++) {
      // 3. Z = sum_m q_m Z_m and its best rank-one approximation
      const double *Zp = dZm.as<double>();
      if (M > 1) {
        ops.h2d(dq.as<double>(), q.data(), sizeof(double) * (size_t)M);
        ops.npls_contract(dZm.as<double>(), F64, LT, M, 1, dq.as<double>(), 1, dZ.as<double>());
        Zp = dZ.as<double>();
      }
      bool capped = false;
      ok = npls_rank_one(ops, d, Zp, o, w, wdev, dW.as<double>(), dS.as<double>(), dE.as<double>(), &capped);
      if (!ok) break;
      status = (status & ~1) | (capped ? 1 : 0);
      npls_outer(ops, d, wdev, -1, dW.as<double>());
      // 4. q'_m = <Z_m, W>, normalised
      ops.npls_slice_inner(dZm.as<double>(), F64, LT, M, 1, dW.as<double>(), 1, dS.as<double>());
      ops.d2h(qn.data(), dS.as<double>(), sizeof(double) * (size_t)M);
      if (!normalise(qn.data(), M)) {
        ok = false;
        break;
      }
      double moved = 0;
      for (int c = 0; c < M; c++) moved = std::max(moved, std::fabs(qn[(size_t)c] - q[(size_t)c]));
      q = qn;
      if (M == 1 || moved <= o.inner_tol) break;
      if (round + 1 >= o.inner_max) {
        status |= 2;
        break;
      }
    }
    if (!ok) break;
    // 5. the raw scores, one pass; t_f of the deflated tensor from them
    ops.npls_slice_inner(X.data, X.dtype, s.L, I, s.T, dW.as<double>(), 1, dS.as<double>());
    ops.d2h(&S[(size_t)I * f], dS.as<double>(), sizeof(double) * (size_t)I);
    std::copy(&S[(size_t)I * f], &S[(size_t)I * f] + I, &T[(size_t)I * f]);
    for (int g = 0; g < f; g++) {
      const double ww = npls_ww(d, wall.data(), g, f);
      for (int64_t i = 0; i < I; i++) T[(size_t)(i + I * f)] -= T[(size_t)(i + I * g)] * ww;
    }
    // 6. inner relation and the residual of Y
    for (int c = 0; c < M; c++) Q[(size_t)(c + M * f)] = q[(size_t)c];
    for (int64_t i = 0; i < I; i++) {
      double u = 0;
      for (int c = 0; c < M; c++) u += Yres[(size_t)(i + I * c)] * q[(size_t)c];
      Uy[(size_t)(i + I * f)] = u;
    }
    const int n = f + 1;
    std::vector<double> G((size_t)n * n), b((size_t)n);
    for (int g = 0; g < n; g++) {
      for (int h = 0; h < n; h++) G[g + (size_t)n * h] = dotn(&T[(size_t)I * g], &T[(size_t)I * h], I);
      b[(size_t)g] = dotn(&T[(size_t)I * g], &Uy[(size_t)I * f], I);
    }
    std::vector<double> TtT = G;
    solve_small(G, b, n);
    for (int g = 0; g < n; g++) B[g + (size_t)F * f] = b[(size_t)g];
    Yres.assign(Y, Y + (size_t)I * M);
    for (int h = 0; h < n; h++)
      for (int g = 0; g <= h; g++) {
        const double bgh = B[g + (size_t)F * h];
        if (bgh == 0) continue;
        for (int c = 0; c < M; c++) {
          const double bq = bgh * Q[(size_t)(c + M * h)];
          for (int64_t i = 0; i < I; i++) Yres[(size_t)(i + I * c)] -= T[(size_t)(i + I * g)] * bq;
        }
      }
    // 7. explained variation
    m.ssy.push_back(1.0 - dotn(Yres.data(), Yres.data(), I * M) / normY2);
    double res = normX2;
    for (int g = 0; g < n; g++) {
      res -= 2.0 * dotn(&T[(size_t)I * g], &S[(size_t)I * g], I);
      for (int h = 0; h < n; h++) res += TtT[g + (size_t)n * h] * npls_ww(d, wall.data(), g, h);
    }
    m.ssx.push_back(1.0 - res / normX2);
    m.status.push_back(status);
  }
  m.nf = f;
  m.T.assign(T.begin(), T.begin() + (size_t)I * f);
  m.U.assign(Uy.begin(), Uy.begin() + (size_t)I * f);
  m.Q.assign(Q.begin(), Q.begin() + (size_t)M * f);
  m.B.assign((size_t)f * f, 0.0);
  for (int g = 0; g < f; g++)
    for (int h = 0; h < f; h++) m.B[g + (size_t)f * h] = B[g + (size_t)F * h];
  m.W.resize((size_t)d.K);
  for (int k = 0; k < d.K; k++) {
    m.W[(size_t)k].resize((size_t)d.ext[k] * f);
    for (int g = 0; g < f; g++)
      std::copy(&wall[(size_t)(d.sum * g + d.off[k])], &wall[(size_t)(d.sum * g + d.off[k])] + d.ext[k],
                &m.W[(size_t)k][(size_t)d.ext[k] * g]);
  }
  *out = std::move(m);
}

void npls_predict(Ops &ops, const NplsModel &m, const TensorDesc &Xnew, int ncomp, double *Yhat, double *Tnew) {
  const PrepShape s = prep_shape(Xnew, m.mode);
  const int64_t I = s.J;
  const NplsDims d(m.order, m.lens, m.mode);
  const int k = ncomp;
  std::vector<double> wall((size_t)d.sum * k);
  for (int g = 0; g < k; g++)
    for (int j = 0; j < d.K; j++)
      std::copy(&m.W[(size_t)j][(size_t)d.ext[j] * g], &m.W[(size_t)j][(size_t)d.ext[j] * g] + d.ext[j],
                &wall[(size_t)(d.sum * g + d.off[j])]);
  DeviceBuffer dwall = doubles(ops, d.sum * k), dW = doubles(ops, d.LT * k), dS = doubles(ops, I * k);
  ops.h2d(dwall.as<double>(), wall.data(), sizeof(double) * wall.size());
  for (int g = 0; g < k; g++) npls_outer(ops, d, dwall.as<double>() + d.sum * g, -1, dW.as<double>() + d.LT * g);
  ops.npls_slice_inner(Xnew.data, Xnew.dtype, s.L, I, s.T, dW.as<double>(), k, dS.as<double>());
  std::vector<double> T((size_t)I * k);
  ops.d2h(T.data(), dS.as<double>(), sizeof(double) * T.size());
  for (int f = 0; f < k; f++)
    for (int g = 0; g < f; g++) {
      const double ww = npls_ww(d, wall.data(), g, f);
      for (int64_t i = 0; i < I; i++) T[(size_t)(i + I * f)] -= T[(size_t)(i + I * g)] * ww;
    }
  if (Tnew) std::copy(T.begin(), T.end(), Tnew);
  std::fill(Yhat, Yhat + (size_t)I * m.M, 0.0);
  for (int h = 0; h < k; h++)
    for (int g = 0; g <= h; g++) {
      const double bgh = m.B[g + (size_t)m.nf * h];
      if (bgh == 0) continue;
      for (int c = 0; c < m.M; c++) {
        const double bq = bgh * m.Q[(size_t)(c + m.M * h)];
        for (int64_t i = 0; i < I; i++) Yhat[(size_t)(i + I * c)] += T[(size_t)(i + I * g)] * bq;
      }
    }
}

void tensor_contract_columns(Ops &ops, const TensorDesc &V, int mode, const double *U_host, int C, double *Z_host) {
  const PrepShape s = prep_shape(V, mode);
  DeviceBuffer U = doubles(ops, s.J * C), Z = doubles(ops, s.L * s.T * C);
  ops.h2d(U.as<double>(), U_host, sizeof(double) * (size_t)(s.J * C));
  ops.npls_contract_wide(V.data, V.dtype, s.L, s.J, s.T, U.as<double>(), C, Z.as<double>());
  ops.d2h(Z_host, Z.as<double>(), sizeof(double) * (size_t)(s.L * s.T * C));
}
void tensor_slice_inner_columns(Ops &ops, const TensorDesc &V, int mode, const double *W_host, int C, double *S_host) {
  const PrepShape s = prep_shape(V, mode);
  DeviceBuffer W = doubles(ops, s.L * s.T * C), S = doubles(ops, s.J * C);
  ops.h2d(W.as<double>(), W_host, sizeof(double) * (size_t)(s.L * s.T * C));
  ops.npls_slice_inner_wide(V.data, V.dtype, s.L, s.J, s.T, W.as<double>(), C, S.as<double>());
  ops.d2h(S_host, S.as<double>(), sizeof(double) * (size_t)(s.J * C));
}

int npls_crossval_group(int64_t LT, int M, int S) {
  int64_t G = std::max<int64_t>(1, kNplsCvColumns / M);
  G = std::min(G, std::max<int64_t>(1, kNplsCvBytes / ((int64_t)sizeof(double) * LT * (M + 2))));
  return (int)std::min<int64_t>(G, S);
}

namespace {
// one resampled fit of a cross-validation: everything on the host, the rows of its own segment zero in Yres and
// Ttr, so that every sum over the I samples is a sum over the training samples
struct NplsCvFit {
  int seg = 0, nf = 0;
  bool live = true;
  int64_t ntrain = 0;
  std::vector<char> held;                     // I: 1 for the samples of the segment
  std::vector<double> ymean, Yc, Yres;        // M; I x M, centred on the training samples, held-out rows zero (twice)
  std::vector<double> Tall, Ttr, Uy, Q, B, wall, q, pred;  // Tall: the scores of all I samples; pred: I x M so far
};
// steps 2-4 of npls_fit for one fit: q, Z = sum_m q_m Z_m, its rank-one weights (w on the host, wdev on the device,
// W = their outer product in dW), iterated over q. false: Z is zero or not finite.
bool npls_cv_weights(Ops &ops, const NplsDims &d, int M, int64_t I, const NplsOpts &o, const std::vector<double> &Yres,
                     double *dZm, double *dZ, double *dW, double *dq, double *dS, double *dE, double *w, double *wdev,
                     std::vector<double> &q, int *status_out) {
  const int64_t LT = d.LT;
  int best = 0;
  double bestss = -1;
  for (int c = 0; c < M; c++) {
    const double ss = dotn(&Yres[(size_t)I * c], &Yres[(size_t)I * c], I);
    if (ss > bestss) {
      bestss = ss;
      best = c;
    }
  }
  std::fill(q.begin(), q.end(), 0.0);
  q[(size_t)best] = 1.0;
  std::vector<double> qn((size_t)M);
  int status = 0;
  for (int round = 0;; round++) {
    const double *Zp = dZm;
    if (M > 1) {
      ops.h2d(dq, q.data(), sizeof(double) * (size_t)M);
      ops.npls_contract(dZm, F64, LT, M, 1, dq, 1, dZ);
      Zp = dZ;
    }
    bool capped = false;
    if (!npls_rank_one(ops, d, Zp, o, w, wdev, dW, dS, dE, &capped)) return false;
    status = (status & ~1) | (capped ? 1 : 0);
    npls_outer(ops, d, wdev, -1, dW);
    ops.npls_slice_inner(dZm, F64, LT, M, 1, dW, 1, dS);
    ops.d2h(qn.data(), dS, sizeof(double) * (size_t)M);
    if (!normalise(qn.data(), M)) return false;
    double moved = 0;
    for (int c = 0; c < M; c++) moved = std::max(moved, std::fabs(qn[(size_t)c] - q[(size_t)c]));
    q = qn;
    if (M == 1 || moved <= o.inner_tol) break;
    if (round + 1 >= o.inner_max) {
      status |= 2;
      break;
    }
  }
  *status_out = status;
  return true;
}
}  // namespace

void npls_crossval(Ops &ops, const TensorDesc &X, int mode, const double *Y, int M, int F, const int32_t *segment, int S,
                   int center, const NplsOpts &o, double *Ycv, double *press, int *fitted, int *status,
                   int64_t *x_passes) {
  const PrepShape s = prep_shape(X, mode);
  const int64_t I = s.J;
  const NplsDims d(X.order, X.llens, mode);
  const int64_t LT = d.LT;
  const int G = npls_crossval_group(LT, M, S);
  int64_t passes = 0;
  if (status) std::fill(status, status + (size_t)S * F, 0);
  DeviceBuffer dY = doubles(ops, I * M * G), dZm = doubles(ops, LT * M * G), dW = doubles(ops, LT * G), dZ = doubles(ops, LT);
  DeviceBuffer dwall = doubles(ops, d.sum * F * G), dE = doubles(ops, d.sum), dq = doubles(ops, M);
  DeviceBuffer dS = doubles(ops, std::max<int64_t>(std::max<int64_t>(I * G, M), std::max<int64_t>(d.sum, 2)));
  std::vector<double> Yh((size_t)I * M * G), Sh((size_t)I * G);
  for (int s0 = 0; s0 < S; s0 += G) {
    const int ng = std::min(G, S - s0);
    std::vector<NplsCvFit> fits((size_t)ng);
    for (int j = 0; j < ng; j++) {
      NplsCvFit &ft = fits[(size_t)j];
      ft.seg = s0 + j;
      ft.held.assign((size_t)I, 0);
      for (int64_t i = 0; i < I; i++) ft.held[(size_t)i] = segment[i] == ft.seg;
      for (int64_t i = 0; i < I; i++) ft.ntrain += !ft.held[(size_t)i];
      ft.ymean.assign((size_t)M, 0.0);
      ft.Yc.assign((size_t)I * M, 0.0);
      for (int c = 0; c < M; c++) {
        double sum = 0;
        if (center) {
          for (int64_t i = 0; i < I; i++)
            if (!ft.held[(size_t)i]) sum += Y[i + I * c];
          ft.ymean[(size_t)c] = sum / (double)ft.ntrain;
        }
        for (int64_t i = 0; i < I; i++)
          if (!ft.held[(size_t)i]) ft.Yc[(size_t)(i + I * c)] = Y[i + I * c] - ft.ymean[(size_t)c];
      }
      ft.Yres = ft.Yc;
      ft.Tall.assign((size_t)I * F, 0.0);
      ft.Ttr.assign((size_t)I * F, 0.0);
      ft.Uy.assign((size_t)I * F, 0.0);
      ft.Q.assign((size_t)M * F, 0.0);
      ft.B.assign((size_t)F * F, 0.0);
      ft.wall.assign((size_t)d.sum * F, 0.0);
      ft.q.assign((size_t)M, 0.0);
      ft.pred.assign((size_t)I * M, 0.0);
      for (int c = 0; c < M; c++)
        for (int64_t i = 0; i < I; i++) ft.pred[(size_t)(i + I * c)] = ft.ymean[(size_t)c];
    }
    for (int f = 0; f < F; f++) {
      bool any = false;
      for (const NplsCvFit &ft : fits) any = any || ft.live;
      if (any) {
        // 1. the Z_m of every live fit in one pass: the columns of an ended fit are zero
        for (int j = 0; j < ng; j++) {
          const NplsCvFit &ft = fits[(size_t)j];
          if (ft.live)
            std::copy(ft.Yres.begin(), ft.Yres.end(), Yh.begin() + (size_t)I * M * j);
          else
            std::fill(Yh.begin() + (size_t)I * M * j, Yh.begin() + (size_t)I * M * (j + 1), 0.0);
        }
        ops.h2d(dY.as<double>(), Yh.data(), sizeof(double) * (size_t)I * M * ng);
        ops.npls_contract_wide(X.data, X.dtype, s.L, I, s.T, dY.as<double>(), ng * M, dZm.as<double>());
        passes += (ng * M + kNplsCvColumns - 1) / kNplsCvColumns;
        // 2. per fit: the corrections for the components so far, q and the rank-one weights
        for (int j = 0; j < ng; j++) {
          NplsCvFit &ft = fits[(size_t)j];
          double *Wj = dW.as<double>() + LT * j;
          if (ft.live) {
            double *Zmj = dZm.as<double>() + LT * M * j, *wallj = dwall.as<double>() + d.sum * F * j;
            for (int g = 0; g < f; g++)
              for (int c = 0; c < M; c++) {
                const double coef = dotn(&ft.Ttr[(size_t)I * g], &ft.Yres[(size_t)I * c], I);
                const double *w[MAX_ORDER];
                for (int k = 0; k < d.K; k++) w[k] = wallj + g * d.sum + d.off[k];
                if (coef != 0) ops.npls_outer_axpy(Zmj + LT * c, d.ext, d.K, w, -coef);
              }
            int st = 0;
            ft.live = npls_cv_weights(ops, d, M, I, o, ft.Yres, Zmj, dZ.as<double>(), Wj, dq.as<double>(), dS.as<double>(),
                                      dE.as<double>(), &ft.wall[(size_t)d.sum * f], wallj + d.sum * f, ft.q, &st);
            if (ft.live && status) status[ft.seg + (size_t)S * f] = st;
          }
          if (!ft.live) ops.zero(Wj, sizeof(double) * (size_t)LT);
        }
        // 3. the raw scores of all I samples for every fit in one pass
        ops.npls_slice_inner_wide(X.data, X.dtype, s.L, I, s.T, dW.as<double>(), ng, dS.as<double>());
        passes += (ng + kNplsCvColumns - 1) / kNplsCvColumns;
        ops.d2h(Sh.data(), dS.as<double>(), sizeof(double) * (size_t)I * ng);
      }
      // 4. on the host: centred scores, the inner relation over the training samples, the held-out predictions
      for (int j = 0; j < ng; j++) {
        NplsCvFit &ft = fits[(size_t)j];
        if (ft.live) {
          const double *raw = &Sh[(size_t)I * j];
          double mean = 0;
          if (center) {
            for (int64_t i = 0; i < I; i++)
              if (!ft.held[(size_t)i]) mean += raw[i];
            mean /= (double)ft.ntrain;
          }
          double *t = &ft.Tall[(size_t)I * f];
          for (int64_t i = 0; i < I; i++) t[i] = raw[i] - mean;
          for (int g = 0; g < f; g++) {
            const double ww = npls_ww(d, ft.wall.data(), g, f);
            for (int64_t i = 0; i < I; i++) t[i] -= ft.Tall[(size_t)(i + I * g)] * ww;
          }
          for (int64_t i = 0; i < I; i++) ft.Ttr[(size_t)(i + I * f)] = ft.held[(size_t)i] ? 0.0 : t[i];
          for (int c = 0; c < M; c++) ft.Q[(size_t)(c + M * f)] = ft.q[(size_t)c];
          for (int64_t i = 0; i < I; i++) {
            double u = 0;
            for (int c = 0; c < M; c++) u += ft.Yres[(size_t)(i + I * c)] * ft.q[(size_t)c];
            ft.Uy[(size_t)(i + I * f)] = u;
          }
          const int n = f + 1;
          std::vector<double> Gm((size_t)n * n), b((size_t)n);
          for (int g = 0; g < n; g++) {
            for (int h = 0; h < n; h++) Gm[g + (size_t)n * h] = dotn(&ft.Ttr[(size_t)I * g], &ft.Ttr[(size_t)I * h], I);
            b[(size_t)g] = dotn(&ft.Ttr[(size_t)I * g], &ft.Uy[(size_t)I * f], I);
          }
          solve_small(Gm, b, n);
          for (int g = 0; g < n; g++) ft.B[g + (size_t)F * f] = b[(size_t)g];
          ft.Yres = ft.Yc;
          for (int h = 0; h < n; h++)
            for (int g = 0; g <= h; g++) {
              const double bgh = ft.B[g + (size_t)F * h];
              if (bgh == 0) continue;
              for (int c = 0; c < M; c++) {
                const double bq = bgh * ft.Q[(size_t)(c + M * h)];
                for (int64_t i = 0; i < I; i++) ft.Yres[(size_t)(i + I * c)] -= ft.Ttr[(size_t)(i + I * g)] * bq;
              }
            }
          for (int g = 0; g < n; g++) {
            const double bgf = ft.B[g + (size_t)F * f];
            if (bgf == 0) continue;
            for (int c = 0; c < M; c++) {
              const double bq = bgf * ft.Q[(size_t)(c + M * f)];
              for (int64_t i = 0; i < I; i++)
                if (ft.held[(size_t)i]) ft.pred[(size_t)(i + I * c)] += ft.Tall[(size_t)(i + I * g)] * bq;
            }
          }
          ft.nf = f + 1;
        }
        // (an ended fit repeats its last prediction)
        for (int c = 0; c < M; c++)
          for (int64_t i = 0; i < I; i++)
            if (ft.held[(size_t)i]) Ycv[i + I * (c + (int64_t)M * f)] = ft.pred[(size_t)(i + I * c)];
      }
    }
    if (fitted)
      for (const NplsCvFit &ft : fits) fitted[ft.seg] = ft.nf;
  }
  if (press)
    for (int f = 0; f < F; f++)
      for (int c = 0; c < M; c++) {
        double p = 0;
        for (int64_t i = 0; i < I; i++) {
          const double e = Ycv[i + I * (c + (int64_t)M * f)] - Y[i + I * c];
          p += e * e;
        }
        press[f + (size_t)F * c] = p;
      }
  if (x_passes) *x_passes = passes;
}

// ============================================================================ CpEngine
// total columns of a session: nstarts * R, or the sum of the starts' own ranks
static int total_columns(int R, int nstarts, const int *ranks) {
  if (!ranks) return R * nstarts;
  int t = 0;
  for (int b = 0; b < nstarts; b++) t += ranks[b];
  return t;
}

CpEngine::CpEngine(Ops &ops, Comm &comm, const TensorDesc &V, int R, int nstarts, bool multi, const int *ranks)
    : ops_(ops), comm_(comm), V_(V), N_(V.order), R_(total_columns(R, nstarts, ranks)), P_(comm.size()),
      rank_(comm.rank()), K_(nstarts), Rs_(R), multi_(multi || nstarts > 1 || ranks) {
  dist_ = P_ > 1 || (force_comm_path() && !comm.is_self());
  if (nstarts <= 0) throw std::runtime_error("ppals: the number of starts must be positive");
  if (multi_) {  // the per-start table; equal ranks keep Rs_ and the batched ops (engine.h)
    if (nstarts > kMaxStarts) throw std::runtime_error("ppals: too many starts");
    tab_.nstarts = nstarts;
    Rs_ = 0;
    for (int b = 0; b < nstarts; b++) {
      const int rb = ranks ? ranks[b] : R;
      if (rb <= 0) throw std::runtime_error("ppals: rank must be positive");
      tab_.col[b + 1] = tab_.col[b] + rb;
      tab_.sq[b + 1] = tab_.sq[b] + rb * rb;
      if (rb != tab_.rank(0)) ragged_ = true;
      Rs_ = std::max(Rs_, rb);
    }
  }
  if (Rs_ <= 0) throw std::runtime_error("ppals: rank must be positive");
  if (multi_ && dist_) throw Unsupported("ppals: a multi-start session runs on one rank");
  residual_form_ = residual_form_env();
  slice_work_cap_ = slice_work_cap_env();
  W_.resize(N_);
  gradW_.resize(N_);
  Wprev_.resize(N_);
  Winit_.resize(N_);
  dW_.resize(N_);
  dM_.resize(N_);
  Mm_.resize(N_);
  for (int i = 0; i < N_; i++) {
    size_t n = (size_t)V_.glens[i] * R_ * sizeof(double);
    W_.alloc(ops_, i, n);
    gradW_.alloc(ops_, i, n);
    ops_.zero(W_[i], n);
    ops_.zero(gradW_[i], n);
    maxs_ = std::max(maxs_, V_.glens[i]);
    maxblk_ = std::max(maxblk_, block_rows(V_.glens[i], P_));
  }
  // (a multi-start session keeps the diagonal blocks only: sum_b R_b^2 entries per mode and system)
  const size_t sys_n = multi_ ? (size_t)tab_.sq[K_] : (size_t)R_ * R_;
  G_ = DeviceBuffer(ops_, sizeof(double) * N_ * sys_n);
  S_ = DeviceBuffer(ops_, sizeof(double) * sys_n);
  Sinv_ = DeviceBuffer(ops_, sizeof(double) * sys_n);
  gradsq_ = DeviceBuffer(ops_, sizeof(double) * MAX_ORDER * K_);
  scal_ = DeviceBuffer(ops_, sizeof(double) * 4 * MAX_ORDER);
  ops_.zero(gradsq_.as<double>(), sizeof(double) * MAX_ORDER * K_);
  if (dist_) {
    size_t n = sizeof(double) * (size_t)maxblk_ * P_ * R_;
    sendbuf_ = DeviceBuffer(ops_, n);
    recvbuf_ = DeviceBuffer(ops_, sizeof(double) * (size_t)maxblk_ * R_);
    gatherbuf_ = DeviceBuffer(ops_, n);
    ops_.zero(sendbuf_.as<double>(), n);
    ops_.zero(gatherbuf_.as<double>(), n);
  }
  if (const char *e = std::getenv("PPALS_COMM_SMALL_BYTES")) small_msg_bytes_ = std::atoll(e);
  if (const char *e = std::getenv("PPALS_TEST_BLOCKED_UPDATE")) test_blocks_ = std::atoi(e);
  if (N_ < 3) schedule_ = 0;
  if (const char *e = std::getenv("PPALS_PLACE_TUNE")) ms_tune_enabled_ = std::atoi(e) != 0;
  if (const char *e = std::getenv("PPALS_PACK_LAYOUT")) pack_mode_ = std::atoi(e) >= 0 && std::atoi(e) <= 2 ? std::atoi(e) : -1;
  if (N_ >= 3) {  // multi-sweep structures exist for every session so the schedule can be switched
    ms_set_roots(ms_choose_roots());
    ms_scales_ = DeviceBuffer(ops_, sizeof(double) * 32);
  }
  // The second resident layout is part of the session's set-up, like the tensor itself: built
  // here rather than at the first sweep, whose [dtime] would otherwise carry a one-off multi-GB
  // hipMalloc (≈ 1 s per 44 GB, several seconds on a fresh box) plus the transpose.
  if (V_.generation) tensor_gen_ = *V_.generation;
  {
    Layout nat;
    nat.ptr = V_.data;
    for (int m = 0; m < N_; m++) nat.order.push_back(m);
    lay_.push_back(std::move(nat));
  }
  // The block of the first-level intermediate is sized ONCE, for the largest root set plus the
  // slack the online placement choice moves inside (ms_start_step): growing it later would move
  // every root's result and void what the first visits measured (unequal mode extents,
  // [s/P, s, s, s] shards). A second candidate block is taken BEFORE the second resident layout, the
  // primary one after it: the layout's bytes lie between them. Nothing is launched or measured here.
  size_t xmax = 0;
  const bool place = schedule_ == 1 && N_ >= 3 && ms_tune_enabled_ && ms_X_slack() > 0;
  if (place) {
    for (int r = 0; r < N_; r++) {
      if (ms_set_excluded(r, ms_k_, ms_excl_)) continue;  // never a root set
      xmax = std::max(xmax, ms_X_bytes(r, ms_k_));
    }
    const size_t avail = ops_.mem_available();
    const double tensor_bytes = (double)V_.nloc * dtype_size(V_.dtype);
    if (avail == (size_t)-1 || (double)avail > 2.0 * tensor_bytes + 6.0 * (double)(xmax + ms_X_slack()) + 8e9)
      ms_X_alt_ = DeviceBuffer::try_alloc(ops_, xmax + ms_X_slack());
  }
  ensure_transposed();
  // the packed twins of the multi-sweep roots: set-up as well (several GB each at the headline)
  if (schedule_ == 1 && N_ >= 3)
    for (int r = 0; r < N_; r++) {
      ScanPlan pl;
      PackedSrc pk;
      if (!ms_set_excluded(r, ms_k_, ms_excl_) && plan_scan(r, ms_k_, false, pl) && pl.Lc > 1) packed_for(pl, pk);
    }
  if (place) ms_X_base_ = big_alloc(xmax + ms_X_slack());
  for (int i = 0; i < MAX_ORDER; i++) grad_replicated_[i] = !dist_;
  build_tree(0, N_ - 1, -1);
  leaf_.assign(N_, -1);
  for (size_t k = 0; k < nodes_.size(); k++)
    if (nodes_[k].lo == nodes_[k].hi) leaf_[nodes_[k].lo] = (int)k;
}

// 0 = the reference's two-first-level-node tree (alsCP_DT), 1 = multi-sweep tree (default)
void CpEngine::set_schedule(int schedule) {
  if (schedule != 0 && schedule != 1) throw std::runtime_error("ppals: unknown sweep schedule");
  schedule_ = (N_ < 3) ? 0 : schedule;
  for (auto &n : nodes_) n.valid = false;
  ms_invalidate();
}

CpEngine::~CpEngine() {
  try {
    ops_.sync();
  } catch (...) {
  }
  // (the placement stopwatches still in flight are read before their blocks go away with the members)
  for (auto &ex : ms_place_)
    if (ex.timer >= 0) ops_.timer_read(ex.timer);
}

// Second resident layout of the tensor for the RIGHT first-level node: V viewed as the matrix
// [left modes (fastest) x right modes] is transposed once, so that the "cd" contraction streams
// rows of (c,d) contiguously — the same suffix-scan access pattern as the "ab" node (K1) instead
// of the column-strided prefix scan (K2). Costs one extra copy of V in HBM (288 GB are there for
// it; cfg2: +6.4 GB, cfg4: +102 GB) and one transpose per session; the bytes read per sweep do
// not change. Built once, when the session is created. PPALS_TRANSPOSED_COPY=0 or an allocation
// failure falls back to the prefix scan (and to single-mode root sets).
//
// Padded layouts (engine.h, Layout): the leading block of q modes is padded when that makes more
// root positions 128-B aligned than the plain order has (q < first aligned position) at a cost of
// at most PPALS_PAD_WASTE (default 3 %) extra bytes — s = 50: 2500 -> 2528 elements, +1.1 %.
// PPALS_PAD_LAYOUT=0 never pads, =1 pads whatever the tensor's size (tests); by default tensors
// below 100 MB are left alone. The padded copy in the tensor's own order is a THIRD copy of the
// tensor: built only if the allocation succeeds.
static int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

void CpEngine::fill_layout(const Layout &l) {
  // the layout is the tensor rotated by h modes: transposition of [first h modes | the rest]
  int h = l.order[0];
  const int64_t rows = h == 0 ? 1 : prod_ext(0, h - 1);
  const int64_t cols = h == 0 ? V_.nloc : prod_ext(h, N_ - 1);
  if (l.q == 0)
    ops_.transpose2d(V_.data, V_.dtype, rows, cols, l.ptr);
  else
    ops_.pad_layout(V_.data, V_.dtype, rows, cols, l.blk, l.ld, l.ptr);
}

bool CpEngine::optional_fits(size_t bytes) {
  const size_t esz = dtype_size(V_.dtype);
  int64_t min_ext = ext(0);
  for (int m = 1; m < N_; m++) min_ext = std::min(min_ext, ext(m));
  const size_t xbytes_max = (size_t)(V_.nloc / std::max<int64_t>(1, min_ext)) * R_ * esz;
  const size_t reserve = 3 * xbytes_max + ms_X_slack() + ((size_t)1 << 30);
  const size_t avail = ops_.mem_available();
  return avail == (size_t)-1 || avail >= bytes + reserve;
}

void CpEngine::ensure_transposed() {
  if (vt_state_ != 0) return;
  vt_state_ = -1;
  const char *env = std::getenv("PPALS_TRANSPOSED_COPY");
  if (env && std::atoi(env) == 0) return;
  if (N_ < 3) return;
  const size_t esz = dtype_size(V_.dtype);
  const int64_t line = 128 / (int64_t)esz;  // elements per 128 B
  int pad_mode = -1;                         // auto
  if (const char *e = std::getenv("PPALS_PAD_LAYOUT")) pad_mode = std::atoi(e);
  const double max_waste = pad_mode == 1 ? 100.0 : 0.03;  // (forced: whatever the padding costs — tests)
  const bool may_pad = pad_mode == 1 || (pad_mode != 0 && (double)V_.nloc * esz >= 1e8);
  // leading block of a storage order worth padding: the smallest q whose padding is cheap, if the
  // plain order has no aligned position that early
  auto choose_pad = [&](Layout &l, int qmax) {
    l.q = 0;
    if (!may_pad) return;
    int q_nat = N_;
    int64_t b = 1;
    for (int p = 1; p < N_; p++) {
      b *= ext(l.order[p - 1]);
      if (b % line == 0) {
        q_nat = p;
        break;
      }
    }
    b = 1;
    for (int q = 1; q < q_nat && q <= qmax; q++) {
      b *= ext(l.order[q - 1]);
      const int64_t ld = round_up(b, line);
      if ((double)(ld - b) <= max_waste * (double)b) {
        l.q = q;
        l.blk = b;
        l.ld = ld;
        return;
      }
    }
  };
  auto bytes_of = [&](const Layout &l) {
    return l.q ? (size_t)l.ld * (size_t)(V_.nloc / l.blk) * esz : (size_t)V_.nloc * esz;
  };
  const int mid = (N_ - 1) / 2;
  Layout t;
  for (int m = mid + 1; m < N_; m++) t.order.push_back(m);
  for (int m = 0; m <= mid; m++) t.order.push_back(m);
  choose_pad(t, std::min(N_ - 2, N_ - 1 - mid));  // the block must lie inside the right half
  // An optional copy is taken only if what the session must still allocate fits behind it: the
  // first-level intermediate (+ placement slack), the level-1 scratch of the PP build of the same
  // size, tree nodes / pair operators (a few per cent of that) and a margin. (A Tucker session on
  // the same tensor, or a second CP session, may still find the device full: big_alloc then gives
  // the optional copies back.)
  auto fits = [&](size_t bytes) { return optional_fits(bytes); };
  if (!fits(bytes_of(t))) return;
  t.own = DeviceBuffer::try_alloc(ops_, bytes_of(t));
  if (!t.own) return;
  t.ptr = t.own.get();
  fill_layout(t);
  lay_.push_back(std::move(t));
  vt_state_ = 1;
  Layout a;
  for (int m = 0; m < N_; m++) a.order.push_back(m);
  choose_pad(a, N_ - 2);
  if (a.q > 0 && fits(bytes_of(a))) {
    a.own = DeviceBuffer::try_alloc(ops_, bytes_of(a));
    if (a.own) {
      a.ptr = a.own.get();
      fill_layout(a);
      lay_.push_back(std::move(a));
    }
  }
}

// The scan that contracts modes first .. first+k-1 (cyclic) on the best resident layout: the set
// must be stored adjacently (no wrap-around) and, on a padded layout, behind the padded block.
// Among those, 128-B aligned columns of at least a tile of rows win, then the most rows in front
// of the set (long contiguous runs per reduction index; a leading set would be a column-strided
// prefix scan). false: no layout stores the set adjacently.
bool CpEngine::plan_scan(int first, int k, bool natural_only, ScanPlan &plan) {
  auto in_set = [&](int m) { return ((m - first + N_) % N_) < k; };
  const int64_t line = 128 / (int64_t)dtype_size(V_.dtype);
  const Layout *best = nullptr;
  int best_p0 = 0;
  int64_t best_L = 0;
  bool best_al = false;
  const size_t nlay = natural_only ? 1 : lay_.size();
  for (size_t li = 0; li < nlay; li++) {
    const Layout &l = lay_[li];
    int p0 = -1;
    for (int p = 0; p < N_; p++)
      if (in_set(l.order[p])) {
        p0 = p;
        break;
      }
    int len = 0;
    while (p0 + len < N_ && in_set(l.order[p0 + len])) len++;
    if (len != k || (l.q > 0 && p0 < l.q)) continue;
    int64_t L = 1;
    for (int p = 0; p < p0; p++) L *= ext(l.order[p]);
    const bool al = L >= 256 && (l.q > 0 || L % line == 0);
    if (!best || (al && !best_al) ||
        (al == best_al && (L > best_L || (L == best_L && l.q > 0 && best->q == 0)))) {
      best = &l;
      best_p0 = p0;
      best_L = L;
      best_al = al;
    }
  }
  if (!best) return false;
  plan = ScanPlan();
  plan.lay = best;
  for (int p = 0; p < N_; p++) {
    const int m = best->order[p];
    if (p < best_p0) {
      plan.Lc *= ext(m);
      plan.kept.push_back(m);
    } else if (p < best_p0 + k) {
      plan.J *= ext(m);
      plan.set.push_back(m);
    } else {
      plan.T *= ext(m);
      plan.kept.push_back(m);
    }
  }
  plan.L = plan.Lc;
  if (best->q > 0) {
    plan.L = plan.Lc / best->blk * best->ld;
    plan.pad.ld = best->ld;
    plan.pad.valid = best->blk;
  }
  return true;
}

// Packed twins (ops.h PackedSrc, kernels_pack.hip.h): a lossless copy of 3.25 or 3.5 bytes per element
// (26 bits while at most 1/16 of the blocks need an escape plane, else 28) of an
// unpadded fp32 layout in the block order of ONE scan shape, which the one-n-tile scan then reads
// instead of the layout — the scan is HBM-bound, the tensor does not change between sweeps, and the
// copy is made once like the second resident layout. Optional like the padded third copy: taken
// only if it fits behind what the session must still allocate, given back by big_alloc first.
// Every root of the single-mode multi-sweep schedule has its own scan shape, hence its own twin
// (order 4, s = 200: four of 5.6 GB beside two layouts of 6.4 GB). All or nothing per twin: one
// block whose top bytes span 16 values or more (mixed signs, zeros beside large values) and the
// scan reads the plain layout, as does every launch the packed kernel does not serve (ops.h).
// PPALS_PACK_LAYOUT=0 never packs, =1 / =2 pack in the 28-bit / 26-bit format whatever the size
// (tests), default: tensors of at least 100 MB, the format by the rule above. Sharded, multi-start and rank-sweep sessions do not pack; a session whose tensor
// keeps being rewritten (masked EM) stops packing at the third rewrite.
namespace {
// names the packed twin for the scans inside a scope and takes it back on every way out
struct PackedScope {
  Ops &ops;
  PackedScope(Ops &o, const PackedSrc *pk) : ops(o) { ops.scan_packed_source(pk); }
  ~PackedScope() { ops.scan_packed_source(nullptr); }
};
}  // namespace

void CpEngine::packs_release() { packs_.clear(); }

// Survey the twin's source, choose its format (pack_choose_format), make room and pack. Called for a
// new twin and again when the tensor was rewritten: the buffers are kept where the format is the
// same and the escape planes still fit. On any refusal the twin holds no memory and says why.
bool CpEngine::pack_fill(PackedTwin &t) {
  auto drop = [&](const std::string &why) {
    t.data.reset();
    t.bases.reset();
    t.esc.reset();
    t.bytes = t.esc_room = 0;
    t.format = 0;
    t.escapes = 0;
    t.reason = why;
    return false;
  };
  const bool forced = pack_mode_ == 1 || pack_mode_ == 2;
  const size_t bb = pack_base_bytes(t.L, t.J, t.T);
  if (!t.bases && !(t.bases = DeviceBuffer::try_alloc(ops_, bb))) return drop("allocation failed");
  const PackSurvey sv = ops_.pack_survey(t.src, V_.dtype, t.L, t.J, t.T, t.bases.get());
  if (sv.spread < 0) return drop("scan shape has no packed route");
  if (sv.spread >= PACK_WINDOW)
    return drop("top bytes of a block span " + std::to_string(sv.spread + 1) + " values (window 16)");
  const int fmt = pack_choose_format(pack_mode_, sv.spread, sv.escapes, pack_blocks_of(t.L, t.J, t.T));
  if (!fmt) return drop("more escape blocks than the side word can number");
  const size_t db = pack_data_bytes(fmt, t.L, t.J, t.T);
  const size_t eb = fmt == PACK_FMT26 ? (size_t)sv.escapes * PACK26_ESC_BYTES : 0;
  if (t.data && (fmt != t.format || eb > t.esc_room)) {
    t.data.reset();
    t.esc.reset();
    t.esc_room = 0;
  }
  if (!t.data) {
    if (!forced && db + bb + eb >= (size_t)t.L * (size_t)t.J * (size_t)t.T * 4)
      return drop("row tiles would pad away what packing saves");  // (a batch ends with a whole tile of 256 rows)
    if (!optional_fits(db + eb)) return drop("no room beside what the session still allocates");
    t.data = DeviceBuffer::try_alloc(ops_, db);
    if (t.data && eb) t.esc = DeviceBuffer::try_alloc(ops_, eb);
    if (!t.data || (eb && !t.esc)) return drop("allocation failed");
    t.esc_room = eb;
  }
  t.format = fmt;
  t.escapes = sv.escapes;  // (as surveyed, whichever format was chosen)
  t.bytes = db + bb + eb;
  t.reason.clear();
  ops_.pack_write(t.src, t.L, t.J, t.T, fmt, t.bases.get(), t.data.get(), t.esc.get());
  return true;
}

const PackedSrc *CpEngine::packed_for(const ScanPlan &pl, PackedSrc &out) {
  if (pack_off_reason_.empty()) {
    if (pack_mode_ == 0) pack_off_reason_ = "PPALS_PACK_LAYOUT=0";
    else if (V_.dtype != F32) pack_off_reason_ = "not eligible: storage is not fp32";
    else if (R_ > 16) pack_off_reason_ = "not eligible: more than 16 result columns";
    else if (dist_) pack_off_reason_ = "not eligible: sharded session";
    else if (multi_) pack_off_reason_ = "not eligible: multi-start session";
    else if (pack_mode_ < 0 && (double)V_.nloc * 4.0 < 1e8) pack_off_reason_ = "tensor below 100 MB";
  }
  if (!pack_off_reason_.empty()) return nullptr;
  const int li = (int)(pl.lay - lay_.data());
  PackedTwin *t = nullptr;
  for (auto &c : packs_)
    if (c.layout == li && c.L == pl.L && c.J == pl.J && c.T == pl.T) t = &c;
  if (!t) {
    PackedTwin n;
    n.layout = li;
    n.src = pl.lay->ptr;
    n.L = pl.L;
    n.J = pl.J;
    n.T = pl.T;
    if (pl.lay->q > 0)
      n.reason = "padded layout";
    else if (n.L < 4 || n.L % 4)
      n.reason = "scan shape has no packed route";  // (no whole lanes of 4 rows)
    else
      pack_fill(n);
    packs_.push_back(std::move(n));
    t = &packs_.back();
  }
  if (!t->data) return nullptr;
  out.data = t->data.get();
  out.bases = t->bases.get();
  out.esc = t->esc.get();
  out.format = t->format;
  out.escapes = t->escapes;
  out.L = t->L;
  out.J = t->J;
  out.T = t->T;
  return &out;
}

// The tensor handle stays writable while sessions exist (ppals_tensor_fill_*/upload). Everything
// a session derived from the old contents — the second resident layout, tree nodes, the
// multi-sweep intermediate, PP operators — is rebuilt / dropped when the generation moved.
// Called wherever a session is about to read the tensor.
void CpEngine::check_tensor_generation() {
  if (!V_.generation || *V_.generation == tensor_gen_) return;
  tensor_gen_ = *V_.generation;
  for (const auto &l : lay_)
    if (l.own) fill_layout(l);
  // packed twins: pre-pass and pack again; a twin that no longer qualifies is dropped, one that was
  // refused for its values gets another look at its next scan. The third rewrite ends packing.
  if (++pack_regen_ >= 3) {
    ops_.sync();
    packs_release();
    if (pack_off_reason_.empty()) pack_off_reason_ = "tensor rewritten repeatedly";
  } else {
    ops_.sync();
    for (size_t k = 0; k < packs_.size();) {
      if (packs_[k].data && pack_fill(packs_[k])) {
        k++;
      } else if (!packs_[k].data && packs_[k].reason.compare(0, 9, "top bytes") != 0) {
        k++;  // (refused for its shape or for memory: that has not changed)
      } else {
        packs_.erase(packs_.begin() + k);
      }
    }
  }
  for (auto &n : nodes_) n.valid = false;
  ms_invalidate();
  pp_clear();
}

FactorRef CpEngine::fref(int m, double *const *W) const {
  FactorRef f;
  f.ptr = W[m] + (m == 0 ? V_.row0 : 0);
  f.rows = ext(m);
  f.ld = V_.glens[m];
  return f;
}
int64_t CpEngine::prod_ext(int lo, int hi) const {
  int64_t p = 1;
  for (int m = lo; m <= hi; m++) p *= ext(m);
  return p;
}

// Construct_Dimension_Tree (common.cxx:225-270): split [lo,hi] at (lo+hi)/2; every non-root range
// becomes a node that knows its parent and its sibling range.
void CpEngine::build_tree(int lo, int hi, int parent) {
  if (hi <= lo) return;
  const int mid = (lo + hi) / 2;
  const int ranges[2][2] = {{lo, mid}, {mid + 1, hi}};
  int idx[2];
  for (int c = 0; c < 2; c++) {
    Node n;
    n.lo = ranges[c][0];
    n.hi = ranges[c][1];
    n.parent = parent;
    n.slo = ranges[1 - c][0];
    n.shi = ranges[1 - c][1];
    n.elems = 0;
    nodes_.push_back(std::move(n));
    idx[c] = (int)nodes_.size() - 1;
  }
  build_tree(lo, mid, idx[0]);
  build_tree(mid + 1, hi, idx[1]);
}
int CpEngine::find_node(int lo, int hi) const {
  for (size_t k = 0; k < nodes_.size(); k++)
    if (nodes_[k].lo == lo && nodes_[k].hi == hi) return (int)k;
  return -1;
}

// mttkrp_map_DT (common.cxx:20-133). A node whose parent is the root scans V once with the
// Khatri-Rao product of ALL sibling modes (K1: sibling is a suffix, K2: a prefix); deeper nodes
// contract the cached parent tensor, which already carries the rank index.
void CpEngine::compute_node(int idx) {
  check_tensor_generation();
  Node &n = nodes_[idx];
  if (n.valid) return;
  n.elems = prod_ext(n.lo, n.hi);
  if (!n.buf) n.buf = DeviceBuffer(ops_, sizeof(double) * (size_t)n.elems * R_);
  FactorRef f[MAX_ORDER];
  int nf = 0;
  for (int m = n.slo; m <= n.shi; m++) f[nf++] = fref(m, W_.data());
  const int64_t J = prod_ext(n.slo, n.shi);
  const bool sib_is_suffix = n.slo > n.hi;
  if (n.parent < 0) {
    // a half of the modes is contracted: a suffix scan of the tensor (right half) or of the second
    // resident layout (left half); without that layout the left half is a prefix scan
    ScanPlan pl;
    if (!plan_scan(n.slo, n.shi - n.slo + 1, false, pl))
      throw std::runtime_error("ppals: internal error (tree node not adjacent)");
    if (pl.Lc == 1 && !sib_is_suffix) {
      ops_.scan_contract(V_.data, V_.dtype, 1, J, n.elems, f, nf, R_, n.buf.as<double>(), F64, 1, n.elems);
    } else {
      if (pl.T != 1 || pl.Lc != n.elems || pl.J != J)
        throw std::runtime_error("ppals: internal error (tree node scan shape)");
      PackedSrc pk_store;
      PackedScope scope(ops_, packed_for(pl, pk_store));
      ops_.scan_contract(pl.lay->ptr, V_.dtype, pl.L, J, 1, f, nf, R_, n.buf.as<double>(), F64, n.elems, n.elems,
                         pl.pad);
    }
  } else {
    compute_node(n.parent);
    const Node &p = nodes_[n.parent];
    if (sib_is_suffix)
      ops_.mttv(p.buf.as<double>(), F64, n.elems, J, 1, f, nf, R_, n.buf.as<double>(), n.elems, 0, nullptr);
    else
      ops_.mttv(p.buf.as<double>(), F64, 1, J, n.elems, f, nf, R_, n.buf.as<double>(), n.elems, 0, nullptr);
  }
  n.valid = true;
}

void CpEngine::refresh_grams() {
  if (multi_ && ragged_) {  // Gram (start b, mode i) at G_.as<double>() + N sq_b + i R_b^2
    for (int i = 0; i < N_; i++) ops_.gram_ragged(W_[i], V_.glens[i], V_.glens[i], tab_, N_, i, G_.as<double>());
    return;
  }
  if (multi_) {  // the diagonal blocks only: Gram (start b, mode i) at G_.as<double>() + (b N + i) Rs^2
    for (int i = 0; i < N_; i++)
      ops_.gram_batched(W_[i], V_.glens[i], V_.glens[i], Rs_, K_, G_.as<double>() + (size_t)i * Rs_ * Rs_,
                        (int64_t)N_ * Rs_ * Rs_);
    return;
  }
  for (int i = 0; i < N_; i++)
    ops_.gram(W_[i], V_.glens[i], V_.glens[i], R_, G_.as<double>() + (size_t)i * R_ * R_);
}

void CpEngine::set_factors(const double *Wflat, const double *gradWflat) {
  if (multi_) throw std::logic_error("ppals: a multi-start session takes its factors start by start");
  const double *w = Wflat, *g = gradWflat;
  double gs = 0, gsi[MAX_ORDER] = {0};
  for (int i = 0; i < N_; i++) {
    size_t n = (size_t)V_.glens[i] * R_;
    ops_.h2d(W_[i], w, n * sizeof(double));
    w += n;
    if (g) {
      if (kind_[i] != kModeFixed) {  // (a FIXED mode's gradient is zero and stays zero)
        ops_.h2d(gradW_[i], g, n * sizeof(double));
        for (size_t e = 0; e < n; e++) gsi[i] += g[e] * g[e];
        gs += gsi[i];
      }
      g += n;
    }
  }
  // per-mode ||grad_W[i]||^2 of the caller's gradients: a partial sweep (class API steps) mixes
  // them with the modes updated so far, exactly like CPD::update_gradnorm (src/CP.cxx:89-96)
  ops_.h2d(gradsq_.as<double>(), gsi, sizeof(double) * MAX_ORDER);
  for (int i = 0; i < MAX_ORDER; i++) grad_replicated_[i] = true;
  // iter-0 [gradnorm] is the norm of the caller's initial grad_W (test_ALS.cxx:338,
  // als_CP.cxx:174-181)
  init_gradnorm_ = std::sqrt(gs);
  grad_from_sweep_ = false;
  refresh_grams();
  for (auto &n : nodes_) n.valid = false;
  ms_invalidate();
}

// The session's mode updates become HALS passes (Ops::cp_mode_update_nn; every start of a multi-start
// session: Ops::cp_mode_update_nn_batched). Everything that cannot run that way is refused here, before
// anything is launched, and leaves the flag as it was.
void CpEngine::set_nonneg(bool on) {
  if (on) {
    if (P_ > 1 || dist_) throw Unsupported("ppals: a non-negative session runs on one rank");
    if (Rs_ > 64) throw Unsupported("ppals: a non-negative session supports R <= 64");  // (the largest start)
    if (test_blocks_ > 1)
      throw Unsupported("ppals: PPALS_TEST_BLOCKED_UPDATE has no non-negative update");
  }
  for (int i = 0; i < N_; i++) kind_[i] = on ? kModeNonneg : kModeFree;
  drop_stale_shapes();
}

int CpEngine::check_mode_kinds(const int *kinds, std::string *why) const {
  bool nonfree = false, capped = false;
  for (int i = 0; i < N_; i++) {
    if (kinds[i] < kModeFree || kinds[i] > kModeOrtho) {
      *why = "a kind must be PPALS_MODE_FREE, _NONNEG, _FIXED or _ORTHO";
      return 1;
    }
    nonfree = nonfree || kinds[i] != kModeFree;
    capped = capped || kinds[i] == kModeNonneg || kinds[i] == kModeOrtho;
    // (Rs_ is the largest start's rank: ORTHO needs s_mode >= R for every start)
    if (kinds[i] == kModeOrtho && V_.glens[i] < (multi_ ? Rs_ : R_)) {
      *why = "an orthonormal mode must have at least as many rows as the rank (of every start)";
      return 1;
    }
  }
  if (!nonfree) return 0;
  if (P_ > 1 || dist_) {
    *why = "per-mode constraints run on one rank";
    return 2;
  }
  if (test_blocks_ > 1) {
    *why = "PPALS_TEST_BLOCKED_UPDATE has no constrained update";
    return 2;
  }
  if (capped && (multi_ ? Rs_ : R_) > 64) {
    *why = "a non-negative or orthonormal mode supports R <= 64";
    return 2;
  }
  if (hold_mode_ >= 0 && (kinds[hold_mode_] == kModeFixed || kinds[hold_mode_] == kModeOrtho)) {
    *why = "the hold-out mode cannot be fixed or orthonormal";
    return 2;
  }
  return 0;
}

void CpEngine::set_mode_kinds(const int *kinds) {
  std::string why;
  const int rc = check_mode_kinds(kinds, &why);
  if (rc == 2) throw Unsupported("ppals: " + why);
  if (rc) throw std::invalid_argument("ppals: " + why);
  for (int i = 0; i < N_; i++) {
    if (kinds[i] == kModeFixed && kind_[i] != kModeFixed) {  // its gradient is zero from here on
      ops_.zero(gradW_[i], sizeof(double) * (size_t)V_.glens[i] * R_);
      ops_.zero(gradsq_.as<double>() + (size_t)i * K_, sizeof(double) * K_);
      grad_replicated_[i] = true;
    }
    kind_[i] = kinds[i];
  }
  drop_stale_shapes();
}

int CpEngine::check_mode_shapes(const int *shapes, std::string *why) const {
  for (int i = 0; i < N_; i++) {
    if (shapes[i] < kShapeNone || shapes[i] > kShapeDecreasing) {
      *why = "a shape must be PPALS_SHAPE_NONE, _UNIMODAL, _INCREASING or _DECREASING";
      return 1;
    }
    if (shapes[i] != kShapeNone && kind_[i] != kModeNonneg) {
      *why = "a shape needs a mode of kind PPALS_MODE_NONNEG";
      return 1;
    }
  }
  if (hold_mode_ >= 0 && shapes[hold_mode_] != kShapeNone) {
    *why = "the hold-out mode cannot have a shape";
    return 2;
  }
  return 0;
}

void CpEngine::set_mode_shapes(const int *shapes) {
  std::string why;
  const int rc = check_mode_shapes(shapes, &why);
  if (rc == 2) throw Unsupported("ppals: " + why);
  if (rc) throw std::invalid_argument("ppals: " + why);
  for (int i = 0; i < N_; i++) shape_[i] = shapes[i];
}

bool CpEngine::factors_nonneg(unsigned modes) {
  for (int i = 0; i < N_; i++) {  // (R_ columns: all starts of a multi-start session)
    if (!((modes >> i) & 1u)) continue;
    std::vector<double> h((size_t)V_.glens[i] * R_);
    ops_.d2h(h.data(), W_[i], sizeof(double) * h.size());
    for (double v : h)
      if (!(v >= 0) || !std::isfinite(v)) return false;
  }
  return true;
}

// ---------------------------------------------------------------------------- multi-start sessions
// One start's factors are the column block [col_b, col_b + R_b) of every W_[i]: s_i * R_b contiguous doubles.
void CpEngine::set_factors_start(int start, const double *Wflat, const double *gradWflat) {
  if (!multi_) throw std::logic_error("ppals: not a multi-start session");
  if (start < -1 || start >= K_) throw std::runtime_error("ppals: start out of range");
  const double *w = Wflat, *g = gradWflat;
  const int b0 = start < 0 ? 0 : start, b1 = start < 0 ? K_ : start + 1;
  for (int b = b0; b < b1; b++)
    for (int i = 0; i < N_; i++) {
      const size_t n = (size_t)V_.glens[i] * tab_.rank(b), at = (size_t)V_.glens[i] * tab_.col[b];
      ops_.h2d(W_[i] + at, w, n * sizeof(double));
      w += n;
      // ||grad_W[i]||^2 of the caller's gradients, as set_factors keeps it (0 without gradients)
      double gsq = 0;
      if (g) {
        if (kind_[i] != kModeFixed) {  // (a FIXED mode's gradient is zero and stays zero)
          ops_.h2d(gradW_[i] + at, g, n * sizeof(double));
          for (size_t e = 0; e < n; e++) gsq += g[e] * g[e];
        }
        g += n;
      }
      ops_.h2d(gradsq_.as<double>() + (size_t)i * K_ + b, &gsq, sizeof(double));
    }
  if (hold_mode_ >= 0) {  // the caller's held-out rows of these starts move into the scores
    unsigned sel = 0;
    for (int b = b0; b < b1; b++) sel |= 1u << b;
    hold_apply(sel);
    if (!g) {  // (no gradients: the sums stay 0, whatever the gradient buffer still holds)
      const double zero = 0;
      for (int b = b0; b < b1; b++)
        if ((hold_mask_ >> b) & 1u) ops_.h2d(gradsq_.as<double>() + (size_t)hold_mode_ * K_ + b, &zero, sizeof(double));
    }
  }
  refresh_grams();
  for (auto &n : nodes_) n.valid = false;
  ms_invalidate();
}

// ---------------------------------------------------------------------------- hold-out rows per start
void CpEngine::hold_apply(unsigned starts) {
  const unsigned sel = hold_mask_ & starts;
  if (hold_mode_ < 0 || !sel) return;
  const int64_t s = V_.glens[hold_mode_];
  ops_.cp_hold_rows(W_[hold_mode_], s, gradW_[hold_mode_], s, hold_scores_.as<double>(), s, s, tab_,
                    hold_keep_dev_.as<uint8_t>(), sel, G_.as<double>(), N_,
                    hold_mode_, gradsq_.as<double>() + (size_t)hold_mode_ * K_);
}

void CpEngine::set_holdout(int mode, const uint8_t *keep) {
  if (!multi_) throw std::logic_error("ppals: not a multi-start session");
  if (!keep) {  // the zero rows stay until the next update of the mode
    hold_mode_ = -1;
    hold_mask_ = 0;
    hold_keep_.clear();
    return;
  }
  if (mode < 0 || mode >= N_) throw std::runtime_error("ppals: hold-out mode out of range");
  const int64_t s = V_.glens[mode];
  unsigned mask = 0;
  for (int b = 0; b < K_; b++) {
    int64_t kept = 0;
    for (int64_t x = 0; x < s; x++) kept += keep[(size_t)b * s + x] != 0;
    if (kept == 0) throw std::runtime_error("ppals: a start must keep at least one row");
    if (kept < s) mask |= 1u << b;
  }
  if (!hold_keep_dev_ || hold_rows_ != s) {
    ops_.sync();
    hold_keep_dev_.reset();
    hold_scores_.reset();
    hold_keep_dev_ = DeviceBuffer(ops_, (size_t)K_ * s);
    hold_scores_ = DeviceBuffer(ops_, sizeof(double) * (size_t)s * R_);
    hold_rows_ = s;
  }
  hold_keep_.assign(keep, keep + (size_t)K_ * s);
  ops_.h2d(hold_keep_dev_.as<uint8_t>(), hold_keep_.data(), hold_keep_.size());
  ops_.zero(hold_scores_.as<double>(), sizeof(double) * (size_t)s * R_);
  hold_mode_ = mode;
  hold_mask_ = mask;
  hold_apply(~0u);
  for (auto &n : nodes_) n.valid = false;
  ms_invalidate();
}

void CpEngine::heldout_scores(int start, double *out) {
  if (!multi_ || hold_mode_ < 0) throw std::logic_error("ppals: the session has no hold-out");
  if (start < 0 || start >= K_) throw std::runtime_error("ppals: start out of range");
  const int64_t s = V_.glens[hold_mode_];
  ops_.d2h(out, hold_scores_.as<double>() + (size_t)s * tab_.col[start], sizeof(double) * (size_t)s * tab_.rank(start));
}

void CpEngine::get_factors_start(int start, double *Wflat, double *gradWflat) {
  if (!multi_) throw std::logic_error("ppals: not a multi-start session");
  if (start < -1 || start >= K_) throw std::runtime_error("ppals: start out of range");
  double *w = Wflat, *g = gradWflat;
  const int b0 = start < 0 ? 0 : start, b1 = start < 0 ? K_ : start + 1;
  for (int b = b0; b < b1; b++)
    for (int i = 0; i < N_; i++) {
      const size_t n = (size_t)V_.glens[i] * tab_.rank(b), at = (size_t)V_.glens[i] * tab_.col[b];
      if (w) {
        ops_.d2h(w, W_[i] + at, n * sizeof(double));
        w += n;
      }
      if (g) {
        ops_.d2h(g, gradW_[i] + at, n * sizeof(double));
        g += n;
      }
    }
}

void CpEngine::gradnorms(double *out) {
  if (!multi_) throw std::logic_error("ppals: not a multi-start session");
  std::vector<double> h((size_t)N_ * K_);
  ops_.d2h(h.data(), gradsq_.as<double>(), sizeof(double) * h.size());
  for (int b = 0; b < K_; b++) {
    double sum = 0;
    for (int i = 0; i < N_; i++) sum += h[(size_t)i * K_ + b];
    out[b] = std::sqrt(sum);
  }
}

// one streaming pass over the tensor per start (off the sweep path)
void CpEngine::residuals(double *out) {
  if (!multi_) throw std::logic_error("ppals: not a multi-start session");
  int64_t M, K;
  split_sizes(V_, &M, &K);
  if (!Qbuf_) Qbuf_ = DeviceBuffer(ops_, sizeof(double) * M * Rs_);  // (Rs_: the largest start)
  if (!Pbuf_) Pbuf_ = DeviceBuffer(ops_, sizeof(double) * K * Rs_);
  std::vector<double *> Wb(N_);
  for (int b = 0; b < K_; b++) {
    const int rb = tab_.rank(b);
    for (int i = 0; i < N_; i++) Wb[i] = W_[i] + (size_t)tab_.col[b] * V_.glens[i];
    split_krp(ops_, V_, rb, Wb.data(), Qbuf_.as<double>(), Pbuf_.as<double>(), &M, &K);
    ops_.residual_sq(V_.data, V_.dtype, M, K, Qbuf_.as<double>(), Pbuf_.as<double>(), rb, scal_.as<double>());
    double h = 0;
    ops_.d2h(&h, scal_.as<double>(), sizeof(double));
    out[b] = std::sqrt(h);
  }
}

int CpEngine::run_multi(const CpOpts &o, int *sweeps_out, int *best_out) {
  if (!multi_) throw std::logic_error("ppals: not a multi-start session");
  const double t0 = now();
  std::vector<double> gn(K_), res(K_);
  int sweeps = 0, best = 0;
  bool stopped = false;
  for (;;) {
    if (sweeps % o.resprint == 0 || sweeps >= o.maxiter) {
      gradnorms(gn.data());
      residuals(res.data());
      best = (int)(std::min_element(res.begin(), res.end()) - res.begin());
      if (o.verbose)
        std::printf("  [sweeps]=  %d  [best]  %d  [gradnorm]  %.13g  [residual]  %.13g  [dtime]  %g\n", sweeps,
                    best, gn[best], res[best], now() - t0);
      // starts of different ranks: the smallest residual is (almost always) the largest rank, whose
      // gradient says nothing about the others — the run goes on until every start is below tol
      // (a hold-out session likewise: every start is a fit of its own that the caller wants finished)
      const double gstop = ragged_ || hold_mode_ >= 0 ? *std::max_element(gn.begin(), gn.end()) : gn[best];
      stopped = gstop < o.tol || now() - t0 > o.timelimit;
      if (stopped || sweeps >= o.maxiter) break;
    }
    update_modes(0, N_, o.lambda);
    sweeps++;
  }
  ops_.sync();
  if (sweeps_out) *sweeps_out = sweeps;
  if (best_out) *best_out = best;
  return stopped && sweeps < o.maxiter ? 1 : 0;
}

void CpEngine::take_from(CpEngine &src, int start, bool predicted) {
  if (multi_ || dist_) throw std::logic_error("ppals: the destination must be an ordinary one-rank session");
  // (a non-negative multi-start session's factors are >= the floor by construction)
  if (!takes_nonneg_from(src))
    throw Unsupported("ppals: a non-negative session does not take an unconstrained multi-start's factors");
  if (!src.multi_ || start < 0 || start >= src.K_ || src.tab_.rank(start) != R_ || src.N_ != N_ ||
      src.V_.data != V_.data)
    throw std::runtime_error("ppals: take: sessions do not match");
  if (predicted && src.hold_mode_ < 0) throw std::runtime_error("ppals: take: the session has no hold-out");
  for (int i = 0; i < N_; i++) {
    const size_t n = (size_t)V_.glens[i] * R_;
    const size_t at = (size_t)V_.glens[i] * src.tab_.col[start];
    ops_.d2d(W_[i], src.W_[i] + at, n * sizeof(double));
    ops_.d2d(gradW_[i], src.gradW_[i] + at, n * sizeof(double));
    ops_.d2d(gradsq_.as<double>() + i, src.gradsq_.as<double>() + (size_t)i * src.K_ + start, sizeof(double));
    if (kind_[i] == kModeFixed) {  // (a FIXED mode's gradient is zero and stays zero)
      ops_.zero(gradW_[i], n * sizeof(double));
      ops_.zero(gradsq_.as<double>() + i, sizeof(double));
    }
  }
  if (predicted) {  // the scores into the (zero) held-out rows: W + scores, the kept rows of the scores are 0
    const int m = src.hold_mode_;
    ops_.add_inplace(W_[m], src.hold_scores_.as<double>() + (size_t)V_.glens[m] * src.tab_.col[start],
                     V_.glens[m] * R_);
  }
  // (gradnorm() reads the copied per-mode sums: the same number set_factors would have formed on the
  // host from these gradients, with no read-back here)
  for (int i = 0; i < MAX_ORDER; i++) grad_replicated_[i] = true;
  grad_from_sweep_ = true;
  refresh_grams();
  for (auto &n : nodes_) n.valid = false;
  ms_invalidate();
  pp_clear();
}

void CpEngine::get_factors(double *Wflat, double *gradWflat) {
  if (multi_) throw std::logic_error("ppals: a multi-start session hands out its factors start by start");
  double *w = Wflat, *g = gradWflat;
  for (int i = 0; i < N_; i++) {
    size_t n = (size_t)V_.glens[i] * R_;
    if (w) {
      ops_.d2h(w, W_[i], n * sizeof(double));
      w += n;
    }
    if (g) {
      if (dist_ && grad_from_sweep_ && !grad_replicated_[i]) {
        // every rank holds only its own row block of grad_W: gather it
        const int64_t blk = block_rows(V_.glens[i], P_);
        ops_.pack_blocks(gradW_[i], V_.glens[i], V_.glens[i], R_, blk, P_, gatherbuf_.as<double>());
        comm_.allgather(gatherbuf_.as<double>() + (size_t)rank_ * blk * R_, gatherbuf_.as<double>(), blk * R_);
        ops_.unpack_blocks(gatherbuf_.as<double>(), V_.glens[i], V_.glens[i], R_, blk, P_, gradW_[i]);
      }
      ops_.d2h(g, gradW_[i], n * sizeof(double));
      g += n;
    }
  }
}

// one mode update: K4 (S), K5 (gradient with the pre-update W), K6 (solve), Gram refresh;
// with P > 1 ranks: C1 reduce-scatter of the partial rows, C2 all-gather of the updated rows.
void CpEngine::mode_update(int i, const double *M, int64_t ldm, double lambda, bool pp,
                           double ratio) {
  const int64_t s = V_.glens[i];
  double *const G = G_.as<double>(), *const S = S_.as<double>(), *const Sinv = Sinv_.as<double>();
  double *const gradsq = gradsq_.as<double>(), *const sendbuf = sendbuf_.as<double>();
  double *const recvbuf = recvbuf_.as<double>(), *const gatherbuf = gatherbuf_.as<double>();
  const bool hals = kind_[i] == kModeNonneg;  // this mode's update is the HALS pass
  if (kind_[i] == kModeFixed) throw std::logic_error("ppals: a FIXED mode has no update");
  if (kind_[i] == kModeOrtho) {  // the polar factor of M, start by start through the table (one start here
    // when the session is an ordinary one); the hold-out mode is never ORTHO (set_mode_kinds, set_holdout)
    if (pp || dist_) throw std::logic_error("ppals: an orthonormal mode updates exactly, on one rank");
    ops_.cp_mode_update_ortho_ragged(G, N_, i, start_table(), lambda, M, ldm, W_[i], s, gradW_[i], s, s,
                                     gradsq + (size_t)i * K_, S);
    return;
  }
  if (hals && shape_[i] != kShapeNone) {  // column by column onto the shape's set, through the table as ORTHO
    // goes; the hold-out mode never has a shape (set_mode_shapes, set_holdout)
    if (pp || dist_) throw std::logic_error("ppals: a shaped mode updates exactly, on one rank");
    ops_.cp_mode_update_shape_ragged(G, N_, i, start_table(), lambda, M, ldm, W_[i], s, gradW_[i], s, s,
                                     gradsq + (size_t)i * K_, S, shape_[i]);
    return;
  }
  if (multi_) {  // block-diagonal over starts: one batched update, every start its own system
    if (pp) throw std::logic_error("ppals: no PP update in a multi-start session");
    if (ragged_) {  // starts of different ranks: the same updates, addressed through the table
      if (hals)
        ops_.cp_mode_update_nn_ragged(G, N_, i, tab_, lambda, M, ldm, W_[i], s, gradW_[i], s, s,
                                      gradsq + (size_t)i * K_, S);
      else
        ops_.cp_mode_update_ragged(G, N_, i, tab_, lambda, M, ldm, W_[i], s, gradW_[i], s, s,
                                   gradsq + (size_t)i * K_, S, Sinv);
    } else if (hals) {  // one HALS pass per start, all starts in one batched update
      ops_.cp_mode_update_nn_batched(G, N_, i, Rs_, K_, lambda, M, ldm, W_[i], s, gradW_[i], s, s,
                                     gradsq + (size_t)i * K_, S);
    } else {
      ops_.cp_mode_update_batched(G, N_, i, Rs_, K_, lambda, M, ldm, W_[i], s, gradW_[i], s, s,
                                  gradsq + (size_t)i * K_, S, Sinv);
    }
    // the sample mode of a hold-out session: the rows just computed for held-out samples are their
    // predicted scores — moved aside, and zero again before another mode reads the factor
    if (i == hold_mode_) hold_apply(~0u);
    return;
  }
  double *Gi = G + (size_t)i * R_ * R_;
  if (hals) {  // one HALS pass in place of the solve (set_nonneg admits one-rank sessions only)
    if (pp || dist_) throw std::logic_error("ppals: a non-negative session updates exactly, on one rank");
    ops_.cp_mode_update_nn(G, N_, i, R_, lambda, M, ldm, W_[i], s, gradW_[i], s, s, gradsq + i, S);
    return;
  }
  if (!dist_) {
    if (test_blocks_ > 1 && s % test_blocks_ == 0 && !pp) {
      // test hook (PPALS_TEST_BLOCKED_UPDATE=P, one rank): the update reads its M in P row blocks, as the
      // sharded mode's update reads the all-gather's receive buffer on P ranks — the blocked
      // addressing of the fused launch with more than one block, on one GPU
      const int64_t blk = s / test_blocks_;
      const size_t bytes = sizeof(double) * (size_t)s * R_;
      if (!test_blkbuf_) {
        test_blkbuf_ = DeviceBuffer(ops_, 2 * sizeof(double) * (size_t)maxs_ * R_);
      }
      ops_.pack_blocks(M, s, ldm, R_, blk, test_blocks_, test_blkbuf_.as<double>());
      ops_.cp_mode_update_blocked(G, N_, i, R_, lambda, test_blkbuf_.as<double>(), blk, test_blocks_,
                                  test_blkbuf_.as<double>() + bytes / sizeof(double), W_[i], s, gradW_[i], s, s,
                                  gradsq + i, nullptr, s, nullptr, s, ratio, S, Sinv);
      return;
    }
    ops_.cp_mode_update(G, N_, i, R_, lambda, M, ldm, W_[i], s, gradW_[i], s, s, gradsq + i,
                        pp ? Winit_[i] : nullptr, s, pp ? dW_[i] : nullptr, s, ratio, S, Sinv,
                        (pp && pp_norms_.as<double>()) ? pp_norms_.as<double>() + 2 * i : nullptr);
    return;
  } else if (i != 0 && (int64_t)sizeof(double) * s * R_ <= small_msg_bytes_) {
    // latency regime (s x R is a few KB): ONE all-reduce of the partial rows, then every rank runs
    // the whole (tiny) mode update redundantly — the reduce-scatter + all-gather pair below
    // collapsed into a single collective, and the same fused launch as on one GPU.
    if (ldm != s) throw std::runtime_error("ppals: partial MTTKRP must be contiguous");
    comm_.allreduce_sum(const_cast<double *>(M), s * R_);
    ops_.cp_mode_update(G, N_, i, R_, lambda, M, ldm, W_[i], s, gradW_[i], s, s, gradsq + i,
                        pp ? Winit_[i] : nullptr, s, pp ? dW_[i] : nullptr, s, ratio, S, Sinv);
    grad_replicated_[i] = true;
    return;
  } else if (i == 0 && (int64_t)sizeof(double) * s * R_ <= small_msg_bytes_) {
    // same regime, sharded mode: the local rows are complete, so the owners' row blocks are
    // all-gathered (the cheapest collective: blk x R doubles per rank) and every rank runs the
    // fused update on the assembled s x R matrix.
    const int64_t blk = block_rows(s, P_);
    const int64_t nr = std::max<int64_t>(0, std::min(blk, s - blk * rank_));
    double *mine = gatherbuf + (size_t)rank_ * blk * R_;
    if (blk * P_ == s && ldm == blk && nr == blk) {
      // equal blocks: the local leaf IS this rank's block as the all-gather wants it (no pack launch),
      // and the fused update reads the gathered blocks as they lie (no unpack launch)
      comm_.allgather(M, gatherbuf, blk * R_);
      ops_.cp_mode_update_blocked(G, N_, i, R_, lambda, gatherbuf, blk, P_, sendbuf, W_[i], s, gradW_[i],
                                  s, s, gradsq + i, pp ? Winit_[i] : nullptr, s, pp ? dW_[i] : nullptr, s,
                                  ratio, S, Sinv);
      grad_replicated_[i] = true;
      return;
    }
    ops_.pack_blocks(M, nr, ldm, R_, blk, 1, mine);
    comm_.allgather(mine, gatherbuf, blk * R_);
    ops_.unpack_blocks(gatherbuf, s, s, R_, blk, P_, sendbuf);
    ops_.cp_mode_update(G, N_, i, R_, lambda, sendbuf, s, W_[i], s, gradW_[i], s, s, gradsq + i,
                        pp ? Winit_[i] : nullptr, s, pp ? dW_[i] : nullptr, s, ratio, S, Sinv);
    grad_replicated_[i] = true;
    return;
  } else {
    grad_replicated_[i] = false;
    ops_.gram_system(G, N_, i, R_, lambda, S, Sinv);
    const int64_t blk = block_rows(s, P_);
    const int64_t r0 = blk * rank_;
    const int64_t nr = std::max<int64_t>(0, std::min(blk, s - r0));
    const double *Mblk;
    int64_t ldb;
    if (i == 0) {  // rows of mode 0 are complete on their owner
      Mblk = M;
      ldb = ldm;
    } else {
      ops_.pack_blocks(M, s, ldm, R_, blk, P_, sendbuf);
      comm_.reduce_scatter_sum(sendbuf, recvbuf, blk * R_);
      Mblk = recvbuf;
      ldb = blk;
    }
    double *mine = gatherbuf + (size_t)rank_ * blk * R_;
    // SVD_solve_mod tail (common.cxx:753-756): the row block is written as W_init + ratio *
    // (M S^-1 - W_init) already, so after the gather dW = W - W_init holds for every row
    ops_.cp_update(Mblk, ldb, W_[i] + r0, s, mine, blk, gradW_[i] + r0, s, nr, R_, S, Sinv,
                   gradsq + i, pp ? Winit_[i] + r0 : nullptr, s, pp ? dW_[i] + r0 : nullptr, s,
                   ratio);
    comm_.allgather(mine, gatherbuf, blk * R_);
    ops_.unpack_blocks(gatherbuf, s, s, R_, blk, P_, W_[i]);
    if (pp) {
      double *A[1] = {W_[i]}, *B[1] = {Winit_[i]}, *D[1] = {dW_[i]};
      int64_t n[1] = {s * R_};
      ops_.diff_norms(A, B, n, 1, 1, D, 0, scal_.as<double>() + 2 * MAX_ORDER);
    }
  }
  ops_.gram(W_[i], s, s, R_, Gi);
}

// cached MSDT tensors were built from the un-normalised factors of their contracted modes: a
// Normalize multiplies every live tensor's pending scalar by prod_{m contracted} f_m (same launch).
// Returns the set of live slots, marks them pending; skip_node: a leaf about to be consumed.
unsigned CpEngine::ms_collect_scales(unsigned *masks, unsigned *fresh, int skip_node) {
  unsigned active = 0;
  *fresh = 0;
  if (!(schedule_ == 1 && ms_root_ >= 0)) return 0;
  auto visit = [&](RTensor &t) {
    if (!t.valid) return;
    masks[t.slot] = t.contracted;
    active |= 1u << t.slot;
    if (!t.pending) *fresh |= 1u << t.slot;
    t.pending = true;
  };
  visit(ms_X_);
  for (size_t q = 0; q < ms_nodes_.size(); q++)
    if ((int)q != skip_node) visit(ms_nodes_[q].t);
  return active;
}

void CpEngine::normalize() {
  // (one scalar per mode over the whole factor matrix: it would couple the starts)
  if (multi_) throw std::logic_error("ppals: no Normalize in a multi-start session");
  int64_t rows[MAX_ORDER];
  for (int i = 0; i < N_; i++) rows[i] = V_.glens[i];
  unsigned masks[32] = {0}, fresh = 0;
  const unsigned active = ms_collect_scales(masks, &fresh, -1);
  ops_.normalize_ms(W_.data(), rows, N_, R_, G_.as<double>(), ms_scales_.as<double>(), masks, active, fresh,
                    pp_norms_live_ ? pp_norms_.as<double>() + 1 : nullptr);
}

// ---------------------------------------------------------------------------- multi-sweep tree
// Binary tree (same split rule as Construct_Dimension_Tree) over the POSITIONS 0..N-2 of the
// step's mode list; node [lo,hi] = X contracted with the listed modes outside [lo,hi].
void CpEngine::ms_build_tree(int lo, int hi, int parent) {
  if (hi < lo) return;
  if (hi == lo && parent < 0) {  // N == 2: single leaf directly under X
    MsNode n;
    n.lo = n.hi = lo;
    n.parent = -1;
    n.slo = 1;
    n.shi = 0;
    ms_nodes_.push_back(std::move(n));
    return;
  }
  if (hi <= lo) return;
  const int mid = (lo + hi) / 2;
  const int ranges[2][2] = {{lo, mid}, {mid + 1, hi}};
  int idx[2];
  for (int c = 0; c < 2; c++) {
    MsNode n;
    n.lo = ranges[c][0];
    n.hi = ranges[c][1];
    n.parent = parent;
    n.slo = ranges[1 - c][0];
    n.shi = ranges[1 - c][1];
    ms_nodes_.push_back(std::move(n));
    idx[c] = (int)ms_nodes_.size() - 1;
  }
  ms_build_tree(lo, mid, idx[0]);
  ms_build_tree(mid + 1, hi, idx[1]);
}

// ---- which root sets the multi-sweep schedule uses ----
bool CpEngine::ms_set_excluded(int first, int k, unsigned excl) const {
  for (int q = 0; q < k; q++)
    if ((excl >> ((first + q) % N_)) & 1u) return true;
  return false;
}

// The root set that serves the update of mode i when the running step cannot: the k modes updated
// last, slid back past excluded modes. A slid-back set is older but still current (none of its modes
// has been updated since); the step is then entered in the middle of its mode list and serves fewer
// updates (order 4, k = 1, mode 0 excluded: runs 3,3,2 -> 3 scans per 2 sweeps instead of 8/3).
int CpEngine::ms_next_root(int i, int k, unsigned excl) const {
  int first = (i - k + N_) % N_, guard = 0;
  while (ms_set_excluded(first, k, excl) && guard++ < N_) first = (first - 1 + N_) % N_;
  if (ms_set_excluded(first, k, excl) || ((i - first + N_) % N_) < k) return -1;
  return first;
}

// What a sweep costs under (k, excl), in reads of the tensor: the schedule is walked for a few sweeps
// (the transient of the root rotation dropped), every first-level scan costs 1 + 4.5 x (size of its
// X relative to the tensor): X is written once — a written byte costs ~2.5 read bytes on this part,
// profiles/README.md — and read twice by the step's tree.
double CpEngine::ms_schedule_cost(int k, unsigned excl) const {
  int root = -1;
  double cost = 0;
  const int sweeps = 2 * N_;
  for (int u = 0; u < (sweeps + 2) * N_; u++) {
    const int i = u % N_;
    if (root < 0 || ((i - root + N_) % N_) < k) {
      root = ms_next_root(i, k, excl);
      if (root < 0) return 1e300;
      if (u >= 2 * N_) {
        double J = 1;
        for (int q = 0; q < k; q++) J *= (double)ext((root + q) % N_);
        cost += 1.0 + 4.5 * (double)R_ / J;
      }
    }
  }
  return cost / sweeps;
}

// How many modes one first-level contraction removes (the "root set" of a step) and which modes are
// never roots. k = 1 with no exclusion wins at order 4 with equal extents (cfg2: 1.33 x 1.23 vs 2.0),
// k = 2 at order 6 with s = 50, R = 6 (1.2 x 1.54 vs 1.5 x 1.01); a mode of extent 3 at R = 10
// (coil-100: 3 x 128 x 128 x 7200) is excluded: 1.5 scans of the tensor per sweep instead of 1.33
// scans plus an X of 3.3 x the tensor written once and read twice every third step.
// PPALS_MSDT_ROOTS=k fixes k (the exclusion is still chosen by cost).
int CpEngine::ms_choose_roots() {
  const unsigned mandatory = (dist_ && N_ > 2) ? 1u : 0u;  // sharded: mode 0 is never in a root set
  // sharded: the root set is slid back past mode 0; it still has to end before the mode about to be
  // updated, which needs 2k < N
  const int kcap = dist_ ? std::max(1, (N_ - 1) / 2) : N_;
  int kfix = 0;
  if (const char *e = std::getenv("PPALS_MSDT_ROOTS")) {
    const int k = std::atoi(e);
    if (k >= 1 && k <= N_ - 2) kfix = std::min(k, kcap);
  }
  // candidates for exclusion: modes whose X would be at least 5 % of the tensor
  unsigned small = 0;
  for (int m = 0; m < N_; m++)
    if ((double)R_ >= 0.05 * (double)ext(m)) small |= 1u << m;
  int best = 1;
  unsigned best_excl = mandatory;
  double best_cost = 1e300;
  for (int k = 1; k <= std::max(1, N_ / 2) && k <= N_ - 2 && k <= kcap; k++) {
    if (kfix && k != kfix) continue;
    for (unsigned sub = small;; sub = (sub - 1) & small) {  // every subset of the short modes
      const unsigned excl = sub | mandatory;
      const double cost = ms_schedule_cost(k, excl);
      // (ties: fewer excluded modes, then smaller k — the subsets are walked from the fullest down, so a
      // tie has to be broken explicitly)
      const bool tie = cost <= best_cost * (1.0 + 1e-9) && cost >= best_cost * (1.0 - 1e-9);
      if (cost < best_cost * (1.0 - 1e-9) ||
          (tie && k == best && __builtin_popcount(excl) < __builtin_popcount(best_excl))) {
        best_cost = cost;
        best = k;
        best_excl = excl;
      }
      if (sub == 0) break;
    }
  }
  if (best_cost >= 1e299) {  // nothing schedulable with the requested k: single roots, mandatory exclusion only
    best = 1;
    best_excl = mandatory;
  }
  ms_excl_ = best_excl;
  return best;
}

// (re)build the step tree for k root modes: binary tree over the N - k positions of the step's
// mode list. Cached tensors of the old tree are released.
void CpEngine::ms_set_roots(int k) {
  ms_nodes_.clear();
  ms_k_ = k;
  ms_build_tree(0, N_ - k - 1, -1);
  ms_leaf_.assign(N_ - k, -1);
  for (size_t q = 0; q < ms_nodes_.size(); q++)
    if (ms_nodes_[q].lo == ms_nodes_[q].hi) ms_leaf_[ms_nodes_[q].lo] = (int)q;
  if (ms_nodes_.size() + 1 > 32) throw std::runtime_error("ppals: tensor order too large");
  ms_X_.slot = 0;
  for (size_t q = 0; q < ms_nodes_.size(); q++) ms_nodes_[q].t.slot = (int)q + 1;
  ms_invalidate();
}

// room for the placement candidates of X (ms_start_step): none for small tensors, where a scan is
// too short to time from the host and the effect does not matter
// tensors below this size are not worth a placement measurement (their scans are short against the
// host-side timing); PPALS_PLACE_MIN_MB lowers it so that the CPU tests exercise the machinery
double CpEngine::place_min_bytes() {
  const char *e = std::getenv("PPALS_PLACE_MIN_MB");
  return e ? std::atof(e) * 1048576.0 : 1.5e9;
}

size_t CpEngine::ms_X_slack() const {
  const double bytes = (double)V_.nloc * dtype_size(V_.dtype);
  return bytes >= place_min_bytes() ? ((size_t)64 << 20) + 4096 : 0;
}

// ---- online placement choice (engine.h, PlaceExplore) ----
// the sample of the visit in flight, if any, goes to its candidate
void CpEngine::ms_place_collect(PlaceExplore &ex) {
  if (ex.timer < 0) return;
  const double t = ops_.timer_read(ex.timer);
  ex.timer = -1;
  if (t <= 0 || ex.timer_cand < 0 || ex.timer_cand >= (int)ex.cands.size()) return;
  PlaceCand &c = ex.cands[ex.timer_cand];
  c.best = std::min(c.best, t);
  c.samples++;
  ex.worst = std::max(ex.worst, t);
}

// at the head of a visit: the candidate this visit runs (-1: none, the root has settled). Phase 0
// walks the offsets once (store kind by the back end's rule), phase 1 runs the three fastest
// offsets with both store kinds, then the root keeps the fastest sample of all; a later candidate
// must win by more than the timing noise. The sample of the previous visit is a whole cycle of the
// schedule old when it is read here: nothing waits.
int CpEngine::ms_place_pick(PlaceExplore &ex) {
  ms_place_collect(ex);
  // Evidence gate (round 6): on the driver's boxes five rounds of headlines showed the choice worth
  // nothing (tuned 537.6 against untuned 537.8 sweeps/s, fastest and slowest candidate 2.6 % apart),
  // on others 2 %. After the first 8 samples of a root, a spread below 4 % between its fastest and
  // slowest candidate ends the exploration: the root keeps the fastest sample IN THE FIRST BLOCK, so
  // that the second block goes back to the device at once.
  if (ex.phase == 0) {
    int n = 0, best0 = -1;
    double lo = 1e300, hi = 0;
    for (size_t q = 0; q < ex.cands.size(); q++)
      if (ex.cands[q].samples > 0) {
        n++;
        lo = std::min(lo, ex.cands[q].best);
        hi = std::max(hi, ex.cands[q].best);
        if (ex.cands[q].blk == 0 && (best0 < 0 || ex.cands[q].best < ex.cands[best0].best)) best0 = (int)q;
      }
    if (n >= kPlaceGateSamples && best0 >= 0 && hi < lo * (1.0 + kPlaceGateSpread)) {
      ex.chosen = best0;
      ex.gated = true;
      ex.phase = 2;
      ms_place_release_unchosen();
      return -1;
    }
  }
  if (ex.phase == 0 && ex.next >= ex.cands.size()) {
    std::vector<int> idx(ex.cands.size());
    for (size_t q = 0; q < idx.size(); q++) idx[q] = (int)q;
    std::stable_sort(idx.begin(), idx.end(),
                     [&](int a, int b) { return ex.cands[a].best < ex.cands[b].best; });
    const size_t nfin = std::min<size_t>(3, idx.size());
    for (size_t q = 0; q < nfin; q++)
      for (int kind = 0; kind < 2; kind++) {
        PlaceCand c;
        c.blk = ex.cands[idx[q]].blk;
        c.off = ex.cands[idx[q]].off;
        c.nt = kind;
        ex.cands.push_back(c);
      }
    ex.phase = 1;
  }
  if (ex.phase == 1 && ex.next >= ex.cands.size()) {
    int best = -1;
    for (size_t q = 0; q < ex.cands.size(); q++)
      if (ex.cands[q].samples > 0 && (best < 0 || ex.cands[q].best < ex.cands[best].best * 0.995))
        best = (int)q;
    ex.chosen = best;  // (-1: no stopwatch ever answered — offset 0, store kind by size)
    ex.phase = 2;
    ms_place_release_unchosen();
  }
  return ex.phase < 2 ? (int)ex.next++ : -1;
}

// once every exploring root has settled: a candidate block nobody chose goes back to the device
void CpEngine::ms_place_release_unchosen() {
  if (!ms_X_alt_) return;
  bool use[2] = {false, false};
  for (const auto &ex : ms_place_) {
    if (ex.phase == 0 || ex.phase == 1) return;  // somebody still explores
    if (ex.phase == 2) use[ex.chosen >= 0 ? ex.cands[ex.chosen].blk : 0] = true;
  }
  if (use[0] && use[1]) return;
  ops_.sync();
  if (!use[1]) {
    ms_X_alt_.reset();
  } else {  // every root prefers the block in front of the layout: it becomes the only one
    ms_X_base_ = std::move(ms_X_alt_);
    for (auto &ex : ms_place_)
      for (auto &c : ex.cands) c.blk = 0;
  }
  // (called at the head of a step, before its scan: no first-level intermediate is alive)
}

// bytes of the first-level intermediate of the root set first .. first+k-1 (layout-independent)
size_t CpEngine::ms_X_bytes(int first, int k) const {
  int64_t J = 1;
  for (int q = 0; q < k; q++) J *= ext((first + q) % N_);
  return (size_t)(V_.nloc / J) * R_ * dtype_size(work_dt(V_.dtype));
}

// Allocation of one of the session's large buffers. The optional resident layouts (the padded
// third copy, then the second copy) were taken while the device still had room; when a MANDATORY
// buffer does not fit any more they are given back, one at a time, and the allocation is retried —
// the scans then read the layouts that are left (plan_scan), slower but correct. Callers must not
// hold a ScanPlan across this call.
DeviceBuffer CpEngine::big_alloc(size_t bytes) {
  for (;;) {
    DeviceBuffer b = DeviceBuffer::try_alloc(ops_, bytes);
    if (b) return b;
    // first what is merely optional for SPEED OF CHOICE: the second candidate block of the placement
    // exploration (unless the intermediate alive right now lies in it) — a resident layout is worth
    // more to every later sweep than a few more candidates to ~24 visits
    if (ms_X_alt_ && !(ms_X_.valid && (char *)ms_X_.buf >= ms_X_alt_.as<char>() &&
                       (char *)ms_X_.buf < ms_X_alt_.as<char>() + ms_X_alt_.size())) {
      ops_.sync();
      for (auto &ex : ms_place_) {
        if (ex.timer >= 0) {  // a sample of a candidate in the block that goes away is dropped
          ops_.timer_read(ex.timer);
          ex.timer = -1;
        }
        for (auto &c : ex.cands) c.blk = 0;  // (its candidates now alias offsets of the first block)
      }
      ms_X_alt_.reset();
      continue;
    }
    bool had_packs = false;
    for (const auto &t : packs_) had_packs = had_packs || t.data;
    if (had_packs) {  // the packed twins go first, and for good: a layout serves every scan, a twin one
      ops_.sync();
      packs_release();
      pack_off_reason_ = "given back for a mandatory buffer";
      continue;
    }
    if (lay_.size() > 1 && lay_.back().own) {
      ops_.sync();
      lay_.pop_back();
      if (lay_.size() == 1) vt_state_ = -1;
      for (auto &n : nodes_) n.valid = false;
      continue;
    }
    return DeviceBuffer(ops_, bytes);  // throws with the back end's message
  }
}

// new step: X = V contracted with the k root modes first, ..., first + k - 1 (cyclic) in ONE
// tensor scan on whichever resident layout stores them next to each other and behind at least one
// other mode; X is kept in the tensor's own precision
void CpEngine::ms_start_step(int first) {
  const int k = ms_k_;
  ms_root_ = first;
  ms_order_.clear();
  for (int q = k; q < N_; q++) ms_order_.push_back((first + q) % N_);
  for (auto &n : ms_nodes_) n.t.valid = false;
  // X at this root's offset inside the over-allocated block (see engine.h, PlaceExplore); sized
  // before the scan is planned (big_alloc may give a resident layout back)
  const size_t xbytes = ms_X_bytes(first, k);
  const size_t slack = ms_tune_enabled_ ? ms_X_slack() : 0;
  // (an override — the LR optimizers' per-root caches — receives the scan's result itself: no block)
  if (!ms_X_override_ && ms_X_base_.size() < xbytes + slack) {
    // (the block moves: what the roots measured so far is void, they start over)
    for (auto &ex : ms_place_) {
      if (ex.timer >= 0) ops_.timer_read(ex.timer);
      ex = PlaceExplore();
    }
    ms_X_base_.reset();
    ms_X_alt_.reset();
    ms_X_base_ = big_alloc(xbytes + slack);
  }
  ScanPlan pl;
  if (!plan_scan(first, k, false, pl)) {
    // a root set that wraps around the last mode is adjacent only in the second layout; without
    // it (allocation failed / PPALS_TRANSPOSED_COPY=0) fall back to single-mode roots for good
    if (k == 1) throw std::runtime_error("ppals: internal error (single root not adjacent)");
    ms_set_roots(1);
    // the mode just before the one about to be updated, slid back past modes that are never roots
    // (an older root is still current: none of the skipped modes' successors has been updated since)
    int r = (first + k - 1) % N_, guard = 0;
    while (((ms_excl_ >> r) & 1u) && guard++ < N_) r = (r - 1 + N_) % N_;
    ms_start_step(r);
    return;
  }
  const void *src = pl.lay->ptr;
  const int64_t L = pl.Lc, J = pl.J, T = pl.T;
  ms_X_.modes = pl.kept;
  std::vector<FactorRef> f;
  unsigned mask = 0;
  for (int m : pl.set) {
    f.push_back(fref(m, W_.data()));  // storage order: first listed = fastest
    mask |= 1u << m;
  }
  ms_X_.dt = work_dt(V_.dtype);
  ms_X_.contracted = mask;
  if ((size_t)L * T * R_ * dtype_size(ms_X_.dt) != xbytes)
    throw std::runtime_error("ppals: internal error (first-level intermediate size)");
  PackedSrc pk_store;
  const PackedSrc *pk = pl.Lc > 1 ? packed_for(pl, pk_store) : nullptr;
  auto launch_scan = [&](int blk, int64_t off, int nt) {
    ms_X_.buf = ms_X_override_ ? (char *)ms_X_override_
                               : (blk == 1 && ms_X_alt_ ? ms_X_alt_ : ms_X_base_).as<char>() + off;
    ops_.scan_store_mode(nt);
    PackedScope scope(ops_, pk);
    ops_.scan_contract(src, V_.dtype, pl.L, J, T, f.data(), (int)f.size(), R_, ms_X_.buf, ms_X_.dt,
                       L, L * T, pl.pad);
    ops_.scan_store_mode(-1);
  };
  PlaceExplore &ex = ms_place_[first];
  if (slack > 0 && !ms_X_override_ && ex.phase < 0) {
    // first visit of the root: is its placement worth choosing? Only where the result stream
    // matters — an HBM-bound scan (up to two n-tiles) of a tensor large enough for a launch to be
    // long against the stopwatch, that writes at least 1 % of what it reads.
    static const int64_t cand_small[] = {0, 1, 2, 3, 4, 5, 6, 8, 12, 16, 24, 32, 48, 64};
    static const int64_t cand_large[] = {0, 3, 5, 12, 16, 24, 48, 64};
    const double bytes = (double)L * J * T * dtype_size(V_.dtype);
    ex.phase = 3;
    ex.layout = (int)(pl.lay - lay_.data());
    if (bytes >= place_min_bytes() && R_ <= 32 && (double)xbytes >= 0.01 * bytes) {
      const bool large = bytes >= 2e10;  // a scan takes >= 4 ms: fewer candidates
      const int64_t *mb = large ? cand_large : cand_small;
      for (int ci = 0; ci < (large ? 8 : 14); ci++) {
        if ((size_t)(mb[ci] << 20) > slack) break;
        PlaceCand c;
        c.off = mb[ci] << 20;
        ex.cands.push_back(c);
      }
      static const int64_t cand_alt[] = {0, 4, 16, 64};  // in the second block
      for (int ci = 0; ms_X_alt_ && ci < 4; ci++) {
        if ((size_t)(cand_alt[ci] << 20) > slack) break;
        PlaceCand c;
        c.blk = 1;
        c.off = cand_alt[ci] << 20;
        ex.cands.push_back(c);
      }
      ex.phase = 0;
    }
  }
  const int cand = (slack > 0 && !ms_X_override_ && ex.phase >= 0 && ex.phase < 2) ? ms_place_pick(ex) : -1;
  if (cand >= 0) {
    // an exploring visit: the sweep's own scan, at this candidate, under the stopwatch
    ex.visits++;
    ex.timer_cand = cand;
    ex.timer = ops_.timer_begin();
    launch_scan(ex.cands[cand].blk, ex.cands[cand].off, ex.cands[cand].nt);
    if (ex.timer >= 0) ops_.timer_end(ex.timer);
  } else if (ex.phase == 2 && ex.chosen >= 0 && slack > 0 && !ms_X_override_) {
    launch_scan(ex.cands[ex.chosen].blk, ex.cands[ex.chosen].off, ex.cands[ex.chosen].nt);
  } else {
    launch_scan(0, 0, -1);
  }
  ms_X_.pending = false;
  ms_X_.valid = true;
  if (const char *tr = std::getenv("PPALS_TRACE_STEPS")) {  // tests: which root sets were scanned
    if (FILE *f = std::fopen(tr, "a")) {
      const int li = (int)(pl.lay - lay_.data());
      std::fprintf(f, "rank=%d root=%d k=%d layout=%s%s L=%lld J=%lld T=%lld\n", rank_, first, k,
                   li == 1 ? "VT" : "V", pl.lay->q > 0 ? "pad" : "", (long long)L, (long long)J,
                   (long long)T);
      std::fclose(f);
    }
  }
}

// one mode update of the multi-sweep schedule: starts a new step when mode i belongs to the root
// set of the running one (its factor was frozen into X), i.e. after N - k updates
void CpEngine::ms_mode_update(int i, double lambda, bool last_of_sweep) {
  check_tensor_generation();
  // A FIXED mode: no step is started for it, no leaf contracted, nothing launched. Its factor does not
  // change, so every cached contraction stays what it was — the step whose root set it belongs to goes
  // on serving the other modes (see the invalidation below the update).
  if (kind_[i] == kModeFixed) return;
  if (ms_root_ < 0 || ((i - ms_root_ + N_) % N_) < ms_k_) {
    // the k modes updated last serve the next N - k updates — unless one of them is never a root
    // (ms_excl_: the partitioned mode of a sharded session, whose X would be a PARTIAL sum of full
    // global size — s^(N-1) R per rank whatever P is: 5.1 GB against a 12.8 GB shard at cfg4 / P = 8 —,
    // or a mode too short for X to be smaller than the tensor): then the set is slid back past it
    const int first = ms_next_root(i, ms_k_, ms_excl_);
    if (first < 0) throw std::runtime_error("ppals: no root set without the excluded modes");
    ms_start_step(first);
  }
  int pos = -1;
  for (size_t q = 0; q < ms_order_.size(); q++)
    if (ms_order_[q] == i) pos = (int)q;
  const int leaf = ms_leaf_[pos];
  // (S and S^-1 of this update depend on the other modes' Grams only: the contraction launched
  // next may prepare them on the side)
  const bool free_i = kind_[i] == kModeFree;  // the solve: the only update that takes an armed S / Normalize
  if (!multi_ && free_i) ops_.arm_gram_system(G_.as<double>(), N_, i, R_, lambda, S_.as<double>(), Sinv_.as<double>());
  ms_compute(leaf);
  ms_norm_fused_ = false;
  // the sweep's Normalize at the tail of its last update launch, with the pending scales of the cached
  // tensors that outlive the update (everything valid now but the leaf it consumes) — where the update
  // is the fused launch: one rank, or the one-all-reduce plan of a sharded session (never mode 0's)
  if (last_of_sweep && !multi_ && free_i && !skips_normalize() && (!dist_ || (i != 0 && (int64_t)sizeof(double) * V_.glens[i] * R_ <= small_msg_bytes_))) {
    int64_t rows[MAX_ORDER];
    for (int q = 0; q < N_; q++) rows[q] = V_.glens[q];
    // (asked first with no cached tensors — a back end that cannot fold it must not see them marked)
    if (ops_.arm_normalize(W_.data(), rows, N_, R_, G_.as<double>(), i, nullptr)) {
      unsigned masks[32] = {0}, fresh = 0;
      const unsigned active = ms_collect_scales(masks, &fresh, leaf);
      ms_norm_fused_ = ops_.arm_normalize(W_.data(), rows, N_, R_, G_.as<double>(), i, nullptr,
                                          ms_scales_.as<double>(), masks, active, fresh);
    }
  }
  mode_update(i, (const double *)ms_nodes_[leaf].t.buf, ext(i), lambda, false, 1.0);
  ms_nodes_[leaf].t.valid = false;  // a leaf is consumed by its own update
  // A node that contracted mode i holds the factor from before this update. While every root mode is
  // updated in its turn, such a node is never asked for again before the next step starts; but a step whose
  // root modes are FIXED — now, or made so by a later set_mode_kinds, which leaves the caches alone — is not
  // restarted and goes round its mode list again, and then the node must be rebuilt (from its parent, in the
  // end from X, which contracted root modes only). So it is marked in every session: the mark costs nothing
  // where the node is dead anyway, and the kinds may change between any two updates.
  for (auto &nd : ms_nodes_)
    if (nd.t.contracted & (1u << i)) nd.t.valid = false;
}

// dst = src contracted with `mode` (rank index shared), fp64 result; in_scale = pending factor of
// src folded into dst, so dst starts with a clean scale of its own
void CpEngine::ms_contract(const RTensor &src, int mode, RTensor &dst, DeviceBuffer &own, const double *in_scale) {
  int64_t L = 1, T = 1;
  bool before = true;
  dst.modes.clear();
  for (int m : src.modes) {
    if (m == mode) {
      before = false;
      continue;
    }
    (before ? L : T) *= ext(m);
    dst.modes.push_back(m);
  }
  dst.dt = F64;
  dst.contracted = src.contracted | (1u << mode);
  own.reserve(ops_, sizeof(double) * (size_t)L * T * R_);
  dst.buf = own.get();
  FactorRef f = fref(mode, W_.data());
  ops_.mttv(src.buf, src.dt, L, ext(mode), T, &f, 1, R_, (double *)dst.buf, L * T, 0, in_scale);
}

void CpEngine::ms_compute(int idx) {
  MsNode &n = ms_nodes_[idx];
  if (n.t.valid) return;
  const RTensor *src;
  if (n.parent < 0) {
    src = &ms_X_;
  } else {
    ms_compute(n.parent);
    src = &ms_nodes_[n.parent].t;
  }
  // contract the sibling's modes; the one stored slowest first (longest contiguous runs)
  std::vector<int> sib;
  for (int pos = n.slo; pos <= n.shi; pos++) sib.push_back(ms_order_[pos]);
  auto storage_pos = [&](int mode) {
    for (size_t k = 0; k < src->modes.size(); k++)
      if (src->modes[k] == mode) return (int)k;
    return -1;
  };
  std::sort(sib.begin(), sib.end(), [&](int a, int b) { return storage_pos(a) > storage_pos(b); });
  if (n.tmp.size() + 1 < sib.size()) {
    n.tmp.resize(sib.size() - 1);
    n.tmp_own.resize(sib.size() - 1);
  }
  const RTensor *cur = src;
  for (size_t k = 0; k < sib.size(); k++) {
    const bool last = k + 1 == sib.size();
    RTensor &dst = last ? n.t : n.tmp[k];
    ms_contract(*cur, sib[k], dst, last ? n.own : n.tmp_own[k], k == 0 ? ms_scale_of(*src) : nullptr);
    cur = &dst;
  }
  if (sib.empty()) throw std::runtime_error("ppals: empty sibling set in the multi-sweep tree");
  n.t.pending = false;
  n.t.valid = true;
}

void CpEngine::sweep_msdt(double lambda) {
  for (int i = 0; i < N_; i++) ms_mode_update(i, lambda, i == N_ - 1);
  if (!ms_norm_fused_ && !skips_normalize()) normalize();
  ms_norm_fused_ = false;
  grad_from_sweep_ = true;
}

void CpEngine::sweep_dt(double lambda) {
  if (schedule_ == 1) {
    sweep_msdt(lambda);
    return;
  }
  for (auto &n : nodes_) n.valid = false;  // mttkrp_map.clear(), als_CP.cxx:215
  bool norm_fused = false;
  for (int i = 0; i < N_; i++) {
    if (kind_[i] == kModeFixed) continue;  // neither its leaf contraction nor an update
    compute_node(leaf_[i]);
    const Node &lf = nodes_[leaf_[i]];
    // Normalize at the tail of the sweep's last update launch (the solve's: a FREE mode)
    if (i == N_ - 1 && !dist_ && kind_[i] == kModeFree && !skips_normalize()) {
      int64_t rows[MAX_ORDER];
      for (int q = 0; q < N_; q++) rows[q] = V_.glens[q];
      norm_fused = ops_.arm_normalize(W_.data(), rows, N_, R_, G_.as<double>(), i, nullptr);
    }
    mode_update(i, lf.buf.as<double>(), ext(i), lambda, false, 1.0);
    // every cached node that does NOT contain mode i stays valid; nodes containing mode i were
    // built from W_j, j != i only, so they stay valid too until the cache is cleared.
  }
  if (!norm_fused && !skips_normalize()) normalize();
  grad_from_sweep_ = true;
}

// `count` consecutive mode updates starting at mode `first` (cyclic), NO Normalize — the step of
// the class-API optimizers (src/optimizer/*::step). The multi-sweep state carries over between
// calls, so a step that starts where the previous one ended reuses the cached contraction.
void CpEngine::update_modes(int first, int count, double lambda) {
  for (int k = 0; k < count; k++) {
    const int i = (first + k) % N_;
    if (schedule_ == 1) {
      ms_mode_update(i, lambda);
    } else {
      if (i == 0 || k == 0)
        for (auto &n : nodes_) n.valid = false;
      if (kind_[i] == kModeFixed) continue;
      compute_node(leaf_[i]);
      mode_update(i, nodes_[leaf_[i]].buf.as<double>(), ext(i), lambda, false, 1.0);
    }
  }
  grad_from_sweep_ = true;
}

// CPD<dtype, Optimizer>::als (src/CP.cxx:100-186). The optimizer kind fixes the step granularity
// and the fractional sweep counter (Simple 1, DT 0.5 [modes 0..N-2 | mode N-1], MSDT (N-1)/N);
// the ALS iterates are the same cyclic mode updates for all three, computed with this engine's
// own contraction schedule. No Normalize (src/CP.cxx:171).
// ---------------------------------------------------------------------------- low-rank updates
void CpEngine::lr_release() {
  for (int m = 0; m < MAX_ORDER; m++) {
    lr_cache_[m].reset();
    lr_have_[m] = false;
  }
  lr_X_.reset();
  lr_Us_.reset();
  lr_G2_.reset();
  lr_small_.reset();
  lr_T_.reset();
}

// mttkrp_map_init of the LR optimizers (cp_dt_lr_optimizer.cxx:36-94, cp_msdt_lr_optimizer.cxx:
// 31-75): the step's first contraction X = V x_left W_left in the root's own buffer — computed by
// one tensor scan, or (reuse) the kept one brought up to date with the rank-r change of W_left
// that lr_mode_update left in lr_Us_.as<double>() (rows x r) and lr_small_.as<double>() (VT, r x R).
void CpEngine::lr_step_begin(int left, bool reuse, int r) {
  check_tensor_generation();
  if (ms_k_ != 1) ms_set_roots(1);
  if (!lr_cache_[left]) lr_cache_[left] = big_alloc(ms_X_bytes(left, 1));
  if (reuse && lr_have_[left]) {
    ScanPlan pl;
    if (!plan_scan(left, 1, false, pl)) throw std::runtime_error("ppals: internal error (LR scan plan)");
    const int64_t n = pl.Lc * pl.T;
    lr_T_.reserve(ops_, sizeof(double) * (size_t)n * r);
    FactorRef f;
    f.ptr = lr_Us_.as<double>() + (left == 0 ? V_.row0 : 0);
    f.rows = ext(left);
    f.ld = V_.glens[left];
    ops_.scan_contract(pl.lay->ptr, V_.dtype, pl.L, ext(left), pl.T, &f, 1, r, lr_T_.as<double>(), F64, pl.Lc, n,
                       pl.pad);
    ops_.lowrank_accumulate(lr_cache_[left].get(), work_dt(V_.dtype), n, R_, lr_T_.as<double>(), r,
                            lr_small_.as<double>());
    ms_X_ = lr_desc_[left];
    ms_X_.buf = lr_cache_[left].get();
    ms_X_.valid = true;
    ms_X_.pending = false;
    ms_root_ = left;
    ms_order_.clear();
    for (int q = 1; q < N_; q++) ms_order_.push_back((left + q) % N_);
    for (auto &nd : ms_nodes_) nd.t.valid = false;
  } else {
    ms_X_override_ = lr_cache_[left].get();
    ms_start_step(left);
    ms_X_override_ = nullptr;
    lr_desc_[left] = ms_X_;
    lr_have_[left] = true;
  }
}

// One mode update of an LR step. r == 0: the exact update (cholesky_solve in the reference).
// Host helpers of the randomized variant (small dense algebra, R x r and r x r).
// Orthonormal basis of the columns of A (n x k, column-major, in place): modified Gram-Schmidt,
// twice (the second pass restores orthogonality to rounding when the columns are nearly dependent);
// a column that vanishes is left zero.
static void host_qr_mgs2(int n, int k, double *A) {
  for (int j = 0; j < k; j++) {
    double *aj = A + (size_t)n * j;
    for (int pass = 0; pass < 2; pass++)
      for (int p = 0; p < j; p++) {
        const double *ap = A + (size_t)n * p;
        double d = 0;
        for (int i = 0; i < n; i++) d += ap[i] * aj[i];
        for (int i = 0; i < n; i++) aj[i] -= d * ap[i];
      }
    double nn = 0;
    for (int i = 0; i < n; i++) nn += aj[i] * aj[i];
    nn = std::sqrt(nn);
    for (int i = 0; i < n; i++) aj[i] = nn > 0 ? aj[i] / nn : 0.0;
  }
}
// eigen-decomposition of a symmetric n x n matrix (column-major, destroyed) by cyclic Jacobi:
// ev descending, V columns = eigenvectors
static void host_jacobi_eig(int n, double *A, double *ev, double *V) {
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) V[i + (size_t)n * j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 60; sweep++) {
    double off = 0, diag = 0;
    for (int i = 0; i < n; i++)
      for (int j = 0; j < n; j++) (i == j ? diag : off) += A[i + (size_t)n * j] * A[i + (size_t)n * j];
    if (off <= 1e-30 * (diag + 1e-300)) break;
    for (int p = 0; p < n - 1; p++)
      for (int q = p + 1; q < n; q++) {
        const double apq = A[p + (size_t)n * q];
        if (apq == 0.0) continue;
        const double theta = (A[q + (size_t)n * q] - A[p + (size_t)n * p]) / (2.0 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), sn = t * c;
        for (int k = 0; k < n; k++) {  // columns p, q
          const double akp = A[k + (size_t)n * p], akq = A[k + (size_t)n * q];
          A[k + (size_t)n * p] = c * akp - sn * akq;
          A[k + (size_t)n * q] = sn * akp + c * akq;
        }
        for (int k = 0; k < n; k++) {  // rows p, q
          const double apk = A[p + (size_t)n * k], aqk = A[q + (size_t)n * k];
          A[p + (size_t)n * k] = c * apk - sn * aqk;
          A[q + (size_t)n * k] = sn * apk + c * aqk;
        }
        for (int k = 0; k < n; k++) {
          const double vkp = V[k + (size_t)n * p], vkq = V[k + (size_t)n * q];
          V[k + (size_t)n * p] = c * vkp - sn * vkq;
          V[k + (size_t)n * q] = sn * vkp + c * vkq;
        }
      }
  }
  std::vector<int> idx(n);
  for (int i = 0; i < n; i++) idx[i] = i;
  std::sort(idx.begin(), idx.end(), [&](int a, int b) { return A[a + (size_t)n * a] > A[b + (size_t)n * b]; });
  std::vector<double> Vs((size_t)n * n);
  for (int k = 0; k < n; k++) {
    ev[k] = A[idx[k] + (size_t)n * idx[k]];
    for (int i = 0; i < n; i++) Vs[i + (size_t)n * k] = V[i + (size_t)n * idx[k]];
  }
  std::copy(Vs.begin(), Vs.end(), V);
}
static const uint64_t LR_RANDOM_SEED = 0x52414e44535644ull;  // "RANDSVD"

// r > 0: get_rankR_update_cholesky (common.cxx:768-786; random == true: lr_random_) relative to `base`
// (device, s x R; null: the current W_i): gamma = L L^T, X = (M - base gamma) L^-T, its leading r
// singular triplets, W_i = base + (U_r s_r)(VT_r L^-1). Leaves Us = U_r s_r in lr_Us_.as<double>() (s x r) and
// VT in lr_small_.as<double>() (r x R) for the next lr_step_begin. The R x R algebra runs on the host.
void CpEngine::lr_mode_update(int i, double lambda, int r, const double *base) {
  int pos = -1;
  for (size_t q = 0; q < ms_order_.size(); q++)
    if (ms_order_[q] == i) pos = (int)q;
  if (pos < 0) throw std::runtime_error("ppals: internal error (LR update of the root mode)");
  const int leaf = ms_leaf_[pos];
  ms_compute(leaf);
  const double *M = (const double *)ms_nodes_[leaf].t.buf;
  const int64_t s = V_.glens[i];
  if (r <= 0) {
    mode_update(i, M, ext(i), lambda, false, 1.0);
    ms_nodes_[leaf].t.valid = false;
    return;
  }
  const size_t nsr = (size_t)s * R_;
  if (!lr_X_) {
    lr_X_ = DeviceBuffer(ops_, sizeof(double) * (size_t)maxs_ * R_);
    lr_Us_ = DeviceBuffer(ops_, sizeof(double) * (size_t)maxs_ * R_);
    lr_G2_ = DeviceBuffer(ops_, sizeof(double) * (size_t)maxs_ * R_);
    lr_small_ = DeviceBuffer(ops_, sizeof(double) * 4 * (size_t)R_ * R_);
  }
  ops_.gram_system(G_.as<double>(), N_, i, R_, lambda, S_.as<double>(), Sinv_.as<double>());
  // the gradient with the CURRENT factor (what [gradnorm] reports), W_new of the exact solve unused
  ops_.cp_update(M, s, W_[i], s, lr_X_.as<double>(), s, gradW_[i], s, s, R_, S_.as<double>(), Sinv_.as<double>(),
                 gradsq_.as<double>() + i, nullptr, 0,
                 nullptr, 0, 1.0);
  grad_replicated_[i] = true;
  const double *negrhs = gradW_[i];  // -(M - base gamma)
  if (base && base != W_[i]) {
    ops_.cp_update(M, s, base, s, lr_X_.as<double>(), s, lr_G2_.as<double>(), s, s, R_, S_.as<double>(),
                   Sinv_.as<double>(), scal_.as<double>() + 3 * MAX_ORDER,
                   nullptr, 0, nullptr, 0, 1.0);
    negrhs = lr_G2_.as<double>();
  } else {
    base = W_[i];
  }
  // host: L = chol(gamma), T1 = -L^-T  (X = negrhs * T1)
  std::vector<double> Sg((size_t)R_ * R_), L((size_t)R_ * R_, 0.0), Li((size_t)R_ * R_, 0.0),
      T1((size_t)R_ * R_, 0.0);
  ops_.d2h(Sg.data(), S_.as<double>(), sizeof(double) * R_ * R_);
  for (int j = 0; j < R_; j++) {
    double d = Sg[j + (size_t)R_ * j];
    for (int k = 0; k < j; k++) d -= L[j + (size_t)R_ * k] * L[j + (size_t)R_ * k];
    if (!(d > 0)) throw std::runtime_error("ppals: low-rank update: S is not positive definite");
    d = std::sqrt(d);
    L[j + (size_t)R_ * j] = d;
    for (int q = j + 1; q < R_; q++) {
      double v = Sg[q + (size_t)R_ * j];
      for (int k = 0; k < j; k++) v -= L[q + (size_t)R_ * k] * L[j + (size_t)R_ * k];
      L[q + (size_t)R_ * j] = v / d;
    }
  }
  for (int c = 0; c < R_; c++)  // Li = L^-1 (lower), column by column
    for (int q = c; q < R_; q++) {
      double v = (q == c) ? 1.0 : 0.0;
      for (int k = c; k < q; k++) v -= L[q + (size_t)R_ * k] * Li[k + (size_t)R_ * c];
      Li[q + (size_t)R_ * c] = v / L[q + (size_t)R_ * q];
    }
  for (int a = 0; a < R_; a++)
    for (int b = 0; b < R_; b++) T1[a + (size_t)R_ * b] = -Li[b + (size_t)R_ * a];  // -(L^-1)^T
  double *dT1 = lr_small_.as<double>() + (size_t)R_ * R_, *dGX = dT1 + (size_t)R_ * R_, *dV = dGX + (size_t)R_ * R_;
  ops_.h2d(dT1, T1.data(), sizeof(double) * R_ * R_);
  ops_.rows_times_small(negrhs, s, R_, dT1, R_, nullptr, lr_X_.as<double>());    // X = rhs L^-T
  ops_.gram(lr_X_.as<double>(), s, s, R_, dGX);                                   // X^T X
  std::vector<double> Vr((size_t)R_ * r), VT((size_t)r * R_, 0.0);
  if (!lr_random_) {
    ops_.top_eigvecs(dGX, R_, r, dV);                                // leading right singular vectors
    ops_.d2h(Vr.data(), dV, sizeof(double) * R_ * r);
  } else {
    // randomized_svd(X, r, iter = 1) (common.cxx:691-709), on the R x R Gram G = X^T X alone:
    //   Q0 = qr(Omega), Omega ~ U(0,1)^{R x r};  Q = qr(G Q0);  B = X Q;  B = U s Vb^T
    //   => the rank-r factor is X (Q Vb) (Q Vb)^T: right vectors Q Vb, with Vb the eigenvectors of
    //   Q^T G Q (r x r). Everything but the two tall products stays on the host. Omega comes from
    //   the build's counter generator (CTF's stream is not reproducible): seed LR_RANDOM_SEED,
    //   one block of R*r draws per call.
    std::vector<double> G((size_t)R_ * R_), Q((size_t)R_ * r), Y((size_t)R_ * r), C((size_t)r * r),
        Vb((size_t)r * r), ev(r);
    ops_.d2h(G.data(), dGX, sizeof(double) * R_ * R_);
    const uint64_t base_idx = lr_random_calls_++ * (uint64_t)(R_ * r);
    for (int k = 0; k < r; k++)
      for (int a = 0; a < R_; a++) Q[a + (size_t)R_ * k] = u01_host(LR_RANDOM_SEED, base_idx + a + (uint64_t)R_ * k);
    host_qr_mgs2(R_, r, Q.data());
    for (int k = 0; k < r; k++)
      for (int a = 0; a < R_; a++) {
        double v = 0;
        for (int b = 0; b < R_; b++) v += G[a + (size_t)R_ * b] * Q[b + (size_t)R_ * k];
        Y[a + (size_t)R_ * k] = v;
      }
    host_qr_mgs2(R_, r, Y.data());  // Y = Q of the second factorisation
    for (int k = 0; k < r; k++)     // C = Y^T G Y
      for (int l = 0; l < r; l++) {
        double v = 0;
        for (int a = 0; a < R_; a++) {
          double ga = 0;
          for (int b = 0; b < R_; b++) ga += G[a + (size_t)R_ * b] * Y[b + (size_t)R_ * l];
          v += Y[a + (size_t)R_ * k] * ga;
        }
        C[k + (size_t)r * l] = v;
      }
    for (int k = 0; k < r; k++)  // exactly symmetric input for the Jacobi sweeps
      for (int l = k + 1; l < r; l++) C[k + (size_t)r * l] = C[l + (size_t)r * k] = 0.5 * (C[k + (size_t)r * l] + C[l + (size_t)r * k]);
    host_jacobi_eig(r, C.data(), ev.data(), Vb.data());
    for (int k = 0; k < r; k++)
      for (int a = 0; a < R_; a++) {
        double v = 0;
        for (int l = 0; l < r; l++) v += Y[a + (size_t)R_ * l] * Vb[l + (size_t)r * k];
        Vr[a + (size_t)R_ * k] = v;
      }
    ops_.h2d(dV, Vr.data(), sizeof(double) * R_ * r);
  }
  for (int k = 0; k < r; k++)  // VT[k, :] = v_k^T L^-1
    for (int c = 0; c < R_; c++) {
      double v = 0;
      for (int q = c; q < R_; q++) v += Vr[q + (size_t)R_ * k] * Li[q + (size_t)R_ * c];
      VT[k + (size_t)r * c] = v;
    }
  ops_.h2d(lr_small_.as<double>(), VT.data(), sizeof(double) * r * R_);
  ops_.rows_times_small(lr_X_.as<double>(), s, R_, dV, r, nullptr, lr_Us_.as<double>());       // Us = X V_r = U_r s_r
  ops_.rows_times_small(lr_Us_.as<double>(), s, r, lr_small_.as<double>(), R_, base, W_[i]);   // W = base + Us VT
  ops_.gram(W_[i], s, s, R_, G_.as<double>() + (size_t)i * R_ * R_);
  (void)nsr;
  ms_nodes_[leaf].t.valid = false;
}

int CpEngine::run_class(int kind, const CpOpts &o, double *sweeps_out, int *iters_out) {
  if (kind < 0 || kind > 4) throw std::runtime_error("ppals: unknown class-API optimizer");
  const bool lr = kind >= 3;
  if (lr && nonneg()) throw Unsupported("ppals: a non-negative session has no low-rank-update optimizer");
  if (lr && any_nonfree()) throw Unsupported("ppals: a session with constrained modes has no low-rank-update optimizer");
  if (lr) {
    if (dist_) throw std::runtime_error("ppals: the low-rank-update optimizers run on one GPU");
    if (N_ < 3) throw std::runtime_error("ppals: the low-rank-update optimizers need order >= 3");
    if (o.update_rank < 1 || o.update_rank > R_)
      throw std::runtime_error("ppals: update rank must be in [1, R]");
    for (int m = 0; m < MAX_ORDER; m++) lr_have_[m] = false;
    for (auto &nd : nodes_) nd.valid = false;
    ms_invalidate();
    lr_random_ = o.randomsvd != 0;
    lr_random_calls_ = 0;
  }
  // CPDTLROptimizer state (cp_dt_optimizer.cxx:24-37, cp_dt_lr_optimizer.cxx:9-33)
  bool lr_first = true, lr_low = false;
  int lr_left1 = N_ - 1, lr_left2 = N_ - 2, lr_special = 0, lr_count = 0;
  // CPMSDTLROptimizer state (cp_msdt_optimizer.cxx:28, cp_msdt_lr_optimizer.cxx:9-27)
  int lr_msleft = N_;
  bool lr_cached[MAX_ORDER] = {false};
  DeviceBufferTable lr_oldW;
  lr_oldW.resize(N_);
  const int ur = o.update_rank;
  auto lr_step = [&]() -> double {
    if (kind == 3) {
      const int left = lr_first ? lr_left1 : lr_left2;
      lr_step_begin(left, lr_low && lr_count > 1, ur);
      for (int p = 0; p < N_ - 1; p++) {
        if (lr_first && p < lr_special) continue;
        if (!lr_first && p > lr_special) break;
        const int mode = (left + 1 + p) % N_;
        if (((lr_first && p == N_ - 2) || (!lr_first && p == 0)) && lr_count >= 1) {
          lr_mode_update(mode, o.lambda, ur, nullptr);
          lr_low = true;
        } else {
          lr_mode_update(mode, o.lambda, 0, nullptr);
        }
      }
      if (!lr_first) lr_count++;
      if (lr_count == 5 && !lr_first) {
        lr_special = (lr_special + 1) % (N_ - 1);
        lr_count = 0;
        lr_low = false;
        if (lr_special != 0) {
          lr_left1 = (lr_left1 + N_ - 1) % N_;
          lr_left2 = (lr_left2 + N_ - 1) % N_;
        } else {
          lr_left1 = N_ - 1;
          lr_left2 = N_ - 2;
        }
        // the reference keeps two cached first contractions (cached_tensor1 / cached_tensor2,
        // cp_dt_lr_optimizer.cxx:21-35): the roots that just left the pair give theirs back
        // (s^(N-1) R each — at order 5-6 holding all N of them runs the device out of memory)
        for (int m = 0; m < N_; m++)
          if (m != lr_left1 && m != lr_left2 && lr_cache_[m]) {
            ops_.sync();
            lr_cache_[m].reset();
            lr_have_[m] = false;
          }
      }
      lr_first = !lr_first;
      return 0.5;
    }
    lr_msleft = (lr_msleft + N_ - 1) % N_;
    const int left = lr_msleft;
    const bool reuse = lr_low && lr_cached[left];
    lr_step_begin(left, reuse, ur);
    if (!lr_oldW[left]) lr_oldW.alloc(ops_, left, sizeof(double) * V_.glens[left] * R_);
    ops_.d2d(lr_oldW[left], W_[left], sizeof(double) * V_.glens[left] * R_);
    lr_cached[left] = true;
    for (int p = 0; p < N_ - 1; p++) {
      const int mode = (left + 1 + p) % N_;
      if (!lr_cached[mode] || p != N_ - 2) {
        lr_mode_update(mode, o.lambda, 0, nullptr);
      } else {
        lr_mode_update(mode, o.lambda, ur, lr_oldW[mode]);
        lr_low = true;
      }
    }
    return 1.0 * (N_ - 1) / N_;
  };
  std::ofstream csv;
  std::ofstream *pcsv = nullptr;
  if (rank_ == 0 && !o.csv_path.empty()) {
    csv.open(o.csv_path, o.csv_append ? std::ios::app : std::ios::out);
    pcsv = &csv;
    if (!o.bench) csv << "[dim],[iter],[gradnorm],[tol],[pp_update],[diffV],[dtime]\n";
  }
  double st_time = now();
  int iters = 0, next_mode = 0;
  bool first_subtree = true;
  double sweeps = 0, projnorm = 0, diffV = 1000.;
  const int maxsweep = o.maxiter;
  while ((int)sweeps <= maxsweep) {
    if (iters % o.resprint == 0 || sweeps >= maxsweep || sweeps == 0) {
      ops_.sync();
      const double st_time1 = now();
      projnorm = gradnorm();
      diffV = residual();
      st_time += now() - st_time1;
      const double dtime = now() - st_time;
      if (rank_ == 0) {
        if (!o.bench) {
          if (o.verbose) {
            std::cout.precision(13);
            std::cout << "  [dim]=  " << V_.glens[0] << "  [sweeps]=  " << sweeps
                      << "  [gradnorm]  " << projnorm << "  [tol]  " << o.tol
                      << "  [pp_update]  " << 0 << "  [residual]  " << diffV << "  [dtime]  "
                      << dtime << "\n";
          }
          if (pcsv) {
            (*pcsv) << V_.glens[0] << "," << sweeps << "," << projnorm << "," << o.tol << "," << 0
                    << "," << diffV << "," << dtime << "\n";
            if (iters % 100 == 0 && iters != 0) (*pcsv) << std::endl;
          }
        } else if (iters != 0) {
          if (o.verbose) std::cout << "  [dimension tree step time]  " << dtime << "\n";
          if (pcsv) (*pcsv) << "[DTtime]" << "," << dtime << "\n";
        }
      }
      if (agree(projnorm < o.tol || now() - st_time > o.timelimit)) break;
    }
    int count;
    double frac;
    if (lr) {
      sweeps += lr_step();
      grad_from_sweep_ = true;
      iters += 1;
      if (iters % 10 == 0 && rank_ == 0 && o.verbose) printf(".");
      continue;
    }
    if (kind == 0) {
      count = N_;
      frac = 1.0;
    } else if (kind == 1) {
      count = first_subtree ? N_ - 1 : 1;
      first_subtree = !first_subtree;
      frac = 0.5;
    } else {
      count = N_ - 1;
      frac = 1.0 * (N_ - 1) / N_;
    }
    update_modes(next_mode, count, o.lambda);
    next_mode = (next_mode + count) % N_;
    sweeps += frac;
    iters += 1;
    if (iters % 10 == 0 && rank_ == 0 && o.verbose) printf(".");
  }
  ops_.sync();
  if (rank_ == 0 && o.verbose) {
    printf("\nIters = %d Final proj-grad norm %E \n", iters, projnorm);
    printf("tf took %lf seconds\n", now() - st_time);
  }
  if (pcsv) csv.close();
  if (sweeps_out) *sweeps_out = sweeps;
  if (iters_out) *iters_out = iters;
  return sweeps == maxsweep + 1 ? 0 : 1;
}

double CpEngine::allreduce_scalar(double x) {
  if (!dist_) return x;
  ops_.h2d(scal_.as<double>(), &x, sizeof(double));
  comm_.allreduce_sum(scal_.as<double>(), 1);
  double y = 0;
  ops_.d2h(&y, scal_.as<double>(), sizeof(double));
  return y;
}

// A stop decision that involves this rank's own wall clock (the time limit) must be the same on
// every rank, or one rank leaves the loop while the others enter the next sweep's collective:
// any rank over the limit stops all of them (one scalar all-reduce, print blocks only).
bool CpEngine::agree(bool local) {
  if (!dist_) return local;
  return allreduce_scalar(local ? 1.0 : 0.0) > 0.0;
}

double CpEngine::gradnorm() {
  if (!grad_from_sweep_) return init_gradnorm_;
  double h[MAX_ORDER];
  ops_.d2h(h, gradsq_.as<double>(), sizeof(double) * N_);
  double part = 0, repl = 0;  // row-block partial sums vs. sums every rank already holds in full
  for (int i = 0; i < N_; i++) (grad_replicated_[i] ? repl : part) += h[i];
  return std::sqrt(allreduce_scalar(part) + repl);
}

double CpEngine::residual() {
  int64_t M, K;
  split_sizes(V_, &M, &K);
  if (!Qbuf_) Qbuf_ = DeviceBuffer(ops_, sizeof(double) * M * R_);
  if (!Pbuf_) Pbuf_ = DeviceBuffer(ops_, sizeof(double) * K * R_);
  split_krp(ops_, V_, R_, W_.data(), Qbuf_.as<double>(), Pbuf_.as<double>(), &M, &K);
  ops_.residual_sq(V_.data, V_.dtype, M, K, Qbuf_.as<double>(), Pbuf_.as<double>(), R_, scal_.as<double>());
  if (dist_) comm_.allreduce_sum(scal_.as<double>(), 1);
  double h = 0;
  ops_.d2h(&h, scal_.as<double>(), sizeof(double));
  return std::sqrt(h);
}

int residual_form_env() {
  const char *v = getenv("PPALS_MODEL_RESIDUAL");
  if (!v || !*v || !strcmp(v, "fused")) return RESIDUAL_FUSED;
  if (!strcmp(v, "two_pass")) return RESIDUAL_TWO_PASS;
  throw std::runtime_error("ppals: PPALS_MODEL_RESIDUAL must be fused or two_pass");
}

void model_export_run(Ops &ops, ModelExportCall &c, const ModelPlan &mp, const double *Q, const double *P,
                      int K) {
  const TensorDesc &V = *c.V;
  bool two = false;
  if (c.residual) {
    const bool exact = V.dtype != F64 || c.a->dtype == DV_F64;  // the export into the view rounds nothing
    two = exact && c.form == RESIDUAL_TWO_PASS;
  }
  if (!two) {
    ops.model_to_view(mp, Q, P, K, c.residual, c.dst, c.a->dtype, V.data, V.dtype, c.stream);
    return;
  }
  if (!c.exported) {
    const ViewPlan p = dv_plan(*c.a, V.glens, V.row0, V.llens[0]);
    if (p.kind != DV_EMPTY) ops.copy_view(p, DV_EXPORT, c.dst, c.a->dtype, V.data, V.dtype, c.stream);
    c.exported = true;
  }
  ops.model_to_view(dv_model_rmw(mp), Q, P, K, true, c.dst, c.a->dtype, c.dst, c.a->dtype, c.stream);
}

// The operands of a grouped plan (groups A and B chosen, box cut): xq_ / xp_ = the Khatri-Rao products
// of the box rows of the groups' factors (grow-only buffers kept by the session), and the plan's offsets
// and leading dimensions. Shared by the model export and the imputation, which differ in the grouping.
void CpEngine::model_operands(const ModelBox &bx, ModelPlan &mp) {
  auto refs = [&](const ModelGroup &g, FactorRef *f) {
    for (int i = 0; i < g.n; i++) {
      const int m = g.mode[i];
      f[i].ptr = W_[m] + bx.lo[m];
      f[i].rows = bx.len[m];
      f[i].ld = V_.glens[m];
    }
  };
  const int64_t A = mp.ga.count, B = mp.gb.count;
  xq_.reserve(ops_, sizeof(double) * A * R_);
  xp_.reserve(ops_, sizeof(double) * B * R_);
  FactorRef fa[MAX_ORDER], fb[MAX_ORDER];
  refs(mp.ga, fa);
  refs(mp.gb, fb);
  ops_.krp(xq_.as<double>(), fa, mp.ga.n, 0, R_);
  ops_.krp(xp_.as<double>(), fb, mp.gb.n, 0, R_);
  mp.voff = bx.voff;
  mp.roff = bx.roff;
  mp.ldq = A;
  mp.pL = B;
  mp.pLK = 0;
}

// The model through a view: [[W]] is symmetric in how the modes are grouped, so the
// grouping follows the VIEW. Group A = the view's fastest modes (by stride) until A reaches the square
// root of the box, group B = the rest in the shard's order (a residual's V reads run along it when A is
// not the shard's fast side); Q and P are their Khatri-Rao products, and the kernel stores Q P^T with the
// lane index along the view's unit-stride run.
void CpEngine::export_model(const ViewArgs &a, void *dst, bool residual, void *stream) {
  ModelBox bx;
  if (!dv_model_box(a, V_.glens, V_.row0, V_.llens[0], &bx)) return;
  int ord[MAX_ORDER], n = 0;
  int64_t total = 1;
  for (int m = 0; m < N_; m++) {
    total *= bx.len[m];
    if (bx.len[m] > 1) ord[n++] = m;
  }
  std::stable_sort(ord, ord + n, [&](int x, int y) { return bx.vs[x] < bx.vs[y]; });
  ModelPlan mp;
  bool inA[MAX_ORDER] = {};
  for (int i = 0; i < n && (mp.ga.count < 64 || mp.ga.count * mp.ga.count < total); i++) {
    mp.ga.add(bx, ord[i]);
    inA[ord[i]] = true;
  }
  for (int m = 0; m < N_; m++)
    if (!inA[m]) mp.gb.add(bx, m);
  model_operands(bx, mp);
  ModelExportCall c{&a, &V_, dst, residual, residual_form_, false, stream};
  model_export_run(ops_, c, mp, xq_.as<double>(), xp_.as<double>(), R_);
}

// The imputation: the stores go to the shard, so here the grouping follows the SHARD.
// Group A = the shard's fastest modes (its own order) until A reaches the square root of the box: the
// lane index of the store pass runs along it, and so do the V reads of the observed residual. Group B =
// the rest, a mode in which the mask is unit-stride first: when the mask is not contiguous along A its
// bytes, 1 B per element, are the side read along b through LDS. (The weighted step groups the same way:
// its first side view, the data, in the mask's place, and `second`, the strides of its weights view, asked
// only when the first has no unit-stride mode outside A.)
void CpEngine::shard_groups(const ModelBox &bx, const int64_t *second, ModelPlan &mp) const {
  int64_t total = 1;
  for (int m = 0; m < N_; m++) total *= bx.len[m];
  bool inA[MAX_ORDER] = {};
  for (int m = 0; m < N_ && (mp.ga.count < 64 || mp.ga.count * mp.ga.count < total); m++)
    if (bx.len[m] > 1) {
      mp.ga.add(bx, m);
      inA[m] = true;
    }
  int first = -1;
  for (int m = 0; m < N_ && first < 0; m++)
    if (!inA[m] && bx.len[m] > 1 && bx.vs[m] == 1) first = m;
  for (int m = 0; second && m < N_ && first < 0; m++)
    if (!inA[m] && bx.len[m] > 1 && second[m] == 1) first = m;
  if (first >= 0) mp.gb.add(bx, first);
  for (int m = 0; m < N_; m++)
    if (!inA[m] && m != first) mp.gb.add(bx, m);
}

void CpEngine::impute(const ViewArgs &a, const void *mask, void *stream, double *observed_sq) {
  if (multi_) throw std::logic_error("ppals: a multi-start session does not impute (take the winner first)");
  ModelBox bx;
  if (dv_model_box(a, V_.glens, V_.row0, V_.llens[0], &bx)) {
    ModelPlan mp;
    shard_groups(bx, nullptr, mp);
    model_operands(bx, mp);
    ops_.model_impute(mp, xq_.as<double>(), xp_.as<double>(), R_, false, mask, V_.data, V_.dtype,
                      observed_sq ? scal_.as<double>() : nullptr, stream);
    // the contents changed with that launch: every session on the tensor, this one too, rebuilds what
    // it derived at its next read (a rank none of whose rows lie in the box has changed nothing)
    if (V_.generation) ++*V_.generation;
  } else if (observed_sq) {
    ops_.zero(scal_.as<double>(), sizeof(double));  // none of the box in this rank's rows
  }
  if (!observed_sq) return;
  if (dist_) comm_.allreduce_sum(scal_.as<double>(), 1);
  ops_.d2h(observed_sq, scal_.as<double>(), sizeof(double));
}

// The loop of ppals_cp_em and ppals_cp_wls: iteration k is step(&sq or nullptr) followed by inner_sweeps
// sweeps; sq is looked at every o.resprint iterations, and one last step with it runs on the way out
// unless the stopping look just did. Returns 1: a look found sqrt(sq) <= o.tol; 2: from the second look
// on, the residual fell by no more than rel_change of the look before (0: no such rule); 0 otherwise.
template <typename Step>
int CpEngine::em_loop(Step &&step, const CpOpts &o, int inner_sweeps, double rel_change, int *iters, double *res) {
  const double t0 = now();
  double sq = 0, prev = -1;
  int k = 0, why = 0;
  bool fresh = false;  // fresh: the tensor and sq belong to the current factors
  while (k < o.maxiter) {
    const bool look = k % o.resprint == 0;
    step(look ? &sq : nullptr);
    fresh = look;
    if (look) {
      const double cur = std::sqrt(sq);
      if (cur <= o.tol)
        why = 1;
      else if (rel_change > 0 && prev >= 0 && prev - cur <= rel_change * prev)
        why = 2;
      prev = cur;
      if (why || agree(now() - t0 > o.timelimit)) break;
    }
    for (int i = 0; i < inner_sweeps; i++) sweep_dt(o.lambda);
    fresh = false;
    k++;
  }
  if (!fresh) step(&sq);
  if (iters) *iters = k;
  if (res) *res = std::sqrt(sq);
  return why;
}

int CpEngine::run_em(const ViewArgs &a, const void *mask, void *stream, const CpOpts &o, int inner_sweeps,
                     int *iters, double *observed_res) {
  return em_loop([&](double *sq) { impute(a, mask, stream, sq); }, o, inner_sweeps, 0.0, iters, observed_res);
}

// The weighted step: the imputation's plan with the data view in the mask's place, and the
// weights view beside it (ModelSide). Every element of the box is stored.
const char *CpEngine::wls_refusal() const {
  if (V_.dtype == BF16)
    return "BF16 storage is not supported: a bf16 rounding of the working tensor is coarser than the "
           "h (x - m) correction it carries, so the majorization no longer holds";
  if (R_ > 128) return "R > 128 is not supported: the factor tile is kept in LDS";
  return nullptr;
}

// The body of wls_step and huber_step: `c` < 0 asks for the weighted rule (then `w` is given), otherwise the
// Huber rule at that threshold, `w` == nullptr for the family without weights. out[0] = the loss, out[1] =
// the clipped count (Huber only), both over all ranks; out == nullptr: asynchronous.
void CpEngine::side_step(const char *what, const ViewArgs &a, const void *data, const ViewArgs *w,
                         const void *weights, void *stream, double c, double *out) {
  if (multi_)
    throw std::logic_error(std::string("ppals: a multi-start session takes no ") + what +
                           " step (take the winner first)");
  if (const char *why = wls_refusal()) throw Unsupported(std::string("ppals: ") + why);
  const bool huber = c >= 0;
  const int nout = huber ? 2 : 1;
  ModelBox bx;
  if (dv_model_box(a, V_.glens, V_.row0, V_.llens[0], &bx)) {
    ModelPlan mp;
    shard_groups(bx, w ? w->stride : nullptr, mp);
    model_operands(bx, mp);
    ModelSide ws;
    if (w) ws = dv_model_side(*w, bx, mp);
    if (huber)
      ops_.model_huber(mp, w ? &ws : nullptr, xq_.as<double>(), xp_.as<double>(), R_, data, weights, a.dtype, V_.data,
                       V_.dtype, c,
                       out ? scal_.as<double>() : nullptr, stream);
    else
      ops_.model_wls(mp, ws, xq_.as<double>(), xp_.as<double>(), R_, data, weights, a.dtype, V_.data, V_.dtype,
                     out ? scal_.as<double>() : nullptr, stream);
    if (V_.generation) ++*V_.generation;  // (as after an imputation)
  } else if (out) {
    ops_.zero(scal_.as<double>(), sizeof(double) * nout);  // none of the box in this rank's rows
  }
  if (!out) return;
  if (dist_) comm_.allreduce_sum(scal_.as<double>(), nout);
  ops_.d2h(out, scal_.as<double>(), sizeof(double) * nout);
}

void CpEngine::wls_step(const ViewArgs &a, const void *data, const ViewArgs &w, const void *weights, void *stream,
                        double *weighted_sq) {
  side_step("weighted", a, data, &w, weights, stream, -1.0, weighted_sq);
}

int CpEngine::run_wls(const ViewArgs &a, const void *data, const ViewArgs &w, const void *weights, void *stream,
                      const CpOpts &o, int inner_sweeps, double rel_change, int *iters, double *weighted_res) {
  return em_loop([&](double *sq) { wls_step(a, data, w, weights, stream, sq); }, o, inner_sweeps, rel_change, iters,
                 weighted_res);
}

// The Huber step: the weighted step with the residual clipped to [-c, c] first.
void CpEngine::huber_step(const ViewArgs &a, const void *data, const ViewArgs *w, const void *weights, void *stream,
                          double c, double *huber_loss, int64_t *clipped) {
  double out[2] = {0, 0};
  side_step("Huber", a, data, w, weights, stream, c, (huber_loss || clipped) ? out : nullptr);
  if (huber_loss) *huber_loss = out[0];
  if (clipped) *clipped = (int64_t)out[1];
}

int CpEngine::run_robust(const ViewArgs &a, const void *data, const ViewArgs *w, const void *weights, void *stream,
                         double c, const CpOpts &o, int inner_sweeps, double rel_change, int *iters,
                         double *robust_res) {
  return em_loop([&](double *sq) { huber_step(a, data, w, weights, stream, c, sq, nullptr); }, o, inner_sweeps,
                 rel_change, iters, robust_res);
}

int CpEngine::run_steps(const std::function<void(double *)> &step, const CpOpts &o, int inner_sweeps,
                        double rel_change, int *iters, double *res) {
  if (multi_) throw std::logic_error("ppals: a multi-start session drives no step loop (take the winner first)");
  return em_loop(step, o, inner_sweeps, rel_change, iters, res);
}

const char *CpEngine::quantile_refusal() const {
  if (R_ > 128) return "R > 128 is not supported: the factor tile is kept in LDS";
  if (P_ > 1) return "the residual quantile runs on one rank";
  return nullptr;
}

// The k-th smallest (k = min(n - 1, max(0, ceil(p n) - 1))) of (float)|x - m| over the box's elements with
// h > 0, by a radix select on the fp32 patterns: 11, 10 and 10 bits, one histogram pass each, the bin picked
// here between the passes. Nothing of the tensor is read: only its shape and this rank's rows.
void CpEngine::abs_residual_quantile(const ViewArgs &a, const void *data, const ViewArgs *w, const void *weights,
                                     void *stream, double p, double *value, int64_t *count) {
  if (multi_) throw std::logic_error("ppals: a multi-start session has no residual quantile (take the winner first)");
  if (const char *why = quantile_refusal()) throw Unsupported(std::string("ppals: ") + why);
  ModelBox bx;
  uint64_t n = 0;
  uint32_t key = 0;
  if (dv_model_box(a, V_.glens, V_.row0, V_.llens[0], &bx)) {
    ModelPlan mp;
    shard_groups(bx, w ? w->stride : nullptr, mp);
    model_operands(bx, mp);
    ModelSide ws;
    if (w) ws = dv_model_side(*w, bx, mp);
    std::vector<uint64_t> hist(Ops::ABSRES_BINS);
    uint64_t k = 0;
    const int shifts[3] = {20, 10, 0}, bits[3] = {11, 10, 10};
    for (int pass = 0; pass < 3; pass++) {
      const int pshift = pass == 0 ? 31 : shifts[pass - 1];
      ops_.model_absres_hist(mp, w ? &ws : nullptr, xq_.as<double>(), xp_.as<double>(), R_, data, weights, a.dtype,
                             pshift, key >> pshift,
                             shifts[pass], (1u << bits[pass]) - 1, hist.data(), stream);
      if (pass == 0) {
        for (uint64_t h : hist) n += h;
        if (n == 0) break;
        const double want = std::ceil(p * (double)n) - 1.0;
        k = want <= 0 ? 0 : (want >= (double)(n - 1) ? n - 1 : (uint64_t)want);
      }
      uint32_t b = 0;
      while (k >= hist[b]) k -= hist[b++];  // (the pass counted exactly the keys of the chosen prefix: k < their sum)
      key |= b << shifts[pass];
    }
  }
  if (count) *count = (int64_t)n;
  float f;
  std::memcpy(&f, &key, sizeof f);
  *value = n ? (double)f : std::numeric_limits<double>::quiet_NaN();
}

// ---------------------------------------------------------------------------- core consistency
int64_t CpEngine::core_entries(int start) const {
  const int64_t R = start_rank(start);
  int64_t n = 1;
  for (int i = 0; i < N_ && n <= kCoreMaxEntries; i++) n *= R;
  return n;
}

// The diagnostic of engine.h. Launches: one for the pseudo-inverse factors of all modes and starts, ONE tensor
// scan Y = V x_m P_m on the columns of all selected starts (m: the longest mode a resident layout scans
// row-contiguously, so Y is as small as it gets), then per start N - 1 mode products on its column block of
// Y — the kept mode stored slowest first, so every product but the last reads contiguous rows; the last one
// writes the start's core — and one score launch. Y has the tensor's work type, everything behind it is fp64.
// The chain's products are booked with the other kernels in the launch profile: the tensor is read once.
void CpEngine::core_consistency(int only, double *cc_host, double *core_host) {
  if (P_ > 1) throw Unsupported("ppals: the core consistency runs on one rank");
  if (N_ < 2) throw Unsupported("ppals: the core consistency needs a tensor of order >= 2");
  StartTable tab = tab_;
  if (!multi_) {  // an ordinary session is one start: its Grams lie where the table says
    tab = StartTable();
    tab.nstarts = 1;
    tab.col[1] = R_;
    tab.sq[1] = R_ * R_;
  }
  const int K = tab.nstarts;
  if (only >= K) throw std::runtime_error("ppals: start out of range");
  const int b0 = only < 0 ? 0 : only, b1 = only < 0 ? K : only + 1;
  if (core_host && b1 - b0 != 1) throw std::runtime_error("ppals: a core is read one start at a time");
  if (tab.max_rank() > Ops::kPinvMaxRank) throw Unsupported("ppals: the core consistency supports ranks <= 64");
  for (int b = b0; b < b1; b++)
    if (core_entries(b) > kCoreMaxEntries) throw Unsupported("ppals: the core has more than 2^24 entries");
  check_tensor_generation();
  int64_t rows[MAX_ORDER];
  for (int i = 0; i < N_; i++) rows[i] = V_.glens[i];
  if (cc_P_.empty()) {
    cc_P_.resize(N_);
    for (int i = 0; i < N_; i++) cc_P_.alloc(ops_, i, sizeof(double) * (size_t)rows[i] * R_);
    cc_flag_ = DeviceBuffer(ops_, sizeof(int) * K);
    cc_out_ = DeviceBuffer(ops_, sizeof(double) * K);
  }
  // the contracted mode, before anything is sized (LT = the kept modes' extents)
  int m = -1;
  bool m_rows = false;
  for (int c = 0; c < N_; c++) {
    ScanPlan pc;
    if (!plan_scan(c, 1, false, pc)) continue;
    const bool rc = pc.Lc > 1;
    if (m < 0 || (rc && !m_rows) || (rc == m_rows && ext(c) >= ext(m))) {
      m = c;
      m_rows = rc;
    }
  }
  if (m < 0) throw std::runtime_error("ppals: internal error (no scan for the core consistency)");
  const int wdt = work_dt(V_.dtype);
  const int64_t LT = V_.nloc / ext(m);
  const int cA = tab.col[b0], ncols = tab.col[b1] - cA;
  size_t chain_max = 0, core_total = 0;
  ScanPlan pl;
  plan_scan(m, 1, false, pl);
  const int nk = (int)pl.kept.size();
  for (int b = b0; b < b1; b++) {
    const size_t Rb = (size_t)tab.rank(b);
    size_t elems = (size_t)LT * Rb;
    for (int p = nk - 1; p >= 1; p--) {  // (the product of p == 0 writes the core)
      elems = elems / (size_t)ext(pl.kept[p]) * Rb;
      chain_max = std::max(chain_max, elems);
    }
    core_total += (size_t)core_entries(b);
  }
  cc_Y_.reserve(ops_, (size_t)LT * ncols * dtype_size(wdt));
  if (chain_max) cc_chain_[0].reserve(ops_, sizeof(double) * chain_max);
  if (chain_max && nk > 2) cc_chain_[1].reserve(ops_, sizeof(double) * chain_max);
  cc_core_.reserve(ops_, sizeof(double) * core_total);

  ops_.zero(cc_flag_.as<int>(), sizeof(int) * K);
  ops_.cp_pinv_ragged(G_.as<double>(), N_, tab, W_.data(), rows, cc_P_.data(), cc_flag_.as<int>());
  {
    FactorRef f = fref(m, cc_P_.data());
    f.ptr += (size_t)cA * f.ld;
    ops_.scan_contract(pl.lay->ptr, V_.dtype, pl.L, pl.J, pl.T, &f, 1, ncols, cc_Y_.get(), wdt, pl.Lc,
                       pl.Lc * pl.T, pl.pad);
  }
  ops_.scan_profile_slot(1);
  try {
    size_t core_off = 0;
    for (int b = b0; b < b1; b++) {
      const int Rb = tab.rank(b);
      double *core = cc_core_.as<double>() + core_off;
      const void *X = cc_Y_.as<char>() + (size_t)(tab.col[b] - cA) * LT * dtype_size(wdt);
      int xdt = wdt;
      int64_t tail = Rb;  // what lies behind the mode being contracted: r_m, then the modes already done
      for (int p = nk - 1; p >= 0; p--) {
        int64_t L = 1;
        for (int q = 0; q < p; q++) L *= ext(pl.kept[q]);
        const int km = pl.kept[p];
        FactorRef f = fref(km, cc_P_.data());
        double *out = p == 0 ? core : cc_chain_[(nk - 1 - p) & 1].as<double>();
        ops_.ttm_keep(X, xdt, L, ext(km), tail, f.ptr + (size_t)tab.col[b] * f.ld, f.ld, Rb, out);
        tail *= Rb;
        X = out;
        xdt = F64;
      }
      ops_.core_score(core, Rb, N_, cc_flag_.as<int>() + b, cc_out_.as<double>() + b);
      core_off += (size_t)core_entries(b);
    }
  } catch (...) {
    ops_.scan_profile_slot(0);
    throw;
  }
  ops_.scan_profile_slot(0);
  ops_.d2h(cc_host, cc_out_.as<double>() + b0, sizeof(double) * (b1 - b0));  // the flag travels as the NaN of the score
  if (!core_host) return;
  // the device holds the core with its indices in the order (kept modes as stored, then m)
  const int64_t n = core_entries(b0), Rb = tab.rank(b0);
  bool natural = m == N_ - 1;
  for (int q = 0; q < nk; q++) natural = natural && pl.kept[q] == q;
  if (natural) {
    ops_.d2h(core_host, cc_core_.get(), sizeof(double) * n);
    return;
  }
  std::vector<double> tmp((size_t)n);
  ops_.d2h(tmp.data(), cc_core_.get(), sizeof(double) * n);
  int64_t stride[MAX_ORDER];  // of the device's q-th index in the caller's layout
  for (int q = 0; q <= nk; q++) {
    const int mode = q < nk ? pl.kept[q] : m;
    stride[q] = 1;
    for (int i = 0; i < mode; i++) stride[q] *= Rb;
  }
  for (int64_t e = 0; e < n; e++) {
    int64_t rem = e, dst = 0;
    for (int q = 0; q <= nk; q++) {
      dst += (rem % Rb) * stride[q];
      rem /= Rb;
    }
    core_host[dst] = tmp[(size_t)e];
  }
}

// ---------------------------------------------------------------------------- influence plot
size_t slice_work_cap_env() {
  const char *v = getenv("PPALS_TEST_SLICE_WORK_BYTES");
  if (!v || !*v) return (size_t)256 << 20;
  char *end = nullptr;
  const long long n = strtoll(v, &end, 10);
  if (*end || n < 1) throw std::runtime_error("ppals: PPALS_TEST_SLICE_WORK_BYTES must be a positive number of bytes");
  return (size_t)n;
}

// The model is residual()'s: the same split, the same Khatri-Rao operands in the same buffers.
void CpEngine::slice_residuals(double *ss_host, double *total_host) {
  if (P_ > 1) throw Unsupported("ppals: the per-slice residuals run on one rank");
  if (multi_) throw Unsupported("ppals: the per-slice residuals take an ordinary session");
  int64_t M, K, nout = 0;
  split_sizes(V_, &M, &K);
  for (int i = 0; i < N_; i++) nout += V_.glens[i];
  if (!Qbuf_) Qbuf_ = DeviceBuffer(ops_, sizeof(double) * M * R_);
  if (!Pbuf_) Pbuf_ = DeviceBuffer(ops_, sizeof(double) * K * R_);
  sl_row_.reserve(ops_, sizeof(double) * M);
  double *row = sl_row_.as<double>();
  sl_col_.reserve(ops_, sizeof(double) * K);
  double *col = sl_col_.as<double>();
  sl_out_.reserve(ops_, sizeof(double) * (nout + 1));
  double *out = sl_out_.as<double>();
  split_krp(ops_, V_, R_, W_.data(), Qbuf_.as<double>(), Pbuf_.as<double>(), &M, &K);
  // the op frees its partial sums' buffer and takes a larger one as it needs (ops.h): handed over for the call,
  // taken back on every way out
  size_t work_bytes = sl_work_.size();
  void *work = sl_work_.release();
  try {
    ops_.residual_slices(V_.data, V_.dtype, M, K, Qbuf_.as<double>(), Pbuf_.as<double>(), R_, row, col, out + nout,
                         slice_work_cap_, work, work_bytes);
  } catch (...) {
    sl_work_ = DeviceBuffer(ops_, work, work_bytes);
    throw;
  }
  sl_work_ = DeviceBuffer(ops_, work, work_bytes);
  const int h = N_ / 2;
  int64_t left = 0;
  for (int i = 0; i < h; i++) left += V_.glens[i];
  if (h > 0) ops_.fold_slice_sums(row, V_.glens, h, out);
  ops_.fold_slice_sums(col, V_.glens + h, N_ - h, out + left);
  ops_.d2h(ss_host, out, sizeof(double) * nout);
  if (total_host) ops_.d2h(total_host, out + nout, sizeof(double));
}

void CpEngine::leverages(double *lev_host) {
  if (P_ > 1) throw Unsupported("ppals: the leverages run on one rank");
  if (multi_) throw Unsupported("ppals: the leverages take an ordinary session");
  if (R_ > Ops::kPinvMaxRank) throw Unsupported("ppals: the leverages support ranks <= 64");
  StartTable tab;
  tab.nstarts = 1;
  tab.col[1] = R_;
  tab.sq[1] = R_ * R_;
  int64_t rows[MAX_ORDER], nout = 0;
  for (int i = 0; i < N_; i++) nout += (rows[i] = V_.glens[i]);
  if (cc_P_.empty()) {  // (the buffers of the core consistency: the same pseudo-inverse factors)
    cc_P_.resize(N_);
    for (int i = 0; i < N_; i++) cc_P_.alloc(ops_, i, sizeof(double) * (size_t)rows[i] * R_);
    cc_flag_ = DeviceBuffer(ops_, sizeof(int));
    cc_out_ = DeviceBuffer(ops_, sizeof(double));
  }
  sl_out_.reserve(ops_, sizeof(double) * (nout + 1));
  double *out = sl_out_.as<double>();
  ops_.zero(cc_flag_.as<int>(), sizeof(int));
  ops_.cp_pinv_ragged(G_.as<double>(), N_, tab, W_.data(), rows, cc_P_.data(), cc_flag_.as<int>());
  int64_t off = 0;
  for (int i = 0; i < N_; i++) {
    ops_.row_dots(cc_P_[i], W_[i], rows[i], R_, rows[i], out + off);
    off += rows[i];
  }
  int bad = 0;
  ops_.d2h(&bad, cc_flag_.as<int>(), sizeof(int));
  ops_.d2h(lev_host, out, sizeof(double) * nout);
  if (bad)  // a Gram without a positive finite pivot: no projector to speak of
    for (int64_t e = 0; e < nout; e++) lev_host[e] = std::numeric_limits<double>::quiet_NaN();
}

// ---------------------------------------------------------------------------- factor match score
StartTable CpEngine::start_table() const {
  if (multi_) return tab_;
  StartTable t;
  t.nstarts = 1;
  t.col[1] = R_;
  t.sq[1] = R_ * R_;
  return t;
}

void CpEngine::congruence(CpEngine &b, int skip_mode, std::vector<double> &out) {
  if (P_ > 1 || b.P_ > 1) throw Unsupported("ppals: the factor congruence runs on one rank");
  if (&ops_ != &b.ops_) throw std::runtime_error("ppals: the sessions belong to different contexts");
  if (N_ != b.N_) throw std::runtime_error("ppals: the sessions differ in order");
  if (skip_mode < -1 || skip_mode >= N_) throw std::runtime_error("ppals: skip_mode out of range");
  if (R_ > Ops::kCongruenceMaxCols || b.R_ > Ops::kCongruenceMaxCols)
    throw Unsupported("ppals: the factor congruence supports at most 128 columns a session");
  Ops::CongruenceSide sa, sb;
  unsigned mask = 0;
  for (int i = 0; i < MAX_ORDER; i++) {
    const bool in = i < N_;
    sa.w[i] = in ? W_[i] : nullptr;
    sb.w[i] = in ? b.W_[i] : nullptr;
    sa.ld[i] = sa.rows[i] = in ? V_.glens[i] : 0;
    sb.ld[i] = sb.rows[i] = in ? b.V_.glens[i] : 0;
    if (in && i != skip_mode) {
      if (sa.rows[i] != sb.rows[i]) throw std::runtime_error("ppals: the sessions differ in a compared extent");
      mask |= 1u << i;
    }
  }
  sa.cols = R_;
  sb.cols = b.R_;
  const size_t n = (size_t)R_ * b.R_ + (size_t)R_ + (size_t)b.R_;
  fms_out_.reserve(ops_, sizeof(double) * n);
  double *dev = fms_out_.as<double>();
  const size_t wbytes = ops_.factor_congruence_work(N_, sa, sb);
  if (wbytes) fms_work_.reserve(ops_, wbytes);
  void *work = wbytes ? fms_work_.get() : nullptr;
  ops_.factor_congruence(N_, sa, sb, mask, work, dev, dev + (size_t)R_ * b.R_, dev + (size_t)R_ * b.R_ + R_);
  out.resize(n);
  ops_.d2h(out.data(), dev, sizeof(double) * n);
}

void CpEngine::fms_pairs(CpEngine &b, int skip_mode, bool weights, bool pairwise, double *fms, int *perm) {
  const StartTable ta = start_table(), tb = b.start_table();
  if (!pairwise && ta.nstarts != tb.nstarts) throw std::runtime_error("ppals: the numbers of starts differ");
  if (perm && (ta.nstarts != 1 || tb.nstarts != 1))
    throw std::logic_error("ppals: a matching is handed out for one pair of models");
  std::vector<double> h;
  congruence(b, skip_mode, h);
  const int Ca = R_, Cb = b.R_;
  const double *Phi = h.data(), *wa = Phi + (size_t)Ca * Cb, *wb = wa + Ca;
  for (int x = 0; x < ta.nstarts; x++)
    for (int y = pairwise ? 0 : x; y < (pairwise ? tb.nstarts : x + 1); y++) {
      double *dst = pairwise ? fms + x + (size_t)ta.nstarts * y : fms + x;
      if (!fms_from_congruence(Phi + ta.col[x] + (size_t)Ca * tb.col[y], Ca, wa + ta.col[x], wb + tb.col[y],
                               ta.rank(x), tb.rank(y), weights, perm, dst))
        throw std::runtime_error("ppals: internal error (a congruence that is not finite)");
    }
}

// ---------------------------------------------------------------------------- kernel-level access
static bool parse_range(const std::string &key, int N, int *lo, int *hi) {
  if (key.empty()) return false;
  *lo = key[0] - 'a';
  *hi = key.back() - 'a';
  if (*lo < 0 || *hi >= N || *hi - *lo + 1 != (int)key.size()) return false;
  for (size_t k = 0; k < key.size(); k++)
    if (key[k] != 'a' + *lo + (int)k) return false;
  return true;
}
int64_t CpEngine::tree_node(const std::string &key, double *out_host) {
  int lo, hi;
  if (!parse_range(key, N_, &lo, &hi)) return -1;
  int idx = find_node(lo, hi);
  if (idx < 0) return -1;
  for (auto &n : nodes_) n.valid = false;
  compute_node(idx);
  const Node &n = nodes_[idx];
  if (out_host) ops_.d2h(out_host, n.buf.as<double>(), sizeof(double) * (size_t)n.elems * R_);
  return n.elems * R_;
}
void CpEngine::mttkrp(int mode, double *M_host) {
  for (auto &n : nodes_) n.valid = false;
  compute_node(leaf_[mode]);
  const Node &lf = nodes_[leaf_[mode]];
  const int64_t s = V_.glens[mode];
  if (!dist_) {
    ops_.d2h(M_host, lf.buf.as<double>(), sizeof(double) * s * R_);
    return;
  }
  const int64_t blk = block_rows(s, P_);
  if (mode == 0) {
    ops_.zero(sendbuf_.as<double>(), sizeof(double) * blk * P_ * R_);
    // place the owner's complete rows into its block, then sum (other blocks are zero)
    double *mine = sendbuf_.as<double>() + (size_t)rank_ * blk * R_;
    for (int r = 0; r < R_; r++)
      ops_.d2d(mine + (size_t)r * blk, lf.buf.as<double>() + (size_t)r * ext(0), sizeof(double) * ext(0));
  } else {
    ops_.pack_blocks(lf.buf.as<double>(), s, s, R_, blk, P_, sendbuf_.as<double>());
  }
  comm_.allreduce_sum(sendbuf_.as<double>(), blk * P_ * R_);
  DeviceBuffer natbuf(ops_, sizeof(double) * s * R_);
  double *nat = natbuf.as<double>();
  ops_.unpack_blocks(sendbuf_.as<double>(), s, s, R_, blk, P_, nat);
  ops_.d2h(M_host, nat, sizeof(double) * s * R_);
}
void CpEngine::gram_system(int mode, double lambda, double *S_host, double *Sinv_host) {
  ops_.gram_system(G_.as<double>(), N_, mode, R_, lambda, S_.as<double>(), Sinv_.as<double>());
  ops_.d2h(S_host, S_.as<double>(), sizeof(double) * R_ * R_);
  ops_.d2h(Sinv_host, Sinv_.as<double>(), sizeof(double) * R_ * R_);
}

// ---------------------------------------------------------------------------- PP operators
// Build_mttkrp_map (als_CP.cxx:352-409): key = contracted modes in ascending order; built by
// dropping the last contracted mode. Level 1 scans V (K8), deeper levels contract the cache.
// Build_mttkrp_map (als_CP.cxx:385-390) derives the operator with the contracted modes `seq` from the
// one without seq's LAST mode, so every chain starts by contracting its lowest mode. Here the mode
// removed last is the SHORTEST of seq — the chain's level-1 tensor then contracts its longest mode and
// is the smallest possible (coil-100, 3 x 128 x 128 x 7200, R = 10: V x_a W_a is 3.3 x the tensor,
// 4.7 GB written once and read three times per build; V x_d W_d is 2 MB). Same operators, another
// association order; ties keep the reference's order, so equal extents change nothing.
int CpEngine::pp_last_mode(const std::string &seq) const {
  int best = seq.back() - 'a';
  for (int q = (int)seq.size() - 2; q >= 0; q--)
    if (ext(seq[q] - 'a') < ext(best)) best = seq[q] - 'a';
  return best;
}
std::string CpEngine::pp_parent(const std::string &seq) const {
  std::string p = seq;
  p.erase(p.find((char)('a' + pp_last_mode(seq))), 1);
  return p;
}

const CpEngine::PPOp &CpEngine::pp_get(const std::string &seq) {
  check_tensor_generation();
  auto it = pp_.find(seq);
  if (it != pp_.end()) return it->second;
  const int mode = pp_last_mode(seq);
  PPOp op;
  FactorRef f = fref(mode, W_.data());
  int64_t L = 1, T = 1;
  if (seq.size() == 1) {
    // level 1 = one tensor scan. Modes of the left half are contracted on the second resident
    // layout, where they sit behind the right half, so that EVERY level-1 scan is a
    // row-contiguous suffix-type scan; the s^(N-1) R result is kept in the tensor's precision.
    ScanPlan pl;
    if (!plan_scan(mode, 1, !(pp_fast_ && N_ >= 3), pl))
      throw std::runtime_error("ppals: internal error (single mode not adjacent)");
    L = pl.Lc;
    T = pl.T;
    op.modes = pl.kept;
    op.elems = L * T;
    // (at order 3 a level-1 result already IS a pair operator: those stay fp64 like all the others)
    op.dt = (pp_fast_ && N_ > 3) ? work_dt(V_.dtype) : F64;
    if (pp_fast_ && N_ > 3 && schedule_ == 1 && ms_k_ == 1 && ms_root_ == mode && ms_X_.valid &&
        ms_X_.dt == op.dt && !pp_no_borrow_) {
      // The exact sweep that ended just now left its first-level intermediate X = V x_mode W_mode
      // in the multi-sweep cache, and W_mode has not changed since (a step never updates its own
      // root; Normalize is the pending scalar): that IS this level-1 operator. One of the three
      // tensor scans of the build (als_CP.cxx:377-379) is already there.
      op.buf = ms_X_.buf;
      op.owned = false;
      op.scale = ms_scale_of(ms_X_);
      op.modes = ms_X_.modes;
    } else {
      op.buf = pp_buffer(seq, dtype_size(op.dt) * (size_t)(V_.nloc / ext(mode)) * R_);
      // (planned again: the allocation may have given a resident layout back)
      if (!plan_scan(mode, 1, !(pp_fast_ && N_ >= 3), pl))
        throw std::runtime_error("ppals: internal error (single mode not adjacent)");
      L = pl.Lc;
      T = pl.T;
      op.modes = pl.kept;
      ops_.scan_contract(pl.lay->ptr, V_.dtype, pl.L, ext(mode), T, &f, 1, R_, op.buf, op.dt, L,
                         op.elems, pl.pad);
    }
  } else {
    const PPOp &par = pp_get(pp_parent(seq));
    bool before = true;
    for (int m : par.modes) {
      if (m == mode) {
        before = false;
        continue;
      }
      (before ? L : T) *= ext(m);
      op.modes.push_back(m);
    }
    op.elems = L * T;
    op.buf = pp_buffer(seq, sizeof(double) * (size_t)op.elems * R_);
    ops_.mttv(par.buf, par.dt, L, ext(mode), T, &f, 1, R_, (double *)op.buf, op.elems, 0, par.scale);
  }
  pp_[seq] = op;
  return pp_[seq];
}
void CpEngine::pp_contract_pair(const PPOp &T, int cmode, const FactorRef &f, double *out,
                                int64_t out_rows) {
  if (T.modes.size() != 2 || T.dt != F64) throw std::runtime_error("ppals: not a pair operator");
  if (T.modes[0] == cmode)  // T[cmode, keep, r]
    ops_.mttv(T.buf, F64, 1, ext(cmode), ext(T.modes[1]), &f, 1, R_, out, out_rows, 1, nullptr);
  else  // T[keep, cmode, r]
    ops_.mttv(T.buf, F64, ext(T.modes[0]), ext(cmode), 1, &f, 1, R_, out, out_rows, 1, nullptr);
}
void CpEngine::pp_clear() { pp_.clear(); }  // the buffers stay in the pool
// Buffer of the operator `seq` from the grow-only pool. What the approximate sweeps read — the pair
// operators (N-2 modes contracted) and the full MTTKRPs — has a buffer of its own per key.
// Everything above them in the recursion of Build_mttkrp_map is scaffolding, read only while the
// operators below it are built; pp_build_all visits the keys in an order in which all users of a
// prefix are consecutive, so ONE buffer per level serves every scaffold of that level (order 4:
// one s^3 R level-1 tensor instead of three; order 6, s = 50, R = 6: 7.5 GB instead of 37.5 GB).
// A scaffold that takes the level's buffer over evicts the previous holder from the cache.
void *CpEngine::pp_buffer(const std::string &seq, size_t bytes) {
  const bool scaffold = (int)seq.size() < N_ - 2;
  const std::string key = scaffold ? "#" + std::to_string(seq.size()) : seq;
  if (scaffold) {
    for (auto it = pp_.begin(); it != pp_.end();) {
      if (it->first.size() == seq.size() && it->second.owned) {
        it = pp_.erase(it);
      } else {
        ++it;
      }
    }
  }
  DeviceBuffer &b = pp_pool_[key];
  if (b.size() < bytes) {
    b.reset();
    b = big_alloc(bytes);
  }
  return b.get();
}
static std::string all_but(int N, int i, int j = -1) {
  std::string s;
  for (int m = 0; m < N; m++)
    if (m != i && m != j) s.push_back((char)('a' + m));
  return s;
}
// als_CP.cxx:678-694: all pair operators, then all N full MTTKRPs
void CpEngine::pp_build_all() {
  struct Timer {  // (only while a caller asked for it: ppals_cp_pp_build_stats)
    CpEngine &e;
    double t0 = 0;
    explicit Timer(CpEngine &eng) : e(eng) {
      e.pp_builds_++;
      if (e.pp_build_timed_) {
        e.ops_.sync();
        t0 = now();
      }
    }
    ~Timer() {
      if (e.pp_build_timed_) {
        try {
          e.ops_.sync();
        } catch (...) {
        }
        e.pp_build_s_ += now() - t0;
      }
    }
  } timer(*this);
  pp_clear();
  // the pair operators in an order in which all users of a scaffold are consecutive (pp_buffer keeps
  // ONE buffer per scaffold level): sorted by their chain of ancestors, level 1 first
  std::vector<std::pair<std::string, std::string>> pairs;  // (chain, key)
  for (int ii = 0; ii < N_; ii++)
    for (int jj = ii + 1; jj < N_; jj++) {
      const std::string key = all_but(N_, ii, jj);
      std::string chain = key;
      for (std::string k = key; k.size() > 1;) {
        k = pp_parent(k);
        chain = k + "|" + chain;
      }
      pairs.emplace_back(chain, key);
    }
  std::stable_sort(pairs.begin(), pairs.end(),
                   [](const std::pair<std::string, std::string> &a, const std::pair<std::string, std::string> &b) {
                     return a.first < b.first;
                   });
  for (const auto &pk : pairs) pp_get(pk.second);
  for (int ii = 0; ii < N_; ii++) pp_get(all_but(N_, ii));
  // the approximate sweeps read the pair operators (N-2 modes contracted) and the full MTTKRPs
  // only; everything above them in the recursion was scaffolding — at order 6 that is 45 GB of
  // level-1 tensors
  for (auto it = pp_.begin(); it != pp_.end();) {
    if ((int)it->first.size() < N_ - 2) {
      it = pp_.erase(it);
    } else {
      ++it;
    }
  }
  // ... and its buffers go back to the device when they are large (above 2 GiB: below that, keeping
  // one per level saves the hipMalloc / hipFree of every phase)
  const size_t keep = (size_t)2 << 30;
  for (auto it = pp_pool_.begin(); it != pp_pool_.end();) {
    if (it->first[0] == '#' && it->second.size() > keep) {
      it = pp_pool_.erase(it);
    } else {
      ++it;
    }
  }
}
std::string CpEngine::placement_report() const {
  char buf[512];
  std::string out = "{\"mode\": ";
  out += ms_tune_enabled_ && ms_X_slack() > 0 ? "\"online\"" : "\"off\"";
  out += ", \"setup_s\": 0.0, \"candidate_blocks_held\": ";
  out += ms_X_alt_ ? "2" : "1";
  out += ", \"roots\": [";
  bool firstrow = true;
  for (int r = 0; r < N_; r++) {
    const PlaceExplore &ex = ms_place_[r];
    if (ex.phase < 0 || ex.phase == 3 || ex.cands.empty()) continue;
    const PlaceCand *c = ex.chosen >= 0 ? &ex.cands[ex.chosen] : nullptr;
    double best = 1e300;
    for (const auto &q : ex.cands)
      if (q.samples > 0) best = std::min(best, q.best);
    snprintf(buf, sizeof buf,
             "%s{\"root\": %d, \"layout\": \"%s\", \"settled\": %s, \"visits\": %d, \"block\": %d, \"offset_mb\": %lld, "
             "\"store\": \"%s\", \"best_ms\": %.4f, \"worst_ms\": %.4f, \"gated\": %s}",
             firstrow ? "" : ", ", r, ex.layout == 1 ? "second (transposed) copy" : "tensor",
             ex.phase == 2 ? "true" : "false", ex.visits, c ? c->blk : 0, c ? (long long)(c->off >> 20) : 0LL,
             !c || c->nt < 0 ? "by size" : (c->nt == 1 ? "non-temporal" : "ordinary"),
             best < 1e299 ? best * 1e3 : 0.0, ex.worst * 1e3, ex.gated ? "true" : "false");
    out += buf;
    firstrow = false;
  }
  out += "]";
  // packed twins of the layouts, one row per scan shape that asked for one
  out += ", \"packed\": {\"mode\": ";
  out += pack_mode_ == 0 ? "\"off\"" : (pack_mode_ > 0 ? "\"on\"" : "\"auto\"");
  out += ", \"refused\": \"" + pack_off_reason_ + "\", \"packed_scans\": " + std::to_string(ops_.scan_packed_launches()) +
         ", \"layouts\": [";
  for (size_t k = 0; k < packs_.size(); k++) {
    const PackedTwin &t = packs_[k];
    snprintf(buf, sizeof buf,
             "%s{\"layout\": \"%s\", \"rows\": %lld, \"reduced\": %lld, \"batches\": %lld, \"packed\": %s, "
             "\"bytes_per_element\": %.4f, \"format\": %d, \"escape_blocks\": %lld, \"reason\": \"%s\"}",
             k ? ", " : "", t.layout == 0 ? "tensor" : (t.layout == 1 ? "second (transposed) copy" : "padded copy"),
             (long long)t.L, (long long)t.J, (long long)t.T, t.data ? "true" : "false",
             t.data ? (double)t.bytes / ((double)t.L * (double)t.J * (double)t.T) : 4.0, t.format,
             (long long)t.escapes, t.reason.c_str());
    out += buf;
  }
  out += "]}}";
  return out;
}

int64_t CpEngine::pp_operator(const std::string &contracted, double *out_host) {
  for (size_t k = 0; k < contracted.size(); k++) {
    int m = contracted[k] - 'a';
    if (m < 0 || m >= N_ || (k > 0 && contracted[k] <= contracted[k - 1])) return -1;
  }
  if (contracted.empty() || (int)contracted.size() >= N_) return -1;
  pp_clear();
  // (never the borrowed multi-sweep intermediate here: it carries a Normalize factor that only the
  // contractions below it apply — this entry point hands the operator itself to the caller)
  struct Restore {  // (pp_get may throw: the flags must not outlive the call)
    CpEngine &e;
    bool fast;
    ~Restore() {
      e.pp_fast_ = fast;
      e.pp_no_borrow_ = false;
    }
  } restore{*this, pp_fast_};
  pp_no_borrow_ = true;
  const PPOp *op = &pp_get(contracted);
  if (op->dt != F64 || !std::is_sorted(op->modes.begin(), op->modes.end())) {
    // the entry point returns fp64 with the remaining modes ascending: rebuild on the plain route
    pp_clear();
    pp_fast_ = false;
    op = &pp_get(contracted);
  }
  if (out_host) ops_.d2h(out_host, op->buf, sizeof(double) * (size_t)op->elems * R_);
  int64_t n = op->elems * R_;
  pp_clear();
  return n;
}

// one approximate sweep: als_CP.cxx:754-825. Per mode: ONE launch for M = M_i^0 + the N-1
// first-order corrections, ONE for the whole mode update (which also leaves ||dW_i||^2); the
// Normalize launch leaves ||W_i||^2: the restart test of the next iteration costs no launch.
void CpEngine::sweep_pp(double lambda, double ratio) {
  // (the armed S / Normalize below are consumed by cp_mode_update, which a non-negative session never calls)
  if (nonneg()) throw Unsupported("ppals: a non-negative session has no pairwise-perturbation sweep");
  if (any_nonfree()) throw Unsupported("ppals: a session with constrained modes has no pairwise-perturbation sweep");
  ms_invalidate();  // PP moves the factors without touching the multi-sweep cache
  if (!Mbuf_) Mbuf_ = DeviceBuffer(ops_, sizeof(double) * (size_t)maxs_ * R_);
  if (!pp_norms_) {
    pp_norms_ = DeviceBuffer(ops_, sizeof(double) * 2 * MAX_ORDER);
    ops_.zero(pp_norms_.as<double>(), sizeof(double) * 2 * MAX_ORDER);
  }
  bool norm_fused = false;
  for (int i = 0; i < N_; i++) {
    const int64_t si = ext(i);
    const PPOp &M0 = pp_get(all_but(N_, i));
    PPTerm terms[MAX_ORDER];
    int nt = 0;
    for (int ii = 0; ii < N_; ii++) {
      if (ii == i) continue;
      const PPOp &T = pp_get(all_but(N_, std::min(i, ii), std::max(i, ii)));
      if (T.modes.size() != 2 || T.dt != F64) throw std::runtime_error("ppals: not a pair operator");
      FactorRef f = fref(ii, dW_.data());  // als_CP.cxx:785 / :793
      terms[nt].T = (const double *)T.buf;
      terms[nt].ny = ext(ii);
      terms[nt].keep_first = T.modes[0] == i ? 1 : 0;
      terms[nt].dW = f.ptr;
      terms[nt].lddw = f.ld;
      nt++;
    }
    // (S and S^-1 of this mode depend on the other modes' Grams only: a back end may prepare
    // them on the side of the correction's launch)
    ops_.arm_gram_system(G_.as<double>(), N_, i, R_, lambda, S_.as<double>(), Sinv_.as<double>());
    ops_.pp_correct((const double *)M0.buf, si, R_, terms, nt, Mbuf_.as<double>());
    if (i == N_ - 1 && !dist_) {  // Normalize at the tail of the sweep's last update launch
      int64_t rows[MAX_ORDER];
      for (int q = 0; q < N_; q++) rows[q] = V_.glens[q];
      norm_fused = ops_.arm_normalize(W_.data(), rows, N_, R_, G_.as<double>(), i, pp_norms_.as<double>() + 1);
    }
    mode_update(i, Mbuf_.as<double>(), si, lambda, true, ratio);
  }
  if (!norm_fused) {
    pp_norms_live_ = !dist_;
    normalize();
    pp_norms_live_ = false;
  }
  grad_from_sweep_ = true;
}

// ---------------------------------------------------------------------------- drivers
// print block: als_CP.cxx:166-213 / :457-498 / :697-752; bench: pp_bench's timings instead of the
// row (als_CP.cxx:203-209 / :735-748)
bool CpEngine::print_block(RunReport &rep, const CpOpts &o, int iter, int pp_flag, double &projnorm,
                           bool bench) {
  ops_.sync();  // the sweeps enqueued so far belong to [dtime]
  double diffV = 0;
  rep.off_clock([&] {
    projnorm = gradnorm();
    diffV = residual();
  });
  if (!bench)
    rep.row(iter, projnorm, pp_flag, diffV);
  else if (pp_flag)
    rep.pp_bench_time(iter, o.maxiter);
  else if (iter != 0)
    rep.dt_bench_time();
  return agree(projnorm < o.tol || rep.elapsed() > o.timelimit);
}

int CpEngine::run_dt(const CpOpts &o, int *iters) {
  RunReport rep(o, rank_ == 0, V_.glens[0], "gradnorm");
  double projnorm = 0;
  int iter;
  for (iter = 0; iter <= o.maxiter; iter++) {
    if (iter % o.resprint == 0 || iter == o.maxiter) {
      if (print_block(rep, o, iter, 0, projnorm, o.bench)) break;
    }
    sweep_dt(o.lambda);
    rep.dot(iter);
  }
  ops_.sync();
  rep.finish(iter, "proj-grad", projnorm);
  if (iters) *iters = iter;
  return iter == o.maxiter + 1 ? 0 : 1;
}

// ||dW_i|| and ||W_i|| for all modes. dt_phase: dW = W - W_prev, W_prev = W (als_CP.cxx:594-
// 603); otherwise dW as left by the PP updates (als_CP.cxx:659-663).
ModeNorms CpEngine::read_norms(bool dt_phase) {
  int64_t n[MAX_ORDER];
  for (int i = 0; i < N_; i++) n[i] = V_.glens[i] * R_;
  ops_.diff_norms(W_.data(), dt_phase ? Wprev_.data() : nullptr, n, N_, dt_phase, dW_.data(),
                  dt_phase, scal_.as<double>());
  return ModeNorms(ops_, scal_.as<double>(), N_);
}

void CpEngine::dt_sub(RunReport &rep, const CpOpts &o, double &projnorm, int &iter) {
  for (int i = 0; i < N_; i++)  // W_prev starts at zero (als_CP.cxx:428-431)
    ops_.zero(Wprev_[i], sizeof(double) * V_.glens[i] * R_);
  for (; iter <= o.maxiter; iter++) {
    if (iter % o.resprint == 0 || iter == o.maxiter) {
      if (print_block(rep, o, iter, 0, projnorm, false)) break;
    }
    sweep_dt(o.lambda);
    // iter is NOT incremented (als_CP.cxx:604-605)
    if (read_norms(true).count(o.tol_init, false) == N_) return;
    rep.dot(iter);
  }
}

// the restart point of a PP phase (als_CP.cxx:672-694): W_init = W, dW = 0, fresh operators
void CpEngine::pp_restart() {
  for (int j = 0; j < N_; j++) {
    size_t n = sizeof(double) * V_.glens[j] * R_;
    ops_.d2d(Winit_[j], W_[j], n);
    ops_.zero(dW_[j], n);
  }
  pp_build_all();
}

void CpEngine::pp_sub(RunReport &rep, const CpOpts &o, double &projnorm, int &iter) {
  const int init_iter = iter;
  rep.start_pp_phase();  // (bench: a phase restarted after 15 sweeps is called again)
  for (; iter <= o.maxiter; iter++) {
    int num_dw_break = 0;
    if (!o.bench) {
      // dW as the exact phase left it, later as the launches of the previous approximate sweep did
      const bool fused = iter != init_iter && !dist_ && pp_norms_.as<double>();
      const ModeNorms m = fused ? ModeNorms(ops_, pp_norms_.as<double>(), N_) : read_norms(false);
      num_dw_break = m.count(o.tol_init, true);
    }
    if ((iter - init_iter) % 15 == 0 || num_dw_break > 0) {
      if (num_dw_break > 0 || iter != init_iter) return;
      pp_restart();
    }
    if (iter % o.resprint == 0 || iter == o.maxiter || iter == init_iter) {
      if (print_block(rep, o, iter, 1, projnorm, o.bench)) break;
    }
    sweep_pp(o.lambda, o.ratio_step);
    rep.dot(iter);
  }
  if (o.bench) iter++;
}

// alsCP_PP_partupdate_sub (als_CP.cxx:852-1073): PP phase that updates only the modes with the
// largest relative MTTKRP perturbation ||dM_i|| / ||M_i|| and propagates every update to the other
// modes' dM through the cached pair operators. Sharded: dM_i (i != 0) is a partial sum, completed
// on a copy for its norm; M_i is completed in place by its own mode update.
void CpEngine::pp_partupdate_sub(RunReport &rep, const CpOpts &o, double &projnorm, int &iter) {
  const int init_iter = iter;
  std::vector<double> relpert(N_, 0.0);
  for (int i = 0; i < N_; i++) {
    size_t n = sizeof(double) * V_.glens[i] * R_;
    ops_.zero(dM_[i], n);
    ops_.zero(Mm_[i], n);
  }
  const int update_size = (int)(N_ * o.update_percentage);
  for (; iter <= o.maxiter; iter++) {
    const int num_dw_break = read_norms(false).count(o.tol_init, true);
    if ((iter - init_iter) % 15 == 0 || num_dw_break > 0) {
      if (num_dw_break > 0 || iter != init_iter) return;
      pp_restart();
    }
    if (iter % o.resprint == 0 || iter == o.maxiter || iter == init_iter) {
      // (rows under o.bench too: -pp 2 has no bench form)
      if (print_block(rep, o, iter, 1, projnorm, false)) break;
    }
    // sort_indexes (als_CP.cxx:835-843): descending, ties keep index order
    std::vector<int> idx(N_);
    for (int i = 0; i < N_; i++) idx[i] = i;
    std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return relpert[a] > relpert[b]; });
    if (rank_ == 0 && o.verbose) std::cout << "new round" << std::endl;
    ms_invalidate();
    for (int t = 0; t < update_size; t++) {
      const int i = idx[t];
      if (rank_ == 0 && o.verbose) std::cout << i << std::endl;
      const int64_t si = ext(i);
      const PPOp &M0 = pp_get(all_but(N_, i));
      ops_.d2d(Mm_[i], M0.buf, sizeof(double) * si * R_);
      ops_.add_inplace(Mm_[i], dM_[i], si * R_);
      mode_update(i, Mm_[i], si, o.lambda, true, o.ratio_step);
      ops_.zero(dM_[i], sizeof(double) * si * R_);
      for (int ii = 0; ii < N_; ii++) {  // propagate (als_CP.cxx:1036-1053)
        if (ii == i) continue;
        const PPOp &T = pp_get(all_but(N_, std::min(i, ii), std::max(i, ii)));
        FactorRef f = fref(i, dW_.data());
        pp_contract_pair(T, i, f, dM_[ii], ext(ii));
      }
    }
    for (int i = 0; i < N_; i++) {
      if (dist_ && i != 0) {
        // dM_i is a partial sum over this rank's rows of the sharded mode: complete a copy of it.
        // (Mm_i was completed in place by the all-reduce inside its own mode update.)
        ops_.d2d(sendbuf_.as<double>(), dM_[i], sizeof(double) * ext(i) * R_);
        comm_.allreduce_sum(sendbuf_.as<double>(), ext(i) * R_);
        ops_.sumsq(sendbuf_.as<double>(), ext(i) * R_, scal_.as<double>() + 2 * i);
      } else {
        ops_.sumsq(dM_[i], ext(i) * R_, scal_.as<double>() + 2 * i);
      }
      ops_.sumsq(Mm_[i], ext(i) * R_, scal_.as<double>() + 2 * i + 1);
    }
    // the sharded mode holds complete ROWS: its two sums of squares add up over the ranks
    if (dist_) comm_.allreduce_sum(scal_.as<double>(), 2);
    const ModeNorms m(ops_, scal_.as<double>(), N_);  // ||dM_i||, ||M_i||
    for (int i = 0; i < N_; i++) relpert[i] = m.d[i] / m.w[i];
    normalize();
    grad_from_sweep_ = true;
    rep.dot(iter);
  }
}

int CpEngine::run_pp(const CpOpts &o, int *iters) { return run_pp_common(o, iters, false); }
int CpEngine::run_pp_partupdate(const CpOpts &o, int *iters) {
  if (dist_) {
    // sharded: needs the plan in which every rank sees the complete s x R matrices
    for (int i = 0; i < N_; i++)
      if ((int64_t)sizeof(double) * V_.glens[i] * R_ > small_msg_bytes_)
        throw std::runtime_error(
            "ppals: -pp 2 on several GPUs needs s x R matrices below PPALS_COMM_SMALL_BYTES");
  }
  return run_pp_common(o, iters, true);
}

int CpEngine::run_pp_common(const CpOpts &o, int *iters, bool partupdate) {
  if (nonneg()) throw Unsupported("ppals: a non-negative session has no pairwise-perturbation driver");
  if (any_nonfree()) throw Unsupported("ppals: a session with constrained modes has no pairwise-perturbation driver");
  if (partupdate && rank_ == 0 && o.verbose) std::cout << "alsCP_PP_partupdate starts. " << std::endl;
  for (int i = 0; i < N_; i++) {
    size_t n = sizeof(double) * V_.glens[i] * R_;
    if (!Wprev_[i]) Wprev_.alloc(ops_, i, n);
    if (!Winit_[i]) Winit_.alloc(ops_, i, n);
    if (!dW_[i]) dW_.alloc(ops_, i, n);
    if (partupdate && !dM_[i]) dM_.alloc(ops_, i, n);
    if (partupdate && !Mm_[i]) Mm_.alloc(ops_, i, n);
    ops_.zero(dW_[i], n);
  }
  RunReport rep(o, rank_ == 0, V_.glens[0], "gradnorm");
  int iter = 0;
  double gradnorm_v = 10.;
  while (gradnorm_v > o.tol && iter <= o.maxiter) {
    if (!o.bench) {
      rep.starts("DT", iter);
      dt_sub(rep, o, gradnorm_v, iter);
    }
    rep.starts("pairwise perturbation", iter);
    if (partupdate)
      pp_partupdate_sub(rep, o, gradnorm_v, iter);
    else
      pp_sub(rep, o, gradnorm_v, iter);
    // deviation from the reference: a timelimit hit terminates instead of looping forever
    // (als_CP.cxx:1105 with breaks at :496 and :750)
    if (agree(rep.elapsed() > o.timelimit)) break;
  }
  ops_.sync();
  pp_clear();
  rep.finish(iter, "grad", gradnorm_v);
  if (iters) *iters = iter;
  return iter == o.maxiter + 1 ? 0 : 1;
}

}  // namespace ppals
