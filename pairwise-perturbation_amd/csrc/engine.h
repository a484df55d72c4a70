// engine.h — ALS sweep engine for CP (dimension tree + pairwise perturbation) written against the
// abstract Ops/Comm interfaces (ops.h). Pure host control flow: which contraction, which cache,
// which collective, when to restart — the part the reference implements in als_CP.cxx.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "device_buffer.h"
#include "ops.h"

namespace ppals {

struct TensorDesc {
  int order = 0;
  int64_t glens[MAX_ORDER];  // global extents
  int64_t llens[MAX_ORDER];  // local extents (differs from glens only in mode 0)
  int64_t row0 = 0;          // first leading-mode row owned by this rank
  int dtype = F32;
  void *data = nullptr;
  int64_t nloc = 0;
  // bumped by every fill / upload / imputation of the tensor (owned by the ppals_tensor handle; nullptr: the
  // contents never change). Sessions compare it with the generation their derived data (second
  // resident layout, cached contractions) was built from and rebuild when it moved.
  uint64_t *generation = nullptr;
  // bumped, beside the generation, by the calls that preprocess the contents in place (ppals_tensor_center / _shift /
  // _scale / _rescale): what follows is another data set, not the next iterate of the same one. A Tucker session
  // then also drops what it learnt from its earlier steps (warm-start slots of its eigen-steps, a multi-sweep
  // schedule it switched off), so that it goes on as a new session on the new contents would. nullptr: never.
  uint64_t *prep_epoch = nullptr;
};

// leading-mode block partition shared by the tensor shard and the factor-matrix row blocks
inline int64_t block_rows(int64_t s, int P) { return (s + P - 1) / P; }
// PPALS_FORCE_COMM=1: run the sharded code paths (pack, reduce-scatter, all-gather, all-reduce) even
// with one rank, so a single-GPU box exercises the RCCL plumbing end to end (tests only)
inline bool force_comm_path() {
  const char *v = getenv("PPALS_FORCE_COMM");
  return v && atoi(v) != 0;
}

// How a model export forms V - model (ppals_cp/tucker_export_model_device). Fused (the default): V is
// read inside the model kernel. Two passes: the tensor export into the destination, then destination -=
// model — possible only where that export rounds nothing (F32 / BF16 storage, or F64 into F64; else the
// fused form runs). Measured at the headline extents the fused form wins every case;
// PPALS_MODEL_RESIDUAL=two_pass keeps the other one reachable for that A/B. Read at session creation.
enum ResidualForm { RESIDUAL_FUSED = 0, RESIDUAL_TWO_PASS = 1 };
int residual_form_env();
// PPALS_TEST_SLICE_WORK_BYTES=n (tests): the cap of the partial sums of slice_residuals, 256 MB without it —
// so that small shapes reach the walk in slabs. Read at session creation.
size_t slice_work_cap_env();
// the model (or the residual) of the plan through the view: picks the residual's form, and for two
// passes runs the tensor export of the whole view `a` first (the plan may be one slab of it)
struct ModelExportCall {
  const ViewArgs *a;
  const TensorDesc *V;
  void *dst;
  bool residual;
  int form;          // ResidualForm
  bool exported = false;  // two passes: the view already holds V
  void *stream;
};
void model_export_run(Ops &ops, ModelExportCall &c, const ModelPlan &mp, const double *Q, const double *P,
                      int K);

int tensor_create(Ops &ops, Comm &comm, int order, const int64_t *glens, int dtype,
                  TensorDesc *out, std::string *err);
void tensor_fill_cp(Ops &ops, const TensorDesc &V, int R, const double *Wtrue_flat);
void tensor_fill_uniform(Ops &ops, const TensorDesc &V, uint64_t seed, double lo, double hi);
void tensor_upload(Ops &ops, const TensorDesc &V, const double *host_full);
void tensor_download(Ops &ops, const TensorDesc &V, double *host_full);
// `-tensor p/p2` (laplacian_tensor + fold_unfold, common.cxx:575-642,870-880): ndigits = -dim, s = -size
void tensor_fill_laplacian(Ops &ops, const TensorDesc &V, int ndigits, int s);
// `-tensor c` (Gen_collinearity + noise, common.cxx:361-423, test_ALS.cxx:246-264)
void collinear_factors(const int64_t *lens, int N, int R, double col_min, double col_max,
                       uint64_t seed, double *Wflat);
void tensor_fill_collinear(Ops &ops, Comm &comm, const TensorDesc &V, int R, double col_min,
                           double col_max, double ratio_noise, uint64_t seed);
double tensor_norm(Ops &ops, Comm &comm, const TensorDesc &V);
// Preprocessing in place (ppals_tensor_center / _shift / _slice_sumsq / _scale / _rescale; one rank): the tensor
// viewed as [L, J, T] around `mode`, J = lens[mode], L / T the products of the extents before / after it.
struct PrepShape {
  int64_t L = 1, J = 1, T = 1;
};
PrepShape prep_shape(const TensorDesc &V, int mode);
// V[l,j,t] -= mean_j V[l,.,t]; offsets (device, L*T doubles, may be nullptr) receives the means
void tensor_center(Ops &ops, const TensorDesc &V, int mode, double *offsets_dev);
// V[l,j,t] += alpha * offsets[l + L*t] (device)
void tensor_shift(Ops &ops, const TensorDesc &V, int mode, const double *offsets_dev, double alpha);
// ss[x] = sum over slice x of V^2, on the host
void tensor_slice_sumsq(Ops &ops, const TensorDesc &V, int mode, double *ss_host);
// slice x multiplied by factors[x] (host)
void tensor_rescale(Ops &ops, const TensorDesc &V, int mode, const double *factors_host);
// rms[x] = sqrt(ss[x] / n); slice x multiplied by 1 / rms[x] unless rms[x] is not a positive finite number (the
// slice then stays bit for bit); rms_host (lens[mode] doubles, may be nullptr) receives rms as computed
void tensor_scale(Ops &ops, const TensorDesc &V, int mode, double *rms_host);

// N-PLS regression (ppals_npls_fit / _predict; Bro, J. Chemometrics 10 (1996) 47-61; one rank). The tensor is only
// read, through Ops::npls_contract / npls_slice_inner on its primary layout: the deflated tensor is never formed.
// Z[l,t,c] = sum_i X[l,i,t] U[i,c] and S[i,c] = sum_{l,t} X[l,i,t] W[l,t,c] with host arrays (column-major)
void tensor_contract_mode(Ops &ops, const TensorDesc &V, int mode, const double *U_host, int C, double *Z_host);
void tensor_slice_inner(Ops &ops, const TensorDesc &V, int mode, const double *W_host, int C, double *S_host);
struct NplsOpts {
  double hopm_tol = 1e-12;
  int hopm_max = 500;
  double inner_tol = 1e-12;
  int inner_max = 200;
};
// everything on the host, column-major; nf <= F components were fitted (a zero or non-finite Z ends the fit)
struct NplsModel {
  int order = 0, mode = 0, M = 0, F = 0, nf = 0;
  int64_t lens[MAX_ORDER];             // the training extents
  std::vector<double> T, U;            // I x nf: scores of X and of Y
  std::vector<std::vector<double>> W;  // the order - 1 modes off the sample mode, in order: lens x nf, unit columns
  std::vector<double> Q, B;            // M x nf; nf x nf, upper triangular
  std::vector<double> ssx, ssy;        // nf: explained variation, cumulative (ssx is a difference: it loses
                                       // digits when the residual is tiny)
  std::vector<int> status;             // nf: bit 0 HOPM ran into hopm_max, bit 1 the loop over q into inner_max
  int64_t slice_size() const {
    int64_t n = 1;
    for (int i = 0; i < order; i++)
      if (i != mode) n *= lens[i];
    return n;
  }
};
void npls_fit(Ops &ops, const TensorDesc &X, int mode, const double *Y, int M, int F, const NplsOpts &o,
              NplsModel *out);
// Yhat: Inew x M from the first ncomp components; Tnew: Inew x ncomp (may be nullptr)
void npls_predict(Ops &ops, const NplsModel &m, const TensorDesc &Xnew, int ncomp, double *Yhat, double *Tnew);
// The two passes through Ops::npls_contract_wide / npls_slice_inner_wide (ppals_tensor_contract_columns /
// _slice_inner_columns): the layouts of the calls above, deterministic, not bit-equal to them.
void tensor_contract_columns(Ops &ops, const TensorDesc &V, int mode, const double *U_host, int C, double *Z_host);
void tensor_slice_inner_columns(Ops &ops, const TensorDesc &V, int mode, const double *W_host, int C, double *S_host);
// Leave-segments-out cross-validation of N-PLS (ppals_npls_crossval; DESIGN.md §3, "Cross-validation"): the S
// resampled fits run in groups of G that share every pass over X. G is the largest count with G M <= kNplsCvColumns
// columns (what one read of X carries in the wide ops) and a working set of G (M + 2) fp64 slices within kNplsCvBytes.
constexpr int kNplsCvColumns = 64;
constexpr int64_t kNplsCvBytes = (int64_t)2 << 30;
int npls_crossval_group(int64_t LT, int M, int S);
// segment: I labels in [0, S); Ycv: I x M x F; press: F x M, fitted: S, status: S x F, x_passes (each may be nullptr)
void npls_crossval(Ops &ops, const TensorDesc &X, int mode, const double *Y, int M, int F, const int32_t *segment, int S,
                   int center, const NplsOpts &o, double *Ycv, double *press, int *fitted, int *status,
                   int64_t *x_passes);

struct CpOpts {
  double tol = 0, timelimit = 5e3;
  int maxiter = 0;
  double lambda = 0;
  int resprint = 10;
  int bench = 0;
  double tol_init = 1e-2, ratio_step = 1.0;
  double update_percentage = 1.0;  // -pp 2: fraction of the modes updated per PP sweep
  int update_rank = 0;             // class API, low-rank-update optimizers (run.cxx -updaterank)
  int randomsvd = 0;               // ... and their randomized range finder (run.cxx -randomsvd)
  std::string csv_path;
  bool csv_append = false;
  bool verbose = false;
};

class RunReport;
struct ModeNorms;

class CpEngine {
 public:
  // nstarts > 1 (or multi): a multi-start session — `nstarts` independent rank-R models share every
  // contraction of the sweep. The factor matrices hold nstarts * R columns, start-major (start b owns
  // columns [b R, (b+1) R)); only the R x R normal equations know about starts. One rank only.
  // ranks != nullptr (a rank sweep): start b is a rank-ranks[b] model and owns the columns
  // [col_b, col_b + ranks[b]), col_b = sum_{c<b} ranks[c]; R is ignored. Scans, leaves and schedules work on
  // the R_ columns in total and know nothing of this. A session whose ranks are all equal — however it
  // was created — takes exactly the batched ops of nstarts x R; only differing ranks take the ragged ops.
  CpEngine(Ops &ops, Comm &comm, const TensorDesc &V, int R, int nstarts = 1, bool multi = false,
           const int *ranks = nullptr);
  ~CpEngine();

  void set_factors(const double *Wflat, const double *gradWflat);
  void set_schedule(int schedule);
  // Non-negative CP: every mode update is one HALS pass (Ops::cp_mode_update_nn; all starts of a
  // multi-start session in one Ops::cp_mode_update_nn_batched) instead of the solve.
  // Exact sweeps and what is built on them (run_dt, run_class 0-2, run_em, run_multi) work unchanged; PP,
  // the low-rank optimizers, more than one rank and R > 64 per start throw Unsupported.
  void set_nonneg(bool on);  // all modes kModeNonneg, or all modes kModeFree
  bool nonneg() const {      // every mode is kModeNonneg
    for (int i = 0; i < N_; i++)
      if (kind_[i] != kModeNonneg) return false;
    return true;
  }
  // downloads the factors (of all starts) of the modes of `modes` (bit i: mode i): every entry finite and >= 0
  bool factors_nonneg(unsigned modes = ~0u);
  // Per-mode constraints (include/ppals.h, PPALS_MODE_*): the update of mode i is the solve (kModeFree), one
  // HALS pass (kModeNonneg), nothing at all (kModeFixed: no leaf contraction either; its gradient is
  // zeroed here and stays zero) or the orthonormal polar factor of the MTTKRP (kModeOrtho,
  // Ops::cp_mode_update_ortho_ragged). One kind per mode, shared by all starts of a multi-start session.
  // Everything that cannot run that way is refused before anything is launched or changed: Unsupported
  // for more than one rank, the blocked-update test hook, NONNEG / ORTHO at a start rank above 64 and a
  // FIXED / ORTHO hold-out mode; std::invalid_argument for a kind outside 0..3 and ORTHO on a mode shorter
  // than a start's rank. Factors, Grams and caches are untouched.
  void set_mode_kinds(const int *kinds);
  // the refusals of set_mode_kinds, nothing changed: 0 fine, 1 a bad argument, 2 unsupported; *why says which
  int check_mode_kinds(const int *kinds, std::string *why) const;
  // the kinds as they were a moment ago (set_nonneg taken back by the C ABI): no check, nothing zeroed
  void restore_mode_kinds(const int *kinds) {
    for (int i = 0; i < N_; i++) kind_[i] = kinds[i];
  }
  int mode_kind(int i) const { return kind_[i]; }
  // Shapes (include/ppals.h, PPALS_SHAPE_*): a NONNEG mode whose shape is not kShapeNone is updated by
  // Ops::cp_mode_update_shape_ragged through start_table() — one path for ordinary, multi-start and rank-sweep
  // sessions — instead of the HALS pass; a mode of shape kShapeNone takes exactly the launches it took before.
  // Refused before anything changes: std::invalid_argument for a shape outside 0..3 and for a shape on a mode
  // that is not NONNEG, Unsupported for a shape on the hold-out mode (zeroed rows break any shape). Factors,
  // Grams and caches are untouched. set_mode_kinds and set_nonneg drop the shape of a mode that ends up not
  // NONNEG (a set_nonneg the C ABI takes back had turned every mode NONNEG and so dropped none).
  void set_mode_shapes(const int *shapes);
  int check_mode_shapes(const int *shapes, std::string *why) const;  // 0 fine, 1 a bad argument, 2 unsupported
  int mode_shape(int i) const { return shape_[i]; }
  bool all_free() const { return !any_nonfree(); }
  bool any_nonfree() const {
    for (int i = 0; i < N_; i++)
      if (kind_[i] != kModeFree) return true;
    return false;
  }
  // Normalize would rescale a FIXED factor and destroy orthonormal columns: sweeps of such a session end
  // without it (a positive scaling keeps FREE and NONNEG)
  bool skips_normalize() const {
    for (int i = 0; i < N_; i++)
      if (kind_[i] == kModeFixed || kind_[i] == kModeOrtho) return true;
    return false;
  }
  // take_from: a mode that is NONNEG here must be NONNEG in the multi-start session `src`
  bool takes_nonneg_from(const CpEngine &src) const {
    for (int i = 0; i < N_ && i < src.N_; i++)
      if (kind_[i] == kModeNonneg && src.kind_[i] != kModeNonneg) return false;
    return true;
  }
  unsigned nonneg_modes() const {
    unsigned m = 0;
    for (int i = 0; i < N_; i++)
      if (kind_[i] == kModeNonneg) m |= 1u << i;
    return m;
  }
  int schedule() const { return schedule_; }
  // one JSON object: where the online placement choice put every root's first-level intermediate
  // (block, offset, store kind, fastest / slowest sample, settled or still exploring)
  std::string placement_report() const;
  // operator builds of the PP phases (Build_mttkrp_map, als_CP.cxx:678-694): how many, and — while
  // timing is on (a stream synchronisation on both sides of a build) — how long they took
  void pp_build_stats(int mode, int64_t *builds, double *seconds) {
    if (builds) *builds = pp_builds_;
    if (seconds) *seconds = pp_build_s_;
    if (mode != 0) {
      pp_builds_ = 0;
      pp_build_s_ = 0;
      pp_build_timed_ = mode > 0;
    }
  }
  void get_factors(double *Wflat, double *gradWflat);

  // body of the reference's sweep loop: als_CP.cxx:215-303 (clear cache, N mode updates,
  // Normalize). Asynchronous on the Ops stream.
  void sweep_dt(double lambda);
  double gradnorm();  // sqrt(sum_i ||grad_W[i]||^2), als_CP.cxx:174-181; synchronises
  double residual();  // ||V - [[W]]||_F, als_CP.cxx:183-187; synchronises
  // the model [[W]] (residual: V - [[W]], V as stored) into this rank's rows of a checked export view
  // (ppals_cp_export_model_device); reads the session, changes nothing of it
  void export_model(const ViewArgs &a, void *dst, bool residual, void *stream);
  // The missing entries (mask byte 0) of this rank's rows of a checked U8 import view `a` at `mask`
  // become the model [[W]], rounded once to the storage type; everything else of the tensor stays bit
  // for bit (ppals_cp_impute_device). Bumps the tensor's generation; the session's factors, Grams and
  // gradients do not change. observed_sq == nullptr: asynchronous; otherwise *observed_sq = the sum of
  // (V - model)^2 over the observed entries of the box, all ranks, and the call waits for it.
  void impute(const ViewArgs &a, const void *mask, void *stream, double *observed_sq);
  // EM with missing entries (ppals_cp_em): repeat { impute; inner_sweeps exact sweeps }, the observed
  // residual looked at every o.resprint iterations; one last impute with the residual on the way out.
  // Returns 1 if a look found the residual <= o.tol.
  int run_em(const ViewArgs &a, const void *mask, void *stream, const CpOpts &o, int inner_sweeps,
             int *iters, double *observed_res);
  // The majorization step of weighted CP (ppals_cp_wls_device): every element of this rank's rows of the
  // box becomes x, the model, or fma(h, x - model, model) by its weight h, rounded once to the storage type;
  // `a` / `w`: checked import views of one box (F32 or F64, the same type) at `data` / `weights`. Bumps the
  // tensor's generation; factors, Grams and gradients do not change. weighted_sq == nullptr: asynchronous;
  // otherwise *weighted_sq = the weighted loss over the box, all ranks, and the call waits for it.
  void wls_step(const ViewArgs &a, const void *data, const ViewArgs &w, const void *weights, void *stream,
                double *weighted_sq);
  // why this session's tensor or rank admits no weighted step (BF16 storage, R > 128), or nullptr
  const char *wls_refusal() const;
  // ppals_cp_wls: repeat { wls_step; inner_sweeps exact sweeps }, the looks and the last step as run_em.
  // Returns 1 on tol, 2 when the weighted residual fell by no more than rel_change of the look before.
  int run_wls(const ViewArgs &a, const void *data, const ViewArgs &w, const void *weights, void *stream,
              const CpOpts &o, int inner_sweeps, double rel_change, int *iters, double *weighted_res);
  // The Huber step (ppals_cp_huber_device): wls_step with the residual clipped to [-c, c], c > 0 (+inf: the
  // weighted step's bits and loss). w == nullptr: no weights view, h = 1. huber_loss / clipped (either may be
  // nullptr; both nullptr: asynchronous): sum h rho_c(x - m) and the number of elements with |x - m| > c, all ranks.
  void huber_step(const ViewArgs &a, const void *data, const ViewArgs *w, const void *weights, void *stream, double c,
                  double *huber_loss, int64_t *clipped);
  // ppals_cp_robust: run_wls with the Huber step at a fixed c; *robust_res = sqrt(the Huber loss).
  int run_robust(const ViewArgs &a, const void *data, const ViewArgs *w, const void *weights, void *stream, double c,
                 const CpOpts &o, int inner_sweeps, double rel_change, int *iters, double *robust_res);
  // ppals_cp_abs_residual_quantile: *count = the elements of the box with h > 0 (w == nullptr: all), *value =
  // the k-th smallest (float)|x - m| among them, k = min(n - 1, max(0, ceil(p n) - 1)), NaN last; NaN if there
  // are none. Reads the factors and the views only (any storage type); waits for the result.
  const char *quantile_refusal() const;  // R > 128, more than one rank; or nullptr
  void abs_residual_quantile(const ViewArgs &a, const void *data, const ViewArgs *w, const void *weights,
                             void *stream, double p, double *value, int64_t *count);
  // PARAFAC2 (ppals_parafac2_*): the owner's projection step reads this session's factors on the device
  // (mode i: glens[i] x R, column-major) and drives { step; sweeps } through the loop of run_wls, `step`
  // in the weighted step's place (it hands back the quantity looked at when its argument is not nullptr).
  const double *factor_device(int i) const { return W_[i]; }
  int run_steps(const std::function<void(double *)> &step, const CpOpts &o, int inner_sweeps, double rel_change,
                int *iters, double *res);
  const TensorDesc &tensor() const { return V_; }
  // The core consistency diagnostic (Bro & Kiers 2003; include/ppals.h): per start b, with
  // P_i = W_i (W_i^T W_i)^-1 of its current factors, the core G_b = V x_0 P_0^T ... x_{N-1} P_{N-1}^T
  // (R_b^N entries) and cc_b = 100 (1 - sum (G_b - T)^2 / R_b). `only` = -1: every start (an ordinary
  // session is one start), cc_host[nstarts]; `only` = b: that start alone, cc_host[1]. core_host (may be
  // nullptr; one start only): that start's core, first index fastest. The first contraction of all selected
  // starts is ONE tensor scan; the rest works start by start on its column block of the result. Reads the
  // session and changes nothing of it: the buffers are the call's own (grow-only, kept). Synchronises.
  void core_consistency(int only, double *cc_host, double *core_host);
  // R_b^N of a start, or a number above kCoreMaxEntries when it exceeds that
  static constexpr int64_t kCoreMaxEntries = (int64_t)1 << 24;
  int64_t core_entries(int start) const;
  // The factor congruence and the factor match score (include/ppals.h): all columns of this session (side
  // a: every start of a multi-start session, side by side as the column table says) against all columns
  // of `b` — another session of the same context and order, or this one. skip_mode = -1 compares every
  // mode, 0 <= skip_mode < N all but that one. ONE Ops::factor_congruence and one download of
  // Phi (Ca x Cb), w_a (Ca), w_b (Cb) into `out`, in this order. Reads both sessions and changes nothing of
  // them; the buffers are the call's own, grow-only, kept by this session. Synchronises.
  void congruence(CpEngine &b, int skip_mode, std::vector<double> &out);
  // the scores of starts from one such download, matched on the host (assignment.h), each start with its
  // own rank. pairwise: fms[a + K * b] for every start a of this session and b of `b` (K = nstarts());
  // otherwise fms[k] of start k against start k (equal numbers of starts). perm (may be nullptr; ordinary
  // sessions only): rank_r() ints, the matched column of b or -1.
  void fms_pairs(CpEngine &b, int skip_mode, bool weights, bool pairwise, double *fms, int *perm);
  int64_t mode_extent(int i) const { return V_.glens[i]; }
  // The influence plot of an ordinary session (Bro 1997; include/ppals.h). Both lay their N vectors out one
  // after the other, mode 0's s_0 values first. They read the session and change nothing of it; the buffers
  // are the calls' own (grow-only, kept). Synchronise. One rank, no multi-start session.
  //   slice_residuals: ss_i[x] = the sum of (V - [[W]])^2 over the slice x of mode i, of exactly the model
  //     residual() measures (the same operands); *total_host (may be nullptr) = the sum over everything. ONE
  //     pass over the tensor (Ops::residual_slices: the sums over the rows and the columns of the M x K
  //     split), then one fold of each marginal onto its modes (Ops::fold_slice_sums).
  //   leverages: lev_i[x] = w^T (W_i^T W_i)^-1 w, w = row x of W_i, from the pseudo-inverse factors of the
  //     core consistency (Ops::cp_pinv_ragged, Ops::row_dots); all NaN when a Gram has no such inverse. The
  //     tensor is not read.
  void slice_residuals(double *ss_host, double *total_host);
  void leverages(double *lev_host);

  // kernel-level access for parity tests
  int64_t tree_node(const std::string &key, double *out_host);
  void mttkrp(int mode, double *M_host);
  int64_t pp_operator(const std::string &contracted, double *out_host);
  void gram_system(int mode, double lambda, double *S_host, double *Sinv_host);

  // drivers
  int run_dt(const CpOpts &o, int *iters);  // alsCP_DT, als_CP.cxx:127-320
  int run_pp(const CpOpts &o, int *iters);  // alsCP_PP, als_CP.cxx:1082-1137
  int run_pp_partupdate(const CpOpts &o, int *iters);  // alsCP_PP_partupdate, als_CP.cxx:1146-1207
  // CPD<dtype,Optimizer>::als, src/CP.cxx:100-186; kind 0 Simple, 1 DT, 2 MSDT optimizer
  int run_class(int kind, const CpOpts &o, double *sweeps, int *iters);
  void update_modes(int first, int count, double lambda);


  // ---- multi-start sessions (start = -1: every start, concatenated start-major) ----
  bool is_multi() const { return multi_; }
  int nstarts() const { return K_; }
  int start_rank() const { return Rs_; }  // the largest start's rank (every start's, when they are equal)
  int start_rank(int b) const { return multi_ ? tab_.rank(b) : R_; }
  void set_factors_start(int start, const double *Wflat, const double *gradWflat);
  void get_factors_start(int start, double *Wflat, double *gradWflat);
  void gradnorms(double *out);  // [nstarts], each what gradnorm() of a session of that start returns
  void residuals(double *out);  // [nstarts], each ||V - [[W_b]]||_F; synchronises
  // start `start` of the multi session `src` (same tensor, same R) becomes this ordinary session's
  // factors and gradients, device to device; otherwise the effect of set_factors
  void take_from(CpEngine &src, int start, bool predicted = false);
  // sweeps until maxiter / timelimit / the best start's gradient norm < tol (looked at every resprint
  // sweeps); returns 1 if it stopped before maxiter sweeps
  int run_multi(const CpOpts &o, int *sweeps, int *best);
  // Hold-out rows of ONE mode, per start (include/ppals.h): keep[b * s_mode + x] == 0 holds row x of W_mode
  // out of start b — it is 0 in the factor and the gradient whenever another mode reads them, so start b
  // evolves as a session on the tensor without those slices does, and what the update of `mode` computes
  // for the row (its least-squares score under that model) is moved to the scores buffer right behind the
  // update (Ops::cp_hold_rows: one launch; starts that hold nothing out are not touched). Setting it moves
  // the rows as they are now and drops the cached contractions; keep == nullptr clears it: the zero rows
  // stay until the next update of the mode. Every start keeps at least one row (checked).
  void set_holdout(int mode, const uint8_t *keep);
  int holdout_mode() const { return hold_mode_; }  // -1: none
  const std::vector<uint8_t> &holdout_keep() const { return hold_keep_; }
  void heldout_scores(int start, double *out);  // s_mode x rank(start), column-major; kept rows 0
  // take_from with the scores added into the held-out rows of the sample mode's factor (W + scores: the rows
  // are disjoint)
  void take_predicted_from(CpEngine &src, int start) { take_from(src, start, true); }

  int order() const { return N_; }
  int rank_r() const { return R_; }

 private:
  struct Node {
    int lo, hi;
    int parent = -1;   // index into nodes_, -1: parent is the root
    int slo, shi;      // sibling range
    DeviceBuffer buf;
    int64_t elems = 0;  // without the rank index
    bool valid = false;
  };
  struct PPOp {
    void *buf = nullptr;
    int dt = F64;            // level-1 operators are kept in the tensor's own precision
    int64_t elems = 0;
    std::vector<int> modes;  // remaining modes in STORAGE order (first fastest)
    bool owned = true;       // true: buf lies in pp_pool_; false: borrowed from the multi-sweep cache
    const double *scale = nullptr;  // pending Normalize factor of a borrowed tensor (device scalar)
  };
  // grow-only pool of the PP operator buffers: a PP phase re-uses the buffers of the previous one
  // instead of allocating / freeing ~1 GB of operators around every phase. Keyed by operator for
  // what the approximate sweeps read, by LEVEL ("#1", "#2", ...) for the scaffolding above it
  std::map<std::string, DeviceBuffer> pp_pool_;
  void *pp_buffer(const std::string &seq, size_t bytes);
  bool pp_norms_live_ = false;  // Normalize is asked for ||W_i||^2 (inside sweep_pp)
  DeviceBuffer pp_norms_;  // [2N]: ||dW_i||^2, ||W_i||^2 left by the fused PP mode updates

  // a cached intermediate of the multi-sweep schedule: modes in storage order (first fastest),
  // rank index last; `scale` (device scalar) is the Normalize factor still owed to its contents
  struct RTensor {
    void *buf = nullptr;  // a view: into own / tmp_own of its MsNode, a placement block or an lr_cache_
    int dt = F64;
    std::vector<int> modes;
    unsigned contracted = 0;
    int slot = -1;         // index into ms_scales_ (device scalars)
    bool pending = false;  // a Normalize happened after this tensor was built: scale is owed
    bool valid = false;
  };
  struct MsNode {
    int lo, hi, parent, slo, shi;  // ranges over positions of the step's cyclic mode list
    RTensor t;
    std::vector<RTensor> tmp;
    DeviceBuffer own;                   // the storage of t
    std::vector<DeviceBuffer> tmp_own;  // ... and of tmp[k]
  };
  void ms_build_tree(int lo, int hi, int parent);
  void ms_start_step(int root);
  void ms_compute(int idx);
  void ms_contract(const RTensor &src, int mode, RTensor &dst, DeviceBuffer &own, const double *in_scale);
  void sweep_msdt(double lambda);
  void ms_invalidate() { ms_root_ = -1; }
  int schedule_ = 1;  // 1: multi-sweep dimension tree (default), 0: the reference's two-node tree
  int ms_root_ = -1;  // first mode of the running step's root set (-1: no step)
  int ms_k_ = 1;      // modes contracted by one first-level scan (ms_choose_roots)
  // modes that are never part of a root set: the partitioned mode 0 of a sharded session (its X would
  // be a partial sum of global size) and modes so short that X = V x_m W_m is no smaller than the tensor
  // (extent 3 at R = 10: X is 3.3 x the tensor — the reference's coil-100 / time-lapse shapes). The root
  // set is slid back past them (ms_next_root); the cost model prices both (ms_schedule_cost).
  int test_blocks_ = 0;            // PPALS_TEST_BLOCKED_UPDATE (test hook, see mode_update)
  DeviceBuffer test_blkbuf_;
  unsigned ms_excl_ = 0;
  bool ms_set_excluded(int first, int k, unsigned excl) const;
  int ms_next_root(int i, int k, unsigned excl) const;  // first mode of the root set that serves update i, -1: none
  double ms_schedule_cost(int k, unsigned excl) const;  // tensor-scan equivalents per sweep, 1e300: not schedulable
  int ms_choose_roots();
  void ms_set_roots(int k);
  void ms_mode_update(int i, double lambda, bool last_of_sweep = false);
  bool ms_norm_fused_ = false;  // the sweep's Normalize went into its last update launch (Ops::arm_normalize)
  unsigned ms_collect_scales(unsigned *masks, unsigned *fresh, int skip_node);
  RTensor ms_X_;
  // Placement of the first-level intermediate: the scan reads the tensor and writes X at the same
  // time, and how the two streams fall onto the HBM channels depends on where X lies relative to
  // the tensor buffer — 6-9 % of the launch between placements of one and the same kernel
  // (profiles/r02l_place_bench_*.txt) — and on the kind of store. X lives at a per-root offset
  // inside one of TWO blocks over-allocated by a slack of 64 MB — one taken before the session's
  // second resident layout, one after it, so that they lie several GB apart at no cost (which block
  // suits which source is a property of the pair, profiles/r03_place_regions.md). Block, offset and
  // store kind are found ONLINE: the first visits of a root run the sweep's REAL scan at one candidate each, timed
  // by a pair of events on the stream (Ops::timer_*), read when the root comes round again; after
  // ~24 visits the root keeps the fastest; a block no root chose is freed. No trial launches, no
  // set-up time, the results do not depend on where X lies. PPALS_PLACE_TUNE=0: one block, offset 0,
  // store kind by size.
  struct PlaceCand {
    int blk = 0;           // 0: the block allocated behind the second resident layout, 1: the one in front of it
    int64_t off = 0;
    int nt = -1;           // store kind: -1 the back end's rule, 0 ordinary, 1 non-temporal
    double best = 1e300;   // fastest sample, seconds
    int samples = 0;
  };
  struct PlaceExplore {
    int phase = -1;        // -1 not started, 0 offsets, 1 finalists x store kinds, 2 settled, 3 not worth it
    size_t next = 0;       // candidate of the next visit
    int timer = -1;        // stopwatch of the visit in flight (Ops::timer_begin)
    int timer_cand = -1;
    int chosen = -1;
    int layout = 0;        // which resident layout the root's scan reads
    double worst = 0;      // slowest sample seen, seconds
    int visits = 0;
    bool gated = false;    // settled early: the candidates' spread was inside the gate (ms_place_pick)
    std::vector<PlaceCand> cands;
  };
  static constexpr int kPlaceGateSamples = 8;       // samples of a root before the gate is consulted
  static constexpr double kPlaceGateSpread = 0.04;  // fastest / slowest candidate closer than this: stop
  PlaceExplore ms_place_[MAX_ORDER];
  void ms_place_collect(PlaceExplore &ex);
  int ms_place_pick(PlaceExplore &ex);
  DeviceBuffer ms_X_base_;
  DeviceBuffer ms_X_alt_;  // the second candidate block, as large as the first (empty: none / released)
  void ms_place_release_unchosen();
  int64_t pp_builds_ = 0;
  double pp_build_s_ = 0;
  bool pp_build_timed_ = false;
  bool ms_tune_enabled_ = true;
  size_t ms_X_slack() const;
  static double place_min_bytes();
  size_t ms_X_bytes(int first, int k) const;
  DeviceBuffer big_alloc(size_t bytes);  // gives optional resident layouts back when the device is full
  std::vector<MsNode> ms_nodes_;
  // ---- low-rank-update optimizers of the class API (CPDTLROptimizer / CPMSDTLROptimizer,
  // src/optimizer/cp_dt_lr_optimizer.cxx, cp_msdt_lr_optimizer.cxx; randomsvd = 0). The first
  // contraction of a step, V x_left W_left, is KEPT per root (lr_cache_) and, when W_left has
  // changed by a rank-r update Us * VT only, brought up to date with r tensor columns instead of
  // R: cached += (V x_left Us) * VT.
  void lr_step_begin(int left, bool reuse, int r);
  void lr_mode_update(int i, double lambda, int r, const double *base);
  void lr_release();
  DeviceBuffer lr_cache_[MAX_ORDER];
  bool lr_have_[MAX_ORDER] = {false};
  bool lr_random_ = false;        // randomized_svd in the rank-r update (common.cxx:691-709)
  uint64_t lr_random_calls_ = 0;  // blocks of R*r draws consumed in this run
  RTensor lr_desc_[MAX_ORDER];
  void *ms_X_override_ = nullptr;  // ms_start_step writes the first-level intermediate here
  DeviceBuffer lr_X_, lr_Us_, lr_G2_, lr_small_;
  DeviceBuffer lr_T_;  // (grow-only)


  std::vector<int> ms_order_;  // the N-k modes of the step in update order
  std::vector<int> ms_leaf_;   // node index of each list position
  DeviceBuffer ms_scales_;  // one pending-Normalize scalar per cached tensor (<= 32)
  const double *ms_scale_of(const RTensor &t) const { return t.pending ? ms_scales_.as<double>() + t.slot : nullptr; }

  int64_t ext(int m) const { return m == 0 ? V_.llens[0] : V_.glens[m]; }
  FactorRef fref(int m, double *const *W) const;
  int64_t prod_ext(int lo, int hi) const;
  void build_tree(int lo, int hi, int parent);
  int find_node(int lo, int hi) const;
  void compute_node(int idx);
  void refresh_grams();
  void mode_update(int i, const double *M, int64_t ldm, double lambda, bool pp, double ratio);
  void normalize();
  const PPOp &pp_get(const std::string &seq);
  int pp_last_mode(const std::string &seq) const;      // the contracted mode of `seq` that is removed last
  std::string pp_parent(const std::string &seq) const;  // `seq` without it
  // out (+)= T contracted over `cmode` with f; T is a pair operator (two modes, any storage order)
  void pp_contract_pair(const PPOp &T, int cmode, const FactorRef &f, double *out, int64_t out_rows);
  bool pp_fast_ = true;  // both resident layouts + typed level-1 operators (pp_operator() switches it off for its fp64 hand-out)
  bool pp_no_borrow_ = false;  // pp_operator(): never hand out the (scaled) multi-sweep intermediate
  void pp_clear();
  void pp_build_all();
  void sweep_pp(double lambda, double ratio);
  double allreduce_scalar(double x);
  bool agree(bool local);
  // the drivers (their console lines, CSV and clock: run_report.h)
  ModeNorms read_norms(bool dt_phase);
  bool print_block(RunReport &rep, const CpOpts &o, int iter, int pp_flag, double &projnorm,
                   bool bench);
  void dt_sub(RunReport &rep, const CpOpts &o, double &projnorm, int &iter);
  void pp_restart();
  void pp_sub(RunReport &rep, const CpOpts &o, double &projnorm, int &iter);
  void pp_partupdate_sub(RunReport &rep, const CpOpts &o, double &projnorm, int &iter);
  int run_pp_common(const CpOpts &o, int *iters, bool partupdate);

  Ops &ops_;
  Comm &comm_;
  TensorDesc V_;
  int N_, R_, P_, rank_;
  // multi-start: K_ starts of Rs_ columns each, R_ = K_ * Rs_. G_ then holds, start by start, the N
  // Grams (Rs_ x Rs_) of that start — the blocks between starts are never formed —, S_ / Sinv_ one
  // system per start, gradsq_ K_ sums per mode (gradsq_[mode * K_ + start])
  // tab_ is the per-start table (rank, column offset col_b, system offset sq_b = sum_{c<b} R_c^2 into
  // S_ / Sinv_, Gram offset N sq_b: start b, mode i at G_ + N sq_b + i R_b^2); equal ranks make it the
  // arithmetic above, Rs_ the common rank. ragged_: the ranks differ, Rs_ is the largest.
  int K_ = 1, Rs_ = 0;
  StartTable tab_;
  bool ragged_ = false;
  bool multi_ = false;
  int kind_[MAX_ORDER] = {0};  // set_mode_kinds / set_nonneg: kModeFree everywhere at first
  int shape_[MAX_ORDER] = {0};  // set_mode_shapes: kShapeNone everywhere at first; != 0 only where kind_ is NONNEG
  void drop_stale_shapes() {    // (after every change of kind_)
    for (int i = 0; i < N_; i++)
      if (kind_[i] != kModeNonneg) shape_[i] = kShapeNone;
  }
  bool any_fixed() const {
    for (int i = 0; i < N_; i++)
      if (kind_[i] == kModeFixed) return true;
    return false;
  }
  // hold-out (set_holdout): the sample mode (-1: none), the keep table on the host and on the device
  // (K_ x s_mode bytes), bit b set for a start that holds something out, the scores shaped like W_[mode]
  int hold_mode_ = -1;
  std::vector<uint8_t> hold_keep_;
  DeviceBuffer hold_keep_dev_;
  unsigned hold_mask_ = 0;
  DeviceBuffer hold_scores_;
  int64_t hold_rows_ = 0;  // the extent the two device buffers were allocated for
  void hold_apply(unsigned starts);  // Ops::cp_hold_rows on the starts of hold_mask_ & starts
  bool dist_ = false;  // take the collective code paths (P_ > 1, or PPALS_FORCE_COMM=1 for tests)
  DeviceBufferTable W_, gradW_, Wprev_, Winit_, dW_, dM_, Mm_;
  DeviceBuffer G_;            // N Gram matrices, R*R each
  DeviceBuffer S_, Sinv_;
  DeviceBuffer gradsq_;  // per-mode local sum of grad^2 (device)
  DeviceBuffer scal_;    // small device scalar scratch (>= 4*MAX_ORDER)
  DeviceBuffer sendbuf_, recvbuf_, gatherbuf_;
  DeviceBuffer Mbuf_;    // PP: M_i^0 + corrections
  DeviceBuffer Qbuf_, Pbuf_;  // residual KRP operands
  DeviceBuffer xq_, xp_;      // model export KRP operands (grow-only, kept)
  int residual_form_ = RESIDUAL_FUSED;        // PPALS_MODEL_RESIDUAL
  // core_consistency: the pseudo-inverse factors (laid out like W_), the per-start flag and score, the
  // first contraction Y, the two chain buffers and the cores (all grow-only, kept for the next call)
  DeviceBufferTable cc_P_;
  DeviceBuffer cc_flag_, cc_out_;
  DeviceBuffer cc_Y_, cc_chain_[2], cc_core_;
  // slice_residuals / leverages: the two marginals, the folded result, the partial sums of the pass
  DeviceBuffer sl_row_, sl_col_, sl_out_, sl_work_;
  size_t slice_work_cap_ = (size_t)256 << 20;  // of the back end's partial sums (PPALS_TEST_SLICE_WORK_BYTES)
  DeviceBuffer fms_out_, fms_work_;  // congruence: Phi | w_a | w_b, and the back end's partial sums
  StartTable start_table() const;  // tab_, or the one start of an ordinary session
  // Resident storage orders of the local tensor that the scans may read. [0] is the tensor itself.
  // [1] (if built) lists the right-half modes first, so that contractions of left-half modes are
  // row-contiguous suffix scans too. When the tensor's column strides are not multiples of 128 B
  // (s = 50, 324: the reference scripts' shapes) — a scan then runs at 0.61 instead of 0.82 of
  // peak, profiles/r02s_stride_bench.txt — [1] is stored with its leading block of `q` modes
  // padded to 128 B, and [2] is such a padded copy in the tensor's own mode order; every root set
  // at a position >= q of a padded layout reads 128-B aligned columns, and the scan writes its
  // result compact (RowPad), so nothing else knows about the padding.
  struct Layout {
    void *ptr = nullptr;      // the tensor itself, or own
    DeviceBuffer own;         // the copy (empty: [0])
    std::vector<int> order;   // modes, fastest first
    int q = 0;                // leading modes in the padded block (0: not padded)
    int64_t blk = 0, ld = 0;  // real / stored elements of that block
  };
  std::vector<Layout> lay_;
  // Packed twins of unpadded fp32 layouts (engine.cpp, packed_for): one per (layout, scan shape)
  // that asked for one, with the reason where there is no copy
  struct PackedTwin {
    int layout = 0;             // index into lay_
    const void *src = nullptr;  // that layout's elements
    int64_t L = 0, J = 0, T = 0;
    DeviceBuffer data, bases, esc;
    int format = 0;             // PACK_FMT28 / PACK_FMT26 (0: no copy)
    int64_t escapes = 0;        // blocks that need an escape plane in format 26, as surveyed
    size_t esc_room = 0;        // bytes behind esc
    size_t bytes = 0;           // blocks + side words + escape planes
    std::string reason;         // why there is no copy ("" while there is one)
  };
  std::vector<PackedTwin> packs_;
  // PPALS_PACK_LAYOUT: 0 never, 1 / 2 the 28-bit / 26-bit format whatever the size, -1 auto
  int pack_mode_ = -1;
  int pack_regen_ = 0;            // times the tensor changed under this session
  std::string pack_off_reason_;   // why this session does not pack at all ("" while it may)
  bool optional_fits(size_t bytes);  // an optional copy of `bytes` fits behind what is still to come
  bool pack_fill(PackedTwin &t);
  void packs_release();
  int vt_state_ = 0;          // 0 not tried, 1 second layout built, -1 unavailable (disabled / no memory)
  uint64_t tensor_gen_ = 0;   // generation of the tensor contents the layouts and caches were built from
  void ensure_transposed();   // builds lay_[1] (and [2]) once
  void fill_layout(const Layout &l);
  // one tensor scan that contracts the (cyclically) consecutive modes first .. first+k-1
  struct ScanPlan {
    const Layout *lay = nullptr;
    int64_t L = 1, Lc = 1, J = 1, T = 1;  // stored / compact rows in front, contracted, behind
    RowPad pad;
    std::vector<int> set, kept;  // contracted / kept modes in storage order
  };
  bool plan_scan(int first, int k, bool natural_only, ScanPlan &plan);
  // the packed twin of plan.lay for plan's scan shape (built at the first request), nullptr: none
  const PackedSrc *packed_for(const ScanPlan &pl, PackedSrc &out);
  void check_tensor_generation();
  void model_operands(const ModelBox &bx, ModelPlan &mp);  // xq_ / xp_ and the offsets of a grouped plan
  // groups that follow the shard (the imputation, the weighted step); `second`: a second side view's strides
  void shard_groups(const ModelBox &bx, const int64_t *second, ModelPlan &mp) const;
  // the body wls_step and huber_step share (engine.cpp)
  void side_step(const char *what, const ViewArgs &a, const void *data, const ViewArgs *w, const void *weights,
                 void *stream, double c, double *out);
  template <typename Step>  // the loop run_em, run_wls and run_robust share (engine.cpp)
  int em_loop(Step &&step, const CpOpts &o, int inner_sweeps, double rel_change, int *iters, double *res);
  // s x R partials up to this size use one all-reduce + redundant update instead of
  // reduce-scatter + row-block update + all-gather (PPALS_COMM_SMALL_BYTES overrides)
  int64_t small_msg_bytes_ = 1 << 20;
  bool grad_replicated_[MAX_ORDER];
  int64_t maxs_ = 0, maxblk_ = 0;
  std::vector<Node> nodes_;
  std::vector<int> leaf_;  // node index of each leaf
  std::map<std::string, PPOp> pp_;
  bool grad_from_sweep_ = false;
  double init_gradnorm_ = 0;
};

}  // namespace ppals
