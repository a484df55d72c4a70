// tucker.h — HOOI sweep engine for Tucker decomposition (als_Tucker.cxx) over abstract ops.
#pragma once
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "engine.h"

namespace ppals {

class TuckerEngine {
 public:
  TuckerEngine(Ops &ops, Comm &comm, const TensorDesc &V, const int *ranks);
  ~TuckerEngine();
  void set_factors(const double *Wflat);
  void get_factors(double *Wflat, double *core);
  void set_core(const double *core);  // nullptr: recompute from V and the factors
  void hosvd();                          // als_Tucker.cxx:12-70
  int64_t ttmc(int skip, double *Yhost);  // als_Tucker.cxx:76-110
  void sweep_dt();                       // als_Tucker.cxx:340-408
  void settle() { settle_all(); }        // every eigen-step behind the current factors is a checked one
  int rollbacks() const { return defer_rollbacks_; }
  // core x_i W_i (residual: V - that, V as stored) into this rank's rows of a checked export view
  // (ppals_tucker_export_model_device), from the factors and core get_factors would return
  void export_model(const ViewArgs &a, void *dst, bool residual, void *stream);
  // The missing entries of the tensor (mask byte 0) overwritten with that model, rounded once to the
  // storage type, the others left bit for bit (ppals_tucker_impute_device); settles the rotations as
  // export_model does. Bumps the tensor's generation; factors and core do not change. observed_sq != nullptr:
  // the sum of (V - model)^2 over the observed elements of the box, all ranks (the call then waits for it).
  void impute(const ViewArgs &a, const void *mask, void *stream, double *observed_sq);
  // EM with missing entries (ppals_tucker_em): repeat { impute; inner_sweeps HOOI sweeps }, the looks, the
  // stop rules and the last impute on the way out as CpEngine::run_em. Returns 1 if it stopped on tol.
  int run_em(const ViewArgs &a, const void *mask, void *stream, const CpOpts &o, int inner_sweeps, int *iters,
             double *observed_res);
  // ||V - core x_i W_i||_F of the factors and core get_factors would return now (ppals_tucker_residual)
  double residual_now() {
    finalize_rotations();
    return residual();
  }
  // The influence plot of a Tucker session (ppals_tucker_slice_residuals / _leverages; one rank). Both settle
  // the rotations as export_model does, change nothing else of the session and nothing of the tensor.
  //   slice_residuals: ss_i[x] = the sum of (V - core x_j W_j)^2 over the slice x of mode i, all modes from
  //     ONE pass over the tensor: the slabs of impute (model_slabs: Z = core x_{i != 0} W_i within the chain
  //     buffers), per slab Ops::model_slice_sums — the sums over b onto ss_0 in slab order, the sums over a
  //     folded onto modes 1..N-1 (Ops::fold_slice_sums): the slab mode's entries at the slab's offset, the
  //     other modes' added in slab order. total = the sum of ss_0 in index order. The host does not wait
  //     between slabs.
  //   leverages: lev_i[x] = the x-th diagonal entry of the projector onto the columns of W_i = the row sums of
  //     squares of an orthonormal basis of them (Ops::orthonormalize on a scratch copy, Ops::row_dots); NaN in
  //     every entry when ONE factor is rank deficient. Never reads the tensor.
  void slice_residuals(double *ss_host, double *total_host);
  void leverages(double *lev_host);
  const TensorDesc &tensor() const { return V_; }
  int run_dt(const CpOpts &o, int *iters);  // alsTucker_DT, als_Tucker.cxx:240-424
  int run_pp(const CpOpts &o, int *iters);  // alsTucker_PP, als_Tucker.cxx:906-962

 private:
  struct Node {
    int lo, hi, parent, slo, shi;
    DeviceBuffer buf;  // (grow-only)
    bool valid = false;
    bool front = false;  // a leaf stored [s_mode | ranks of the other modes] instead of the tree's order
  };
  void build_tree(int lo, int hi, int parent);
  // dims of a node's tensor: ranks on the contracted modes, full extent elsewhere
  void compute_node(int idx);
  void compute_left_half_on_vt(Node &n);
  double *ttmc_chain(int skip, int64_t *elems);  // result lives in the chain scratch
  int64_t ext(int m) const { return m == 0 ? V_.llens[0] : V_.glens[m]; }
  const double *wptr(int m) const { return W_[m] + (m == 0 ? V_.row0 : 0); }
  // leaf tensor Y_i complete on every rank (all-gather of the leading-mode rows for i = 0,
  // all-reduce of the partial sums otherwise); returns the buffer holding it
  double *complete_leaf(int i, double *Yloc, int64_t elems_local);
  // W_i = the r_i leading left singular vectors of the mode-i unfolding of Y = [L, s_i, T]
  void factor_update(int i, const double *Y, int64_t L, int64_t T);
  void compute_core_full();
  void ensure_core();  // the core the last exact sweep owes: Y_end x_{N-1} W_{N-1}
  bool core_owed_ = false;
  const double *yend_src_ = nullptr;
  int64_t yend_T_ = 1;  // layout of yend_src_: [ranks before, s_{N-1}] (1) or [s_{N-1} | ranks] (their product)
  double core_norm();
  bool agree(bool local);
  double residual();
  int64_t node_elems(const Node &n) const;

  Ops &ops_;
  Comm &comm_;
  TensorDesc V_;
  int N_;
  std::vector<int> r_;
  DeviceBufferTable W_;
  DeviceBuffer core_, core_prev_, Yend_, G_, scal_;
  int64_t ncore_ = 1, yend_elems_ = 0;
  std::vector<Node> nodes_;
  std::vector<int> leaf_;
  std::vector<char> contracted_;  // scratch
  int P_ = 1, rank_ = 0;
  bool dist_ = false;
  // pairwise perturbation (als_Tucker.cxx:426-962)
  struct PPOp {
    DeviceBuffer buf;
    int64_t elems = 0;
    std::vector<int64_t> dims;
  };
  std::map<std::string, PPOp> pp_;
  DeviceBufferTable Wprev_, Winit_, dW_;
  DeviceBuffer Ytmp_, Yacc_;  // (grow-only, as thin_, Yfull_, gather_, chain_, ms3_X_, ms3_Y_, xwt_ and xz_)
  DeviceBuffer thin_;  // [s_i x (L*T) unfolding | (L*T) x r_i right vectors] of the thin route
  int eig_base_ = 0;  // block of warm-start slots drawn from the back end (Ops::eig_session_new)
  void finalize_rotations();
  void drop_rotations();
  bool thin_enabled_ = true;  // PPALS_TUCKER_THIN=0: always the s_i x s_i Gram (A/B, tests)
  DeviceBuffer VT_;  // second resident layout [(right modes), (left modes)], empty: not held
  // Order 3, one GPU: the multi-sweep dimension tree (as the CP engine's, cp_msdt_optimizer.cxx:172-207).
  // ONE first-level intermediate X_r = V x_r W_r serves the TWO mode updates that follow mode r's, then
  // the root moves on to the mode updated last: 3 tensor scans per 2 HOOI sweeps instead of 4, the same
  // factors in the same order (every product of a step sees exactly the factor versions alsTucker_DT's
  // tree gives it). Needs the tensor in all three rotations (V, VT_ = [2 | 0 1], VT2_ = [1 2 | 0]) so
  // that every root is contracted by a row-contiguous scan. PPALS_TUCKER_CHAIN=tree: the per-sweep tree.
  // Cost: 3 x the tensor's bytes resident for the session's life (the third rotation is taken only with
  // 2 x the tensor + 2 GB free at creation); X_r is kept in the TENSOR's precision, so with fp32 storage
  // the two schedules agree to ~1e-7 (X_r rounded like the tensor), with fp64 storage to rounding.
  bool ms3_ = false;
  DeviceBuffer VT2_;
  DeviceBuffer ms3_X_;
  int ms3_root_ = -1, ms3_left_ = 0;
  bool ms3_perm_ = false;  // the leaf just served has its two rank indices in descending mode order
  DeviceBuffer ms3_Y_[3];
  double *ms3_leaf(int i, int64_t *T);
  void ms3_invalidate() {
    ms3_root_ = -1;
    ms3_left_ = 0;
  }
  uint64_t tensor_gen_ = 0;  // generation of the tensor contents VT_ and the caches were built from
  void check_tensor_generation();
  // TensorDesc::prep_epoch as this session last saw it. When it has moved (the contents were centred or scaled in
  // place) the session settles what is pending and then forgets its history — the warm-start slots of its
  // eigen-steps are drawn anew and the order-3 multi-sweep schedule is back to what the session was created with —
  // so that its next hosvd / sweeps are, bit for bit, those of a new session on the new contents.
  uint64_t prep_epoch_ = 0;
  bool ms3_created_ = false;
  void check_prep_epoch();
  DeviceBuffer chain_[2];  // ping-pong scratch of the mode-product chains
  const PPOp &pp_get(const std::string &args);
  void pp_clear();
  void sweep_body(const DeviceBufferTable *align_ref);
  // one mode of a HOOI sweep: leaf tensor, eigen-step, (last mode) the core
  void mode_step(int i, const DeviceBufferTable *align_ref, bool may_defer);
  // Deferred acceptance of eigen-steps (Ops::eig_defer / eig_verify): inside plain sweeps the host
  // does not wait for a step's checks — it enqueues ahead of the device — and asks for them when it
  // comes back to the mode (or before anything is published: print blocks, get_factors, the PP
  // phases). `defer_log_` = the modes stepped since the oldest unchecked step, in order; Wsave_[m] =
  // the factor the latest step of mode m replaced. A step that was NOT accepted: every factor
  // stepped since goes back to what it was and those steps are repeated, checked one by one.
  std::vector<int> defer_log_;
  DeviceBufferTable Wsave_;
  bool defer_enabled_ = true;  // (the back end decides per slot: PPALS_EIG_DEFER=0 switches every deferral off)
  int defer_rollbacks_ = 0;
  void settle_mode(int i);  // before mode i is stepped again
  void settle_all();        // before anything derived from the factors is read
  void rollback_and_redo();
  void sweep_pp();
  bool print_block(RunReport &rep, const CpOpts &o, int iter, int pp_flag, double &diffnorm,
                   bool stop_at_maxiter);
  ModeNorms read_norms(bool dt_phase);
  void dt_sub(RunReport &rep, const CpOpts &o, double tol_init, double &diffnorm, int &iter);
  void pp_sub(RunReport &rep, const CpOpts &o, double tol_init, double &diffnorm, int &iter);
  // model export and imputation: the transposed factors and the ping-pong buffers of
  // Z = core x_{i != f} W_i; run(plan, Q, Z) is what the caller does with a slab
  using SlabRun = std::function<void(const ModelPlan &, const double *, const double *)>;
  void model_slabs(const ModelBox &bx, int f, int s, const SlabRun &run);
  void export_slab(const ModelBox &bx, int f, const std::vector<int> &chain, const SlabRun &run);
  // (kept for the session's next export: freeing them would wait for the device)
  DeviceBuffer xwt_, xz_[2];
  // slice_residuals / leverages (grow-only): the slab's marginal over b, its fold, the N result vectors, the
  // back end's partial sums, the scratch copy of a factor
  DeviceBuffer sl_col_, sl_fold_, sl_out_, sl_work_, sl_q_;
  size_t slice_work_cap_ = (size_t)256 << 20;  // of the partial sums (PPALS_TEST_SLICE_WORK_BYTES)
  int residual_form_ = RESIDUAL_FUSED;  // PPALS_MODEL_RESIDUAL
  DeviceBuffer Yfull_, gather_;
};

}  // namespace ppals
