// tucker.cpp — host control flow of the Tucker HOOI engine. Mirrors:
//   ttmc_map_DT        als_Tucker.cxx:178-230  -> compute_node
//   alsTucker_DT       als_Tucker.cxx:240-424  -> sweep_dt / run_dt
//   hosvd              als_Tucker.cxx:12-70    -> hosvd
//   TTMc               als_Tucker.cxx:76-110   -> ttmc_chain
// Multi-GPU: V is block-partitioned along mode 0, factors are replicated. Every
// contraction over mode 0 uses the local rows of W_0 and yields a PARTIAL sum that stays partial
// down to the leaf tensor Y_i (TTMc is linear), where it is all-reduced (i != 0) or its rows are
// all-gathered (i = 0); Gram + eigenvectors are then computed redundantly on every rank.
// Order generalisation as for CP: a node is "first level" iff its parent is the root, which is
// the reference's length test for N = 4,6,7,8 and defines N = 3 (BASELINE config 5).
#include "tucker.h"
#include "run_report.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <limits>
#include <stdexcept>
#include <string>

namespace ppals {

TuckerEngine::TuckerEngine(Ops &ops, Comm &comm, const TensorDesc &V, const int *ranks)
    : ops_(ops), comm_(comm), V_(V), N_(V.order) {
  P_ = comm.size();
  dist_ = P_ > 1 || (force_comm_path() && !comm.is_self());
  rank_ = comm.rank();
  residual_form_ = residual_form_env();
  slice_work_cap_ = slice_work_cap_env();
  eig_base_ = ops_.eig_session_new();  // this session's warm-start slots: base + {i, 8 + i, 16 + i}
  // (the back end sets up what lazy eigen-steps need now, not inside the first sweep)
  if (!dist_)
    for (int i = 0; i < N_ && i < MAX_ORDER; i++)
      if (V_.glens[i] > 64) ops_.eig_lazy(eig_base_ + i, true);
  int64_t maxs = 0;
  W_.resize(N_);
  for (int i = 0; i < N_; i++) {
    if (ranks[i] <= 0 || ranks[i] > V_.glens[i])
      throw std::runtime_error("ppals: Tucker rank out of range");
    r_.push_back(ranks[i]);
    ncore_ *= ranks[i];
    maxs = std::max(maxs, V_.glens[i]);
    W_.alloc(ops_, i, sizeof(double) * V_.glens[i] * ranks[i]);
    ops_.zero(W_[i], sizeof(double) * V_.glens[i] * ranks[i]);
  }
  core_ = DeviceBuffer(ops_, sizeof(double) * ncore_);
  core_prev_ = DeviceBuffer(ops_, sizeof(double) * ncore_);
  ops_.zero(core_.as<double>(), sizeof(double) * ncore_);
  ops_.zero(core_prev_.as<double>(), sizeof(double) * ncore_);
  G_ = DeviceBuffer(ops_, sizeof(double) * maxs * maxs);
  if (const char *e = std::getenv("PPALS_TUCKER_THIN")) thin_enabled_ = std::atoi(e) != 0;
  scal_ = DeviceBuffer(ops_, sizeof(double) * 64);
  yend_elems_ = ncore_ / r_[N_ - 1] * V_.glens[N_ - 1];
  Yend_ = DeviceBuffer(ops_, sizeof(double) * yend_elems_);
  build_tree(0, N_ - 1, -1);
  leaf_.assign(N_, -1);
  for (size_t k = 0; k < nodes_.size(); k++)
    if (nodes_[k].lo == nodes_[k].hi) leaf_[nodes_[k].lo] = (int)k;
  // second resident layout V^T[(right modes), (left modes)] (as in the CP engine): the first-level
  // node that contracts the LEFT half of the modes then runs as row-contiguous scans too, instead
  // of a column-strided scan of the leading mode followed by scans with a handful of rows
  const char *env = std::getenv("PPALS_TRANSPOSED_COPY");
  if (N_ >= 3 && !(env && std::atoi(env) == 0)) {
    const int mid = (N_ - 1) / 2;
    int64_t rows = 1, cols = 1;
    for (int m = 0; m <= mid; m++) rows *= ext(m);
    for (int m = mid + 1; m < N_; m++) cols *= ext(m);
    VT_ = DeviceBuffer::try_alloc(ops_, (size_t)rows * cols * dtype_size(V_.dtype));
    if (VT_) ops_.transpose2d(V_.data, V_.dtype, rows, cols, VT_.get());
    // the third rotation [1 2 | 0] for the order-3 multi-sweep schedule (tucker.h), room permitting
    const char *chain = std::getenv("PPALS_TUCKER_CHAIN");
    if (N_ == 3 && !dist_ && VT_.get() && !(chain && std::string(chain) == "tree")) {
      const size_t bytes = (size_t)V_.nloc * dtype_size(V_.dtype);
      const size_t avail = ops_.mem_available();
      if (avail == (size_t)-1 || (double)avail > 2.0 * (double)bytes + 2e9) VT2_ = DeviceBuffer::try_alloc(ops_, bytes);
      if (VT2_) {
        ops_.transpose2d(V_.data, V_.dtype, ext(0), ext(1) * ext(2), VT2_.get());
        ms3_ = true;
      }
    }
  }
  if (V_.generation) tensor_gen_ = *V_.generation;
  if (V_.prep_epoch) prep_epoch_ = *V_.prep_epoch;
  ms3_created_ = ms3_;
}

// see tucker.h; called where a session call first comes to read the tensor (hosvd, the sweeps)
void TuckerEngine::check_prep_epoch() {
  if (!V_.prep_epoch || *V_.prep_epoch == prep_epoch_) return;
  prep_epoch_ = *V_.prep_epoch;
  finalize_rotations();  // (settles deferred steps; a rotation still owed to a factor is applied, not lost)
  ops_.sync();
  ops_.eig_session_free(eig_base_);
  eig_base_ = ops_.eig_session_new();
  if (!dist_)
    for (int i = 0; i < N_ && i < MAX_ORDER; i++)
      if (V_.glens[i] > 64) ops_.eig_lazy(eig_base_ + i, true);
  ms3_ = ms3_created_;
  ms3_invalidate();
}

// The leaf of mode i, [s_i | the other two ranks], from the order-3 multi-sweep schedule; nullptr: the
// back end has no leading-mode product for this shape — the schedule is switched off for the session.
double *TuckerEngine::ms3_leaf(int i, int64_t *T) {
  check_tensor_generation();
  if (ms3_root_ < 0 || ms3_root_ == i || ms3_left_ <= 0) {
    // root = the mode updated last before i: serves i and the mode after it
    const int r = (i + 2) % 3;
    const void *lay = r == 2 ? V_.data : (r == 1 ? VT_.get() : VT2_.get());  // storage order (r+1, r+2, r)
    const int64_t d0 = ext((r + 1) % 3), d1 = ext((r + 2) % 3);
    const size_t need = dtype_size(V_.dtype) * (size_t)(d0 * d1 * r_[r]);
    ms3_X_.reserve(ops_, need);
    FactorRef f;
    f.ptr = wptr(r);
    f.rows = ext(r);
    f.ld = V_.glens[r];
    ops_.scan_contract(lay, V_.dtype, d0 * d1, ext(r), 1, &f, 1, r_[r], ms3_X_.get(), V_.dtype, d0 * d1 * r_[r], d0 * d1);
    ms3_root_ = r;
    ms3_left_ = 2;
  }
  const int r = ms3_root_, m0 = (r + 1) % 3, m1 = (r + 2) % 3;  // X[s_m0, s_m1, rank_r]
  const int64_t d0 = ext(m0), d1 = ext(m1);
  const int64_t elems = (int64_t)V_.glens[i] * (i == m0 ? r_[m1] : r_[m0]) * r_[r];
  ms3_Y_[i].reserve(ops_, sizeof(double) * elems);
  if (i == m0) {  // keep the first mode in front, contract the second: [s_m0 | rank_m1, rank_r]
    ops_.ttm_keep(ms3_X_.get(), V_.dtype, d0, d1, r_[r], wptr(m1), V_.glens[m1], r_[m1], ms3_Y_[i].as<double>());
    *T = (int64_t)r_[m1] * r_[r];
  } else {        // contract the leading mode, the second one comes to the front: [s_m1 | rank_m0, rank_r]
    if (!ops_.ttm_lead_front(ms3_X_.get(), V_.dtype, d0, d1, r_[r], wptr(m0), V_.glens[m0], r_[m0],
        ms3_Y_[i].as<double>())) {
      ms3_ = false;
      ms3_invalidate();
      return nullptr;
    }
    *T = (int64_t)r_[m0] * r_[r];
  }
  // rank indices behind the mode: (other, root). Ascending mode order — what ensure_core() reads — when
  // other < root
  ms3_perm_ = (i == m0 ? m1 : m0) > r;
  ms3_left_--;
  return ms3_Y_[i].as<double>();
}

// see CpEngine::check_tensor_generation: the tensor handle stays writable while sessions exist
void TuckerEngine::check_tensor_generation() {
  if (!V_.generation || *V_.generation == tensor_gen_) return;
  tensor_gen_ = *V_.generation;
  if (VT_) {
    const int mid = (N_ - 1) / 2;
    int64_t rows = 1, cols = 1;
    for (int m = 0; m <= mid; m++) rows *= ext(m);
    for (int m = mid + 1; m < N_; m++) cols *= ext(m);
    ops_.transpose2d(V_.data, V_.dtype, rows, cols, VT_.get());
  }
  if (VT2_) ops_.transpose2d(V_.data, V_.dtype, ext(0), ext(1) * ext(2), VT2_.get());
  ms3_invalidate();
  for (auto &n : nodes_) n.valid = false;
  pp_clear();
}

TuckerEngine::~TuckerEngine() {
  try {
    ops_.sync();
  } catch (...) {
  }
  try {
    ops_.eig_session_free(eig_base_);
  } catch (...) {
  }
}

void TuckerEngine::build_tree(int lo, int hi, int parent) {
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
    nodes_.push_back(std::move(n));
    idx[c] = (int)nodes_.size() - 1;
  }
  build_tree(lo, mid, idx[0]);
  build_tree(mid + 1, hi, idx[1]);
}

// a node [lo,hi] keeps modes lo..hi at full extent; every other mode is already contracted to rank
int64_t TuckerEngine::node_elems(const Node &n) const {
  int64_t e = 1;
  for (int m = 0; m < N_; m++) e *= (m >= n.lo && m <= n.hi) ? ext(m) : r_[m];
  return e;
}

// First-level node that contracts the left half [0, shi] of the modes, on the second layout
// [shi+1..N-1 | 0..shi]: the contracted modes are the trailing ones there, so they are removed
// last-first by row-contiguous scans; the result [right extents | left ranks] is transposed into
// the node's own order [left ranks | right extents] (a few hundred MB at most).
void TuckerEngine::compute_left_half_on_vt(Node &n) {
  const int nl = n.shi + 1, nr = N_ - nl;  // left (contracted) / right (kept) mode counts
  std::vector<int64_t> dims;              // extents in VT storage order
  for (int m = nl; m < N_; m++) dims.push_back(ext(m));
  for (int m = 0; m < nl; m++) dims.push_back(ext(m));
  const void *cur = VT_.get();
  int cur_dt = V_.dtype;
  int pp_slot = 0;
  // A LEAF (one mode on the right: order 3) keeps the chain's own order [s_mode | left ranks]: that
  // IS the unfolding with the mode in front which the Gram wants, so neither the transposition into
  // the tree's order nor the one back (2 x 7 us at cfg5) happens; the last scan writes the node.
  const bool front_leaf = (nr == 1) && !dist_;
  int64_t node_elems_total = 1;
  for (int m = 0; m < N_; m++) node_elems_total *= (m >= nl ? ext(m) : r_[m]);
  if (front_leaf) n.buf.reserve(ops_, sizeof(double) * node_elems_total);
  for (int m = n.shi; m >= 0; m--) {
    const int p = nr + m;  // storage position of mode m
    int64_t L = 1, T = 1;
    for (int q = 0; q < p; q++) L *= dims[q];
    for (int q = p + 1; q < N_; q++) T *= dims[q];
    const bool last = (m == 0);
    const int dst_dt = last ? F64 : V_.dtype;
    const size_t need = dtype_size(dst_dt) * (size_t)(L * r_[m] * T);
    void *dst;
    if (last && front_leaf) {
      dst = n.buf.as<double>();
    } else {
      chain_[pp_slot].reserve(ops_, need);
      dst = chain_[pp_slot].get();
      pp_slot ^= 1;
    }
    FactorRef f;
    f.ptr = wptr(m);
    f.rows = dims[p];
    f.ld = V_.glens[m];
    // (the step that reads the tensor is a scan; a later one reads a small intermediate and writes
    // fp64: the back end may run it as one batched GEMM, Ops::ttm_keep)
    if (cur != VT_.get() && dst_dt == F64)
      ops_.ttm_keep(cur, cur_dt, L, dims[p], T, f.ptr, f.ld, r_[m], (double *)dst);
    else
      ops_.scan_contract(cur, cur_dt, L, dims[p], T, &f, 1, r_[m], dst, dst_dt, L * r_[m], L);
    cur = dst;
    cur_dt = dst_dt;
    dims[p] = r_[m];
  }
  n.front = front_leaf;
  if (front_leaf) {
    n.valid = true;
    return;
  }
  int64_t rows = 1, cols = 1;
  for (int q = 0; q < nr; q++) rows *= dims[q];
  for (int q = nr; q < N_; q++) cols *= dims[q];
  n.buf.reserve(ops_, sizeof(double) * rows * cols);
  ops_.transpose2d(cur, F64, rows, cols, n.buf.as<double>());
  n.valid = true;
}

void TuckerEngine::compute_node(int idx) {
  check_tensor_generation();
  Node &n = nodes_[idx];
  if (n.valid) return;
  // (the sharded leaf of mode 0 keeps its own blocked layout: not this route)
  if (n.parent < 0 && n.slo == 0 && n.shi < N_ - 1 && VT_.get() && !(dist_ && n.lo == 0 && n.hi == 0)) {
    compute_left_half_on_vt(n);
    return;
  }
  n.front = false;
  // The leaf of mode 1 under a parent that keeps modes 0 and 1: one product with the LEADING mode,
  // written with mode 1 in front — the unfolding the Gram wants (no leading-mode scan + pack +
  // transposition: 25 -> 14 us at cfg5) — when the back end has the kernel.
  if (!dist_ && n.parent >= 0 && n.lo == 1 && n.hi == 1 && n.slo == 0 && n.shi == 0) {
    compute_node(n.parent);
    const Node &p = nodes_[n.parent];
    if (!p.front && p.lo == 0 && p.hi == 1) {
      int64_t T = 1;
      for (int m = 2; m < N_; m++) T *= r_[m];
      const int64_t elems = (int64_t)ext(1) * r_[0] * T;
      n.buf.reserve(ops_, sizeof(double) * elems);
      if (ops_.ttm_lead_front(p.buf.as<double>(), F64, ext(0), ext(1), T, wptr(0), V_.glens[0], r_[0],
          n.buf.as<double>())) {
        n.front = true;
        n.valid = true;
        return;
      }
    }
  }
  std::vector<int64_t> dims(N_);
  const void *src;
  int dt;
  if (n.parent < 0) {
    for (int m = 0; m < N_; m++) dims[m] = ext(m);
    src = V_.data;
    dt = V_.dtype;
  } else {
    compute_node(n.parent);
    const Node &p = nodes_[n.parent];
    for (int m = 0; m < N_; m++) dims[m] = (m >= p.lo && m <= p.hi) ? ext(m) : r_[m];
    src = p.buf.as<double>();
    dt = F64;
  }
  // contract the sibling's modes one at a time (als_Tucker.cxx:216-227). The intermediates of the
  // chain live in two grow-only scratch buffers of the session (a per-call hipMalloc/hipFree of
  // these multi-GB tensors stalled whole seconds at order 6) and keep the tensor's own precision
  // (like the CP intermediate: fp32 tensor -> fp32 intermediates, fp64 accumulation inside the
  // scan, fp64 node result).
  const void *cur = src;
  int cur_dt = dt;
  int pp_slot = 0;
  // the sharded leaf of mode 0 is written with leading dimension blk (= rows per rank) so that it
  // is directly one block of the all-gather buffer (rows beyond the local extent stay zero)
  const bool leaf0_blocked = (dist_ && n.lo == 0 && n.hi == 0);
  const int64_t blk = block_rows(V_.glens[0], P_);
  // The mode products commute; the reference removes the sibling's modes in ascending order
  // (als_Tucker.cxx:216-227). The FIRST product is the one that reads the tensor: when its columns
  // are 128-B aligned only with the sibling's LAST mode in front (s = 50: 50^3 * 4 B is not a
  // multiple of 128, 50^5 * 4 B is), the chain runs in descending order — 0.80 instead of 0.66
  // of peak for that scan (profiles/r02s_stride_bench.txt). PPALS_TUCKER_CHAIN=asc|desc forces one.
  bool descending = false;
  if (n.parent < 0 && n.shi > n.slo && !leaf0_blocked) {
    const int64_t line = 128 / (int64_t)dtype_size(dt);
    int64_t la = 1, ld = 1;
    for (int q = 0; q < n.slo; q++) la *= dims[q];
    for (int q = 0; q < n.shi; q++) ld *= dims[q];
    descending = (ld % line == 0) && (la % line != 0);
    if (const char *e = std::getenv("PPALS_TUCKER_CHAIN")) descending = std::string(e) == "desc";
  }
  const int nsib = n.shi - n.slo + 1;
  for (int step = 0; step < nsib; step++) {
    const int m = descending ? n.shi - step : n.slo + step;
    int64_t L = 1, T = 1;
    for (int q = 0; q < m; q++) L *= dims[q];
    for (int q = m + 1; q < N_; q++) T *= dims[q];
    const bool last = (step == nsib - 1);
    const int64_t Lout = (last && leaf0_blocked) ? blk : L;
    const int64_t out_elems = Lout * r_[m] * T;
    void *dst;
    int dst_dt;
    if (last) {
      n.buf.reserve(ops_, sizeof(double) * out_elems);
      dst = n.buf.as<double>();
      dst_dt = F64;
      if (leaf0_blocked) ops_.zero(dst, sizeof(double) * out_elems);
    } else {
      dst_dt = V_.dtype;
      const size_t need = dtype_size(dst_dt) * (size_t)out_elems;
      chain_[pp_slot].reserve(ops_, need);
      dst = chain_[pp_slot].get();
      pp_slot ^= 1;
    }
    FactorRef f;
    f.ptr = wptr(m);
    f.rows = dims[m];
    f.ld = V_.glens[m];
    // out[l + Lout*(k + r*t)]: the mode product that keeps the mode in place (als_Tucker.cxx:224)
    if (cur != V_.data && dst_dt == F64 && Lout == L)
      ops_.ttm_keep(cur, cur_dt, L, dims[m], T, f.ptr, f.ld, r_[m], (double *)dst);
    else
      ops_.scan_contract(cur, cur_dt, L, dims[m], T, &f, 1, r_[m], dst, dst_dt, Lout * r_[m], Lout);
    cur = dst;
    cur_dt = dst_dt;
    dims[m] = r_[m];
  }
  n.valid = true;
}

// Make a leaf tensor complete on every rank. i == 0: the rows live on their owners -> all-gather
// of the [blk x rest] blocks, re-assembled to [s0 x rest]. i != 0: partial sums -> all-reduce.
double *TuckerEngine::complete_leaf(int i, double *Yloc, int64_t elems_local) {
  if (!dist_) return Yloc;
  if (i != 0) {
    comm_.allreduce_sum(Yloc, elems_local);
    return Yloc;
  }
  const int64_t s0 = V_.glens[0], blk = block_rows(s0, P_);
  int64_t rest = 1;
  for (int m = 1; m < N_; m++) rest *= r_[m];
  gather_.reserve(ops_, sizeof(double) * blk * rest * P_);
  Yfull_.reserve(ops_, sizeof(double) * s0 * rest);
  ops_.d2d(gather_.as<double>() + (size_t)rank_ * blk * rest, Yloc, sizeof(double) * blk * rest);
  comm_.allgather(gather_.as<double>() + (size_t)rank_ * blk * rest, gather_.as<double>(), blk * rest);
  ops_.unpack_blocks(gather_.as<double>(), s0, s0, (int)rest, blk, P_, Yfull_.as<double>());
  return Yfull_.as<double>();
}

// TTMc (als_Tucker.cxx:76-110): chain of mode products, skipping `skip`
double *TuckerEngine::ttmc_chain(int skip, int64_t *elems) {
  std::vector<int64_t> dims(N_);
  for (int m = 0; m < N_; m++) dims[m] = ext(m);
  const void *cur = V_.data;
  int cur_dt = V_.dtype;
  double *prev = nullptr;
  int pp_slot = 0;
  for (int m = 0; m < N_; m++) {
    if (m == skip) continue;
    int64_t L = 1, T = 1;
    for (int q = 0; q < m; q++) L *= dims[q];
    for (int q = m + 1; q < N_; q++) T *= dims[q];
    const size_t need = sizeof(double) * (size_t)(L * r_[m] * T);
    chain_[pp_slot].reserve(ops_, need);
    double *dst = chain_[pp_slot].as<double>();
    pp_slot ^= 1;
    ops_.ttm_keep(cur, cur_dt, L, dims[m], T, wptr(m), V_.glens[m], r_[m], dst);
    prev = dst;
    cur = dst;
    cur_dt = F64;
    dims[m] = r_[m];
  }
  int64_t e = 1;
  for (int m = 0; m < N_; m++) e *= dims[m];
  *elems = e;
  return prev;  // lives in the session's chain scratch until the next chain runs
}

int64_t TuckerEngine::ttmc(int skip, double *Yhost) {
  settle_all();
  int64_t e;
  double *Y = ttmc_chain(skip, &e);
  // sharded: skip == 0 returns the local rows, every other result is summed over the ranks
  if (dist_ && skip != 0) comm_.allreduce_sum(Y, e);
  if (Yhost) ops_.d2h(Yhost, Y, sizeof(double) * e);
  return e;
}

void TuckerEngine::ensure_core() {
  if (!core_owed_) return;
  if (!yend_src_) {
    compute_core_full();
    return;
  }
  core_owed_ = false;
  const int64_t Lc = ncore_ / r_[N_ - 1], sN = V_.glens[N_ - 1];
  const int rN = r_[N_ - 1];
  if (yend_T_ == 1) {  // the tree's order [ranks before | s_{N-1}]
    ops_.ttm_keep(yend_src_, F64, Lc, sN, 1, W_[N_ - 1], sN, rN, core_.as<double>());
  } else {
    // the last leaf kept the mode in front, [s_{N-1} | ranks]: core^T first, then its order
    DeviceBuffer tmp(ops_, sizeof(double) * ncore_);
    ops_.ttm_keep(yend_src_, F64, 1, sN, Lc, W_[N_ - 1], sN, rN, tmp.as<double>());  // [r_{N-1}, ranks before]
    ops_.transpose2d(tmp.as<double>(), F64, rN, Lc, core_.as<double>());
    ops_.sync();
    tmp.reset();
  }
}

void TuckerEngine::compute_core_full() {
  core_owed_ = false;
  int64_t e;
  double *Y = ttmc_chain(-1, &e);
  if (dist_) comm_.allreduce_sum(Y, ncore_);
  ops_.d2d(core_.as<double>(), Y, sizeof(double) * ncore_);
}

// Eigenvectors on demand. A plain HOOI sweep lets the back end return ANY orthonormal basis of a
// mode's subspace (Ops::eig_lazy): the contractions, ||core|| and the convergence measure depend on
// W_i W_i^T only. Whoever needs the eigenvectors one by one, sorted — the caller reading the
// factors, the PP phases that difference them — asks here: W_i <- W_i Y_i, core <- core x_i Y_i.
void TuckerEngine::finalize_rotations() {
  settle_all();  // (no factor is read, rotated or published with an unchecked step behind it)
  ensure_core();
  for (int i = 0; i < N_; i++) {
    const double *Y = ops_.eig_pending_rotation(eig_base_ + i);
    if (!Y) continue;
    const int r = r_[i];
    ops_.rows_times_small(W_[i], V_.glens[i], r, Y, r, nullptr, W_[i]);
    int64_t L = 1, T = 1;
    for (int q = 0; q < i; q++) L *= r_[q];
    for (int q = i + 1; q < N_; q++) T *= r_[q];
    DeviceBuffer tmp(ops_, sizeof(double) * ncore_);
    ops_.ttm_keep(core_.as<double>(), F64, L, r, T, Y, r, r, tmp.as<double>());
    ops_.d2d(core_.as<double>(), tmp.as<double>(), sizeof(double) * ncore_);
    ops_.sync();
    tmp.reset();
    ops_.eig_rotation_done(eig_base_ + i);
    ms3_invalidate();  // (the multi-sweep intermediate may carry this mode's rank index in the old basis)
  }
}
void TuckerEngine::drop_rotations() {
  settle_all();
  for (int i = 0; i < N_; i++) ops_.eig_rotation_done(eig_base_ + i);
}

void TuckerEngine::set_factors(const double *Wflat) {
  settle_all();
  // (the core the last sweep owes belongs to the factors that are about to be replaced: the core object
  // travels on through a caller's repetitions, pp_bench.cxx:321-345)
  ensure_core();
  drop_rotations();  // (they belonged to the factors being replaced)
  ms3_invalidate();
  const double *w = Wflat;
  for (int i = 0; i < N_; i++) {
    size_t n = (size_t)V_.glens[i] * r_[i];
    ops_.h2d(W_[i], w, n * sizeof(double));
    w += n;
  }
}
// core == nullptr: core = V x_i W_i^T from the current factors (TTMc(core, V, W, -1)); the value
// becomes the `core` argument (and the initial core_prev) of the next alsTucker_DT / _PP call
void TuckerEngine::set_core(const double *core) {
  finalize_rotations();
  if (core) {
    core_owed_ = false;
    ops_.h2d(core_.as<double>(), core, sizeof(double) * ncore_);
  } else
    compute_core_full();
}
void TuckerEngine::get_factors(double *Wflat, double *core) {
  finalize_rotations();
  double *w = Wflat;
  for (int i = 0; i < N_; i++) {
    size_t n = (size_t)V_.glens[i] * r_[i];
    if (w) {
      ops_.d2h(w, W_[i], n * sizeof(double));
      w += n;
    }
  }
  if (core) ops_.d2h(core, core_.as<double>(), sizeof(double) * ncore_);
}

// The model through a view: f = the view's unit-stride mode (its smallest stride),
// Z = core x_{i != f} W_i (the box's rows of each W_i) in fp64 by the mode products of the sweeps, and the
// kernel stores W_f Z^T with the lane index along mode f. Z and the intermediates of its chain stay within
// two buffers of 256 MB: the box is cut into slabs along the view's slowest mode s, which the chain
// expands first, so that every intermediate scales with the slab (a single row of s that alone needs
// more gets buffers of its size). The buffers and the transposed factors are kept for the session's
// next export (freeing them would wait for the device).
void TuckerEngine::export_model(const ViewArgs &a, void *dst, bool residual, void *stream) {
  finalize_rotations();  // (the path of get_factors: deferred checks settled, pending rotations applied)
  ModelBox bx;
  if (!dv_model_box(a, V_.glens, V_.row0, V_.llens[0], &bx)) return;
  int f = -1, s = -1;
  for (int m = 0; m < N_; m++)
    if (bx.len[m] > 1 && (f < 0 || bx.vs[m] < bx.vs[f])) f = m;
  if (f < 0) f = 0;
  for (int m = 0; m < N_; m++)
    if (m != f && bx.len[m] > 1 && (s < 0 || bx.vs[m] > bx.vs[s])) s = m;
  ModelExportCall call{&a, &V_, dst, residual, residual_form_, false, stream};
  model_slabs(bx, f, s, [&](const ModelPlan &mp, const double *Q, const double *Z) {
    model_export_run(ops_, call, mp, Q, Z, r_[f]);
  });
}

// The imputation: the stores go to the shard, so the plan follows the SHARD: f = mode 0,
// its fast side, is group A alone (the lane index of the store pass, and of the V reads of the observed
// residual), group B the other modes in the shard's order, which is the order Z has them in, and the
// slabs are cut along the shard's slowest mode. Per slab one launch of Ops::model_impute with
// Q = W_0 + lo_0, P = Z and K = r_0, the route that keeps Q in LDS when r_0 > 16. The slabs' sums are
// added on the host in order, then one scalar all-reduce.
// On a back end without device views the API's pointer check refuses the call before it gets here.
void TuckerEngine::impute(const ViewArgs &a, const void *mask, void *stream, double *observed_sq) {
  finalize_rotations();  // (as export_model: the factors and core get_factors would return now)
  ModelBox bx;
  double sq = 0;
  if (dv_model_box(a, V_.glens, V_.row0, V_.llens[0], &bx)) {
    int s = -1;
    for (int m = 1; m < N_; m++)
      if (bx.len[m] > 1) s = m;
    // (a slab's sum stays in a device slot of its own until a batch of slots is read in one copy: the host
    // does not wait between slabs, and adds the sums in slab order)
    constexpr int kSlots = 48;
    double *slot = scal_.as<double>() + 8;
    int used = 0;
    auto drain = [&] {
      double h[kSlots];
      if (used) ops_.d2h(h, slot, sizeof(double) * used);
      for (int i = 0; i < used; i++) sq += h[i];
      used = 0;
    };
    model_slabs(bx, 0, s, [&](const ModelPlan &mp, const double *Q, const double *Z) {
      ops_.model_impute(mp, Q, Z, r_[0], true, mask, V_.data, V_.dtype, observed_sq ? slot + used : nullptr,
                        stream);
      if (observed_sq && ++used == kSlots) drain();
    });
    drain();
    // the contents changed: every session on the tensor, this one too, rebuilds what it derived at its
    // next read (a rank none of whose rows lie in the box has changed nothing)
    if (V_.generation) ++*V_.generation;
  }
  if (!observed_sq) return;
  if (dist_) {
    ops_.h2d(scal_.as<double>() + 8, &sq, sizeof(double));
    comm_.allreduce_sum(scal_.as<double>() + 8, 1);
    ops_.d2h(&sq, scal_.as<double>() + 8, sizeof(double));
  }
  *observed_sq = sq;
}

// ppals_tucker_em: CpEngine::run_em with HOOI sweeps in place of the CP sweeps (lambda has no meaning here)
int TuckerEngine::run_em(const ViewArgs &a, const void *mask, void *stream, const CpOpts &o,
                         int inner_sweeps, int *iters, double *observed_res) {
  const double t0 = now();
  double sq = 0;
  int k = 0;
  bool on_tol = false, fresh = false;  // fresh: the tensor and sq belong to the current factors
  while (k < o.maxiter) {
    const bool look = k % o.resprint == 0;
    impute(a, mask, stream, look ? &sq : nullptr);
    fresh = look;
    if (look) {
      on_tol = std::sqrt(sq) <= o.tol;
      if (on_tol || agree(now() - t0 > o.timelimit)) break;
    }
    for (int i = 0; i < inner_sweeps; i++) sweep_dt();
    settle_all();  // (as ppals_tucker_sweeps_dt)
    fresh = false;
    k++;
  }
  if (!fresh) impute(a, mask, stream, &sq);
  if (iters) *iters = k;
  if (observed_res) *observed_res = std::sqrt(sq);
  return on_tol ? 1 : 0;
}

// The influence plot (tucker.h). The plan is the imputation's on the box of the whole local
// shard: f = mode 0 is group A, the slabs are cut along the last mode of extent > 1.
void TuckerEngine::slice_residuals(double *ss_host, double *total_host) {
  if (dist_) throw Unsupported("ppals: the per-slice residuals run on one rank");
  finalize_rotations();  // (as export_model: the factors and core get_factors would return now)
  ViewArgs a;
  std::string err;
  if (!dv_check_args(DV_EXPORT, N_, V_.glens, DV_F64, nullptr, nullptr, nullptr, &a, &err))
    throw std::runtime_error("ppals: " + err);
  ModelBox bx;
  if (!dv_model_box(a, V_.glens, V_.row0, V_.llens[0], &bx)) throw std::logic_error("ppals: empty shard");
  int s = -1;
  int64_t nout = 0, off[MAX_ORDER];
  for (int m = 0; m < N_; m++) {
    if (m >= 1 && bx.len[m] > 1) s = m;
    off[m] = nout;
    nout += V_.glens[m];
  }
  sl_out_.reserve(ops_, sizeof(double) * nout);
  double *out = sl_out_.as<double>();
  // the op frees its partial sums' buffer and takes a larger one as it needs (ops.h): handed over for the
  // call, taken back on every way out
  size_t work_bytes = sl_work_.size();
  void *work = sl_work_.release();
  bool first = true;
  int64_t done = 0;  // rows of the slab mode behind us
  try {
    model_slabs(bx, 0, s, [&](const ModelPlan &mp, const double *Q, const double *Z) {
      int64_t nb = 0;
      for (int j = 0; j < mp.gb.n; j++) nb += mp.gb.len[j];
      // (the first slab is the largest: the buffers move there or never, so no later slab waits for a free)
      sl_col_.reserve(ops_, sizeof(double) * mp.gb.count);
      sl_fold_.reserve(ops_, sizeof(double) * std::max<int64_t>(nb, 1));
      double *col = sl_col_.as<double>(), *fold = sl_fold_.as<double>();
      ops_.model_slice_sums(mp, Q, Z, r_[0], V_.data, V_.dtype, first, out, col, slice_work_cap_, work, work_bytes);
      if (mp.gb.n > 0) ops_.fold_slice_sums(col, mp.gb.len, mp.gb.n, fold);
      int64_t fo = 0, slab_len = 0;
      for (int j = 0; j < mp.gb.n; j++) {
        const int m = mp.gb.mode[j];
        const int64_t len = mp.gb.len[j];
        double *dst = out + off[m] + (m == s ? done : 0);
        if (m == s || first)
          ops_.d2d(dst, fold + fo, sizeof(double) * len);
        else
          ops_.add_inplace(dst, fold + fo, len);
        if (m == s) slab_len = len;
        fo += len;
      }
      done += slab_len;
      first = false;
    });
  } catch (...) {
    sl_work_ = DeviceBuffer(ops_, work, work_bytes);
    throw;
  }
  sl_work_ = DeviceBuffer(ops_, work, work_bytes);
  ops_.d2h(ss_host, out, sizeof(double) * nout);
  if (total_host) {
    double t = 0;
    for (int64_t x = 0; x < V_.glens[0]; x++) t += ss_host[x];
    *total_host = t;
  }
}

void TuckerEngine::leverages(double *lev_host) {
  if (dist_) throw Unsupported("ppals: the leverages run on one rank");
  finalize_rotations();
  int64_t nout = 0, most = 0;
  for (int i = 0; i < N_; i++) {
    nout += V_.glens[i];
    most = std::max(most, V_.glens[i] * r_[i]);
  }
  sl_out_.reserve(ops_, sizeof(double) * nout);
  sl_q_.reserve(ops_, sizeof(double) * most);
  double *out = sl_out_.as<double>(), *Qs = sl_q_.as<double>();
  bool bad = false;
  int64_t off = 0;
  for (int i = 0; i < N_ && !bad; i++) {
    const int64_t rows = V_.glens[i];
    ops_.d2d(Qs, W_[i], sizeof(double) * rows * r_[i]);
    if (!ops_.orthonormalize(Qs, rows, r_[i]))
      bad = true;  // rank deficient: no projector to speak of
    else
      ops_.row_dots(Qs, Qs, rows, r_[i], rows, out + off);
    off += rows;
  }
  if (bad) {
    ops_.sync();
    for (int64_t e = 0; e < nout; e++) lev_host[e] = std::numeric_limits<double>::quiet_NaN();
    return;
  }
  ops_.d2h(lev_host, out, sizeof(double) * nout);
}

// The slabs of box bx for fast mode f, cut along mode s (-1: none): the transposed factors, the chain
// buffers and, per slab, run(plan, Q = the box's rows of W_f, Z). Shared by the export and the imputation.
void TuckerEngine::model_slabs(const ModelBox &bx, int f, int s, const SlabRun &run) {
  std::vector<int> chain;
  if (s >= 0) chain.push_back(s);
  for (int m = 0; m < N_; m++)
    if (m != f && m != s) chain.push_back(m);
  // W_m^T (r_m x s_m) of the chain's modes, at offsets in mode order (mode f's slot stays unused)
  int64_t nwt = 0;
  for (int m = 0; m < N_; m++) nwt += V_.glens[m] * r_[m];
  xwt_.reserve(ops_, sizeof(double) * nwt);
  int64_t off = 0;
  for (int m = 0; m < N_; off += V_.glens[m] * r_[m], m++)
    if (m != f) ops_.transpose2d(W_[m], F64, V_.glens[m], r_[m], xwt_.as<double>() + off);
  // the largest intermediate of the chain per row of the slab mode, and the slab that fits
  constexpr int64_t budget = int64_t(1) << 25;  // doubles per buffer (256 MB)
  std::vector<int64_t> dims(r_.begin(), r_.end());
  int64_t unit = 1;
  for (int m : chain) {
    dims[m] = m == s ? 1 : bx.len[m];
    int64_t e = 1;
    for (int q = 0; q < N_; q++) e *= dims[q];
    unit = std::max(unit, e);
  }
  const int64_t ns = s >= 0 ? bx.len[s] : 1;
  const int64_t cs = std::max<int64_t>(1, std::min(ns, budget / unit));
  xz_[0].reserve(ops_, sizeof(double) * unit * cs);
  xz_[1].reserve(ops_, sizeof(double) * unit * cs);
  for (int64_t c = 0; c < ns; c += cs) {
    ModelBox sb = bx;
    if (s >= 0) {
      sb.lo[s] += c;
      sb.len[s] = std::min(cs, ns - c);
      sb.voff += c * bx.vs[s];
      sb.roff += c * bx.rs[s];
    }
    export_slab(sb, f, chain, run);
  }
}

void TuckerEngine::export_slab(const ModelBox &bx, int f, const std::vector<int> &chain, const SlabRun &run) {
  std::vector<int64_t> dims(r_.begin(), r_.end()), wtoff(N_, 0);
  for (int m = 1; m < N_; m++) wtoff[m] = wtoff[m - 1] + V_.glens[m - 1] * r_[m - 1];
  const double *cur = core_.as<double>();
  int pi = 0;
  for (int m : chain) {  // expansion of mode m: out[l, a, t] = sum_k cur[l, k, t] * W_m[lo_m + a, k]
    int64_t L = 1, T = 1;
    for (int q = 0; q < m; q++) L *= dims[q];
    for (int q = m + 1; q < N_; q++) T *= dims[q];
    ops_.ttm_keep(cur, F64, L, r_[m], T, xwt_.as<double>() + wtoff[m] + r_[m] * bx.lo[m], r_[m], (int)bx.len[m],
                  xz_[pi].as<double>());
    dims[m] = bx.len[m];
    cur = xz_[pi].as<double>();
    pi ^= 1;
  }
  // Z = cur: [modes before f | r_f | modes after f]; P[b, k] with b over the modes other than f
  ModelPlan mp;
  mp.ga.add(bx, f);
  for (int m = 0; m < N_; m++)
    if (m != f) mp.gb.add(bx, m);
  mp.voff = bx.voff;
  mp.roff = bx.roff;
  mp.ldq = V_.glens[f];
  mp.pL = 1;
  for (int q = 0; q < f; q++) mp.pL *= bx.len[q];
  mp.pLK = mp.pL * r_[f];
  run(mp, W_[f] + bx.lo[f], cur);
}

// hosvd (als_Tucker.cxx:12-70): W_i = leading eigenvectors of the Gram of the mode-i unfolding of
// V (K13), then core = V x_i W_i^T
void TuckerEngine::hosvd() {
  check_prep_epoch();
  settle_all();
  ms3_invalidate();
  for (int i = 0; i < N_; i++) {
    int64_t L = 1, T = 1;
    for (int q = 0; q < i; q++) L *= ext(q);
    for (int q = i + 1; q < N_; q++) T *= ext(q);
    if (dist_ && i == 0) {
      // the Gram of the sharded mode needs every pair of rows: gather the shards once (needs room
      // for two extra copies of the tensor; HOSVD is a one-off initialisation)
      const int64_t s0 = V_.glens[0], blk = block_rows(s0, P_);
      const size_t esz = dtype_size(V_.dtype);
      const int64_t chunk_bytes = ((blk * T * (int64_t)esz + 7) / 8) * 8;
      DeviceBuffer stage_buf(ops_, (size_t)chunk_bytes * P_), full_buf(ops_, (size_t)s0 * T * esz);
      char *stage = stage_buf.as<char>();
      void *full = full_buf.get();
      ops_.zero(stage, (size_t)chunk_bytes * P_);
      ops_.d2d(stage + (size_t)rank_ * chunk_bytes, V_.data, (size_t)V_.nloc * esz);
      comm_.allgather((const double *)(stage + (size_t)rank_ * chunk_bytes), (double *)stage,
                      chunk_bytes / 8);
      ops_.unpack_shards(stage, V_.dtype, s0, T, blk, P_, chunk_bytes, full);
      ops_.unfold_gram(full, V_.dtype, 1, s0, T, G_.as<double>());
      ops_.sync();
    } else {
      ops_.unfold_gram(V_.data, V_.dtype, L, V_.glens[i], T, G_.as<double>());
      if (dist_) comm_.allreduce_sum(G_.as<double>(), V_.glens[i] * V_.glens[i]);
    }
    // (slots 8.. : a cold start of their own — the Gram of the full unfolding has little to do
    // with the one the first HOOI sweep will see in slot i)
    ops_.top_eigvecs_warm(G_.as<double>(), V_.glens[i], r_[i], W_[i], eig_base_ + MAX_ORDER + i);
  }
  compute_core_full();
  ops_.d2d(core_prev_.as<double>(), core_.as<double>(), sizeof(double) * ncore_);
  ops_.sync();
}

// K12 (als_Tucker.cxx:399-406: Gram of the unfolding by unroll_tensor_contraction, then
// `MTM.svd(U,S,VT,rank)`): the factor is the r_i leading left singular vectors of the s_i x (L*T)
// unfolding Y_(i). The reference always takes them from the s_i x s_i Gram Y_(i) Y_(i)^T. When the
// unfolding is TALL (s_i > L*T: the long mode of an image stack, 7200 x 300 for the coil-100
// shape) the same vectors come from the small side: eigenvectors v_k of the (L*T)^2 Gram
// Y_(i)^T Y_(i), then u_k = Y_(i) v_k / |Y_(i) v_k| — same squared conditioning, O(s c^2) instead
// of O(s^3) work. The columns are re-orthonormalised (they are orthogonal only to
// eps * lambda_1 / lambda_k); a numerically rank-deficient unfolding takes the s_i x s_i route.
void TuckerEngine::factor_update(int i, const double *Y, int64_t L, int64_t T) {
  const int64_t s = V_.glens[i], c = L * T;
  if (thin_enabled_ && c < s && r_[i] <= c) {
    const int64_t need = s * c + c * r_[i];
    thin_.reserve(ops_, sizeof(double) * need);
    const double *Ym = Y;  // [s, c] with the mode fastest
    if (L > 1) {
      ops_.transpose_batched(Y, F64, L, s, T, thin_.as<double>());
      Ym = thin_.as<double>();
    }
    double *Vr = thin_.as<double>() + s * c;
    ops_.unfold_gram(Ym, F64, s, c, 1, G_.as<double>());  // c x c (c < s: fits G_.as<double>())
    // (a slot of its own: the c x c problem and the s x s fallback below are different sequences)
    ops_.top_eigvecs_warm(G_.as<double>(), c, r_[i], Vr, eig_base_ + 2 * MAX_ORDER + i);
    ops_.ttm_keep(Ym, F64, s, c, 1, Vr, c, r_[i], W_[i]);
    if (ops_.orthonormalize(W_[i], s, r_[i])) return;
  }
  // (a slot that defers its checks keeps the Gram itself: they are finished on a second stream)
  double *G = ops_.eig_gram(eig_base_ + i, s);
  if (!G) G = G_.as<double>();
  ops_.unfold_gram(Y, F64, L, s, T, G);
  ops_.top_eigvecs_warm(G, s, r_[i], W_[i], eig_base_ + i);
}

void TuckerEngine::sweep_dt() { sweep_body(nullptr); }

// one HOOI sweep; align_ref != nullptr: column signs aligned with that factor set after every
// eigen-step (alsTucker_DT_sub, als_Tucker.cxx:632-643)
void TuckerEngine::sweep_body(const DeviceBufferTable *align_ref) {
  check_prep_epoch();
  const bool may_defer = defer_enabled_ && align_ref == nullptr && !dist_;
  if (!may_defer) settle_all();
  for (auto &n : nodes_) n.valid = false;  // ttmc_map.clear(), als_Tucker.cxx:340
  for (int i = 0; i < N_; i++) {
    if (may_defer) settle_mode(i);
    mode_step(i, align_ref, may_defer);
  }
}

void TuckerEngine::mode_step(int i, const DeviceBufferTable *align_ref, bool may_defer) {
  int64_t L = 1, T = 1;
  double *Y = ms3_ ? ms3_leaf(i, &T) : nullptr;
  const bool from_ms3 = Y != nullptr;
  if (!from_ms3) {
    compute_node(leaf_[i]);
    const Node &lf = nodes_[leaf_[i]];
    for (int q = 0; q < i; q++) L *= r_[q];
    T = 1;
    for (int q = i + 1; q < N_; q++) T *= r_[q];
    if (lf.front) {  // [s_i | ranks of the other modes] (compute_left_half_on_vt)
      T = L * T;
      L = 1;
    }
    Y = complete_leaf(i, lf.buf.as<double>(), L * V_.glens[i] * T);
  }
  if (i == N_ - 1) {  // als_Tucker.cxx:395
    yend_T_ = T;
    // (one GPU: the leaf's own buffer stays as it is until this mode is stepped again — no copy)
    if (dist_) {
      ops_.d2d(Yend_.as<double>(), Y, sizeof(double) * yend_elems_);
      yend_src_ = Yend_.as<double>();
    } else {
      // (a multi-sweep leaf with its rank indices in descending mode order: the core is recomputed from
      // the tensor when somebody asks for it)
      yend_src_ = (from_ms3 && ms3_perm_) ? nullptr : Y;
    }
  }
  ops_.eig_lazy(eig_base_ + i, align_ref == nullptr && !dist_);
  ops_.eig_defer(eig_base_ + i, may_defer);
  if (may_defer) {
    // the step writes the new factor into the spare buffer; the one it replaces stays intact
    if (Wsave_.empty()) Wsave_.resize(N_);
    if (!Wsave_[i]) Wsave_.alloc(ops_, i, sizeof(double) * V_.glens[i] * r_[i]);
    W_.swap_entry(i, Wsave_);
  }
  factor_update(i, Y, L, T);  // K12
  ops_.eig_defer(eig_base_ + i, false);
  if (align_ref) ops_.sign_align(W_[i], (*align_ref)[i], V_.glens[i], r_[i]);
  // core = Y_end x_{N-1} W[N-1]  (als_Tucker.cxx:408): owed until somebody reads it (ensure_core) —
  // the print blocks recompute the core from the tensor anyway (als_Tucker.cxx:290), so inside a run
  // of sweeps this product (a launch-bound 30 us at cfg5) served nobody
  if (i == N_ - 1) core_owed_ = true;
  if (may_defer && (!defer_log_.empty() || ops_.eig_deferred(eig_base_ + i))) defer_log_.push_back(i);
}

void TuckerEngine::settle_mode(int i) {
  if (defer_log_.empty()) return;
  const int v = ops_.eig_verify(eig_base_ + i);
  if (v < 0) return;  // nothing of this mode is waiting
  if (defer_log_.front() != i) throw std::logic_error("ppals: deferred eigen-steps out of order");
  if (v == 1) {
    rollback_and_redo();
    return;
  }
  defer_log_.erase(defer_log_.begin());
  while (!defer_log_.empty() && !ops_.eig_deferred(eig_base_ + defer_log_.front()))
    defer_log_.erase(defer_log_.begin());  // (steps that were checked on the spot)
}

void TuckerEngine::settle_all() {
  while (!defer_log_.empty()) {
    const int i = defer_log_.front();
    if (ops_.eig_verify(eig_base_ + i) == 1) {
      rollback_and_redo();
      return;
    }
    defer_log_.erase(defer_log_.begin());
  }
}

// The oldest step of the log was not accepted: its factor and everything computed from it since
// is void. Every mode stepped since then gets back the factor that step replaced (a basis of the
// right subspace is all the sweep needs of it), unchecked steps among them are dropped, and the
// same steps are made again in the same order, each checked before the next one starts.
void TuckerEngine::rollback_and_redo() {
  const std::vector<int> steps = defer_log_;
  defer_log_.clear();
  defer_rollbacks_++;
  ms3_invalidate();
  ops_.sync();
  for (size_t k = 0; k < steps.size(); k++) {
    const int j = steps[k];
    if (k > 0) ops_.eig_verify(eig_base_ + j, true);
    W_.swap_entry(j, Wsave_);
    ops_.eig_rotation_done(eig_base_ + j);  // (the rotation owed belonged to the discarded factor)
  }
  for (int j : steps) {
    for (auto &n : nodes_) n.valid = false;
    ms3_invalidate();
    mode_step(j, nullptr, false);
  }
  ms3_invalidate();
  // (whatever the sweep in progress needs of the tree is rebuilt from the factors as they are now:
  // a leaf left valid here would be taken for this sweep's by the step that comes to it)
  for (auto &n : nodes_) n.valid = false;
}

// rank-agreed stop decision (see CpEngine::agree): the time limit reads a rank-local clock
bool TuckerEngine::agree(bool local) {
  if (!dist_) return local;
  double x = local ? 1.0 : 0.0, y = 0;
  ops_.h2d(scal_.as<double>() + 3, &x, sizeof(double));
  comm_.allreduce_sum(scal_.as<double>() + 3, 1);
  ops_.d2h(&y, scal_.as<double>() + 3, sizeof(double));
  return y > 0.0;
}

double TuckerEngine::core_norm() {
  ensure_core();
  ops_.sumsq(core_.as<double>(), ncore_, scal_.as<double>());
  ops_.sumsq(core_prev_.as<double>(), ncore_, scal_.as<double>() + 1);
  double h[2];
  ops_.d2h(h, scal_.as<double>(), sizeof(double) * 2);
  return std::fabs(std::sqrt(h[0]) - std::sqrt(h[1]));
}

// ||core x_i W_i - V||_F (als_Tucker.cxx:296-310) without materialising the model tensor: expand
// every mode but the last into Q (prod s_0..s_{N-2} x r_{N-1}), then V^ = Q W_{N-1}^T is streamed.
double TuckerEngine::residual() {
  ensure_core();
  std::vector<int64_t> dims(N_);
  for (int m = 0; m < N_; m++) dims[m] = r_[m];
  const double *cur = core_.as<double>();
  DeviceBuffer prev;
  for (int m = 0; m < N_ - 1; m++) {
    int64_t L = 1, T = 1;
    for (int q = 0; q < m; q++) L *= dims[q];
    for (int q = m + 1; q < N_; q++) T *= dims[q];
    // expansion: out[l, a, t] = sum_k cur[l,k,t] * W_m[a,k]  ==  ttm_keep with W^T (J=r, K=s)
    // W^T as a column-major r x s matrix is W (s x r, ld = s) read with swapped strides; build it.
    const int64_t sg = V_.glens[m], s = ext(m), r0 = (m == 0 ? V_.row0 : 0);
    const int rk = r_[m];
    std::vector<double> Wh((size_t)sg * rk), WT((size_t)s * rk);
    ops_.d2h(Wh.data(), W_[m], sizeof(double) * sg * rk);
    for (int64_t a = 0; a < s; a++)  // local rows of the sharded mode only
      for (int k = 0; k < rk; k++) WT[k + (size_t)rk * a] = Wh[(a + r0) + sg * k];
    DeviceBuffer WTd(ops_, sizeof(double) * s * rk);
    ops_.h2d(WTd.as<double>(), WT.data(), sizeof(double) * s * rk);
    DeviceBuffer dst(ops_, sizeof(double) * L * s * T);
    ops_.ttm_keep(cur, F64, L, rk, T, WTd.as<double>(), rk, (int)s, dst.as<double>());
    WTd.reset();
    prev = std::move(dst);
    cur = prev.as<double>();
    dims[m] = s;
  }
  int64_t M = 1;
  for (int m = 0; m < N_ - 1; m++) M *= ext(m);
  ops_.residual_sq(V_.data, V_.dtype, M, V_.glens[N_ - 1], cur, W_[N_ - 1], r_[N_ - 1], scal_.as<double>() + 2);
  if (dist_) comm_.allreduce_sum(scal_.as<double>() + 2, 1);
  double h = 0;
  ops_.d2h(&h, scal_.as<double>() + 2, sizeof(double));
  return std::sqrt(h);
}

int TuckerEngine::run_dt(const CpOpts &o, int *iters) {
  RunReport rep(o, rank_ == 0, V_.glens[0], "diffnorm");
  ensure_core();
  ops_.d2d(core_prev_.as<double>(), core_.as<double>(), sizeof(double) * ncore_);  // Tensor<> core_prev(core)
  double diffnorm = 1000;
  int iter;
  for (iter = 0; iter <= o.maxiter; iter++) {
    if ((iter % o.resprint == 0 && iter != 0) || iter == 1 || iter == o.maxiter) {
      if (print_block(rep, o, iter, 0, diffnorm, false)) break;
    }
    sweep_dt();
    rep.dot(iter);
  }
  settle_all();
  ops_.sync();
  rep.finish(iter, "Diff", diffnorm);
  if (iters) *iters = iter;
  return iter == o.maxiter + 1 ? 0 : 1;
}

// ============================================================================ Tucker PP
static std::string tk_all_but(int N, int i, int j = -1) {
  std::string s;
  for (int m = 0; m < N; m++)
    if (m != i && m != j) s.push_back((char)('a' + m));
  return s;
}

// Build_ttmc_map (als_Tucker.cxx:426-466): key = contracted modes (ascending), recursion drops the
// last one; every contraction keeps the tensor order. Level 1 scans V (K11), deeper levels
// contract the cached fp64 intermediate.
const TuckerEngine::PPOp &TuckerEngine::pp_get(const std::string &args) {
  check_tensor_generation();
  auto it = pp_.find(args);
  if (it != pp_.end()) return it->second;
  const int mode = args.back() - 'a';
  PPOp op;
  const void *src;
  int dt;
  if (args.size() == 1) {
    op.dims.resize(N_);
    for (int m = 0; m < N_; m++) op.dims[m] = ext(m);
    src = V_.data;
    dt = V_.dtype;
  } else {
    const PPOp &par = pp_get(args.substr(0, args.size() - 1));
    op.dims = par.dims;
    src = par.buf.as<double>();
    dt = F64;
  }
  int64_t L = 1, T = 1;
  for (int q = 0; q < mode; q++) L *= op.dims[q];
  for (int q = mode + 1; q < N_; q++) T *= op.dims[q];
  const int64_t J = op.dims[mode];
  op.dims[mode] = r_[mode];
  op.elems = L * r_[mode] * T;
  op.buf = DeviceBuffer(ops_, sizeof(double) * op.elems);
  ops_.ttm_keep(src, dt, L, J, T, wptr(mode), V_.glens[mode], r_[mode], op.buf.as<double>());
  return pp_[args] = std::move(op);
}
void TuckerEngine::pp_clear() { pp_.clear(); }

// one approximate sweep (als_Tucker.cxx:824-891): Y_i = Y_i^0 + sum_{j != i} T_ij x_j dW_j
void TuckerEngine::sweep_pp() {
  ms3_invalidate();  // (PP moves the factors without touching the multi-sweep intermediate)
  for (int i = 0; i < N_; i++) {
    const PPOp &Y0 = pp_get(tk_all_but(N_, i));
    Yacc_.reserve(ops_, sizeof(double) * Y0.elems);
    Ytmp_.reserve(ops_, sizeof(double) * Y0.elems);
    ops_.d2d(Yacc_.as<double>(), Y0.buf.as<double>(), sizeof(double) * Y0.elems);
    for (int ii = 0; ii < N_; ii++) {
      if (ii == i) continue;
      const PPOp &Tp = pp_get(tk_all_but(N_, std::min(i, ii), std::max(i, ii)));
      int64_t L = 1, T = 1;
      for (int q = 0; q < ii; q++) L *= Tp.dims[q];
      for (int q = ii + 1; q < N_; q++) T *= Tp.dims[q];
      // sharded mode: the local rows of dW_0 (the operator keeps the local extent of mode 0)
      const double *dwp = dW_[ii] + (ii == 0 ? V_.row0 : 0);
      ops_.ttm_keep(Tp.buf.as<double>(), F64, L, ext(ii), T, dwp, V_.glens[ii], r_[ii], Ytmp_.as<double>());
      ops_.add_inplace(Yacc_.as<double>(), Ytmp_.as<double>(), Y0.elems);
    }
    int64_t L = 1, T = 1;
    for (int q = 0; q < i; q++) L *= r_[q];
    for (int q = i + 1; q < N_; q++) T *= r_[q];
    double *Y = Yacc_.as<double>();
    if (dist_) {
      // same completion as the exact sweep: partial sums are all-reduced, the rows of the sharded
      // mode gathered (from a copy padded to the uniform block height)
      if (i == 0) {
        const int64_t blk = block_rows(V_.glens[0], P_);
        Ytmp_.reserve(ops_, sizeof(double) * blk * T);
        ops_.pack_blocks(Yacc_.as<double>(), ext(0), ext(0), (int)T, blk, 1, Ytmp_.as<double>());
        Y = complete_leaf(0, Ytmp_.as<double>(), blk * T);
      } else {
        Y = complete_leaf(i, Yacc_.as<double>(), Y0.elems);
      }
    }
    if (i == N_ - 1) ops_.d2d(Yend_.as<double>(), Y, sizeof(double) * yend_elems_);
    // (the PP phase differences the eigenvectors one by one: never "any basis of the subspace",
    // whatever the slot's last exact sweep allowed — pp_bench enters here without a dt_sub)
    ops_.eig_lazy(eig_base_ + i, false);
    factor_update(i, Y, L, T);  // K12
    ops_.sign_align(W_[i], Winit_[i], V_.glens[i], r_[i]);  // als_Tucker.cxx:874-885
    double *A[1] = {W_[i]}, *B[1] = {Winit_[i]}, *D[1] = {dW_[i]};
    int64_t n[1] = {V_.glens[i] * r_[i]};
    ops_.diff_norms(A, B, n, 1, 1, D, 0, scal_.as<double>() + 4);  // dW = W - W_init (als_Tucker.cxx:887)
  }
  int64_t L = ncore_ / r_[N_ - 1];
  core_owed_ = false;
  ops_.ttm_keep(Yend_.as<double>(), F64, L, V_.glens[N_ - 1], 1, W_[N_ - 1], V_.glens[N_ - 1], r_[N_ - 1],
                core_.as<double>());
}

// print block (als_Tucker.cxx:288-338 / :521-564 / :764-822); bench: pp_bench's timings instead of
// the row. (pp_bench's PP phase has no deferred eigen-step to settle: run_pp settled them all.)
bool TuckerEngine::print_block(RunReport &rep, const CpOpts &o, int iter, int pp_flag,
                               double &diffnorm, bool stop_at_maxiter) {
  settle_all();
  ops_.sync();
  double diffV = 0;
  rep.off_clock([&] {
    compute_core_full();  // TTMc(core, V, W, -1)
    diffnorm = core_norm();
    diffV = residual();
  });
  if (!o.bench)
    rep.row(iter, diffnorm, pp_flag, diffV);
  else if (pp_flag)
    rep.pp_bench_time(iter, o.maxiter);
  else
    rep.dt_bench_time();
  if (agree(diffnorm < o.tol || rep.elapsed() > o.timelimit ||
            (stop_at_maxiter && iter == o.maxiter)))
    return true;
  ops_.d2d(core_prev_.as<double>(), core_.as<double>(), sizeof(double) * ncore_);
  return false;
}

ModeNorms TuckerEngine::read_norms(bool dt_phase) {
  int64_t n[MAX_ORDER];
  for (int i = 0; i < N_; i++) n[i] = V_.glens[i] * r_[i];
  ops_.diff_norms(W_.data(), dt_phase ? Wprev_.data() : nullptr, n, N_, dt_phase, dW_.data(),
                  dt_phase, scal_.as<double>() + 8);
  return ModeNorms(ops_, scal_.as<double>() + 8, N_);
}

// alsTucker_DT_sub (als_Tucker.cxx:476-669)
void TuckerEngine::dt_sub(RunReport &rep, const CpOpts &o, double tol_init, double &diffnorm,
                          int &iter) {
  for (int i = 0; i < N_; i++) ops_.zero(Wprev_[i], sizeof(double) * V_.glens[i] * r_[i]);
  for (; iter <= o.maxiter; iter++) {
    if ((iter % o.resprint == 0 && iter != 0) || iter == 1 || iter == o.maxiter) {
      if (print_block(rep, o, iter, 0, diffnorm, false)) break;
    }
    sweep_body(&Wprev_);
    if (read_norms(true).count(tol_init, false) == N_) return;
    rep.dot(iter);
  }
}

// alsTucker_PP_sub (als_Tucker.cxx:679-896); o.bench: pp_bench's form (:722-730 no restart test,
// :799-814 [PPfirst]/[PPsecond], :892-893 iter++ on exit)
void TuckerEngine::pp_sub(RunReport &rep, const CpOpts &o, double tol_init, double &diffnorm,
                          int &iter) {
  const int init_iter = iter;
  rep.start_pp_phase();
  for (; iter <= o.maxiter; iter++) {
    const int num_dw_break = o.bench ? 0 : read_norms(false).count(tol_init, true);
    if (iter == init_iter || num_dw_break > 0) {
      if (num_dw_break > 0) return;
      for (int j = 0; j < N_; j++) {
        size_t n = sizeof(double) * V_.glens[j] * r_[j];
        ops_.d2d(Winit_[j], W_[j], n);
        ops_.zero(dW_[j], n);
      }
      pp_clear();
      for (int ii = 0; ii < N_; ii++)
        for (int jj = ii + 1; jj < N_; jj++) pp_get(tk_all_but(N_, ii, jj));
      for (int ii = 0; ii < N_; ii++) pp_get(tk_all_but(N_, ii));
    }
    if ((iter % o.resprint == 0 && iter != 0) || iter == 1 || iter == o.maxiter ||
        iter == init_iter) {
      if (print_block(rep, o, iter, 1, diffnorm, true)) break;
    }
    sweep_pp();
  }
  if (o.bench) iter++;
}

int TuckerEngine::run_pp(const CpOpts &o, int *iters) {
  finalize_rotations();  // the PP phases difference the eigenvectors themselves
  for (int i = 0; i < N_; i++) ops_.eig_lazy(eig_base_ + i, false);
  if (Wprev_.empty()) {
    Wprev_.resize(N_);
    Winit_.resize(N_);
    dW_.resize(N_);
  }
  for (int i = 0; i < N_; i++) {
    size_t n = sizeof(double) * V_.glens[i] * r_[i];
    if (!Wprev_[i]) Wprev_.alloc(ops_, i, n);
    if (!Winit_[i]) Winit_.alloc(ops_, i, n);
    if (!dW_[i]) dW_.alloc(ops_, i, n);
  }
  for (int i = 0; i < N_; i++) ops_.zero(dW_[i], sizeof(double) * V_.glens[i] * r_[i]);
  RunReport rep(o, rank_ == 0, V_.glens[0], "diffnorm");
  int iter = 0;
  ops_.d2d(core_prev_.as<double>(), core_.as<double>(), sizeof(double) * ncore_);  // Tensor<> core_prev(core)
  double diffnorm = 10.;
  double tol_init = o.tol_init;
  while (diffnorm > o.tol && iter <= o.maxiter) {
    if (!o.bench) {
      rep.starts("DT", iter);
      dt_sub(rep, o, tol_init, diffnorm, iter);
    }
    rep.starts("pairwise perturbation", iter);
    pp_sub(rep, o, tol_init, diffnorm, iter);
    if (tol_init > 5e-3) tol_init *= 0.9;  // als_Tucker.cxx:947-948
    if (agree(rep.elapsed() > o.timelimit)) break;
  }
  ops_.sync();
  pp_clear();
  rep.finish(iter, "Diff", diffnorm);
  if (iters) *iters = iter;
  return iter == o.maxiter + 1 ? 0 : 1;
}

}  // namespace ppals
