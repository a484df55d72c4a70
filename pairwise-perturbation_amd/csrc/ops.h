// ops.h — the device-operation and collective interfaces the ALS engine is written against.
//
// engine.cpp contains only control flow (which contraction, which cache, which collective, when to
// restart PP — the part of the reference that is "pure algorithm orchestration") and
// talks to the hardware through these two abstract classes. The product implements them with
// hand-written HIP kernels (hip_ops.hip) and RCCL (rccl_comm.cpp). tests/hostsim/ implements them
// with plain host loops + callbacks so the engine's host logic and the multi-rank shard plan can be
// exercised on a CPU-only box (test infrastructure, never shipped in libppals.so).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <string>
#include <vector>

#include "bf16.h"
#include "device_view.h"
#include "pack_codec.h"
#include "preload_policy.h"

namespace ppals {

// BF16 (= PPALS_BF16) is a storage type of the resident tensor only: everything computed from it
// (tree nodes, the multi-sweep intermediate, PP operators, caches) is held in work_dt(BF16) = F32
// or wider. F16 (= PPALS_F16) is never a storage type.
enum DType { F32 = 0, F64 = 1, BF16 = 3 };
inline size_t dtype_size(int dt) { return dt == F32 ? 4 : (dt == BF16 ? 2 : 8); }
// the precision of an intermediate "in the tensor's own precision"
inline int work_dt(int storage) { return storage == BF16 ? F32 : storage; }

// row blocks of a padded layout: `ld` stored rows per block, the first `valid` of them real
struct RowPad {
  int64_t ld = 0, valid = 0;  // ld == 0: not padded
};

// The packed twin (28 or 26 bits per element) of a resident fp32 layout for ONE scan shape [L, J, T]
// (formats: kernels_pack.hip.h, pack_codec.h). A block is 256 rows x 16 reduction indices: a code
// plane and four k-quads; a short last k-block stores only the quads that reach below J. A 26-bit
// twin keeps the upper code bits of its few wide blocks in escape planes beside the blocks.
struct PackedSrc {
  const void *data = nullptr;   // the blocks: pack_tile_bytes(format, J) per (row tile, batch)
  const void *bases = nullptr;  // the side words: one 32-bit word per block
  const void *esc = nullptr;    // format 26: PACK26_ESC_BYTES per escape block, by ordinal
  int format = 0;               // PACK_FMT28 / PACK_FMT26
  int64_t escapes = 0;          // escape blocks
  int64_t L = 0, J = 0, T = 0;
};
inline int64_t pack_tiles(int64_t L, int64_t T) { return (L + 255) / 256 * T; }
inline int64_t pack_blocks_of(int64_t L, int64_t J, int64_t T) { return pack_tiles(L, T) * ((J + 15) / 16); }
inline size_t pack_data_bytes(int fmt, int64_t L, int64_t J, int64_t T) {
  return (size_t)pack_tiles(L, T) * (size_t)pack_tile_bytes(fmt, J);
}
inline size_t pack_base_bytes(int64_t L, int64_t J, int64_t T) { return (size_t)pack_blocks_of(L, J, T) * 4; }
// what pack_survey found: the largest spread of top bytes in a block (-1: this back end, or this
// shape, has no packed scans) and the blocks whose spread needs an escape plane in format 26
struct PackSurvey {
  int spread = -1;
  int64_t escapes = 0;
};

constexpr int MAX_ORDER = 8;
// the floor of a non-negative factor entry (PPALS_NN_FLOOR of the C ABI): not zero, so that no column
// can die and make Normalize divide by zero
constexpr double kNnFloor = 1e-16;
// the orthonormal mode update leaves a factor as it is when the eigenvalues theta of M^T M have
// theta_min <= theta_max * 2^-40 (PPALS_ORTHO_MIN_RATIO of the C ABI): u kappa(M)^2 is 2^-13 there
constexpr double kOrthoMinRatio = 0x1p-40;
// the kind of a mode's update (PPALS_MODE_* of the C ABI)
enum ModeKind { kModeFree = 0, kModeNonneg = 1, kModeFixed = 2, kModeOrtho = 3 };
// the shape of a NONNEG mode's columns (PPALS_SHAPE_* of the C ABI)
enum ModeShape { kShapeNone = 0, kShapeUnimodal = 1, kShapeIncreasing = 2, kShapeDecreasing = 3 };
// the shaped update's column loop (kernels_shape.hip.h) keeps S (R^2 doubles, R the largest rank of the call) and
// its work arrays of shape_work_bytes(rows) in LDS while both fit in kShapeLdsBytes — 152 of the 160 KiB a
// gfx950 workgroup may declare, the rest for its static arrays — and the work arrays in global memory above
constexpr size_t kShapeLdsBytes = 152 * 1024;
inline size_t shape_work_bytes(int64_t rows) { return 64 * (size_t)rows + 8; }

// a factor-matrix operand of a Khatri-Rao product: `rows` rows starting at `ptr`, leading dim ld
// The starts of a multi-start session whose ranks differ (a rank sweep), handed to the ragged ops — and to
// their kernels BY VALUE, as a kernel argument: start b has rank col[b+1] - col[b], owns the columns
// [col[b], col[b+1]) of every factor, gradient and MTTKRP result; sq[b] = sum_{c<b} R_c^2 is its offset into
// S / Sinv, N * sq[b] the offset of its N Grams.
constexpr int kMaxStarts = 32;
struct StartTable {
  int nstarts = 0;
  int col[kMaxStarts + 1] = {0};
  int sq[kMaxStarts + 1] = {0};
  int rank(int b) const { return col[b + 1] - col[b]; }
  int max_rank() const {
    int m = 0;
    for (int b = 0; b < nstarts; b++) m = rank(b) > m ? rank(b) : m;
    return m;
  }
};
struct FactorRef {
  const double *ptr;
  int64_t rows;
  int64_t ld;
};

// one first-order correction term of a PP mode update (als_CP.cxx:778-794): a pair operator
// T (two modes + the rank index, fp64) contracted over its mode of extent ny with dW (ny x R, lddw)
struct PPTerm {
  const double *T;
  int64_t ny;
  int keep_first;  // 1: T[x + rows*(y + ny*r)] (the kept mode is stored fastest), 0: T[y + ny*(x + rows*r)]
  const double *dW;
  int64_t lddw;
};

struct ProfileSlot {
  int64_t launches = 0;
  double ms = 0;
  double bytes = 0;
};

class Ops {
 public:
  virtual ~Ops() {}
  // ---- memory (all pointers returned by alloc are "device" pointers of this Ops) ----
  virtual void *alloc(size_t bytes) = 0;
  virtual void free(void *p) = 0;
  virtual void h2d(void *dst, const void *src, size_t bytes) = 0;  // returns when dst is usable
  virtual void d2h(void *dst, const void *src, size_t bytes) = 0;  // synchronises the stream
  virtual void d2d(void *dst, const void *src, size_t bytes) = 0;  // stream-ordered
  virtual void zero(void *p, size_t bytes) = 0;
  virtual void sync() = 0;
  virtual void *stream() { return nullptr; }
  virtual void bind() {}  // make this Ops' device current on the calling thread
  // whether the tensor kernels of this back end can hold a tensor stored as `dt`
  virtual bool supports_storage(int dt) { return dt == F32 || dt == F64; }

  // ---- tensor generation / norms ----
  // V[e_local] = lo + (hi-lo)*u01(seed, global linear index); local shard = rows [row0,row0+l0)
  // of a leading mode of global extent g0; `rest` = product of the other extents
  virtual void fill_uniform(void *V, int dt, int64_t l0, int64_t g0, int64_t row0, int64_t rest,
                            uint64_t seed, double lo, double hi) = 0;
  // `-tensor p/p2` (laplacian_tensor, common.cxx:575-642): the element with global linear index e
  // has `ndigits` base-s digits (a_1,b_1,...,a_d,b_d); value = sum_k D[a_k,b_k] prod_{j!=k}
  // [a_j==b_j], D = tridiag(-1,2,-1)
  virtual void fill_laplacian(void *V, int dt, int64_t l0, int64_t g0, int64_t row0, int64_t rest,
                              int ndigits, int s) = 0;
  // V[e] += alpha * (lo + (hi-lo)*u01(seed, global index))   (`-tensor c` noise, test_ALS.cxx:259-264)
  virtual void add_uniform_noise(void *V, int dt, int64_t l0, int64_t g0, int64_t row0,
                                 int64_t rest, uint64_t seed, double lo, double hi,
                                 double alpha) = 0;
  // *out = sum over the local elements of (lo + (hi-lo)*u01(seed, global index))^2
  virtual void uniform_sumsq(int64_t l0, int64_t g0, int64_t row0, int64_t rest, uint64_t seed,
                             double lo, double hi, double *out) = 0;
  // V[m,k] = sum_r Q[m,r]*P[k,r]  (Q: M x R, P: K x R, column-major fp64)   (build_V)
  virtual void fill_rank(void *V, int dt, int64_t M, int64_t K, const double *Q, const double *P,
                         int R) = 0;
  // *out (device scalar) = sum_{m,k} (V[m,k] - sum_r Q[m,r]P[k,r])^2 ; Q==nullptr: sum V^2
  virtual void residual_sq(const void *V, int dt, int64_t M, int64_t K, const double *Q,
                           const double *P, int R, double *out) = 0;
  // upload fp64 host rows into the local shard (converting to dt): host is the FULL tensor
  virtual void upload_shard(void *V, int dt, const double *host_full, int64_t l0, int64_t g0,
                            int64_t row0, int64_t rest) = 0;

  // the reverse: the local shard's rows, widened to fp64, into their places of the FULL host tensor
  // (rows of other ranks are left untouched). Synchronises.
  virtual void download_shard(const void *V, int dt, double *host_full, int64_t l0, int64_t g0,
                              int64_t row0, int64_t rest) = 0;

  // dst[c + cols*r] = src[r + rows*c] (same element type dt): builds the second resident layout
  // of the tensor (right-half modes fastest) so that BOTH first-level tree nodes are suffix scans
  virtual void transpose2d(const void *src, int dt, int64_t rows, int64_t cols, void *dst) = 0;
  // `batch` independent transposes of consecutive rows x cols blocks:
  //   dst[c + cols*(r + rows*b)] = src[r + rows*(c + cols*b)]
  virtual void transpose_batched(const void *src, int dt, int64_t rows, int64_t cols, int64_t batch,
                                 void *dst) {
    const size_t step = (size_t)rows * cols * dtype_size(dt);
    for (int64_t b = 0; b < batch; b++)
      transpose2d((const char *)src + b * step, dt, rows, cols, (char *)dst + b * step);
  }
  // A resident layout whose leading block of `blk` elements is padded to `ld` (a multiple of
  // 128 B), optionally transposing on the way:
  //   dst[(c % blk) + ld*(c / blk + (cols / blk)*r)] = src[r + rows*c]    (cols % blk == 0)
  // rows == 1 is a plain pitched copy. Pad elements are set to zero. See CpEngine::build_layouts.
  virtual void pad_layout(const void *src, int dt, int64_t rows, int64_t cols, int64_t blk,
                          int64_t ld, void *dst) = 0;
  // full[a + s0*c] = stage_p[(a - p*blk) + l_p*c] for the rank p that owns row a (l_p rows each,
  // element type dt); stage_p starts at byte offset p*chunk_bytes. Re-assembles the leading-mode
  // shards of a tensor after an all-gather (Tucker HOSVD of the sharded mode).
  virtual void unpack_shards(const void *stage, int dt, int64_t s0, int64_t rest, int64_t blk,
                             int P, int64_t chunk_bytes, void *full) = 0;
  // alloc that returns nullptr instead of throwing when the device is out of memory
  virtual void *try_alloc(size_t bytes) { return alloc(bytes); }
  // how the next scans store a large result: -1 the back end's rule, 0 ordinary, 1 non-temporal
  virtual void scan_store_mode(int mode) { (void)mode; }
  // free device memory in bytes, (size_t)-1: unknown / unlimited
  virtual size_t mem_available() { return (size_t)-1; }
  // Packed twins of fp32 layouts (PackedSrc), in two steps so that the caller can choose the format
  // (pack_choose_format) and size the buffers in between. pack_survey looks at src viewed as
  // [L, J, T] and leaves a provisional word per block in `bases` (pack_base_bytes); a back end
  // without packed scans answers spread -1 and never sees a PackedSrc. pack_write (after a survey of
  // the same contents whose spread is below PACK_WINDOW) finishes the side words for `format` and fills
  // `data` (pack_data_bytes) and, in format 26, `esc` (PACK26_ESC_BYTES per surveyed escape block).
  // Both synchronise.
  virtual PackSurvey pack_survey(const void * /*src*/, int /*dt*/, int64_t /*L*/, int64_t /*J*/, int64_t /*T*/,
                                 void * /*bases*/) {
    return PackSurvey();
  }
  virtual void pack_write(const void * /*src*/, int64_t /*L*/, int64_t /*J*/, int64_t /*T*/, int /*format*/,
                          void * /*bases*/, void * /*data*/, void * /*esc*/) {}
  // the packed twin of the tensor the NEXT scan_contract calls read (nullptr: none). A scan whose
  // shape matches and whose launch is eligible (fp32, at most 16 result columns, the buffer-load
  // route, unpadded, no k-split) reads the twin instead of V; every other scan reads V. The
  // results are the same bits either way.
  virtual void scan_packed_source(const PackedSrc * /*pk*/) {}
  // launches of the packed scan kernel by this back end so far
  virtual int64_t scan_packed_launches() { return 0; }

  // ---- strided device views (ppals_tensor_import_device / _export_device, device_view.h) ----
  // What the runtime knows of a pointer. is_device: device memory of this Ops' device (not host,
  // pinned host or managed memory); [base, base + size): the allocation holding it. false: the
  // runtime does not know the pointer at all (*why says so).
  struct PtrInfo {
    bool is_device = false;
    int device = -1;
    uint64_t base = 0, size = 0;
  };
  virtual bool device_ptr_info(const void * /*p*/, PtrInfo * /*out*/, std::string * /*why*/) {
    throw Unsupported("ppals: this back end has no device views");
  }
  // Copy what `plan` (dv_plan) describes between the view at `view` (element type vdt, offset by
  // plan.voff) and the shard V (element type dt, offset by plan.roff): dir DV_IMPORT writes the
  // shard, DV_EXPORT the view. Ordered after the work queued on `caller_stream` so far, and work
  // queued there later runs after the copy; the host does not block.
  virtual void copy_view(const ViewPlan & /*plan*/, int /*dir*/, void * /*view*/, int /*vdt*/,
                         void * /*V*/, int /*dt*/, void * /*caller_stream*/) {
    throw Unsupported("ppals: this back end has no device views");
  }
  // A thin-K product stored through a view (the model export, device_view.h ModelPlan):
  //   view[voff + offA(a) + offB(b)] = sum_{k<K} Q[a + ldq*k] * P[(b % pL) + pLK*(b / pL) + pL*k]
  // in fp64, rounded once to vdt (F32 / F64). residual: V[roff + rA(a) + rB(b)] - the sum instead, V
  // the shard (storage type dt). Ordered on `caller_stream` as copy_view; the host does not block.
  virtual void model_to_view(const ModelPlan & /*mp*/, const double * /*Q*/, const double * /*P*/,
                             int /*K*/, bool /*residual*/, void * /*view*/, int /*vdt*/,
                             const void * /*V*/, int /*dt*/, void * /*caller_stream*/) {
    throw Unsupported("ppals: this back end has no device views");
  }
  // The imputation (ppals_cp_impute_device, ppals_tucker_impute_device): where the byte of the mask view is 0,
  //   V[roff + rA(a) + rB(b)] = the sum above, in fp64, rounded once to the storage type dt,
  // and every other element of the shard V stays as it is. Here group A follows the SHARD's fast side and
  // the view of the plan (vs, voff) is the mask, one byte per element. sumsq (device scalar, may be
  // nullptr): the sum of (V - that sum)^2 over the elements whose byte is not 0, V as stored, formed in
  // fp64 and added up in a fixed order. Ordered on `caller_stream` as copy_view; the host does not block.
  // wide_k: the caller's K is habitually above 16 (a Tucker session's leading core rank, up to 112; dt
  // F32 or F64): such a K takes the kernel that keeps Q in LDS. false (CP sessions): the routes CP
  // imputation has always had.
  virtual void model_impute(const ModelPlan & /*mp*/, const double * /*Q*/, const double * /*P*/,
                            int /*K*/, bool /*wide_k*/, const void * /*mask*/, void * /*V*/, int /*dt*/,
                            double * /*sumsq*/, void * /*caller_stream*/) {
    throw Unsupported("ppals: this back end has no device views");
  }

  // The weighted step (ppals_cp_wls_device): every element of the plan's box of the shard V becomes
  //   z = x where h >= 1,  the model sum where h <= 0 or NaN,  fma(h, x - sum, sum) otherwise,
  // rounded once to the storage type dt (F32 / F64), x and h the elements of the data view (the plan's vs /
  // voff, as model_impute's mask) and of the weights view (`ws`, dv_model_side), both of type vdt (DV_F32 /
  // DV_F64). Group A follows the SHARD's fast side; the sum over k runs in model_impute's order, so weights
  // in {0, 1} store the imputation's bits. sumsq (device scalar, may be nullptr): the loss, sum of
  // min(h, 1) (x - sum)^2 over the elements with h > 0, in fp64, in a fixed order. 1 <= K <= 128. Ordered on
  // `caller_stream` as copy_view; the host does not block.
  virtual void model_wls(const ModelPlan & /*mp*/, const ModelSide & /*ws*/, const double * /*Q*/,
                         const double * /*P*/, int /*K*/, const void * /*data*/, const void * /*weights*/,
                         int /*vdt*/, void * /*V*/, int /*dt*/, double * /*sumsq*/, void * /*caller_stream*/) {
    throw Unsupported("ppals: this back end has no device views");
  }

  // The Huber step (ppals_cp_huber_device): model_wls with a clipping threshold c > 0 (+inf: model_wls's
  // bits and loss). Where h > 0 and |x - sum| > c the value stored is sum +- c (h >= 1) or
  // fma(h, +-c, sum), the loss contribution min(h, 1) c (2 |x - sum| - c), and the element counts as clipped.
  // ws == nullptr: no weights view, h = 1 everywhere (`weights` is not read). loss_clipped (device, two
  // doubles, may be nullptr): the loss and the clipped count, both in a fixed order.
  virtual void model_huber(const ModelPlan & /*mp*/, const ModelSide * /*ws*/, const double * /*Q*/,
                           const double * /*P*/, int /*K*/, const void * /*data*/, const void * /*weights*/,
                           int /*vdt*/, void * /*V*/, int /*dt*/, double /*c*/, double * /*loss_clipped*/,
                           void * /*caller_stream*/) {
    throw Unsupported("ppals: this back end has no device views");
  }
  // One pass of the radix select of ppals_cp_abs_residual_quantile: over the elements of the plan's box with
  // h > 0 (all with ws == nullptr), key = the fp32 pattern of (float)|x - sum| (every NaN: 0x7fc00000);
  // hist[(key >> shift) & mask] counts the keys with key >> pshift == prefix. `hist`: ABSRES_BINS counts on
  // the HOST; the call waits for them. Integer counts: the same for every grid. Reads no tensor.
  static constexpr int ABSRES_BINS = 2048;
  virtual void model_absres_hist(const ModelPlan & /*mp*/, const ModelSide * /*ws*/, const double * /*Q*/,
                                 const double * /*P*/, int /*K*/, const void * /*data*/, const void * /*weights*/,
                                 int /*vdt*/, int /*pshift*/, uint32_t /*prefix*/, int /*shift*/, uint32_t /*mask*/,
                                 uint64_t * /*hist*/, void * /*caller_stream*/) {
    throw Unsupported("ppals: this back end has no device views");
  }

  // PARAFAC2 (ppals_parafac2_*): the projection step on a device view X of extents I x J x K
  // with unit stride in mode 0. parafac2_check refuses where the back end has no device views and does
  // nothing else; parafac2_init writes the first R identity columns into every I x R slice of P.
  // parafac2_step, in a number of launches that does not depend on the extents, for every slice k:
  //   Q_k = X_k A diag(C[k, :]) B^T                        (I x R, fp64, column-major at Q + I R k)
  //   C_k = Q_k^T Q_k = U diag(theta) U^T; status[k] = 1 under the rule of cp_mode_update_ortho_ragged
  //   (converged Jacobi, every theta positive and finite, theta_min > theta_max * min_ratio), else 0
  //   P_k = Q_k U diag(theta^-1/2) U^T where status[k] is 1; P_k as it was otherwise
  //   Y[:, j, k] = P_k^T X_k[:, j], rounded once to the storage type dt (F32 or F64), r fastest
  // out (device, 3 doubles, may be nullptr): sum x^2, sum y^2 (fp64, before the rounding) and the number of
  // slices whose status is 0, each formed in a fixed order. The reads of X are ordered after what
  // caller_stream holds, and what the caller queues there later waits for them.
  struct Parafac2Step {
    int64_t I = 0, J = 0, K = 0;
    int R = 0;
    const void *X = nullptr;
    int vdt = 0;                // DV_F32 or DV_F64
    int64_t s1 = 0, s2 = 0;     // the element strides of modes 1 and 2
    const double *B = nullptr;  // R x R, J x R, K x R: column-major, leading dimensions R, J, K
    const double *A = nullptr;
    const double *C = nullptr;
    double *Q = nullptr, *P = nullptr, *T = nullptr;  // I x R x K twice; R x R x K
    int *status = nullptr;
    double min_ratio = 0;
    void *Y = nullptr;
    int dt = 0;
    double *out = nullptr;
  };
  virtual void parafac2_check() { throw Unsupported("ppals: this back end has no device views"); }
  virtual void parafac2_init(double * /*P*/, int64_t /*I*/, int /*R*/, int64_t /*K*/) {
    throw Unsupported("ppals: this back end has no device views");
  }
  virtual void parafac2_step(const Parafac2Step & /*s*/, void * /*caller_stream*/) {
    throw Unsupported("ppals: this back end has no device views");
  }
  // The same step on K slices of unequal length (ppals_parafac2_*_ragged): slice k is rows[k] x J with
  // rows[k] >= R, X_k[i, j] = X[xoff[k] + i + xcs[k] j]. With roff[k] = sum_{l<k} rows[l] and N = roff[K],
  // Q_k and P_k are column-major with leading dimension rows[k] at Q + R roff[k] and P + R roff[k] (R N doubles
  // each); T, status, Y and out are those of parafac2_step. The tables are DEVICE arrays the caller fills once:
  // rows, roff, xoff, xcs of K int64 each; tile0[k] = sum_{l<k} ceil(rows[l] / 64), K ints; tile_slice[t] = the
  // slice of row tile t, `tiles` = tile0[K] ints. The first pass and the apply run one workgroup per row tile, the
  // slice slowest, so the number of launches (seven) depends on nothing. The summation orders are those of
  // parafac2_step: equal rows on the dense layout give its bits. parafac2_init_ragged writes the first R identity
  // columns into every P_k.
  struct Parafac2Ragged {
    int64_t J = 0, K = 0;
    int R = 0;
    int64_t tiles = 0;  // row tiles over all slices
    const int64_t *rows = nullptr, *roff = nullptr;
    const int *tile0 = nullptr, *tile_slice = nullptr;
    const void *X = nullptr;
    int vdt = 0;  // DV_F32 or DV_F64
    const int64_t *xoff = nullptr, *xcs = nullptr;
    const double *B = nullptr, *A = nullptr, *C = nullptr;
    double *Q = nullptr, *P = nullptr, *T = nullptr;
    int *status = nullptr;
    double min_ratio = 0;
    void *Y = nullptr;
    int dt = 0;
    double *out = nullptr;
  };
  virtual void parafac2_init_ragged(const Parafac2Ragged & /*s*/) {
    throw Unsupported("ppals: this back end has no device views");
  }
  virtual void parafac2_step_ragged(const Parafac2Ragged & /*s*/, void * /*caller_stream*/) {
    throw Unsupported("ppals: this back end has no device views");
  }

  // Order work on the engine stream against a caller's stream, as copy_view does it: join_stream makes the
  // work queued on the engine stream from now on wait for what `caller_stream` holds so far, release_stream
  // makes what the caller queues there later wait for the engine stream's work so far. The host does not block.
  virtual void join_stream(void * /*caller_stream*/) { throw Unsupported("ppals: this back end has no device views"); }
  virtual void release_stream(void * /*caller_stream*/) {
    throw Unsupported("ppals: this back end has no device views");
  }

  // ---- preprocessing in place (ppals_tensor_center / _shift / _slice_sumsq / _scale / _rescale) ----
  // V (storage type dt) viewed as [L, J, T], first index fastest. Every element is read as stored, widened to
  // fp64, and the new value rounded once to dt as an import rounds an fp64 source; sums are formed in fp64 in
  // a fixed order (no atomics). The defaults are the fp64 host twins built from d2h / h2d (what the host
  // stand-in runs, as with cp_mode_update_nn); the product back end overrides them with its kernels.
  //   center_fibres: off[l + L*t] = mean_j V[l,j,t] (device, fp64; may be nullptr), V[l,j,t] -= that mean
  //   shift_fibres:  V[l,j,t] += alpha * off[l + L*t]  (alpha = +-1: one rounding in fp64)
  //   slice_sumsq:   ss[j] = sum_{l,t} V[l,j,t]^2      (device, fp64)
  //   scale_slices:  V[l,j,t] *= fac[j]                (device, fp64); a slice with fac[j] == 1.0 is not touched
  static double prep_load(const void *V, int dt, size_t e) {
    return dt == F32 ? (double)((const float *)V)[e] : dt == BF16 ? (double)((const bf16s *)V)[e] : ((const double *)V)[e];
  }
  static void prep_store(void *V, int dt, size_t e, double x) {
    if (dt == F32)
      ((float *)V)[e] = (float)x;
    else if (dt == BF16)
      ((bf16s *)V)[e] = bf16s(x);
    else
      ((double *)V)[e] = x;
  }
  virtual void center_fibres(void *V, int dt, int64_t L, int64_t J, int64_t T, double *off) {
    const size_t n = (size_t)L * J * T;
    std::vector<char> h(n * dtype_size(dt));
    std::vector<double> o((size_t)L * T);
    d2h(h.data(), V, h.size());
    for (int64_t t = 0; t < T; t++)
      for (int64_t l = 0; l < L; l++) {
        double s = 0;
        for (int64_t j = 0; j < J; j++) s += prep_load(h.data(), dt, (size_t)(l + L * (j + J * t)));
        const double m = s / (double)J;
        o[(size_t)(l + L * t)] = m;
        for (int64_t j = 0; j < J; j++) {
          const size_t e = (size_t)(l + L * (j + J * t));
          prep_store(h.data(), dt, e, prep_load(h.data(), dt, e) - m);
        }
      }
    h2d(V, h.data(), h.size());
    if (off) h2d(off, o.data(), sizeof(double) * o.size());
  }
  virtual void shift_fibres(void *V, int dt, int64_t L, int64_t J, int64_t T, const double *off, double alpha) {
    const size_t n = (size_t)L * J * T;
    std::vector<char> h(n * dtype_size(dt));
    std::vector<double> o((size_t)L * T);
    d2h(h.data(), V, h.size());
    d2h(o.data(), off, sizeof(double) * o.size());
    for (int64_t t = 0; t < T; t++)
      for (int64_t j = 0; j < J; j++)
        for (int64_t l = 0; l < L; l++) {
          const size_t e = (size_t)(l + L * (j + J * t));
          prep_store(h.data(), dt, e, prep_load(h.data(), dt, e) + alpha * o[(size_t)(l + L * t)]);
        }
    h2d(V, h.data(), h.size());
  }
  virtual void slice_sumsq(const void *V, int dt, int64_t L, int64_t J, int64_t T, double *ss) {
    const size_t n = (size_t)L * J * T;
    std::vector<char> h(n * dtype_size(dt));
    std::vector<double> s((size_t)J, 0.0);
    d2h(h.data(), V, h.size());
    for (int64_t t = 0; t < T; t++)
      for (int64_t j = 0; j < J; j++)
        for (int64_t l = 0; l < L; l++) {
          const double v = prep_load(h.data(), dt, (size_t)(l + L * (j + J * t)));
          s[(size_t)j] += v * v;
        }
    h2d(ss, s.data(), sizeof(double) * s.size());
  }
  virtual void scale_slices(void *V, int dt, int64_t L, int64_t J, int64_t T, const double *fac) {
    const size_t n = (size_t)L * J * T;
    std::vector<char> h(n * dtype_size(dt));
    std::vector<double> f((size_t)J);
    d2h(h.data(), V, h.size());
    d2h(f.data(), fac, sizeof(double) * f.size());
    for (int64_t t = 0; t < T; t++)
      for (int64_t j = 0; j < J; j++) {
        if (f[(size_t)j] == 1.0) continue;
        for (int64_t l = 0; l < L; l++) {
          const size_t e = (size_t)(l + L * (j + J * t));
          prep_store(h.data(), dt, e, prep_load(h.data(), dt, e) * f[(size_t)j]);
        }
      }
    h2d(V, h.data(), h.size());
  }

  // ---- N-PLS (ppals_npls_fit / _predict, ppals_tensor_contract_mode / _slice_inner) ----
  // X (storage type dt, or an fp64 work array with dt = F64) viewed as [L, I, T], first index fastest, and only
  // read. Elements are widened to fp64 as stored, sums are formed in fp64 in a fixed order (no atomics), and column
  // c of a C-column call has the bits of that column computed alone. All pointers are device memory. The defaults
  // are the fp64 host twins built from d2h / h2d; the product back end overrides them with its kernels.
  //   npls_contract:     Z[l + L*t + L*T*c] = sum_i X[l,i,t] U[i + I*c]
  //   npls_slice_inner:  S[i + I*c] = sum_{l,t} X[l,i,t] W[l + L*t + L*T*c]
  //   npls_outer_axpy:   A[e] += alpha prod_k w[k][e_k], A of order K (1..8) with extents ext, first index fastest
  //   npls_argmax:       out[0] = max |Z[e]| (a non-finite entry counts as +inf), out[1] = its first index
  virtual void npls_contract(const void *X, int dt, int64_t L, int64_t I, int64_t T, const double *U, int C, double *Z) {
    if (L * T <= 0 || C <= 0) return;
    const size_t n = (size_t)L * I * T, LT = (size_t)L * T;
    std::vector<char> h(n * dtype_size(dt));
    std::vector<double> u((size_t)I * C), z(LT * C, 0.0);
    d2h(h.data(), X, h.size());
    d2h(u.data(), U, sizeof(double) * u.size());
    for (int c = 0; c < C; c++)
      for (int64_t t = 0; t < T; t++)
        for (int64_t i = 0; i < I; i++)
          for (int64_t l = 0; l < L; l++)
            z[(size_t)(l + L * t) + LT * c] += prep_load(h.data(), dt, (size_t)(l + L * (i + I * t))) * u[(size_t)i + (size_t)I * c];
    h2d(Z, z.data(), sizeof(double) * z.size());
  }
  virtual void npls_slice_inner(const void *X, int dt, int64_t L, int64_t I, int64_t T, const double *W, int C, double *S) {
    if (I <= 0 || C <= 0) return;
    const size_t n = (size_t)L * I * T, LT = (size_t)L * T;
    std::vector<char> h(n * dtype_size(dt));
    std::vector<double> w(LT * C), s((size_t)I * C, 0.0);
    d2h(h.data(), X, h.size());
    d2h(w.data(), W, sizeof(double) * w.size());
    for (int c = 0; c < C; c++)
      for (int64_t t = 0; t < T; t++)
        for (int64_t i = 0; i < I; i++)
          for (int64_t l = 0; l < L; l++)
            s[(size_t)i + (size_t)I * c] += prep_load(h.data(), dt, (size_t)(l + L * (i + I * t))) * w[(size_t)(l + L * t) + LT * c];
    h2d(S, s.data(), sizeof(double) * s.size());
  }
  // The wide-column forms (ppals_tensor_contract_columns / _slice_inner_columns, ppals_npls_crossval): the meaning
  // and the layouts of the two ops above for many columns at once. Results are deterministic (two calls give the
  // same bits) and within the same error bounds, but a column need not have the bits of the narrow op: the product
  // back end sums on the fp64 matrix cores, 64 columns a read of X. The defaults are the narrow twins.
  virtual void npls_contract_wide(const void *X, int dt, int64_t L, int64_t I, int64_t T, const double *U, int C, double *Z) {
    npls_contract(X, dt, L, I, T, U, C, Z);
  }
  virtual void npls_slice_inner_wide(const void *X, int dt, int64_t L, int64_t I, int64_t T, const double *W, int C, double *S) {
    npls_slice_inner(X, dt, L, I, T, W, C, S);
  }
  virtual void npls_outer_axpy(double *A, const int64_t *ext, int K, const double *const *w, double alpha) {
    if (K < 1 || K > MAX_ORDER) throw Unsupported("ppals: outer_axpy takes 1 to 8 vectors");
    size_t n = 1;
    std::vector<std::vector<double>> hw((size_t)K);
    for (int k = 0; k < K; k++) {
      n *= (size_t)ext[k];
      hw[(size_t)k].resize((size_t)ext[k]);
      d2h(hw[(size_t)k].data(), w[k], sizeof(double) * (size_t)ext[k]);
    }
    if (n == 0) return;
    std::vector<double> a(n);
    d2h(a.data(), A, sizeof(double) * n);
    for (size_t e = 0; e < n; e++) {
      size_t rem = e;
      double p = 1.0;
      for (int k = 0; k < K; k++) {
        const size_t ik = rem % (size_t)ext[k];
        rem /= (size_t)ext[k];
        p = k == 0 ? hw[0][ik] : p * hw[(size_t)k][ik];
      }
      a[e] += alpha * p;
    }
    h2d(A, a.data(), sizeof(double) * n);
  }
  virtual void npls_argmax(const double *Z, int64_t n, double *out) {
    if (n <= 0) return;
    std::vector<double> z((size_t)n);
    d2h(z.data(), Z, sizeof(double) * z.size());
    double o[2] = {-1.0, 0.0};
    for (int64_t e = 0; e < n; e++) {
      double a = std::fabs(z[(size_t)e]);
      if (!(a <= std::numeric_limits<double>::max())) a = std::numeric_limits<double>::infinity();
      if (a > o[0]) {
        o[0] = a;
        o[1] = (double)e;
      }
    }
    h2d(out, o, sizeof(o));
  }

  // ---- Khatri-Rao product, plain: out[j + J*c] = prod_f W_f[j_f + ld_f*(col0+c)], fp64 ----
  virtual void krp(double *out, const FactorRef *f, int nf, int col0, int ncols) = 0;

  // ---- tensor scans (the only kernels that touch the s^N tensor) ----
  // V viewed as [L, J, T] (first fastest), B = KRP of `nf` factors with combined extent J:
  //   out[l + out_tstride*t + out_rstride*r] = sum_j V[l,j,t] * B[j,r]       r in [0,R)
  // This one primitive is K1 (T=1: contract a suffix), K2 (L=1: contract a prefix), the
  // single-mode TTM of the PP operator build (tstride=L, rstride=L*T: rank index last) and the
  // Tucker mode product that keeps the mode in place (tstride=L*R, rstride=L). V may also be a
  // cached fp64 intermediate (dt = F64).
  // The result is written as fp64 (out_dt = F64) or fp32 (out_dt = F32, used for the large
  // first-level intermediate of the multi-sweep schedule).
  // A PADDED resident layout (pad_layout below) stores its rows in blocks of `pad.ld` of which the
  // first `pad.valid` exist: L then counts the stored rows (a multiple of pad.ld), and the result
  // is written COMPACT — stored row l lands at (l / ld) * valid + l % ld, the pad rows nowhere —
  // so nothing downstream of a scan knows about the padding.
  virtual void scan_contract(const void *V, int dt, int64_t L, int64_t J, int64_t T,
                             const FactorRef *f, int nf, int R, void *out, int out_dt,
                             int64_t out_tstride, int64_t out_rstride, RowPad pad) = 0;
  void scan_contract(const void *V, int dt, int64_t L, int64_t J, int64_t T, const FactorRef *f,
                     int nf, int R, void *out, int out_dt, int64_t out_tstride,
                     int64_t out_rstride) {
    scan_contract(V, dt, L, J, T, f, nf, R, out, out_dt, out_tstride, out_rstride, RowPad());
  }
  // Tucker mode product keeping the mode in place (fp64 in/out or V-typed in):
  //   out[l + L*(k + Kc*t)] = sum_j X[l,j,t] * W[j + ldw*k]      (als_Tucker.cxx:102,224)
  virtual void ttm_keep(const void *X, int dt, int64_t L, int64_t J, int64_t T, const double *W,
                        int64_t ldw, int Kc, double *out) {
    FactorRef f;
    f.ptr = W;
    f.rows = J;
    f.ld = ldw;
    scan_contract(X, dt, L, J, T, &f, 1, Kc, out, F64, L * Kc, L);
  }

  // The product with the LEADING mode of a small tensor, the next mode moved to the front of the result:
  //   out[s + S*(k + Kc*t)] = sum_j X[j + J*(s + S*t)] * W[j + ldw*k]
  // (the leaf of mode 1 in a Tucker chain: what the Gram of the unfolding wants, with no transposition
  // behind a leading-mode scan). false: the back end has no such kernel — the caller takes the generic
  // route.
  virtual bool ttm_lead_front(const void * /*X*/, int /*dt*/, int64_t /*J*/, int64_t /*S*/, int64_t /*T*/,
                              const double * /*W*/, int64_t /*ldw*/, int /*Kc*/, double * /*out*/) {
    return false;
  }

  // ---- contraction of a cached intermediate (fp64) that already carries the rank index ----
  //   out[l + L*t + out_rstride*r] (+)= sum_j X[l + L*(j + J*(t + T*r))] * B[j,r]
  // B = KRP of `nf` factor refs (combined extent J). accumulate!=0: add into out.
  // X is fp64 or fp32 (xdt); out_scale (device scalar or nullptr) multiplies the contribution.
  virtual void mttv(const void *X, int xdt, int64_t L, int64_t J, int64_t T, const FactorRef *f,
                    int nf, int R, double *out, int64_t out_rstride, int accumulate,
                    const double *out_scale) = 0;
  // PP correction of one mode in one call (K9, als_CP.cxx:754-794):
  //   M[x + rows*r] = M0[x + rows*r] + sum_t sum_y T_t[x,y,r] * dW_t[y + lddw_t*r]
  // (fixed summation order: results are reproducible run to run)
  virtual void pp_correct(const double *M0, int64_t rows, int R, const PPTerm *terms, int nterms,
                          double *M) {
    d2d(M, M0, sizeof(double) * rows * R);
    for (int t = 0; t < nterms; t++) {
      FactorRef f;
      f.ptr = terms[t].dW;
      f.rows = terms[t].ny;
      f.ld = terms[t].lddw;
      if (terms[t].keep_first)
        mttv(terms[t].T, F64, rows, terms[t].ny, 1, &f, 1, R, M, rows, 1, nullptr);
      else
        mttv(terms[t].T, F64, 1, terms[t].ny, rows, &f, 1, R, M, rows, 1, nullptr);
    }
  }
  // pending-Normalize bookkeeping of cached tensors: *dst = (set_one ? 1 : *dst) * prod_{m in
  // mask} scales[m]; `scales` is what normalize() last applied (see normalize_scales()).
  virtual void scale_update(double *dst, const double *scales, unsigned mask, int set_one) = 0;
  // the same for up to 32 scalars in one launch: dst[k] for every k with (active >> k) & 1;
  // entries with (fresh >> k) & 1 start from 1.0 instead of their old value
  virtual void scale_update_many(double *dst, const double *scales, const unsigned *masks,
                                 unsigned active, unsigned fresh) {
    for (int k = 0; k < 32; k++)
      if ((active >> k) & 1u) scale_update(dst + k, scales, masks[k], (fresh >> k) & 1u);
  }
  // Normalize + the pending-scale update of the cached multi-sweep tensors (active == 0: none);
  // back ends may fold both into one launch
  // wsq (device array, stride 2, may be null): wsq[2i] = ||W_i||_F^2 after the rescaling
  virtual void normalize_ms(double *const *W, const int64_t *rows, int N, int R, double *Gall,
                            double *ms_dst, const unsigned *masks, unsigned active, unsigned fresh,
                            double *wsq = nullptr) {
    normalize(W, rows, N, R, Gall);
    if (active) scale_update_many(ms_dst, normalize_scales(), masks, active, fresh);
    if (wsq)
      for (int i = 0; i < N; i++) sumsq(W[i], rows[i] * R, wsq + 2 * i);
  }
  virtual const double *normalize_scales() = 0;  // device array [N] written by normalize()

  // ---- R x R normal-equation side ----
  // G = W^T W  (rows x R, ld)  ->  G[R*R]
  virtual void gram(const double *W, int64_t rows, int64_t ld, int R, double *G) = 0;
  // S = Hadamard_{j != mode} G_j (+ lambda I); Sinv = S^{-1} through a symmetric eigen-
  // decomposition without truncation (the reference's SVD_solve, common.cxx:717-722)
  virtual void gram_system(const double *Gall, int N, int mode, int R, double lambda, double *S,
                           double *Sinv) = 0;
  // for `rows` rows: grad = -M + Wold*S ; Wnew = M*Sinv ; *gradsq = sum grad^2 (overwritten; 0 when rows == 0)
  // if Winit != nullptr (SVD_solve_mod, common.cxx:739-758): dW = ratio*(Wnew-Winit) and, when
  // ratio != 1, Wnew = Winit + dW.
  virtual void cp_update(const double *M, int64_t ldm, const double *Wold, int64_t ldw,
                         double *Wnew, int64_t ldn, double *grad, int64_t ldg, int64_t rows,
                         int R, const double *S, const double *Sinv, double *gradsq,
                         const double *Winit, int64_t ldi, double *dW, int64_t ldd,
                         double ratio) = 0;
  // one whole single-rank mode update: gram_system + cp_update (W updated in place) + gram of the
  // new W into Gall[mode]. Backends may fuse it into one launch; S/Sinv may be nullptr.
  // dwsq (device scalar, may be null; needs Winit and ldd == rows): *dwsq = ||dW||_F^2 afterwards
  // (the restart test of the PP phase, als_CP.cxx:657-663, without a launch of its own).
  virtual void cp_mode_update(double *Gall, int N, int mode, int R, double lambda, const double *M,
                              int64_t ldm, double *W, int64_t ldw, double *grad, int64_t ldg,
                              int64_t rows, double *gradsq, const double *Winit, int64_t ldi,
                              double *dW, int64_t ldd, double ratio, double *S, double *Sinv,
                              double *dwsq = nullptr) {
    // S / Sinv not wanted: the separate launches still pass them on. (An allocation and a free that
    // waits for the stream, per call: this keeps the contract above, it is not meant for a hot path —
    // the engine always passes both.)
    double *tmp = nullptr;
    if (!S || !Sinv) {
      tmp = (double *)alloc(sizeof(double) * 2 * (size_t)R * R);
      if (!S) S = tmp;
      if (!Sinv) Sinv = tmp + (size_t)R * R;
    }
    gram_system(Gall, N, mode, R, lambda, S, Sinv);
    cp_update(M, ldm, W, ldw, W, ldw, grad, ldg, rows, R, S, Sinv, gradsq, Winit, ldi, dW, ldd,
              ratio);
    gram(W, rows, ldw, R, Gall + (size_t)mode * R * R);
    if (dwsq && Winit) sumsq(dW, rows * R, dwsq);
    if (tmp) free(tmp);  // (free waits for the launches above)
  }
  // `nstarts` independent mode updates of rank R in one call (multi-start sessions): M, W and grad hold
  // nstarts * R columns, start b owns columns [b R, (b+1) R); Gall holds, start by start, the N Grams
  // (R x R) of that start; S / Sinv one R x R system per start; gradsq[b] = ||grad_b||^2. Nothing
  // couples two starts. Back ends may run all of them in one launch.
  virtual void cp_mode_update_batched(double *Gall, int N, int mode, int R, int nstarts, double lambda,
                                      const double *M, int64_t ldm, double *W, int64_t ldw,
                                      double *grad, int64_t ldg, int64_t rows, double *gradsq,
                                      double *S, double *Sinv) {
    for (int b = 0; b < nstarts; b++)
      cp_mode_update(Gall + (size_t)b * N * R * R, N, mode, R, lambda, M + (size_t)b * R * ldm, ldm,
                     W + (size_t)b * R * ldw, ldw, grad + (size_t)b * R * ldg, ldg, rows, gradsq + b,
                     nullptr, rows, nullptr, rows, 1.0, S ? S + (size_t)b * R * R : nullptr,
                     Sinv ? Sinv + (size_t)b * R * R : nullptr);
  }
  // One whole single-rank NON-NEGATIVE mode update (one pass of Cichocki-Phan HALS, fp64): with
  // S = Hadamard_{j != mode} G_j + lambda I, for every row x on its own and r = 0 .. R-1 in this order
  //   w[x,r] <- max(nn_floor, w[x,r] + (M[x,r] - sum_q w[x,q] S[q,r]) / S[r,r])
  // the sum taking the row's entries already updated for q < r; a column whose S[r,r] is not a positive
  // finite number stays as it is. grad = -M + W_old S with the pre-update W, *gradsq = sum grad^2, the
  // Gram of the new W into Gall[mode]; S (device, R x R, may be nullptr) receives the system. R <= 64.
  // This default is built from d2h / h2d and a host loop; the product back end overrides it.
  virtual void cp_mode_update_nn(double *Gall, int N, int mode, int R, double lambda, const double *M,
                                 int64_t ldm, double *W, int64_t ldw, double *grad, int64_t ldg,
                                 int64_t rows, double *gradsq, double *S) {
    const double nn_floor = kNnFloor;
    if (R > 64) throw Unsupported("ppals: the non-negative mode update supports R <= 64");
    const size_t RR = (size_t)R * R;
    std::vector<double> g((size_t)N * RR), s(RR, 1.0), m((size_t)ldm * (R - 1) + rows),
        w((size_t)ldw * (R - 1) + rows), gr((size_t)ldg * (R - 1) + rows);
    d2h(g.data(), Gall, sizeof(double) * g.size());
    d2h(m.data(), M, sizeof(double) * m.size());
    d2h(w.data(), W, sizeof(double) * w.size());
    d2h(gr.data(), grad, sizeof(double) * gr.size());
    for (size_t e = 0; e < RR; e++) {  // the index order of gram_system (als_CP.cxx:219-232)
      bool first = true;
      for (int ii = 0; ii < N - 1; ii++) {
        const double gv = g[(size_t)(ii == mode ? N - 1 : ii) * RR + e];
        s[e] = first ? gv : s[e] * gv;
        first = false;
      }
      if (e % R == e / R) s[e] += lambda;
    }
    double gs = 0;
    for (int r = 0; r < R; r++)
      for (int64_t x = 0; x < rows; x++) {
        double acc = 0;
        for (int q = 0; q < R; q++) acc += w[x + ldw * q] * s[q + (size_t)R * r];
        const double gv = -m[x + ldm * r] + acc;
        gr[x + ldg * r] = gv;
        gs += gv * gv;
      }
    for (int64_t x = 0; x < rows; x++)
      for (int r = 0; r < R; r++) {
        const double d = s[r + (size_t)R * r];
        if (!(d > 0) || d > 1.79769313486231570e308) continue;
        double acc = 0;
        for (int q = 0; q < R; q++) acc += w[x + ldw * q] * s[q + (size_t)R * r];
        const double v = w[x + ldw * r] + (m[x + ldm * r] - acc) / d;
        w[x + ldw * r] = v > nn_floor ? v : nn_floor;  // (a NaN lands on the floor)
      }
    h2d(W, w.data(), sizeof(double) * w.size());
    h2d(grad, gr.data(), sizeof(double) * gr.size());
    h2d(gradsq, &gs, sizeof(double));
    if (S) h2d(S, s.data(), sizeof(double) * RR);
    gram(W, rows, ldw, R, Gall + (size_t)mode * RR);
  }
  // `nstarts` independent non-negative mode updates of rank R in one call (non-negative multi-start
  // sessions), in the layout of cp_mode_update_batched: start b owns columns [b R, (b+1) R) of M, W and
  // grad, its N Grams sit at Gall + b N R^2, gradsq[b] = ||grad_b||^2, S (may be nullptr) receives one
  // R x R system per start. Nothing couples two starts. Back ends may run all of them in one launch.
  virtual void cp_mode_update_nn_batched(double *Gall, int N, int mode, int R, int nstarts, double lambda,
                                         const double *M, int64_t ldm, double *W, int64_t ldw,
                                         double *grad, int64_t ldg, int64_t rows, double *gradsq,
                                         double *S) {
    for (int b = 0; b < nstarts; b++)
      cp_mode_update_nn(Gall + (size_t)b * N * R * R, N, mode, R, lambda, M + (size_t)b * R * ldm, ldm,
                        W + (size_t)b * R * ldw, ldw, grad + (size_t)b * R * ldg, ldg, rows, gradsq + b,
                        S ? S + (size_t)b * R * R : nullptr);
  }
  // G_b = W_b^T W_b of the same column blocks: G + b * gstride, b < nstarts
  virtual void gram_batched(const double *W, int64_t rows, int64_t ld, int R, int nstarts, double *G,
                            int64_t gstride) {
    for (int b = 0; b < nstarts; b++) gram(W + (size_t)b * R * ld, rows, ld, R, G + (size_t)b * gstride);
  }
  // The three ops above for starts of DIFFERENT ranks (rank-sweep sessions, StartTable): start b owns
  // columns [t.col[b], t.col[b+1]) of M, W and grad, its N Grams (R_b x R_b) sit at Gall + N t.sq[b], its
  // system at S / Sinv + t.sq[b]; gradsq[b] = ||grad_b||^2. Nothing couples two starts. Back ends may
  // run all of them in one launch; a session whose ranks are all equal never comes here.
  virtual void cp_mode_update_ragged(double *Gall, int N, int mode, const StartTable &t, double lambda,
                                     const double *M, int64_t ldm, double *W, int64_t ldw, double *grad,
                                     int64_t ldg, int64_t rows, double *gradsq, double *S, double *Sinv) {
    for (int b = 0; b < t.nstarts; b++)
      cp_mode_update(Gall + (size_t)N * t.sq[b], N, mode, t.rank(b), lambda, M + (size_t)t.col[b] * ldm, ldm,
                     W + (size_t)t.col[b] * ldw, ldw, grad + (size_t)t.col[b] * ldg, ldg, rows, gradsq + b,
                     nullptr, rows, nullptr, rows, 1.0, S ? S + t.sq[b] : nullptr,
                     Sinv ? Sinv + t.sq[b] : nullptr);
  }
  virtual void cp_mode_update_nn_ragged(double *Gall, int N, int mode, const StartTable &t, double lambda,
                                        const double *M, int64_t ldm, double *W, int64_t ldw, double *grad,
                                        int64_t ldg, int64_t rows, double *gradsq, double *S) {
    for (int b = 0; b < t.nstarts; b++)
      cp_mode_update_nn(Gall + (size_t)N * t.sq[b], N, mode, t.rank(b), lambda, M + (size_t)t.col[b] * ldm,
                        ldm, W + (size_t)t.col[b] * ldw, ldw, grad + (size_t)t.col[b] * ldg, ldg, rows,
                        gradsq + b, S ? S + t.sq[b] : nullptr);
  }
  // One whole single-rank ORTHONORMAL mode update per start (PPALS_MODE_ORTHO; the layout of the ragged ops
  // above — an ordinary session is a table of one start): with S = Hadamard_{j != mode} G_j + lambda I,
  //   grad = -M + W_old S (as for every kind), gradsq[b] = sum grad_b^2,
  //   W_b <- M_b (M_b^T M_b)^(-1/2) = M_b U diag(theta^-1/2) U^T, the orthonormal polar factor of M_b in fp64
  //   (M_b^T M_b = U diag(theta) U^T by a cyclic Jacobi) — unless some theta is not a positive finite number
  //   or theta_min <= theta_max * kOrthoMinRatio: then the start's factor stays as it is,
  //   the Gram of the (new) W_b into Gall (computed, not assumed to be I); S (may be nullptr) receives the
  //   systems. lambda enters S, and so the gradient, only. Ranks <= 64; rows may be below a rank (the factor
  //   then stays: theta has a zero). Nothing couples two starts; the same state gives the same bits.
  // This default is built from d2h / h2d and a host loop (what the host stand-in runs, as with
  // cp_mode_update_nn); the product back end overrides it with three launches.
  virtual void cp_mode_update_ortho_ragged(double *Gall, int N, int mode, const StartTable &t, double lambda,
                                           const double *M, int64_t ldm, double *W, int64_t ldw, double *grad,
                                           int64_t ldg, int64_t rows, double *gradsq, double *S) {
    if (t.max_rank() > 64) throw Unsupported("ppals: the orthonormal mode update supports R <= 64");
    for (int b = 0; b < t.nstarts; b++) {
      const int R = t.rank(b);
      const size_t RR = (size_t)R * R;
      double *Gb = Gall + (size_t)N * t.sq[b];
      const double *Mb = M + (size_t)t.col[b] * ldm;
      double *Wb = W + (size_t)t.col[b] * ldw, *gb = grad + (size_t)t.col[b] * ldg;
      double gs = 0;
      if (rows <= 0) {
        h2d(gradsq + b, &gs, sizeof(double));
        gram(Wb, rows, ldw, R, Gb + (size_t)mode * RR);
        continue;
      }
      std::vector<double> g((size_t)N * RR), s(RR, 1.0), m((size_t)ldm * (R - 1) + rows),
          w((size_t)ldw * (R - 1) + rows), gr((size_t)ldg * (R - 1) + rows);
      d2h(g.data(), Gb, sizeof(double) * g.size());
      d2h(m.data(), Mb, sizeof(double) * m.size());
      d2h(w.data(), Wb, sizeof(double) * w.size());
      d2h(gr.data(), gb, sizeof(double) * gr.size());
      for (size_t e = 0; e < RR; e++) {  // the index order of gram_system (als_CP.cxx:219-232)
        bool first = true;
        for (int ii = 0; ii < N - 1; ii++) {
          const double gv = g[(size_t)(ii == mode ? N - 1 : ii) * RR + e];
          s[e] = first ? gv : s[e] * gv;
          first = false;
        }
        if (e % R == e / R) s[e] += lambda;
      }
      for (int r = 0; r < R; r++)
        for (int64_t x = 0; x < rows; x++) {
          double acc = 0;
          for (int q = 0; q < R; q++) acc += w[x + ldw * q] * s[q + (size_t)R * r];
          const double gv = -m[x + ldm * r] + acc;
          gr[x + ldg * r] = gv;
          gs += gv * gv;
        }
      // C = M^T M, then the cyclic Jacobi C = U diag(theta) U^T (row-cyclic order, plain C++)
      std::vector<double> c(RR), u(RR, 0.0), tm(RR);
      for (int p = 0; p < R; p++)
        for (int q = p; q < R; q++) {
          double acc = 0;
          for (int64_t x = 0; x < rows; x++) acc += m[x + ldm * p] * m[x + ldm * q];
          c[p + (size_t)R * q] = c[q + (size_t)R * p] = acc;
        }
      for (int k = 0; k < R; k++) u[k + (size_t)R * k] = 1.0;
      for (int sweep = 0; sweep < 60; sweep++) {
        double off = 0, diag = 0;
        for (int p = 0; p < R; p++)
          for (int q = 0; q < R; q++) (p == q ? diag : off) += c[p + (size_t)R * q] * c[p + (size_t)R * q];
        if (!(off > 1e-30 * diag)) break;  // (converged, or NaN: the rule below refuses it)
        for (int p = 0; p < R; p++)
          for (int q = p + 1; q < R; q++) {
            const double apq = c[p + (size_t)R * q];
            if (apq == 0.0) continue;
            const double theta = (c[q + (size_t)R * q] - c[p + (size_t)R * p]) / (2.0 * apq);
            const double tt = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
            const double cc = 1.0 / std::sqrt(tt * tt + 1.0), sn = tt * cc;
            for (int k = 0; k < R; k++) {  // C <- C J, U <- U J
              const double akp = c[k + (size_t)R * p], akq = c[k + (size_t)R * q];
              c[k + (size_t)R * p] = cc * akp - sn * akq;
              c[k + (size_t)R * q] = sn * akp + cc * akq;
              const double ukp = u[k + (size_t)R * p], ukq = u[k + (size_t)R * q];
              u[k + (size_t)R * p] = cc * ukp - sn * ukq;
              u[k + (size_t)R * q] = sn * ukp + cc * ukq;
            }
            for (int k = 0; k < R; k++) {  // C <- J^T C
              const double apk = c[p + (size_t)R * k], aqk = c[q + (size_t)R * k];
              c[p + (size_t)R * k] = cc * apk - sn * aqk;
              c[q + (size_t)R * k] = sn * apk + cc * aqk;
            }
          }
      }
      double off_end = 0, diag_end = 0;  // (not converged after the last sweep: the factor stays)
      for (int p = 0; p < R; p++)
        for (int q = 0; q < R; q++) (p == q ? diag_end : off_end) += c[p + (size_t)R * q] * c[p + (size_t)R * q];
      bool good = off_end <= 1e-30 * diag_end || off_end == 0.0;
      double tmin = 1.79769313486231570e308, tmax = 0;
      for (int k = 0; k < R; k++) {
        const double th = c[k + (size_t)R * k];
        if (!(th > 0) || th > 1.79769313486231570e308) good = false;
        tmin = th < tmin ? th : tmin;
        tmax = th > tmax ? th : tmax;
      }
      if (good && tmin <= tmax * kOrthoMinRatio) good = false;
      if (good) {
        for (int i = 0; i < R; i++)
          for (int j = 0; j < R; j++) {
            double acc = 0;
            for (int k = 0; k < R; k++)
              acc += u[i + (size_t)R * k] * (1.0 / std::sqrt(c[k + (size_t)R * k])) * u[j + (size_t)R * k];
            tm[i + (size_t)R * j] = acc;
          }
        for (int r = 0; r < R; r++)
          for (int64_t x = 0; x < rows; x++) {
            double acc = 0;
            for (int q = 0; q < R; q++) acc += m[x + ldm * q] * tm[q + (size_t)R * r];
            w[x + ldw * r] = acc;
          }
        h2d(Wb, w.data(), sizeof(double) * w.size());
      }
      h2d(gb, gr.data(), sizeof(double) * gr.size());
      h2d(gradsq + b, &gs, sizeof(double));
      if (S) h2d(S + t.sq[b], s.data(), sizeof(double) * RR);
      gram(Wb, rows, ldw, R, Gb + (size_t)mode * RR);
    }
  }
  // One whole single-rank SHAPED non-negative mode update per start (PPALS_SHAPE_* on a PPALS_MODE_NONNEG mode;
  // the layout of the ragged ops above — an ordinary session is a table of one start): with
  // S = Hadamard_{j != mode} G_j + lambda I,
  //   grad = -M + W_old S (as for every kind), gradsq[b] = sum grad_b^2,
  //   for r = 0 .. R_b - 1 in this order (Gauss-Seidel over columns): d = S[r,r]; if d is not a positive finite
  //   number the column stays; v[x] = w[x,r] + (M[x,r] - sum_q w[x,q] S[q,r]) / d with the current W (columns
  //   q < r replaced already); if some v[x] is not finite the column stays; else w[:,r] <- the least-squares
  //   projection of v onto the shape's set: u >= kNnFloor and u non-decreasing (kShapeIncreasing), non-increasing
  //   (kShapeDecreasing), or non-decreasing on rows 0..p and non-increasing on rows p+1..rows-1 for some p
  //   (kShapeUnimodal; the p of least error, the smallest on a tie) — shape_project below,
  //   the Gram of the new W_b into Gall; S (may be nullptr) receives the systems.
  // Ranks <= 64, any rows >= 1. Nothing couples two starts; the same state gives the same bits — of ONE back
  // end. A tie between two splits is decided to rounding: the split errors are sums that cancel, and back ends
  // may form them differently (this default divides, the HIP kernel multiplies by a refined reciprocal), so on
  // errors that agree to about 1e-15 |v|^2 two back ends may choose different p. Any of them is a minimiser to
  // that precision; nothing may rely on the back ends agreeing there.
  // This default is built from d2h / h2d and a host loop (what the host stand-in runs, as with
  // cp_mode_update_ortho_ragged); the product back end overrides it with three launches.
  virtual void cp_mode_update_shape_ragged(double *Gall, int N, int mode, const StartTable &t, double lambda,
                                           const double *M, int64_t ldm, double *W, int64_t ldw, double *grad,
                                           int64_t ldg, int64_t rows, double *gradsq, double *S, int shape) {
    if (t.max_rank() > 64) throw Unsupported("ppals: the shaped mode update supports R <= 64");
    if (shape < kShapeUnimodal || shape > kShapeDecreasing)
      throw std::invalid_argument("ppals: a shaped mode update needs PPALS_SHAPE_UNIMODAL, _INCREASING or _DECREASING");
    for (int b = 0; b < t.nstarts; b++) {
      const int R = t.rank(b);
      const size_t RR = (size_t)R * R;
      double *Gb = Gall + (size_t)N * t.sq[b];
      const double *Mb = M + (size_t)t.col[b] * ldm;
      double *Wb = W + (size_t)t.col[b] * ldw, *gb = grad + (size_t)t.col[b] * ldg;
      double gs = 0;
      if (rows <= 0) {
        h2d(gradsq + b, &gs, sizeof(double));
        gram(Wb, rows, ldw, R, Gb + (size_t)mode * RR);
        continue;
      }
      std::vector<double> g((size_t)N * RR), s(RR, 1.0), m((size_t)ldm * (R - 1) + rows),
          w((size_t)ldw * (R - 1) + rows), gr((size_t)ldg * (R - 1) + rows);
      d2h(g.data(), Gb, sizeof(double) * g.size());
      d2h(m.data(), Mb, sizeof(double) * m.size());
      d2h(w.data(), Wb, sizeof(double) * w.size());
      d2h(gr.data(), gb, sizeof(double) * gr.size());
      for (size_t e = 0; e < RR; e++) {  // the index order of gram_system (als_CP.cxx:219-232)
        bool first = true;
        for (int ii = 0; ii < N - 1; ii++) {
          const double gv = g[(size_t)(ii == mode ? N - 1 : ii) * RR + e];
          s[e] = first ? gv : s[e] * gv;
          first = false;
        }
        if (e % R == e / R) s[e] += lambda;
      }
      for (int r = 0; r < R; r++)
        for (int64_t x = 0; x < rows; x++) {
          double acc = 0;
          for (int q = 0; q < R; q++) acc += w[x + ldw * q] * s[q + (size_t)R * r];
          const double gv = -m[x + ldm * r] + acc;
          gr[x + ldg * r] = gv;
          gs += gv * gv;
        }
      std::vector<double> v((size_t)rows), u((size_t)rows);
      for (int r = 0; r < R; r++) {
        const double d = s[r + (size_t)R * r];
        if (!(d > 0) || d > 1.79769313486231570e308) continue;
        bool finite = true;
        for (int64_t x = 0; x < rows; x++) {
          double acc = 0;
          for (int q = 0; q < R; q++) acc += w[x + ldw * q] * s[q + (size_t)R * r];
          v[x] = w[x + ldw * r] + (m[x + ldm * r] - acc) / d;
          finite = finite && std::fabs(v[x]) <= 1.79769313486231570e308;
        }
        if (!finite) continue;
        shape_project(v.data(), rows, shape, kNnFloor, u.data());
        for (int64_t x = 0; x < rows; x++) w[x + ldw * r] = u[x];
      }
      h2d(Wb, w.data(), sizeof(double) * w.size());
      h2d(gb, gr.data(), sizeof(double) * gr.size());
      h2d(gradsq + b, &gs, sizeof(double));
      if (S) h2d(S + t.sq[b], s.data(), sizeof(double) * RR);
      gram(Wb, rows, ldw, R, Gb + (size_t)mode * RR);
    }
  }
  // u = argmin ||u - v||^2 over the shape's set (cp_mode_update_shape_ragged), on the host: pool-adjacent-
  // violators left to right and right to left, blocks as (sum, count), the fit clipped at `floor` (the bounded
  // isotonic fit is the unbounded one clipped). For kShapeUnimodal the two passes also leave, for every prefix
  // and suffix, the error of its clipped fit — a block's is sumsq - 2 c sum + c^2 count with c = max(mean,
  // floor) — and the split p of least total wins, the smallest on a tie.
  static void shape_project(const double *v, int64_t n, int shape, double floor, double *u) {
    struct Blk {
      double sum, sumsq, err;  // err: the clipped error of all blocks up to and including this one
      int64_t cnt;
    };
    std::vector<Blk> st;
    // the non-decreasing fit of the m entries a[0], a[step], a[2 step], ... as blocks on `st`;
    // err[k] = the clipped error of the fit of the first k + 1 of them
    auto pass = [&st, floor](const double *a, int64_t step, int64_t m, double *err) {
      st.clear();
      for (int64_t k = 0; k < m; k++) {
        const double x = a[k * step];
        Blk nb{x, x * x, 0.0, 1};
        while (!st.empty() && st.back().sum * (double)nb.cnt >= nb.sum * (double)st.back().cnt) {
          nb.sum += st.back().sum;
          nb.sumsq += st.back().sumsq;
          nb.cnt += st.back().cnt;
          st.pop_back();
        }
        const double mean = nb.sum / (double)nb.cnt, c = mean > floor ? mean : floor;
        nb.err = (st.empty() ? 0.0 : st.back().err) + (nb.sumsq - 2.0 * c * nb.sum + c * c * (double)nb.cnt);
        st.push_back(nb);
        if (err) err[k] = nb.err;
      }
    };
    // the blocks' clipped means into o[0], o[step], ...
    auto emit = [&st, floor](double *o, int64_t step) {
      int64_t k = 0;
      for (const Blk &b : st) {
        const double mean = b.sum / (double)b.cnt, c = mean > floor ? mean : floor;
        for (int64_t j = 0; j < b.cnt; j++, k++) o[k * step] = c;
      }
    };
    // (a non-increasing fit is the non-decreasing fit of the sequence read backwards)
    if (shape == kShapeIncreasing) {
      pass(v, 1, n, nullptr);
      emit(u, 1);
      return;
    }
    if (shape == kShapeDecreasing) {
      pass(v + n - 1, -1, n, nullptr);
      emit(u + n - 1, -1);
      return;
    }
    std::vector<double> ep((size_t)n), es((size_t)n);
    pass(v, 1, n, ep.data());
    pass(v + n - 1, -1, n, es.data());
    int64_t best = 0;
    double ebest = 0;
    for (int64_t p = 0; p < n; p++) {  // rows 0..p rise, rows p+1..n-1 fall
      const double e = ep[p] + (p + 1 < n ? es[n - 2 - p] : 0.0);
      if (p == 0 || e < ebest) {
        ebest = e;
        best = p;
      }
    }
    // the winner's two fits, each a pass over its own part (later entries pool a prefix's blocks away)
    pass(v, 1, best + 1, nullptr);
    emit(u, 1);
    if (best + 1 < n) {
      pass(v + n - 1, -1, n - 1 - best, nullptr);
      emit(u + n - 1, -1);
    }
  }
  // G_b = W_b^T W_b of the same column blocks into the session's Gram store: Gram (start b, mode) at
  // Gall + N t.sq[b] + mode R_b^2
  virtual void gram_ragged(const double *W, int64_t rows, int64_t ld, const StartTable &t, int N, int mode,
                           double *Gall) {
    for (int b = 0; b < t.nstarts; b++)
      gram(W + (size_t)t.col[b] * ld, rows, ld, t.rank(b),
           Gall + (size_t)N * t.sq[b] + (size_t)mode * t.rank(b) * t.rank(b));
  }
  // Hold-out rows of one mode per start (CpEngine::set_holdout; include/ppals.h), after that mode's update:
  // keep (device, nstarts x rows bytes) has keep[b * rows + x] == 0 where start b holds row x out. For every
  // start b whose bit of `holds` is set, on its column block [t.col[b], t.col[b + 1]) of W, grad and scores
  // (all rows x t.col[nstarts], column-major, leading dimensions ldw, ldg, lds):
  //   held-out x:  scores[x, :] = W[x, :],  W[x, :] = 0,  grad[x, :] = 0;       kept x:  scores[x, :] = 0
  //   Gall + N t.sq[b] + mode R_b^2 = W_b^T W_b of the zeroed block, gradsq[b] = sum grad_b^2 of the zeroed block
  // A start whose bit is clear is not touched at all. The same state gives the same bits: no atomics, the
  // sums added in a fixed order. This default is built from d2h / h2d and a host loop (what the host
  // stand-in runs, as with cp_mode_update_nn); the product back end overrides it with one launch.
  virtual void cp_hold_rows(double *W, int64_t ldw, double *grad, int64_t ldg, double *scores, int64_t lds,
                            int64_t rows, const StartTable &t, const uint8_t *keep, unsigned holds,
                            double *Gall, int N, int mode, double *gradsq) {
    if (rows <= 0) return;
    std::vector<uint8_t> k((size_t)rows);
    for (int b = 0; b < t.nstarts; b++) {
      if (!((holds >> b) & 1u)) continue;
      const int R = t.rank(b);
      const size_t c0 = (size_t)t.col[b];
      std::vector<double> w((size_t)ldw * (R - 1) + rows), g((size_t)ldg * (R - 1) + rows),
          sc((size_t)lds * (R - 1) + rows);
      d2h(k.data(), keep + (size_t)b * rows, k.size());
      d2h(w.data(), W + c0 * ldw, sizeof(double) * w.size());
      d2h(g.data(), grad + c0 * ldg, sizeof(double) * g.size());
      d2h(sc.data(), scores + c0 * lds, sizeof(double) * sc.size());  // (the gaps of lds > rows go back as they came)
      double gs = 0;
      for (int r = 0; r < R; r++)
        for (int64_t x = 0; x < rows; x++) {
          if (k[(size_t)x]) {
            sc[(size_t)(x + lds * r)] = 0.0;
            gs += g[(size_t)(x + ldg * r)] * g[(size_t)(x + ldg * r)];
          } else {
            sc[(size_t)(x + lds * r)] = w[(size_t)(x + ldw * r)];
            w[(size_t)(x + ldw * r)] = 0.0;
            g[(size_t)(x + ldg * r)] = 0.0;
          }
        }
      h2d(W + c0 * ldw, w.data(), sizeof(double) * w.size());
      h2d(grad + c0 * ldg, g.data(), sizeof(double) * g.size());
      h2d(scores + c0 * lds, sc.data(), sizeof(double) * sc.size());
      h2d(gradsq + b, &gs, sizeof(double));
      gram(W + c0 * ldw, rows, ldw, R, Gall + (size_t)N * t.sq[b] + (size_t)mode * R * R);
    }
  }
  // The same with M handed over in ROW BLOCKS (the receive buffer of an all-gather of the ranks' row
  // blocks: block p = rows [p*blk, (p+1)*blk) stored at Mblk + p*blk*R with leading dimension blk,
  // blk * P == rows). A back end may read the blocks as they are; the default re-assembles them in
  // `scratch` (rows x R) first.
  virtual void cp_mode_update_blocked(double *Gall, int N, int mode, int R, double lambda,
                                      const double *Mblk, int64_t blk, int P, double *scratch,
                                      double *W, int64_t ldw, double *grad, int64_t ldg, int64_t rows,
                                      double *gradsq, const double *Winit, int64_t ldi, double *dW,
                                      int64_t ldd, double ratio, double *S, double *Sinv) {
    unpack_blocks(Mblk, rows, rows, R, blk, P, scratch);
    cp_mode_update(Gall, N, mode, R, lambda, scratch, rows, W, ldw, grad, ldg, rows, gradsq, Winit, ldi,
                   dW, ldd, ratio, S, Sinv);
  }
  // ---- core consistency (CpEngine::core_consistency) ----
  // The transposed pseudo-inverses of all modes and starts in one call: for every mode i < N and start b
  //   P[i][:, col_b .. col_b + R_b) = W[i][:, col_b .. col_b + R_b) * G_{i,b}^{-1}
  // with G_{i,b} the start's R_b x R_b Gram of that mode as the session keeps it (Gall + N t.sq[b] + i R_b^2),
  // inverted in fp64 by Gauss-Jordan sweeps without pivoting. W[i] and P[i] are rows[i] x t.col[nstarts],
  // column-major, leading dimension rows[i]. A start one of whose N Grams meets a pivot that is not a
  // positive finite number gets bad[b] = 1 (device, int[nstarts], zeroed by the caller) and zeros in that
  // block of P. Every rank <= kPinvMaxRank.
  static constexpr int kPinvMaxRank = 64;
  // This default is the fp64 twin of the product's kernel, built from d2h / h2d and host loops (what the
  // host stand-in runs, as with cp_mode_update_nn); the product back end overrides it.
  virtual void cp_pinv_ragged(const double *Gall, int N, const StartTable &t, double *const *W,
                              const int64_t *rows, double *const *P, int *bad) {
    if (t.max_rank() > kPinvMaxRank) throw Unsupported("ppals: the pseudo-inverse factors support ranks <= 64");
    const int K = t.nstarts, C = t.col[K];
    std::vector<double> g((size_t)N * t.sq[K]);
    std::vector<int> flag(K);
    d2h(g.data(), Gall, sizeof(double) * g.size());
    d2h(flag.data(), bad, sizeof(int) * K);
    for (int mode = 0; mode < N; mode++) {
      const int64_t n = rows[mode];
      std::vector<double> w((size_t)n * C), p((size_t)n * C, 0.0);
      d2h(w.data(), W[mode], sizeof(double) * w.size());
      for (int b = 0; b < K; b++) {
        const int R = t.rank(b);
        const double *G = g.data() + (size_t)N * t.sq[b] + (size_t)mode * R * R;
        std::vector<double> A(G, G + (size_t)R * R), prow(R), pcol(R);
        bool ok = true;
        for (int k = 0; k < R; k++) {
          const double pv = A[k + (size_t)R * k];
          if (!(pv > 0.0) || !(pv <= 1.79769313486231570e308)) {
            ok = false;
            break;
          }
          for (int q = 0; q < R; q++) {
            prow[q] = A[k + (size_t)R * q];
            pcol[q] = A[q + (size_t)R * k];
          }
          const double d = 1.0 / pv;
          for (int j = 0; j < R; j++)
            for (int i = 0; i < R; i++) {
              double v;
              if (i == k)
                v = (j == k) ? d : prow[j] * d;
              else if (j == k)
                v = -pcol[i] * d;
              else
                v = A[i + (size_t)R * j] - pcol[i] * (prow[j] * d);
              A[i + (size_t)R * j] = v;
            }
        }
        if (!ok) {
          flag[b] = 1;
          continue;  // (the block of P stays zero)
        }
        for (int j = 0; j < R; j++)  // the two triangles differ by rounding only
          for (int i = 0; i < j; i++) {
            const double v = 0.5 * (A[i + (size_t)R * j] + A[j + (size_t)R * i]);
            A[i + (size_t)R * j] = A[j + (size_t)R * i] = v;
          }
        const double *wb = w.data() + (size_t)t.col[b] * n;
        double *pb = p.data() + (size_t)t.col[b] * n;
        for (int r = 0; r < R; r++)
          for (int64_t x = 0; x < n; x++) {
            double acc = 0;
            for (int q = 0; q < R; q++) acc += wb[x + n * q] * A[q + (size_t)R * r];
            pb[x + n * r] = acc;
          }
      }
      h2d(P[mode], p.data(), sizeof(double) * p.size());
    }
    h2d(bad, flag.data(), sizeof(int) * K);
  }
  // The score of one start from its core G (R^N fp64 entries, first index fastest), summed in a fixed order:
  //   *cc = 100 (1 - sum (G - T)^2 / R),   T[r,...,r] = 1 and zero elsewhere;
  // *bad != 0 (device): *cc = NaN and every entry of the core becomes NaN.
  // (the default: the fp64 twin on the host, as above)
  virtual void core_score(double *core, int R, int N, const int *bad, double *cc) {
    int64_t n = 1, dstride = 0;
    for (int i = 0; i < N; i++) {
      dstride += n;
      n *= R;
    }
    int flag = 0;
    d2h(&flag, bad, sizeof(int));
    std::vector<double> g((size_t)n);
    double out;
    if (flag) {
      out = std::numeric_limits<double>::quiet_NaN();
      g.assign((size_t)n, out);
      h2d(core, g.data(), sizeof(double) * g.size());
    } else {
      d2h(g.data(), core, sizeof(double) * g.size());
      double s = 0;
      for (int64_t e = 0; e < n; e++) {
        const double d = g[(size_t)e] - (e % dstride == 0 ? 1.0 : 0.0);
        s += d * d;
      }
      out = 100.0 * (1.0 - s / (double)R);
    }
    h2d(cc, &out, sizeof(double));
  }
  // ---- factor congruence (CpEngine::congruence; include/ppals.h, "factor match score") ----
  // Two column sets of the same order N: side a has a.cols columns, its mode-i factor a.w[i] is
  // a.rows[i] x a.cols, column-major with leading dimension a.ld[i]; side b likewise. At most
  // kCongruenceMaxCols columns a side. `mask` has bit i set for every COMPARED mode; in those
  // a.rows[i] == b.rows[i]. Outputs on the device, all fp64:
  //   Phi[p + a.cols*q] = prod over compared modes of (a_i[:,p] . b_i[:,q]) / (|a_i[:,p]| |b_i[:,q]|),
  //                       0 when a norm of p or of q in a compared mode is not a positive finite number
  //   wa[p] = prod over ALL N modes of |a_i[:,p]|, wb[q] likewise (as computed: 0, inf and NaN stay)
  // `work`: factor_congruence_work(...) bytes of device memory owned by the caller (nullptr when 0).
  // The same inputs give the same bits: no atomics, partial sums added in a fixed order.
  static constexpr int kCongruenceMaxCols = 128;
  struct CongruenceSide {
    const double *w[MAX_ORDER];
    int64_t ld[MAX_ORDER], rows[MAX_ORDER];
    int cols;
  };
  virtual size_t factor_congruence_work(int /*N*/, const CongruenceSide & /*a*/, const CongruenceSide & /*b*/) {
    return 0;
  }
  // (the default: the fp64 twin on the host, as above)
  virtual void factor_congruence(int N, const CongruenceSide &a, const CongruenceSide &b, unsigned mask,
                                 void * /*work*/, double *Phi, double *wa, double *wb) {
    if (a.cols < 1 || b.cols < 1 || a.cols > kCongruenceMaxCols || b.cols > kCongruenceMaxCols)
      throw Unsupported("ppals: the factor congruence supports 1 .. 128 columns a side");
    const int Ca = a.cols, Cb = b.cols;
    const double dmax = std::numeric_limits<double>::max();
    std::vector<double> phi((size_t)Ca * Cb, 1.0), na(Ca, 1.0), nb(Cb, 1.0);
    std::vector<char> bad_a(Ca, 0), bad_b(Cb, 0);
    auto fetch = [&](const CongruenceSide &s, int i, std::vector<double> &h) {
      h.resize((size_t)s.ld[i] * (s.cols - 1) + (size_t)s.rows[i]);
      d2h(h.data(), s.w[i], sizeof(double) * h.size());
    };
    std::vector<double> ha, hb, xa(Ca), xb(Cb);
    for (int i = 0; i < N; i++) {
      fetch(a, i, ha);
      fetch(b, i, hb);
      const bool compared = (mask >> i) & 1u;
      auto norms = [&](const CongruenceSide &s, const std::vector<double> &h, std::vector<double> &x,
                       std::vector<double> &w, std::vector<char> &bad) {
        for (int c = 0; c < s.cols; c++) {
          double ss = 0;
          for (int64_t r = 0; r < s.rows[i]; r++) ss += h[(size_t)(r + s.ld[i] * c)] * h[(size_t)(r + s.ld[i] * c)];
          x[c] = std::sqrt(ss);
          w[c] *= x[c];
          if (compared && (!(x[c] > 0.0) || !(x[c] <= dmax))) bad[c] = 1;
        }
      };
      norms(a, ha, xa, na, bad_a);
      norms(b, hb, xb, nb, bad_b);
      if (!compared) continue;
      for (int q = 0; q < Cb; q++)
        for (int p = 0; p < Ca; p++) {
          double dot = 0;
          for (int64_t r = 0; r < a.rows[i]; r++)
            dot += ha[(size_t)(r + a.ld[i] * p)] * hb[(size_t)(r + b.ld[i] * q)];
          phi[p + (size_t)Ca * q] *= (dot / xa[p]) / xb[q];
        }
    }
    for (int q = 0; q < Cb; q++)
      for (int p = 0; p < Ca; p++)
        if (bad_a[p] || bad_b[q]) phi[p + (size_t)Ca * q] = 0.0;
    h2d(Phi, phi.data(), sizeof(double) * phi.size());
    h2d(wa, na.data(), sizeof(double) * Ca);
    h2d(wb, nb.data(), sizeof(double) * Cb);
  }
  // ---- per-slice residuals and leverages (CpEngine::slice_residuals / leverages; include/ppals.h) ----
  // The contract of residual_sq (Q != nullptr) with two more outputs, from ONE pass over V: with
  // e[m,k] = V[m,k] - sum_r Q[m,r] P[k,r] (V as stored, everything else fp64)
  //   rowsq[m] = sum_k e^2,  colsq[k] = sum_m e^2,  *total = sum_k colsq[k]     (device, fp64)
  // The same inputs give the same bits: no atomics, partial sums added in a fixed order. A back end's
  // partial sums live in the CALLER's grow-only buffer `work` of `work_bytes` bytes (nullptr / 0 at first): the
  // op frees and allocates it anew (free / alloc of this Ops) when it needs more, the caller keeps it for the
  // next call and frees it in the end. It stays within work_cap_bytes — or what one row tile by one group of
  // k-chunks needs, if that is more — by walking the pass in slabs; the cap changes no bit of the result.
  // This default is the fp64 twin of the product's kernels on the host (it needs no partial sums, leaves
  // `work` alone and ignores the cap), as with cp_pinv_ragged; the product back end overrides it.
  virtual void residual_slices(const void *V, int dt, int64_t M, int64_t K, const double *Q, const double *P,
                               int R, double *rowsq, double *colsq, double *total, size_t /*work_cap_bytes*/,
                               void *& /*work*/, size_t & /*work_bytes*/) {
    std::vector<char> raw((size_t)M * K * dtype_size(dt));
    std::vector<double> q((size_t)M * R), p((size_t)K * R), rs((size_t)M, 0.0), cs((size_t)K, 0.0);
    d2h(raw.data(), V, raw.size());
    d2h(q.data(), Q, sizeof(double) * q.size());
    d2h(p.data(), P, sizeof(double) * p.size());
    double tot = 0;
    for (int64_t k = 0; k < K; k++) {
      double c = 0;
      for (int64_t m = 0; m < M; m++) {
        const size_t e = (size_t)(m + M * k);
        double v = 0;
        for (int r = 0; r < R; r++) v += q[(size_t)(m + M * r)] * p[(size_t)(k + K * r)];
        const double x = dt == F32    ? (double)((const float *)raw.data())[e]
                         : dt == BF16 ? (double)bf16_bits_to_float(((const uint16_t *)raw.data())[e])
                                      : ((const double *)raw.data())[e];
        const double d = x - v;
        rs[(size_t)m] += d * d;
        c += d * d;
      }
      cs[(size_t)k] = c;
      tot += c;
    }
    h2d(rowsq, rs.data(), sizeof(double) * rs.size());
    h2d(colsq, cs.data(), sizeof(double) * cs.size());
    h2d(total, &tot, sizeof(double));
  }
  // A vector indexed by a flattened group of n modes (extents lens[0..n), the first listed fastest; device,
  // fp64) marginalised onto each of them: out = the n per-mode vectors one after the other,
  //   out_j[x] = sum of src[e] over every e whose j-th index is x,
  // in a fixed order. (the default: the host twin, in ascending e)
  virtual void fold_slice_sums(const double *src, const int64_t *lens, int n, double *out) {
    int64_t total = 1, nout = 0;
    for (int j = 0; j < n; j++) {
      total *= lens[j];
      nout += lens[j];
    }
    std::vector<double> s((size_t)total), o((size_t)nout, 0.0);
    d2h(s.data(), src, sizeof(double) * s.size());
    for (int64_t e = 0; e < total; e++) {
      int64_t rem = e, off = 0;
      for (int j = 0; j < n; j++) {
        o[(size_t)(off + rem % lens[j])] += s[(size_t)e];
        rem /= lens[j];
        off += lens[j];
      }
    }
    h2d(out, o.data(), sizeof(double) * o.size());
  }
  // out[x] = sum_r P[x + ld r] W[x + ld r], x < rows, r ascending (device, fp64): with P = W G^-1 the
  // leverages diag(W G^-1 W^T). (the default: the host twin)
  virtual void row_dots(const double *P, const double *W, int64_t rows, int R, int64_t ld, double *out) {
    const size_t n = (size_t)ld * (R - 1) + (size_t)rows;
    std::vector<double> p(n), w(n), o((size_t)rows, 0.0);
    d2h(p.data(), P, sizeof(double) * n);
    d2h(w.data(), W, sizeof(double) * n);
    for (int r = 0; r < R; r++)
      for (int64_t x = 0; x < rows; x++) o[(size_t)x] += p[(size_t)(x + ld * r)] * w[(size_t)(x + ld * r)];
    h2d(out, o.data(), sizeof(double) * o.size());
  }
  // ---- a Tucker session's per-slice residuals (TuckerEngine::slice_residuals; include/ppals.h) ----
  // One slab of the pass, on a plan as TuckerEngine::impute builds it (group A = mode 0, the shard's fast
  // side; group B = the other modes in the shard's order; only the plan's SHARD side is read): with
  //   e(a,b) = V[roff + rA(a) + rB(b)] - sum_{k<K} Q[a + ldq*k] * P[(b % pL) + pLK*(b / pL) + pL*k]
  // (V as stored, dt F32 / F64; everything else fp64, k ascending)
  //   asq[a] = (first ? 0 : asq[a]) + sum_b e^2,   bsq[b] = sum_a e^2                      (device, fp64)
  // from ONE read of the slab of V, nothing else of its size touched. The same inputs give the same bits: no
  // atomics, partial sums added in an order fixed by the geometry. `work`, `work_bytes` and the cap: the
  // caller's grow-only buffer of the partial sums, handed over as to residual_slices; the cap cuts the slab's
  // row tiles into several launches and changes no bit. On the engine stream; the host does not block.
  // This default is the fp64 host twin (it needs no partial sums and leaves `work` alone), which the host
  // stand-in runs; the product back end overrides it.
  virtual void model_slice_sums(const ModelPlan &mp, const double *Q, const double *P, int K, const void *V, int dt,
                                bool first, double *asq, double *bsq, size_t /*work_cap_bytes*/, void *& /*work*/,
                                size_t & /*work_bytes*/) {
    const int64_t A = mp.ga.count, B = mp.gb.count;
    if (A <= 0 || B <= 0) return;
    if (dt != F32 && dt != F64) throw std::runtime_error("ppals: model_slice_sums reads F32 or F64 storage");
    auto offsets = [](const ModelGroup &g) {
      std::vector<int64_t> o((size_t)g.count);
      for (int64_t e = 0; e < g.count; e++) {
        int64_t idx = e, r = 0;
        for (int m = 0; m < g.n; m++) {
          r += (idx % g.len[m]) * g.rs[m];
          idx /= g.len[m];
        }
        o[(size_t)e] = r;
      }
      return o;
    };
    const std::vector<int64_t> ra = offsets(mp.ga), rb = offsets(mp.gb);
    const int64_t bl = B - 1;
    const size_t nv = (size_t)(mp.roff + ra.back() + rb.back() + 1), nq = (size_t)((A - 1) + mp.ldq * (K - 1) + 1),
                 np = (size_t)((bl % mp.pL) + mp.pLK * (bl / mp.pL) + mp.pL * (K - 1) + 1);
    std::vector<char> raw(nv * dtype_size(dt));
    std::vector<double> q(nq), p(np), as((size_t)A, 0.0), bs((size_t)B, 0.0);
    d2h(raw.data(), V, raw.size());
    d2h(q.data(), Q, sizeof(double) * nq);
    d2h(p.data(), P, sizeof(double) * np);
    if (!first) d2h(as.data(), asq, sizeof(double) * as.size());
    for (int64_t b = 0; b < B; b++) {
      const int64_t pb = (b % mp.pL) + mp.pLK * (b / mp.pL);
      for (int64_t a = 0; a < A; a++) {
        double v = 0;
        for (int k = 0; k < K; k++) v += q[(size_t)(a + mp.ldq * k)] * p[(size_t)(pb + mp.pL * k)];
        const size_t e = (size_t)(mp.roff + ra[(size_t)a] + rb[(size_t)b]);
        const double x = dt == F32 ? (double)((const float *)raw.data())[e] : ((const double *)raw.data())[e];
        const double d = x - v;
        as[(size_t)a] += d * d;
        bs[(size_t)b] += d * d;
      }
    }
    h2d(asq, as.data(), sizeof(double) * as.size());
    h2d(bsq, bs.data(), sizeof(double) * bs.size());
  }
  // Where the next scan_contract calls are booked in the launch profile: 0 the tensor scans (the default),
  // 1 the other kernels — for a scan of something that is not the tensor.
  virtual void scan_profile_slot(int /*slot*/) {}
  // Hint: the next cp_mode_update will be for `mode` with these arguments, and the Grams of the
  // other modes are final NOW — a back end may prepare S / S^-1 on the side of the contraction that
  // is launched next (mttv / pp_correct) instead of at the head of the update launch. Optional.
  virtual void arm_gram_system(const double * /*Gall*/, int /*N*/, int /*mode*/, int /*R*/,
                               double /*lambda*/, double * /*S*/, double * /*Sinv*/) {}
  // Hint: the next cp_mode_update is the last of a sweep and a Normalize of these N full factors
  // follows it immediately — a back end may fold it into that launch, together with the pending-scale
  // update of the cached multi-sweep tensors (ms_dst / masks / active / fresh as in normalize_ms;
  // active == 0: none alive). Returns true when it WILL (the caller then skips its normalize call).
  virtual bool arm_normalize(double *const * /*W*/, const int64_t * /*rows*/, int /*N*/, int /*R*/,
                             double * /*Gall*/, int /*mode*/, double * /*wsq*/,
                             double * /*ms_dst*/ = nullptr, const unsigned * /*masks*/ = nullptr,
                             unsigned /*active*/ = 0, unsigned /*fresh*/ = 0) {
    return false;
  }
  // Normalize (common.cxx:680-688) on N full factors using ||W_i||^2 = trace(G_i); rescales the
  // Grams consistently.
  virtual void normalize(double *const *W, const int64_t *rows, int N, int R, double *Gall) = 0;
  // out[2i] = ||A_i - B_i||^2 (B_i may be null -> ||A_i||^2 only in out[2i+1]), out[2i+1]=||A_i||^2
  // and if B_i != null and update_prev: B_i = A_i afterwards. (als_CP.cxx:594-603, :659-663)
  virtual void diff_norms(double *const *A, double *const *B, const int64_t *n, int N,
                          int store_diff, double *const *D, int update_prev, double *out) = 0;
  // row-block pack/unpack for reduce-scatter / all-gather of a column-major rows x R matrix:
  // blocked[p][x + blk*r] <-> nat[p*blk + x + ld*r]; rows beyond `rows` are zero in blocked
  virtual void pack_blocks(const double *nat, int64_t rows, int64_t ld, int R, int64_t blk, int P,
                           double *blocked) = 0;
  virtual void unpack_blocks(const double *blocked, int64_t rows, int64_t ld, int R, int64_t blk,
                             int P, double *nat) = 0;

  // ---- Tucker: Gram of the mode-`pos` unfolding and its leading eigenvectors ----
  // G[p + J*q] = sum_{l,t} X[l,p,t]*X[l,q,t]   (unroll_tensor_contraction, common.cxx:205-223)
  virtual void unfold_gram(const void *X, int dt, int64_t L, int64_t J, int64_t T, double *G) = 0;
  // U (J x rank, column-major) = leading eigenvectors of symmetric PSD G (J x J), descending
  virtual void top_eigvecs(double *G, int64_t J, int rank, double *U) = 0;
  // the same inside a HOOI iteration: `slot` names a sequence of calls on slowly changing matrices
  // (one per mode), so a back end may keep what it learnt from the previous call of the slot —
  // where the gap below the rank-th eigenvalue lies, the previous basis — and skip the full
  // eigen-decomposition. The result is the same invariant subspace, eigenvectors sorted descending.
  virtual void top_eigvecs_warm(double *G, int64_t J, int rank, double *U, int /*slot*/) {
    top_eigvecs(G, J, rank, U);
  }
  // Lazy eigenvectors. With eig_lazy(slot, true) a warm top_eigvecs_warm may return ANY orthonormal
  // basis of the invariant subspace (all a HOOI sweep needs) and finish the eigen-decomposition
  // inside the subspace off the critical path; eig_pending_rotation(slot) then returns the
  // rank x rank matrix Y (device, column-major, columns sorted by descending eigenvalue) with
  // U_eigenvectors = U_returned * Y — nullptr when U already holds the eigenvectors. The caller
  // applies Y (to the factor and to whatever it derived from it) when it needs eigenvectors and
  // says so with eig_rotation_done(slot).
  virtual void eig_lazy(int /*slot*/, bool /*on*/) {}
  // Deferred acceptance. With eig_defer(slot, true) a lazy warm step of a slot whose recent steps
  // were all accepted at the first attempt may RETURN BEFORE ITS CHECKS HAVE BEEN READ: nothing
  // inside a HOOI sweep then waits for the device, and the host enqueues ahead of it. The caller
  // asks with eig_verify(slot) before it uses the slot again and before it publishes anything that
  // was derived from the returned factor:
  //   -1  nothing pending,  0  the pending step has been accepted,
  //    1  it has NOT: the factor it returned is to be thrown away — the caller restores what it
  //       had before that call and repeats the work from there (the slot is back in the state it
  //       had before the step and takes the checked route next time).
  // discard = true: the pending step is dropped whatever its checks say (its input was wrong).
  virtual void eig_defer(int /*slot*/, bool /*on*/) {}
  // A deferring slot finishes its checks on a second stream, from the Gram the step was given — so
  // that Gram must outlive the call. eig_gram() hands out the slot's own J x J buffer to build the
  // Gram in (after waiting for whatever still reads it), or nullptr: use your own workspace.
  virtual double *eig_gram(int /*slot*/, int64_t /*J*/) { return nullptr; }
  virtual bool eig_deferred(int /*slot*/) { return false; }  // a step of the slot awaits eig_verify
  virtual int eig_verify(int /*slot*/, bool /*discard*/ = false) { return -1; }
  virtual const double *eig_pending_rotation(int /*slot*/) { return nullptr; }
  virtual void eig_rotation_done(int /*slot*/) {}
  // A session's block of 64 warm-start slots [base, base + 64) (what a back end remembers under a
  // slot dies with the session that drew the block)
  virtual int eig_session_new() { return 0; }
  virtual void eig_session_free(int /*base*/) {}
  // U (rows x r, column-major, ld = rows) -> orthonormal columns spanning the same nested
  // subspaces (column k stays in span(U[:, :k+1]) with a positive component on the old column k:
  // a QR factorisation's Q). Returns false, leaving U unspecified, when U is numerically rank
  // deficient.
  virtual bool orthonormalize(double *U, int64_t rows, int r) = 0;
  virtual void sumsq(const double *x, int64_t n, double *out) = 0;  // *out = sum x^2
  // ---- low-rank factor updates (class-API optimizers CPDTLR / CPMSDTLR, src/optimizer/) ----
  // out (rows x C) = A (rows x K) * B (K x C) [+ D (rows x C)]; all column-major fp64, ld = rows
  // for the tall ones, ld = K for B; D may be null or alias out
  virtual void rows_times_small(const double *A, int64_t rows, int K, const double *B, int C,
                                const double *D, double *out) = 0;
  // X[e + n*c] += sum_k T[e + n*k] * VT[k + r*c], c < R: the cached first contraction updated by a
  // rank-r change of the contracted factor (update_cached_tensor, cp_dt_lr_optimizer.cxx:142-168);
  // X is stored in xdt (the tensor's precision), T (n x r) and VT (r x R) are fp64
  virtual void lowrank_accumulate(void *X, int xdt, int64_t n, int R, const double *T, int r,
                                  const double *VT) = 0;
  virtual void add_inplace(double *dst, const double *src, int64_t n) = 0;  // dst += src
  // W[:,k] *= (<W[:,k], Wref[:,k]> > 0 ? +1 : -1)   (als_Tucker.cxx:632-643, :874-885)
  virtual void sign_align(double *W, const double *Wref, int64_t rows, int r) = 0;


  // A stopwatch on the launch stream (the online placement choice of the multi-sweep schedule):
  // timer_begin() marks the stream and returns a handle (-1: no stopwatch to be had), timer_end(h)
  // marks it again, timer_read(h) returns the seconds between the two marks once both have been
  // reached — waiting for them if need be — and gives the handle back. Nothing else synchronises.
  virtual int timer_begin() { return -1; }
  virtual void timer_end(int /*h*/) {}
  virtual double timer_read(int /*h*/) { return -1.0; }

  // profiling of the scan kernels (HIP events on the launch stream)
  virtual void profile_enable(int /*level*/) {}
  virtual void profile_collect() {}
  ProfileSlot prof[2];
  // Route log (tests): when set, the product back end appends one short tag per kernel decision of
  // the contraction launchers (tensor scans, mttv, the thin-GEMM mode products, pp_correct) and of the
  // launchers of the R x R side (mode updates, cp_update, gram_system, Normalize) and of the Tucker
  // eigen side (unfold_gram, top_eigvecs(_warm), eig_verify, orthonormalize, rows_times_small) and of
  // the rank-structured stream (fill_rank, residual_sq: rank.mfma / rank.split / rank.stream) — the
  // kernel family and the facts that chose it. Null: nothing is formatted. The host stand-in logs nothing.
  std::vector<std::string> *route_log = nullptr;
};

class Comm {
 public:
  virtual ~Comm() {}
  virtual int rank() const = 0;
  virtual int size() const = 0;
  virtual bool is_self() const { return false; }  // the no-op single-process communicator
  // all on "device" pointers of the paired Ops, fp64, stream-ordered with the Ops' stream
  virtual void allreduce_sum(double *buf, int64_t n) = 0;
  virtual void reduce_scatter_sum(const double *send, double *recv, int64_t recvcount) = 0;
  virtual void allgather(const double *send, double *recv, int64_t sendcount) = 0;
};

class SelfComm : public Comm {
 public:
  int rank() const override { return 0; }
  int size() const override { return 1; }
  bool is_self() const override { return true; }
  void allreduce_sum(double *, int64_t) override {}
  void reduce_scatter_sum(const double *, double *, int64_t) override {}
  void allgather(const double *, double *, int64_t) override {}
};

}  // namespace ppals
