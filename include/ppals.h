/* ppals.h — C ABI of the MI355X-native ALS sweep engine (libppals.so).
 *
 * Drop-in boundary for the reference's function API (LinjianMa/pairwise-perturbation): the
 * reference has no FFI layer; its boundary is the set of free C++ functions test_ALS.cxx:352-396
 * calls. Each entry point below names the reference interface it replaces. Plain pointers and
 * sizes only — no torch / CTF / C++ types cross this boundary.
 *
 * Conventions (identical to the reference's CTF objects):
 *   - tensors are dense, FIRST INDEX FASTEST: V[i0 + lens[0]*(i1 + lens[1]*(i2 + ...))]
 *   - factor matrix W_i is lens[i] x R, column-major; `Wflat` = W_0,...,W_{N-1} concatenated, fp64
 *   - the tensor lives in HBM as fp32 (PPALS_F32), fp64 (PPALS_F64) or bf16 (PPALS_BF16, CP only);
 *     all factor-matrix, Gram, solve and norm arithmetic is fp64 in every mode, and what is computed
 *     from a bf16 tensor is held in fp32 or fp64
 *   - multi-GPU: one process per GPU; the tensor is block-partitioned along its LEADING mode
 *     (rank p owns rows [p*ceil(s0/P), ...)), factor matrices are replicated
 *
 * Every function returns 0 on success and a negative code on failure (never aborts);
 * ppals_last_error() returns the message. There is NO CPU fallback: without a HIP device
 * ppals_ctx_create fails with PPALS_ERR_NO_DEVICE.
 */
#ifndef PPALS_H
#define PPALS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define PPALS_F32 0
#define PPALS_F64 1

#define PPALS_OK 0
#define PPALS_ERR_NO_DEVICE (-1)
#define PPALS_ERR_HIP (-2)
#define PPALS_ERR_ARG (-3)
#define PPALS_ERR_COMM (-4)
#define PPALS_ERR_UNSUPPORTED (-5)
#define PPALS_MAX_ORDER 8
#define PPALS_UNIQUE_ID_BYTES 128

typedef struct ppals_ctx ppals_ctx;       /* device, stream, workspaces, communicator */
typedef struct ppals_tensor ppals_tensor; /* the (local shard of the) dense input tensor in HBM */
typedef struct ppals_cp ppals_cp;         /* a CP-ALS session: factors, Grams, tree caches in HBM */
typedef struct ppals_cp_multi ppals_cp_multi; /* several CP-ALS starts sharing the tensor scans */
typedef struct ppals_tucker ppals_tucker; /* a Tucker-HOOI session */
typedef struct ppals_parafac2 ppals_parafac2; /* a PARAFAC2 fit: projections, compressed tensor, inner CP session */

const char *ppals_last_error(void);
const char *ppals_version(void);

/* Tucker sessions with a mode extent above 64 use the vendor symmetric eigensolver (rocSOLVER
 * dsyevd). Its libraries register their code objects in milliseconds when they enter the process
 * BEFORE the HIP runtime is initialised, and in minutes afterwards (0.013 s vs 253 s measured).
 * Call this first thing — before ppals_ctx_create and before anything else touches the GPU (e.g.
 * torch.cuda) — in a process that will run such a session. Without it they are loaded on demand:
 * the library then prints one line on stderr (what is about to happen, how long it can take, how to
 * avoid it) before it stalls, and with PPALS_STRICT_PRELOAD=1 in the environment the call that needed
 * the solver fails with PPALS_ERR_UNSUPPORTED instead (csrc/preload_policy.h). */
int ppals_preload_eigensolver(void);

/* ---- context (replaces CTF::World dw, test_ALS.cxx:200) ---- */
int ppals_ctx_create(ppals_ctx **out, int device);
void ppals_ctx_destroy(ppals_ctx *ctx);
/* RCCL bootstrap: rank 0 calls ppals_get_unique_id and ships the 128 bytes to all ranks by any
 * means (torch.distributed, a file, a socket); then every rank calls ppals_ctx_init_comm. */
int ppals_get_unique_id(void *out128);
int ppals_ctx_init_comm(ppals_ctx *ctx, int rank, int nranks, const void *unique_id128);
int ppals_ctx_rank(const ppals_ctx *ctx);
int ppals_ctx_nranks(const ppals_ctx *ctx);
int ppals_ctx_sync(ppals_ctx *ctx);
/* HIP-event kernel timing on the engine's own stream (bench.py roofline leg).
 * which: 0 = tensor-scan kernels (K1/K2/K8), 1 = the other bracketed kernels.
 * level: 0 off, 1 = bracket the tensor scans only (an event pair costs ~10 us of stream time, so
 * the timed region of bench.py pays it on the dominant kernel alone), 2 = bracket both groups */
int ppals_profile_enable(ppals_ctx *ctx, int level);
int ppals_profile_read(ppals_ctx *ctx, int which, int64_t *launches, double *total_ms,
                       double *algo_bytes);
int ppals_profile_reset(ppals_ctx *ctx);

/* ---- tensor (replaces CTF::Tensor<> V and its initialisers, test_ALS.cxx:220-326) ---- */
int ppals_tensor_create(ppals_ctx *ctx, int order, const int64_t *global_lens, int dtype,
                        ppals_tensor **out);
void ppals_tensor_destroy(ppals_tensor *t);
int ppals_tensor_local_rows(const ppals_tensor *t, int64_t *lo, int64_t *n); /* leading-mode shard */
/* `-tensor r` (test_ALS.cxx:275-286): V = [[W_true]] built on the device (build_V, common.cxx:135) */
int ppals_tensor_fill_cp(ppals_tensor *t, int R, const double *Wtrue_flat);
/* `-tensor r2` (test_ALS.cxx:272): V[e] = lo + (hi-lo)*u01(seed, e), e = global linear index */
int ppals_tensor_fill_uniform(ppals_tensor *t, uint64_t seed, double lo, double hi);
/* `-tensor p` / `p2` (laplacian_tensor, common.cxx:575-642; `p` is the same data folded to order
 * dim/2 with extents size^2, fold_unfold common.cxx:870-880): the tensor must have been created
 * with those lens; ndigits = -dim, s = -size */
int ppals_tensor_fill_laplacian(ppals_tensor *t, int ndigits, int s);
/* `-tensor c` (Gen_collinearity + U(-1,1) noise of relative norm ratio_noise, common.cxx:361-423,
 * test_ALS.cxx:246-264) */
int ppals_tensor_fill_collinear(ppals_tensor *t, int R, double col_min, double col_max,
                                double ratio_noise, uint64_t seed);
/* the factor vectors Gen_collinearity draws (host only; lambda folded into mode 0) */
int ppals_collinear_factors(int order, const int64_t *lens, int R, double col_min, double col_max,
                            uint64_t seed, double *Wflat);
/* host data: the FULL tensor in fp64, first index fastest (the layout read_dense_from_file
 * implies, test_ALS.cxx:289-325); each rank keeps its own leading-mode rows */
int ppals_tensor_upload(ppals_tensor *t, const double *host_full);
/* A tensor may be re-filled / re-uploaded while CP or Tucker sessions created on it are alive:
 * every fill or upload bumps the tensor's generation, and a session rebuilds what it derived from
 * the old contents (its second resident layout; cached tree nodes and PP operators are dropped)
 * the next time it reads the tensor. Not while one of the session's calls is running. */
/* the reverse (the commented-out V.write_dense_to_file, test_ALS.cxx:347): this rank's leading-mode
 * rows, widened to fp64, into their places of the FULL host tensor; other ranks' rows untouched */
int ppals_tensor_download(ppals_tensor *t, double *host_full);

/* ---- the tensor from and to DEVICE memory (a torch.Tensor in HBM, say) ----
 * A view is a box of the GLOBAL tensor, box_lo[i] <= index_i < box_lo[i] + box_len[i] (NULL/NULL: the
 * whole tensor), whose element (j_0, ..., j_{N-1}) (box-relative) is at ptr + sum_i j_i * strides[i]
 * elements; strides >= 0 (0: broadcast), NULL = dense over the box, first index fastest (a C-contiguous
 * torch tensor has the REVERSED strides). Each rank copies the part of the box in its own leading-mode
 * rows and touches nothing else. `stream` is the hipStream_t the caller works on (NULL: the null
 * stream): the copy starts after the work already queued there, and work queued there later runs
 * after it; the host does not block. Every bad argument is refused before anything is launched. */
#define PPALS_F16 2  /* an import source only                                              */
#define PPALS_BF16 3 /* an import source, or a tensor's storage (ppals_tensor_create):     */
/* values stored as torch rounds float64 to bfloat16 (fp64 -> fp32 -> bf16, each round-to-nearest-even);
 * every tensor entry point and every CP session takes such a tensor, ppals_tucker_create refuses it
 * with PPALS_ERR_UNSUPPORTED. A back end that cannot hold bf16 refuses it at creation, likewise. */
/* Copy the view at src (type F32, F64, F16 or BF16, on the context's device) into the tensor,
 * converting to its storage type on the device (f16/bf16/f32 -> f64 exact; f64 -> f32 rounds to
 * nearest even, bit-identical to ppals_tensor_upload; into bf16 storage a bf16 view copies bit for bit
 * and wider views round as above). Bumps the generation like an upload. */
int ppals_tensor_import_device(ppals_tensor *t, const void *src, int src_dtype, const int64_t *box_lo,
                               const int64_t *box_len, const int64_t *strides, void *stream);
/* The reverse: this rank's rows of the box into the view at dst (type F32 or F64). The destination
 * must not overlap itself: no zero stride on an extent > 1, and with the modes of extent > 1 sorted
 * by stride, each stride beyond the last element of the modes before it. */
int ppals_tensor_export_device(ppals_tensor *t, void *dst, int dst_dtype, const int64_t *box_lo,
                               const int64_t *box_len, const int64_t *strides, void *stream);
/* Every check the two calls make, pointer queries included, and no launch: returns PPALS_OK or the
 * error the call would return, with ppals_last_error() saying why. direction 0 = import, 1 = export.
 * The pointer must be device memory of the context's device (not host, pinned host or managed
 * memory) and the view's byte span (sum_i (len_i - 1) * stride_i + 1) * elem_size must lie inside
 * the allocation that holds it. */
int ppals_tensor_check_device_view(ppals_tensor *t, int direction, const void *ptr, int dtype,
                                   const int64_t *box_lo, const int64_t *box_len,
                                   const int64_t *strides);
int ppals_tensor_norm(ppals_tensor *t, double *out); /* V.norm2(), test_ALS.cxx:328 */

/* ---- centring and scaling in place: PARAFAC preprocessing (R. Bro, A. K. Smilde, "Centering and scaling in
 * component analysis", J. Chemometrics 17 (2003) 16-33; `nprocess` of the N-way toolbox; no counterpart in the
 * reference) ----
 * A constant offset per fibre is not multilinear: "rank-R model + offsets" is not rank R until it has been
 * centred ACROSS the right mode; scaling WITHIN a mode gives every slice of that mode unit root mean square.
 * Throughout, the tensor is viewed as [L, J, T], first index fastest: J = lens[mode], L the product of the
 * extents before `mode`, T of those after it. A fibre of the mode is the J elements with (l, t) fixed, a slice
 * x the n = L*T elements with j = x. Offsets are L*T doubles, index l + L*t.
 * Arithmetic: V is read as stored (bf16, fp32 or fp64), widened to fp64, and the new value is rounded ONCE to
 * the storage type, as ppals_tensor_import_device rounds an fp64 source. Means and sums of squares are formed
 * in fp64 in a fixed order: the same state gives the same bits on every call; no floating-point atomics.
 * shift with alpha = +-1 forms v +- o with one fp64 rounding, so shift(offsets, -1) on a copy of the original
 * tensor gives, bit for bit, what center stored. scale: a slice whose rms is not a positive finite number is
 * left bit for bit as it is and its scales[x] reports the value as computed (0, inf or NaN). No other special
 * cases: a NaN in a fibre makes that fibre NaN.
 * `where` says where the offsets lie. PPALS_HOST: the call returns when the host buffer is filled (center) or
 * consumed (shift); it uses a temporary device buffer of L*T doubles, freed before it returns. PPALS_DEVICE: the
 * pointer must be device memory of the context's device with L*T*8 bytes inside its allocation (the checks and
 * messages of the device views); the call is ordered on `stream` exactly as ppals_tensor_import_device is and
 * the host does not block; a back end without device views answers PPALS_ERR_UNSUPPORTED. With offsets == NULL
 * in center, `where` is ignored and the call does not block. All five calls are ordered after the work already
 * queued on the engine stream, sweeps a session queued asynchronously included.
 * center, shift, scale and rescale bump the tensor's generation exactly as an import does: every CP and Tucker
 * session on the tensor rebuilds its other layouts and packed twins at its next read and drops tree nodes,
 * multi-sweep state and PP operators; a Tucker session also forgets the warm starts of its eigen-steps, so that
 * its next hosvd / sweeps are bit for bit those of a new session on the new contents. slice_sumsq reads only
 * and bumps nothing. A centred fp32 tensor has
 * blocks of mixed sign: the packed 28-bit twin of the CP scans then no longer qualifies and the session reads
 * the plain layouts (the 537 instead of the 632 sweeps/s class at the headline shape).
 * The calls take no mask: centring with missing entries belongs inside the EM loop (Bro & Smilde, section 6)
 * and is not provided.
 * Refused before anything is launched or allocated, the tensor's bytes and generation untouched, the message
 * starting with the function's name — PPALS_ERR_ARG: a NULL tensor or a dead handle, mode outside [0, N), a
 * NULL ss, factors, or offsets in shift, where outside {0, 1}, a non-finite alpha or factors[x], a device
 * pointer that fails the checks above; PPALS_ERR_UNSUPPORTED: a context of more than one rank (centring across
 * the sharded mode needs a collective of L*T values; all five calls refuse alike). */
#define PPALS_HOST 0
#define PPALS_DEVICE 1
/* V[l,j,t] <- V[l,j,t] - mean_j V[l,.,t], for every fibre of `mode`.
 * offsets (may be NULL) receives the L*T means as fp64, index l + L*t. */
int ppals_tensor_center(ppals_tensor *t, int mode, double *offsets, int where, void *stream);
/* V[l,j,t] <- V[l,j,t] + alpha * offsets[l + L*t]. alpha = +1 undoes a centring,
 * alpha = -1 applies a calibration set's means to new data. */
int ppals_tensor_shift(ppals_tensor *t, int mode, const double *offsets, int where, double alpha, void *stream);
/* ss[x] = sum over slice x of V^2, host, lens[mode] doubles. Read-only, no generation bump. */
int ppals_tensor_slice_sumsq(ppals_tensor *t, int mode, double *ss);
/* rms[x] = sqrt(ss[x] / n). Slice x is multiplied by 1/rms[x].
 * scales (host, lens[mode] doubles, may be NULL) receives rms. */
int ppals_tensor_scale(ppals_tensor *t, int mode, double *scales);
/* slice x is multiplied by factors[x] (host). Undoes a scaling, or applies a calibration set's scaling. */
int ppals_tensor_rescale(ppals_tensor *t, int mode, const double *factors);
/* same counter-based generator for host-side factor initialisation (W.fill_random(0,1)) */
void ppals_fill_uniform_host(double *out, int64_t n, uint64_t seed, uint64_t offset, double lo,
                             double hi);

/* ---- kernel-level entry points (per-kernel parity tests; single rank or sharded) ---- */
/* dimension-tree node, e.g. key "ab" -> T[a,b,r] (mttkrp_map_DT, common.cxx:20-133). Sharded:
 * nodes that keep mode 0 return the local rows, others the local PARTIAL sum. out may be NULL
 * to query the element count through *n. */
int ppals_tree_node(ppals_cp *s, const char *key, double *out, int64_t *n);
/* MTTKRP of one mode through the dimension tree (als_CP.cxx:239-284); full s_mode x R result
 * (summed over ranks) */
int ppals_mttkrp(ppals_cp *s, int mode, double *M);
/* PP operator: V contracted with the modes in `contracted` (Build_mttkrp_map, als_CP.cxx:352) */
int ppals_pp_operator(ppals_cp *s, const char *contracted, double *out, int64_t *n);
/* ||V - [[W]]||_F (als_CP.cxx:183-187), streaming, nothing materialised */
int ppals_cp_residual(ppals_cp *s, double *out);
/* S = Hadamard_{j!=mode} W_j^T W_j + lambda I and its inverse as the engine computes them */
int ppals_cp_gram_system(ppals_cp *s, int mode, double lambda, double *S, double *Sinv);

/* ---- CP sessions ---- */
int ppals_cp_create(ppals_ctx *ctx, ppals_tensor *V, int R, ppals_cp **out);
void ppals_cp_destroy(ppals_cp *s);
int ppals_cp_set_factors(ppals_cp *s, const double *Wflat, const double *gradWflat /*may be NULL*/);
int ppals_cp_get_factors(ppals_cp *s, double *Wflat, double *gradWflat /*may be NULL*/);
/* How an exact sweep walks the tensor — the ALS iterates are identical either way.
 * PPALS_SCHEDULE_DT: the two first-level nodes of alsCP_DT (mttkrp_map_DT, common.cxx:20-133), two
 * tensor scans per sweep. PPALS_SCHEDULE_MSDT (default): the multi-sweep tree of the class API
 * (cp_msdt_optimizer.cxx:172-207), N/(N-1) scans per sweep. */
#define PPALS_SCHEDULE_DT 0
#define PPALS_SCHEDULE_MSDT 1
int ppals_cp_set_schedule(ppals_cp *s, int schedule);
int ppals_cp_get_schedule(const ppals_cp *s);
/* Non-negative CP. With the flag on, every mode update of the session is one pass of Cichocki-Phan
 * HALS instead of the solve of the normal equations: with M the mode's MTTKRP and S the Hadamard
 * product of the other modes' Grams + lambda I, for every row x and r = 0 .. R-1 in this order
 *   w[x,r] <- max(PPALS_NN_FLOOR, w[x,r] + (M[x,r] - sum_q w[x,q] S[q,r]) / S[r,r])
 * (fp64; the sum takes the row's entries already updated; a column whose S[r,r] is not a positive
 * finite number stays). The floor is not zero, so no column can die under Normalize, which scales
 * columns by positive numbers and so keeps the constraint. grad_W, gradnorm and the residual keep
 * their meaning. The tensor scans, both schedules and the drivers built on exact sweeps
 * (ppals_cp_sweeps_dt, ppals_cp_dt, ppals_cpd_als, ppals_cp_em) run unchanged on top.
 * PPALS_ERR_UNSUPPORTED, before anything is launched: turning the flag on in a context of more than one
 * rank or at R > 64, and on a non-negative session ppals_cp_pp, ppals_cp_pp_partupdate,
 * ppals_cpd_als_lr and ppals_cp_multi_take from an UNCONSTRAINED multi-start session (whose factors may
 * be negative; a non-negative multi-start session, ppals_cp_multi_set_nonneg below, hands its starts to
 * any ordinary session). PPALS_ERR_ARG: factors with a negative or non-finite entry
 * — those already set when the flag is turned on (the flag then stays off), and those handed to
 * ppals_cp_set_factors later. ppals_cp_get_nonneg: 1 / 0, PPALS_ERR_ARG for a NULL session. */
#define PPALS_NN_FLOOR 1e-16
int ppals_cp_set_nonneg(ppals_cp *s, int on);
int ppals_cp_get_nonneg(const ppals_cp *s);
/* Per-mode constraints: one kind per mode (kinds[N]), FREE everywhere at first. Throughout, M is the
 * mode's MTTKRP and S the Hadamard product of the other modes' Grams + lambda I.
 *   PPALS_MODE_FREE    the solve of the normal equations. A session whose kinds are all FREE is bit for bit
 *                      a session on which the call was never made.
 *   PPALS_MODE_NONNEG  one HALS pass, exactly that of ppals_cp_set_nonneg above. A session whose kinds are
 *                      all NONNEG is bit for bit one with ppals_cp_set_nonneg(s, 1); that call is "all modes
 *                      NONNEG, or all modes FREE", and ppals_cp_get_nonneg returns 1 only if every mode is.
 *   PPALS_MODE_FIXED   the factor is never updated: neither the mode's leaf contraction nor an update is
 *                      launched, the factor and its Gram read back bit for bit as they were set. grad_W of
 *                      the mode and its share of the gradient norm are zero: zeroed when the mode becomes
 *                      FIXED, and gradients handed to ppals_cp_set_factors for it are ignored. Cached
 *                      contractions are not dropped on its account.
 *   PPALS_MODE_ORTHO   orthonormal columns: W <- M (M^T M)^(-1/2), the orthonormal polar factor of M in fp64,
 *                      which minimises the mode's least-squares problem under W^T W = I (lambda does not
 *                      enter it: ||W||^2 is constant). grad = -M + W_old S as for every kind. The Gram of the
 *                      new W is computed, not assumed to be I. With theta the eigenvalues of M^T M: if any is
 *                      not a positive finite number, or theta_min <= theta_max * PPALS_ORTHO_MIN_RATIO
 *                      (u kappa(M)^2 = 2^-13 at that ratio: no polar factor to speak of), the factor stays
 *                      as it is — for that start, in a multi-start session — and the gradient is still
 *                      written. Needs s_mode >= R (of every start). The factor need not be orthonormal when
 *                      it is set: the first update makes it so.
 * Normalize would rescale a FIXED factor and destroy orthonormal columns: in a session with at least one
 * FIXED or ORTHO mode the Normalize step of ppals_cp_sweeps_dt and of every driver built on it (ppals_cp_dt,
 * ppals_cp_em) is skipped — such sweeps are those of ppals_cpd_als. Mixtures of FREE and NONNEG keep it.
 * grad_W, the gradient norm and the residual keep their definitions; as with NONNEG, the unconstrained
 * gradient does not vanish at a constrained optimum. The kinds may be changed between calls; factors,
 * Grams and caches are untouched by the call itself. The read-only diagnostics (core consistency,
 * congruence and factor match score, slice residuals and leverages, model export, imputation) work
 * unchanged.
 * Every refusal happens before anything is launched and leaves the kinds as they were. PPALS_ERR_ARG: a
 * NULL session or kinds, a kind outside 0..3, ORTHO on a mode shorter than the rank, a mode that becomes
 * NONNEG while its factor has a negative or non-finite entry (and such a factor in ppals_cp_set_factors
 * later). PPALS_ERR_UNSUPPORTED: any kind but FREE in a context of more than one rank, with the collective
 * paths forced or under PPALS_TEST_BLOCKED_UPDATE; NONNEG or ORTHO at R > 64 (FREE and FIXED take any rank);
 * ppals_cp_pp, ppals_cp_pp_partupdate and ppals_cpd_als_lr on a session with a mode that is not FREE;
 * ppals_cp_multi_take into a session that is NONNEG in a mode where the multi-start session is not. */
#define PPALS_MODE_FREE 0
#define PPALS_MODE_NONNEG 1
#define PPALS_MODE_FIXED 2
#define PPALS_MODE_ORTHO 3
#define PPALS_ORTHO_MIN_RATIO 9.094947017729282379150390625e-13 /* 2^-40 */
int ppals_cp_set_mode_constraints(ppals_cp *s, const int *kinds /* N */);
int ppals_cp_get_mode_constraints(const ppals_cp *s, int *kinds /* N */);
/* Shapes for non-negative modes: one shape per mode (shapes[N]), NONE everywhere at first. A shape refines a
 * mode of kind PPALS_MODE_NONNEG and no other; the kinds, and ppals_cp_get_mode_constraints, know nothing of it.
 *   PPALS_SHAPE_NONE        the HALS pass as it is. A session whose shapes are all NONE is bit for bit, and
 *                           launch for launch, a session on which the call was never made.
 *   PPALS_SHAPE_UNIMODAL    every column rises to one peak and falls: for some row p it is non-decreasing on rows
 *                           0..p and non-increasing on rows p+1..s-1 (plateaus allowed; monotone columns included)
 *   PPALS_SHAPE_INCREASING  every column is non-decreasing over the rows
 *   PPALS_SHAPE_DECREASING  every column is non-increasing over the rows
 * The update of a shaped mode (Bro & Sidiropoulos, J. Chemometrics 1998), in fp64: grad = -M + W_old S as for
 * every kind; then for r = 0 .. R-1 in this order, with d = S[r,r],
 *   v[x] = w[x,r] + (M[x,r] - sum_q w[x,q] S[q,r]) / d   for all rows x, columns q < r already replaced,
 *   w[:,r] <- the u of least ||u - v||^2 among the sequences of the shape with u >= PPALS_NN_FLOOR
 * (pool-adjacent-violators, clipped at the floor; for UNIMODAL the peak row of least error, the smallest on a
 * tie). A column whose d is not a positive finite number, or whose v has a non-finite entry, stays as it is.
 * Each column step minimises over a set that holds the current column once the factor has the shape, so from
 * the first sweep on the residual does not rise. The factor need not have the shape when the call is made: the
 * first update projects it. Normalize stays on: a positive column scale keeps every shape. Everything a NONNEG
 * mode allows works (both schedules, ppals_cp_sweeps_dt, ppals_cp_dt, ppals_cpd_als, ppals_cp_em, multi-start
 * and rank-sweep sessions; ppals_cp_multi_take copies factors and ignores shapes), and everything it refuses
 * stays refused. ppals_cp_set_mode_constraints and ppals_cp_set_nonneg reset to NONE the shape of every mode
 * that ends up not NONNEG.
 * Every refusal happens before anything is launched and leaves shapes and session as they were, the message
 * starting with the function's name. PPALS_ERR_ARG: a NULL session or shapes, a shape outside 0..3, a shape
 * other than NONE on a mode whose kind is not NONNEG. PPALS_ERR_UNSUPPORTED: a shape on the hold-out mode, and
 * ppals_cp_multi_set_holdout on a shaped mode (zeroed rows break any shape). */
#define PPALS_SHAPE_NONE 0
#define PPALS_SHAPE_UNIMODAL 1
#define PPALS_SHAPE_INCREASING 2
#define PPALS_SHAPE_DECREASING 3
int ppals_cp_set_mode_shapes(ppals_cp *s, const int *shapes /* N */);
int ppals_cp_get_mode_shapes(const ppals_cp *s, int *shapes /* N */);
/* Where the multi-sweep schedule's first-level intermediates lie (no counterpart in the reference:
 * CTF places its own buffers). The choice is made ONLINE: the first ~20 visits of a root run the
 * sweep's own scan at a different offset / store kind of the result, timed on the stream; then the
 * root keeps the fastest. No set-up time, the results do not depend on it. One JSON object
 * {"mode": "online"|"off", "setup_s": 0, "roots": [{"root", "layout", "settled", "visits",
 * "offset_mb", "store", "best_ms", "worst_ms"}]} written to buf (NUL-terminated).
 * PPALS_PLACE_TUNE=0 switches the choice off (offset 0, store kind by size). */
int ppals_cp_placement_report(const ppals_cp *s, char *buf, int cap);
/* The operator builds of the PP phases (Build_mttkrp_map + the N full MTTKRPs, als_CP.cxx:678-694)
 * since the last reset: their number and — while timing is on — their duration, the stream
 * synchronised on both sides of each. mode 0: read only; +1: read, then reset and turn timing on;
 * -1: read, then reset and turn it off. (The reference's [dtime] column counts a build inside the
 * interval that ends at the first PP row, als_CP.cxx:667-697.) */
int ppals_cp_pp_build_stats(ppals_cp *s, int mode, int64_t *builds, double *seconds);
/* n exact dimension-tree sweeps (body of alsCP_DT's loop incl. Normalize, als_CP.cxx:215-303),
 * enqueued asynchronously on the engine stream; no print block, no host sync */
int ppals_cp_sweeps_dt(ppals_cp *s, int n, double lambda);
/* sqrt(sum_i ||grad_W[i]||^2) of the last sweep (als_CP.cxx:174-181) */
int ppals_cp_gradnorm(ppals_cp *s, double *out);

typedef struct {
  double tol;        /* absolute: caller passes -tol * ||V|| (test_ALS.cxx:354) */
  double timelimit;  /* seconds */
  int maxiter;
  double lambda;     /* regularisation (-lambda) */
  int resprint;      /* print/CSV period (-resprint) */
  int bench;         /* pp_bench mode: emit [DTtime]/[PPfirst]/[PPsecond] instead of rows */
  double tol_init;   /* PP restart tolerance (-pp_res_tol) */
  double ratio_step; /* PP update magnitude (-magni) */
  const char *csv_path; /* NULL: no CSV; the file is opened, written and closed by the callee */
  int csv_append;    /* bench mode appends to an existing file */
  int verbose;       /* 1: console output identical to the reference's rank-0 cout/printf */
  double update_percentage; /* -pp 2 only (-update_percentage_pp): fraction of modes per sweep */
} ppals_cp_opts;

/* alsCP_DT (als_CP.h:30-32, als_CP.cxx:127-320). Returns 1 if it stopped before maxiter+1
 * (the reference's `true`), 0 if it ran out of iterations, <0 on error. */
int ppals_cp_dt(ppals_cp *s, const ppals_cp_opts *o, int *iters);
/* alsCP_PP (als_CP.h:105-108, als_CP.cxx:1082-1137) */
int ppals_cp_pp(ppals_cp *s, const ppals_cp_opts *o, int *iters);
/* alsCP_PP_partupdate (als_CP.h:117-122, als_CP.cxx:1146-1207): `-pp 2` */
int ppals_cp_pp_partupdate(ppals_cp *s, const ppals_cp_opts *o, int *iters);

/* ---- class API (src/CP.h, src/optimizer/) ----
 * CPD<dtype, Optimizer>::als(tol, timelimit, maxsweep, resprint, Plot_File, bench)
 * (src/CP.h:42-43, src/CP.cxx:100-186) after CPD::Init (= ppals_cp_set_factors; o->lambda is Init's
 * lambda). `optimizer` names the reference class whose step() cadence and fractional sweep counter
 * are reproduced: CPSimpleOptimizer (1 sweep/step, cp_simple_optimizer.cxx:21-56), CPDTOptimizer
 * (0.5, cp_dt_optimizer.cxx:195-237), CPMSDTOptimizer ((N-1)/N, cp_msdt_optimizer.cxx:172-207).
 * o->maxiter is maxsweep; no Normalize is applied (src/CP.cxx:171). *sweeps = final counter.
 * Returns 1 unless sweeps == maxsweep+1 (the reference's bool), <0 on error. */
#define PPALS_OPT_SIMPLE 0
#define PPALS_OPT_DT 1
#define PPALS_OPT_MSDT 2
int ppals_cpd_als(ppals_cp *s, int optimizer, const ppals_cp_opts *o, double *sweeps, int *iters);
/* The low-rank-update optimizers (run.cxx:401-407, `-pp 2` / `-pp 3`): CPDTLROptimizer
 * (cp_dt_lr_optimizer.cxx:170-236, 0.5 sweep/step) and CPMSDTLROptimizer
 * (cp_msdt_lr_optimizer.cxx:163-205, (N-1)/N sweep/step) with update_rank = run.cxx's -updaterank
 * and randomsvd = run.cxx's -randomsvd: 0 = get_rankR_update_cholesky with the full SVD
 * (common.cxx:768-786), 1 = with randomized_svd(X, r, 1) (common.cxx:691-709; its R x r start
 * matrix comes from this library's counter generator — CTF's stream is not reproducible — with a
 * fixed seed, a fresh block of draws per update, restarted by every call). The first contraction of
 * a step is kept per root and updated with update_rank tensor columns when the contracted factor
 * has changed by a low-rank update only (update_cached_tensor). Single GPU, order >= 3. */
#define PPALS_OPT_DT_LR 3
#define PPALS_OPT_MSDT_LR 4
int ppals_cpd_als_lr(ppals_cp *s, int optimizer, int update_rank, int randomsvd,
                     const ppals_cp_opts *o, double *sweeps, int *iters);

/* ---- multi-start CP sessions (no counterpart in the reference, whose job scripts loop over seeds) ----
 * CP-ALS finds local minima, so one runs several initialisations and keeps the best. A multi-start
 * session sweeps `nstarts` independent rank-R models of ONE tensor together: every contraction of a
 * sweep (the tensor scans above all: HBM-bound, 5 flop/B at R = 10) runs once on nstarts * R columns,
 * and only the R x R normal equations are solved start by start — all of them in one launch. Start b
 * evolves exactly as an ordinary session does under ppals_cpd_als with PPALS_OPT_SIMPLE from the same
 * factors: cyclic mode updates 0..N-1, no Normalize (one scalar per mode would couple the starts).
 * nstarts in [1, 32], R * nstarts <= 128, any storage type a CP session takes (a bf16 tensor is
 * scanned in passes of 16 columns, so above 16 columns it gains nothing over separate sessions);
 * one rank only: a context with more ranks gets PPALS_ERR_UNSUPPORTED. Every bad argument is refused
 * with PPALS_ERR_ARG and a message before anything is launched. */
#define PPALS_MULTI_MAX_STARTS 32
#define PPALS_MULTI_MAX_COLUMNS 128
int ppals_cp_multi_create(ppals_ctx *ctx, ppals_tensor *V, int R, int nstarts, ppals_cp_multi **out);
/* A rank sweep: a multi-start session whose starts have their own ranks, start b a rank-ranks[b] model —
 * ranks 2 .. 10 are 54 columns of ONE tensor scan instead of nine sessions' scans. nstarts in [1, 32],
 * every ranks[b] >= 1, their sum <= 128; a NULL `ranks` and every other bad argument is refused with
 * PPALS_ERR_ARG and a message before anything is allocated or launched. Everything below works on such
 * a session start by start with that start's rank: start b evolves as an ordinary rank-ranks[b] session
 * does; in device memory it owns the columns [off_b, off_b + ranks[b]) of every factor, gradient and
 * MTTKRP result, off_b = ranks[0] + .. + ranks[b-1]. A session whose ranks are all equal is the session
 * ppals_cp_multi_create makes, bit for bit. */
int ppals_cp_multi_create_ranks(ppals_ctx *ctx, ppals_tensor *V, int nstarts, const int *ranks,
                                ppals_cp_multi **out);
/* *nstarts and, when ranks != NULL, ranks[0 .. nstarts) of any multi-start session (nstarts times R for
 * one from ppals_cp_multi_create) */
int ppals_cp_multi_ranks(const ppals_cp_multi *s, int *nstarts, int *ranks /* may be NULL */);
void ppals_cp_multi_destroy(ppals_cp_multi *s);
/* one start's factors (and gradients) in the Wflat layout of ppals_cp_set_factors for a session of that
 * start's rank (sum_i s_i * ranks[start] doubles); start = -1: all starts, one such block after the
 * other, each of its own length */
int ppals_cp_multi_set_factors(ppals_cp_multi *s, int start, const double *Wflat,
                               const double *gradWflat /*may be NULL*/);
int ppals_cp_multi_get_factors(ppals_cp_multi *s, int start, double *Wflat /*may be NULL*/,
                               double *gradWflat /*may be NULL*/);
/* as ppals_cp_set_schedule (default PPALS_SCHEDULE_MSDT) */
int ppals_cp_multi_set_schedule(ppals_cp_multi *s, int schedule);
/* n sweeps of N mode updates each, enqueued asynchronously like ppals_cp_sweeps_dt */
int ppals_cp_multi_sweeps(ppals_cp_multi *s, int n, double lambda);
/* out[nstarts]: per start what ppals_cp_residual / ppals_cp_gradnorm return for that model (the
 * residuals take one streaming pass over the tensor per start) */
int ppals_cp_multi_residuals(ppals_cp_multi *s, double *out);
int ppals_cp_multi_gradnorms(ppals_cp_multi *s, double *out);
/* Sweeps until o->maxiter sweeps, o->timelimit seconds, or the gradient norm of the best start (the
 * one with the smallest residual) is below o->tol; looks every o->resprint sweeps. Uses tol,
 * timelimit, maxiter, lambda and resprint of the options and ignores the rest. *sweeps = sweeps run,
 * *best = the best start at the last look. Returns 1 if it stopped before maxiter, 0 if not.
 * In a session whose ranks DIFFER the smallest residual is almost always the largest rank's, and its
 * gradient says nothing about the others: there the run stops when the LARGEST gradient norm over all
 * starts is below o->tol (or on maxiter / timelimit); *best is still the start with the smallest residual. */
int ppals_cp_multi_run(ppals_cp_multi *s, const ppals_cp_opts *o, int *sweeps, int *best);
/* Start `start`'s factors and gradients, device to device, into an ordinary session of the same
 * context and tensor and of that start's rank (any other rank: PPALS_ERR_ARG, the message names both); on `dst` the effect is that of ppals_cp_set_factors (caches dropped, Grams
 * refreshed): the winner goes on there with Normalize, PP, the drivers and the model export.
 * A non-negative `dst` (ppals_cp_set_nonneg) takes from a non-negative multi-start session only: from
 * an unconstrained one the call is refused with PPALS_ERR_UNSUPPORTED. An ordinary `dst` takes from both. */
int ppals_cp_multi_take(ppals_cp_multi *s, int start, ppals_cp *dst);
/* Non-negative multi-start sessions. With the flag on, every start updates by the HALS pass of
 * ppals_cp_set_nonneg, all starts in one batched update per mode on the unchanged shared tensor scans:
 * start b evolves exactly as an ordinary non-negative session does under ppals_cpd_als with
 * PPALS_OPT_SIMPLE from the same factors (cyclic modes 0..N-1, no Normalize, S that start's Hadamard of
 * Grams + lambda I, grad from the pre-update row, entries >= PPALS_NN_FLOOR). Sweeps, run, residuals,
 * gradnorms, the schedules and get_factors run unchanged on top. PPALS_ERR_UNSUPPORTED, before anything
 * is launched: a start of rank > 64 and PPALS_TEST_BLOCKED_UPDATE. Starts of different ranks each take the
 * HALS pass of their own rank. PPALS_ERR_ARG:
 * factors of any start with a negative or non-finite entry — those already set when the flag is turned
 * on (the flag then stays off), and those handed to ppals_cp_multi_set_factors later (the host buffer
 * is looked at before anything is uploaded). ppals_cp_multi_get_nonneg: 1 / 0, PPALS_ERR_ARG for NULL. */
int ppals_cp_multi_set_nonneg(ppals_cp_multi *s, int on);
int ppals_cp_multi_get_nonneg(const ppals_cp_multi *s);
/* The per-mode constraints of ppals_cp_set_mode_constraints for a multi-start or rank-sweep session: one
 * kind per mode, shared by all starts (kinds[N]). Start b evolves exactly as an ordinary session of its
 * rank with the same kinds does under ppals_cpd_als with PPALS_OPT_SIMPLE; an ORTHO update whose M has no
 * polar factor leaves that start's factor alone. ORTHO needs s_mode >= the largest start's rank, NONNEG
 * and ORTHO every start's rank <= 64. PPALS_ERR_UNSUPPORTED in addition: ppals_cp_multi_set_holdout on a
 * FIXED or ORTHO mode, and making the hold-out mode FIXED or ORTHO. */
int ppals_cp_multi_set_mode_constraints(ppals_cp_multi *s, const int *kinds /* N: one kind per mode, for all starts */);
int ppals_cp_multi_get_mode_constraints(const ppals_cp_multi *s, int *kinds /* N */);
/* The shapes of ppals_cp_set_mode_shapes for a multi-start or rank-sweep session: one shape per mode, shared by
 * all starts, every start's columns projected on their own (nothing couples two starts; a start matches an
 * ordinary session of the same start bit for bit). The same rules and refusals. */
int ppals_cp_multi_set_mode_shapes(ppals_cp_multi *s, const int *shapes /* N, for all starts */);
int ppals_cp_multi_get_mode_shapes(const ppals_cp_multi *s, int *shapes /* N */);

/* ---- core consistency diagnostic (CORCONDIA: R. Bro, H. A. L. Kiers, "A new efficient method for
 * determining the number of components in PARAFAC models", J. Chemometrics 17 (2003) 274-286; no
 * counterpart in the reference) ----
 * The residual falls with the rank and cannot choose one; the core consistency drops sharply at the first
 * rank that over-factors. For a model with the session's current factors W_i (s_i x R, no separate
 * weights) let P_i = W_i (W_i^T W_i)^-1, the transposed pseudo-inverse (no lambda). The core G has R^N
 * entries, first index fastest like every tensor here:
 *   G[r_0,...,r_{N-1}] = sum_{i_0..i_{N-1}} V[i_0,...,i_{N-1}] * prod_k P_k[i_k, r_k]
 *   cc = 100 * (1 - sum (G - T)^2 / R),      T[r,...,r] = 1 and zero elsewhere
 * with V as stored (the bf16 / fp32 / fp64 values the session works on). cc is not clamped: it may be
 * negative. V = [[W]] exactly with factors of full column rank gives G = T and cc = 100.
 * The call reads the session and changes nothing of it — factors, Grams, gradients, cached contractions
 * and the tensor's generation stay, and later sweeps give bit for bit the factors they give without it;
 * its work buffers are its own, grow-only, kept by the session for its next call. Every storage type,
 * both schedules, non-negative sessions, equal-rank and rank-sweep multi-start sessions. The tensor is
 * read ONCE, by one scan on the columns of all starts together; the rest works on that scan's result.
 * A start one of whose Grams W_i^T W_i meets a pivot that is not a positive finite number in the
 * elimination (a zero column; R > s_i, unless rounding leaves the last pivots tiny and positive: the
 * figure is then meaningless and huge) gets cc = NaN, and NaN in every entry of its core; the call still
 * returns PPALS_OK and the other starts are unaffected.
 * PPALS_ERR_UNSUPPORTED, before anything is launched, the message starting with the function's name: a
 * context of more than one rank; a start whose R^N exceeds 2^24 entries (128 MB of fp64 core); a start of
 * rank above 64 (the Grams are inverted in LDS; ranks 65 .. 128 are refused, not routed elsewhere).
 * PPALS_ERR_ARG: a NULL session, a NULL cc, start out of range. */
/* *cc = core consistency of the session's current model. core may be NULL. n may be NULL.
 * *n receives R^N; with core == NULL this is a size query. */
int ppals_cp_core_consistency(ppals_cp *s, double *cc, double *core, int64_t *n);
/* cc[nstarts]: one value per start, each with its own rank */
int ppals_cp_multi_core_consistency(ppals_cp_multi *s, double *cc);
/* start's core, ranks[start]^N doubles; core == NULL: size query through *n (nothing is launched) */
int ppals_cp_multi_core(ppals_cp_multi *s, int start, double *core, int64_t *n);

/* ---- factor match score: Tucker's congruence across starts and between sessions (R. A. Harshman's
 * split-half validation; tlviz factor_match_score, TensorLy congruence_coefficient; no counterpart in the
 * reference) ----
 * Did two fits find the same components? Two column sets are compared: a with columns p < Ca, b with
 * columns q < Cb, of the same order N and with the same extents in every compared mode. The compared
 * modes are all modes (skip_mode = -1) or all but skip_mode (0 <= skip_mode < N), in which the extents
 * may differ: the split mode of a split-half analysis.
 *   Phi[p,q] = prod over compared modes i of (a_i[:,p] . b_i[:,q]) / (|a_i[:,p]| |b_i[:,q]|)    (signed, fp64)
 *   w_a[p]   = prod over ALL N modes of |a_i[:,p]|                                             (likewise w_b)
 * A column whose norm in some compared mode is not a positive finite number gives Phi = 0 in its whole
 * row or column: Phi is never NaN. The sign is kept: CP's sign indeterminacy flips pairs of modes and
 * leaves the product unchanged; an odd number of flips is a different component. Phi is stored
 * column-major, Phi[p + Ca*q]; a multi-start session's columns are those of all its starts, start b owning
 * [off_b, off_b + ranks[b]) as everywhere else.
 * The factor match score of a rank-ra model against a rank-rb one, m = min(ra, rb):
 *   score[p,q] = Phi[p,q]                                                  (flags = 0)
 *              = Phi[p,q] * (1 - |w_a[p] - w_b[q]| / max(w_a[p], w_b[q]))  (flags & PPALS_FMS_WEIGHTS;
 *                                                                          0 where the max is not positive finite)
 *   fms        = (1/m) * max over injective matchings of m pairs of sum score[p, pi(p)]
 * the exact optimum of the rectangular assignment problem, not a greedy matching. With ranks that differ
 * it says how well the smaller model's components persist in the larger one.
 * The calls on sessions are ordered after the work queued on the engine stream and return when the result
 * is on the host. They read the sessions and change nothing of them — factors, Grams, gradients, cached
 * contractions and the tensor's generation stay, and later sweeps give bit for bit the factors they give
 * without the call; the work buffers are the call's own, grow-only, kept by the first session. The tensor
 * is never read, so the two sessions may sit on different tensors of one context. The same state gives
 * the same bits on every call (no floating-point atomics; partial sums are added in a fixed order). Every
 * storage type, both schedules, non-negative sessions. Two kernel launches a call, whatever N, the number of
 * starts and the extents; one download of at most 128 x 128 doubles; the matching runs on the host.
 * Refused before anything is launched, the message starting with the function's name — PPALS_ERR_ARG: a
 * NULL session or output, sessions of different contexts or order, different extents in a compared mode,
 * skip_mode outside [-1, N), unknown flag bits, fms_between with different numbers of starts;
 * PPALS_ERR_UNSUPPORTED: a context of more than one rank, a session of more than 128 columns. */
#define PPALS_FMS_WEIGHTS 1
/* Host only, no context and no device: the assignment above on score[p + ld*q], p < ra, q < rb.
 * perm (ra ints, may be NULL): the matched q, or -1 for a p left out when ra > rb; *sum (may be NULL): the
 * optimal total. O(n^3), deterministic. PPALS_ERR_ARG: score NULL, ra or rb < 1, ld < ra, an entry that is
 * not finite. */
int ppals_match_columns(const double *score, int ra, int rb, int ld, int *perm, double *sum);
/* Phi is Ra x Rb; *n receives Ra*Rb (n may be NULL when Phi is not); Phi == NULL: a size query, nothing
 * is launched */
int ppals_cp_congruence(ppals_cp *a, ppals_cp *b, int skip_mode, double *Phi, int64_t *n);
/* *fms of a against b; perm (Ra ints, may be NULL): the matched column of b, -1 for an unmatched one */
int ppals_cp_fms(ppals_cp *a, ppals_cp *b, int skip_mode, int flags, double *fms, int *perm);
/* all columns of all starts of s against those of other (NULL: s with itself): Ca x Cb */
int ppals_cp_multi_congruence(ppals_cp_multi *s, ppals_cp_multi *other, int skip_mode, double *Phi, int64_t *n);
/* every pair of starts, each start with its own rank: fms[a + K*b], K = nstarts */
int ppals_cp_multi_fms(ppals_cp_multi *s, int skip_mode, int flags, double *fms);
/* fms[k]: start k of a against start k of b (the same number of starts; the ranks may differ) — the
 * split-half call for two rank-sweep sessions on the halves */
int ppals_cp_multi_fms_between(ppals_cp_multi *a, ppals_cp_multi *b, int skip_mode, int flags, double *fms);

/* ---- per-slice residuals and leverages: the influence plot (no counterpart in the reference) ----
 * The third routine validation step of a PARAFAC model (R. Bro, "PARAFAC. Tutorial and applications",
 * Chemom. Intell. Lab. Syst. 38, 1997, section 7; the N-way toolbox draws it from its `nmodel` residuals and the
 * loadings' hat matrices): for every mode i and every index x of it, the sum of squared residuals over the
 * slice x against the leverage of row x of W_i. A slice far up fits badly; one far right dominates the model.
 * ss, lev: sum_i s_i doubles, mode 0's s_0 values first (the layout of one column of Wflat).
 *   ss_i[x]  = sum over all elements whose i-th index is x of (V - [[W_0..W_{N-1}]])^2
 *              V as stored (bf16 / fp32 / fp64), model, differences and sums in fp64. It is exactly the model
 *              whose distance ppals_cp_residual returns (the same Khatri-Rao operands). *total (may be NULL)
 *              = the sum over all elements = ppals_cp_residual()^2 up to rounding; every mode's ss_i sums to it.
 *   lev_i[x] = w^T (W_i^T W_i)^-1 w, w = row x of W_i: the diagonal of the projector onto the column space of
 *              W_i (in [0,1], summing to R over x for full column rank). No lambda. The Gram is the one the
 *              session keeps, inverted as for the core consistency: a session ONE of whose N Grams meets a
 *              pivot that is not a positive finite number gets NaN in EVERY entry of lev, and PPALS_OK.
 * Both calls are ordered after the work queued on the engine stream and return when the result is on the
 * host. They read the session and change nothing of it — factors, Grams, gradients, cached contractions, the
 * multi-sweep intermediate and the tensor's generation stay, and later sweeps give bit for bit the factors
 * they give without the call. The same state gives the same bits on every call (no floating-point atomics;
 * partial sums are added in a fixed order). Every storage type, both schedules, non-negative sessions.
 * Tensor traffic: ppals_cp_slice_residuals reads the tensor exactly ONCE, whatever the order, extents, rank
 * and storage type — the pass of ppals_cp_residual, keeping the sums over the rows and the columns of its
 * M x K split (M the product of the first N/2 extents), each then folded onto its modes; nothing of the
 * tensor's size is materialised. ppals_cp_leverages never reads it.
 * Work memory: the calls' own, grow-only and kept by the session until it is destroyed — the two marginals
 * (M + K doubles), the pseudo-inverse factors and the partial sums of the pass, beside the two Khatri-Rao
 * operands ppals_cp_residual already keeps. The partial sums stay under 256 MB whatever the extents: the row tiles of the pass are walked
 * in slabs (and one tile's column chunks in slabs, should a single tile not fit) and folded between them as
 * running sums in tile and chunk order, so the cap changes no bit of the result.
 * No mask argument: after ppals_cp_impute_device the missing entries equal the model up to one storage
 * rounding, so their share of a slice sum is rounding-sized.
 * Refused before anything is launched or allocated, the message starting with the function's name —
 * PPALS_ERR_ARG: a NULL session, a NULL ss / lev; PPALS_ERR_UNSUPPORTED: a context of more than one rank
 * (both calls), ppals_cp_leverages at R > 64 (ppals_cp_slice_residuals takes every R). Multi-start and
 * rank-sweep sessions: ppals_cp_multi_take hands a start to an ordinary session. */
int ppals_cp_slice_residuals(ppals_cp *s, double *ss, double *total /* may be NULL */);
int ppals_cp_leverages(ppals_cp *s, double *lev);

/* ---- hold-out rows per start of a multi-start session (resampling over one mode: the jackknife of
 * J. Riu, R. Bro, "Jack-knife technique for outlier detection and estimation of standard errors in PARAFAC
 * models", Chemom. Intell. Lab. Syst. 65 (2003) 35-49; segmented leave-samples-out fits; no counterpart in
 * the reference) ----
 * A CP fit of the tensor with some slices of mode `mode` (the "samples") deleted is exactly the fit of the
 * full tensor with the corresponding rows of W_mode held at zero: those rows drop out of every MTTKRP of the
 * other modes and out of W_mode^T W_mode, and the rows of mode `mode` are updated independently of each
 * other. So a multi-start session whose starts each hold out their own rows runs nstarts resampled fits on
 * ONE set of tensor scans, with no reduced tensors and no second resident layouts of them.
 *   keep[b * s_mode + x] (host, nstarts x s_mode bytes): 0 = start b holds sample x out, anything else = kept.
 * With a hold-out set, start b evolves as an ordinary session of its rank does under ppals_cpd_als with
 * PPALS_OPT_SIMPLE on the tensor without the held-out slices of `mode` (a non-negative session: as a
 * non-negative one does); held-out rows of the factor and of the gradient read back as exactly 0 (they are
 * exempt from PPALS_NN_FLOOR), so gradnorms are those of the reduced fits. One small launch follows the
 * update of `mode`; a start that holds nothing out is not touched by it and keeps, bit for bit, what it
 * has in a session without a hold-out. Tensor scans and their traffic do not change.
 * ppals_cp_multi_heldout_scores: scores (s_mode x ranks[start] doubles, column-major) holds, for each held-out
 * row, the row produced by the most recent update of `mode` — the least-squares projection of that sample on
 * the model of the other modes at that moment, fitted without it (from the HALS row update in a non-negative
 * session: >= PPALS_NN_FLOOR). Before any update it holds the rows the caller set: ppals_cp_multi_set_factors
 * and ppals_cp_multi_set_holdout MOVE the held-out rows, as they are at that moment, from the factor into the
 * scores. Rows of kept samples are 0.
 * ppals_cp_multi_take_predicted is ppals_cp_multi_take with the sample-mode factor additionally carrying the
 * scores in the held-out rows: bit for bit W + scores, the rows being disjoint. ppals_cp_slice_residuals on
 * `dst` then gives, per sample, the fit of the kept samples and the prediction error of the held-out ones.
 * ppals_cp_multi_take itself is unchanged (zero rows). ppals_cp_multi_residuals keeps its definition: the
 * model has zero rows there, so a held-out slice x counts with the whole ||V_x||^2. Core consistency,
 * congruence and the factor match score work unchanged: zero rows contribute nothing to the pseudo-inverse,
 * so cc is that of the reduced tensor; across starts compare with skip_mode = mode. ppals_cp_multi_run stops
 * on the LARGEST gradient norm over the starts, as for differing ranks: every start is a fit the caller wants.
 * ppals_cp_multi_set_holdout with keep == NULL clears the hold-out (mode is ignored): the zero rows stay where
 * they are until the next update of that mode. Setting it again replaces it; rows that an earlier hold-out
 * left at zero are moved as the zeros they are. Cached contractions are dropped as by set_factors.
 * ppals_cp_multi_get_holdout: *mode = the sample mode or -1; keep (may be NULL) receives the table when set.
 * Hold-out in one mode only; multi-start sessions only (a one-start session is fine).
 * Refused before anything is launched or allocated, the message starting with the function's name —
 * PPALS_ERR_ARG: a NULL session, mode outside [0, N), a start with no kept row, start out of range, a NULL
 * output, scores or take_predicted on a session without a hold-out, a dst that ppals_cp_multi_take refuses
 * (NULL, another context, another tensor, another rank); PPALS_ERR_UNSUPPORTED: what ppals_cp_multi_take
 * refuses so (a non-negative dst from an unconstrained session). */
int ppals_cp_multi_set_holdout(ppals_cp_multi *s, int mode, const uint8_t *keep /* NULL: clear */);
int ppals_cp_multi_get_holdout(const ppals_cp_multi *s, int *mode, uint8_t *keep /* may be NULL */);
int ppals_cp_multi_heldout_scores(ppals_cp_multi *s, int start, double *scores);
int ppals_cp_multi_take_predicted(ppals_cp_multi *s, int start, ppals_cp *dst);

/* ---- Tucker sessions (als_Tucker.h) ---- */
int ppals_tucker_create(ppals_ctx *ctx, ppals_tensor *V, const int *ranks, ppals_tucker **out);
void ppals_tucker_destroy(ppals_tucker *s);
int ppals_tucker_set_factors(ppals_tucker *s, const double *Wflat);
/* the `core` argument of alsTucker_DT / alsTucker_PP (als_Tucker.h:46,89; it seeds core_prev):
 * prod(ranks) doubles, first index fastest; NULL: core = V x_i W_i^T of the current factors.
 * A new session's core is zero (pp_bench.cxx:327 hands over a fresh tensor). */
int ppals_tucker_set_core(ppals_tucker *s, const double *core);
int ppals_tucker_get_factors(ppals_tucker *s, double *Wflat, double *core);
/* hosvd (als_Tucker.h:14-15, als_Tucker.cxx:66): overwrites the factors and the core */
int ppals_tucker_hosvd(ppals_tucker *s);
/* TTMc skipping mode `skip` (-1: none) (als_Tucker.cxx:76-110) */
int ppals_tucker_ttmc(ppals_tucker *s, int skip, double *Y, int64_t *n);
int ppals_tucker_sweeps_dt(ppals_tucker *s, int n);
/* alsTucker_DT (als_Tucker.h:46-48, als_Tucker.cxx:240-424) */
int ppals_tucker_dt(ppals_tucker *s, const ppals_cp_opts *o, int *iters);
/* alsTucker_PP (als_Tucker.h:89-91, als_Tucker.cxx:906-962); o->tol_init = -pp_res_tol */
int ppals_tucker_pp(ppals_tucker *s, const ppals_cp_opts *o, int *iters);

/* ---- Tucker: residual, per-slice residuals and leverages (the influence plot of a Tucker3 model; no
 * counterpart in the reference) ----
 * The CP section "per-slice residuals and leverages" for a Tucker session: which samples fit badly, which
 * samples or variables carry the model. The model is core x_0 W_0 ... x_{N-1} W_{N-1} of exactly the factors
 * and core ppals_tucker_get_factors would return now (deferred eigen-steps settled, pending rotations
 * applied), whatever they are: orthonormal factors as every sweep leaves them, or any factors and core given
 * by ppals_tucker_set_factors / ppals_tucker_set_core.
 * ss, lev: sum_i s_i doubles, mode 0's s_0 values first, like their CP twins.
 *   *out     = ||V - model||_F, the figure the drivers print.
 *   ss_i[x]  = sum over all elements whose i-th index is x of (V - model)^2; V as stored (fp32 / fp64), model,
 *              differences and sums in fp64 (the products on the fp64 matrix cores). *total (may be NULL) = the
 *              sum over all elements = ppals_tucker_residual()^2 up to rounding; every mode's ss_i sums to it.
 *   lev_i[x] = the x-th diagonal entry of the projector onto the column space of W_i: sum_k W_i[x,k]^2 for the
 *              orthonormal factors every sweep leaves, and for any other factor the same sum over an
 *              orthonormal basis of its columns (a QR factorisation of a scratch copy). In [0,1], summing to
 *              r_i. Every rank a session can hold. A session ONE of whose factors is numerically rank
 *              deficient gets NaN in EVERY entry of lev, and PPALS_OK.
 * All three are ordered after the work queued on the engine stream and return when the result is on the host.
 * They change nothing of the session (beyond what ppals_tucker_get_factors changes: the settle) and nothing of
 * the tensor or its generation: a session that calls them between sweeps continues, bit for bit, like a twin
 * that called ppals_tucker_get_factors at the same points. The same state gives the same bits on every call
 * (no floating-point atomics; partial sums are added in an order fixed by the geometry).
 * Tensor traffic: ppals_tucker_slice_residuals reads the resident tensor exactly ONCE, whatever the order,
 * extents and ranks, and stores nothing but sums: the pass of ppals_tucker_impute_device's observed residual,
 * Z = core x_{i != 0} W_i built slab by slab within two 256 MB buffers and V - W_0 Z^T formed tile by tile,
 * keeping the sums over the rows and the columns of every tile; the column sums are folded onto modes
 * 1..N-1. Nothing of the tensor's size is allocated. ppals_tucker_leverages never reads the tensor.
 * Work memory: the session's own, grow-only — the transposed factors and chain buffers the model export
 * keeps, one slab's marginal and its fold, and the partial sums of the pass, which stay under 256 MB (a
 * slab's row tiles are walked in several launches where they would not, and folded in tile order, so the cap
 * changes no bit of the result).
 * No mask argument, for the reason the CP section gives (after ppals_tucker_impute_device the missing
 * entries equal the model up to one storage rounding).
 * Refused before anything is launched or allocated, the message starting with the function's name —
 * PPALS_ERR_ARG: a NULL session, a NULL out / ss / lev; PPALS_ERR_UNSUPPORTED: a context of more than one
 * rank (ppals_tucker_slice_residuals and ppals_tucker_leverages; ppals_tucker_residual runs sharded). */
int ppals_tucker_residual(ppals_tucker *s, double *out);
int ppals_tucker_slice_residuals(ppals_tucker *s, double *ss, double *total /* may be NULL */);
int ppals_tucker_leverages(ppals_tucker *s, double *lev);

/* ---- a fitted model and its residual into DEVICE memory (TensorLy's cp_to_tensor / tucker_to_tensor)
 * The view is exactly that of ppals_tensor_export_device: a box of the GLOBAL tensor, strides >= 0 in
 * elements (NULL: dense over the box, first index fastest), destination type F32 or F64; every check
 * of that call (ppals_tensor_check_device_view, direction export, the same messages) and a bad `what`
 * are refused with PPALS_ERR_ARG before anything is launched. Each rank writes the part of the box in
 * its own leading-mode rows and leaves every other element alone. The stores are ordered after the
 * work queued on `stream` so far, and work queued there later runs after them; the host does not
 * block. Every element is the fp64 model (products and sums on the fp64 matrix cores) rounded once to
 * the destination type; PPALS_RESIDUAL subtracts it, in fp64, from V as stored (the bf16 / fp32 / fp64
 * values the session works on) before that one rounding.
 *   CP: the model [[W_0, ..., W_{N-1}]] of the current factors: the one whose distance from V
 *       ppals_cp_residual returns (the exported residual's Frobenius norm equals it up to rounding).
 *   Tucker: core x_0 W_0 ... x_{N-1} W_{N-1} of exactly the factors and core ppals_tucker_get_factors
 *       would return now: deferred eigen-checks are settled and pending rotations applied first, by the
 *       same path get_factors takes (and with the same effect on the session as that call).
 * Nothing else of the session changes: no cache is dropped and no sweep is added, so later sweeps give
 * bit for bit the factors they give without the export (for Tucker: with a get_factors call in its place).
 * The session keeps the export's operand buffers (CP: the two Khatri-Rao products of the box; Tucker:
 * the transposed factors and up to 2 x 256 MB of chain buffers) for its next export. */
#define PPALS_MODEL 0    /* the model: CP [[W_0..W_{N-1}]], Tucker core x_0 W_0 ... x_{N-1} W_{N-1} */
#define PPALS_RESIDUAL 1 /* V - model, V as stored                                                */
int ppals_cp_export_model_device(ppals_cp *s, int what, void *dst, int dst_dtype, const int64_t *box_lo,
                                 const int64_t *box_len, const int64_t *strides, void *stream);
int ppals_tucker_export_model_device(ppals_tucker *s, int what, void *dst, int dst_dtype,
                                     const int64_t *box_lo, const int64_t *box_len,
                                     const int64_t *strides, void *stream);

/* ---- CP with missing entries (TensorLy's parafac(mask=...)): imputation and an EM driver ----
 * The mask is a view exactly as in ppals_tensor_import_device, of one byte per element (PPALS_U8: a
 * torch.bool or torch.uint8 tensor): a box of the GLOBAL tensor, strides >= 0 in elements (= bytes; 0
 * broadcasts one mask slice over a mode, i.e. whole fibres missing), NULL strides = dense over the box,
 * first index fastest. A byte of 0 says the element is MISSING, anything else that it is observed. */
#define PPALS_U8 4 /* element type of a mask view only: one byte per element, 0 = missing, anything else = observed */
/* Overwrite the MISSING entries of the session's tensor with the session's current CP model: for every
 * element of the box in this rank's leading-mode rows a non-zero mask byte leaves the element bit for
 * bit as it is, a zero byte replaces it with the fp64 model [[W_0..W_{N-1}]] of the current factors
 * (products and sums on the fp64 matrix cores) rounded once to the storage type, as
 * ppals_tensor_import_device rounds an fp64 source. Elements outside the box and other ranks' rows are
 * untouched; V is not even read unless the residual is wanted.
 *   observed_sq == NULL: the host does not block; ordered on `stream` as the model export is.
 *   observed_sq != NULL: *observed_sq = sum of (V - model)^2 over the OBSERVED elements of the box, V as
 *     stored, differences and sum in fp64, summed over all ranks (one scalar all-reduce) in a fixed
 *     order (the same state gives the same bits); the call returns when the sum is on the host.
 * The call bumps the tensor's generation like an import: every session on the tensor, this one included,
 * rebuilds its second layout and drops tree nodes, the multi-sweep intermediate and PP operators at its
 * next read. The session's factors, Grams and gradients do not change. Every check
 * ppals_tensor_check_device_view makes of an import source is made of the mask, as a view of PPALS_U8,
 * before anything is launched: PPALS_ERR_ARG and a message that starts with "ppals_cp_impute_device: ".
 * (PPALS_U8 is a mask's type only: the tensor import and ppals_tensor_check_device_view refuse it.) */
int ppals_cp_impute_device(ppals_cp *s, const void *mask, const int64_t *box_lo, const int64_t *box_len,
                           const int64_t *strides, void *stream, double *observed_sq /* may be NULL */);
/* EM for CP with missing entries: repeat { impute; inner_sweeps exact sweeps } — iteration k is an
 * imputation followed by ppals_cp_sweeps_dt(inner_sweeps, o->lambda). The observed residual
 * sqrt(observed_sq) is read at the imputation of iterations 0, resprint, 2 resprint, ... (the others
 * never block). The loop stops at the first of: a look that finds the observed residual <= o->tol;
 * o->maxiter iterations; o->timelimit seconds (checked at the looks, agreed across ranks). Uses tol,
 * timelimit, maxiter, lambda and resprint of the options and ignores the rest; inner_sweeps >= 1. On
 * the way out one last imputation with the residual runs (unless the stopping look just did), so the
 * tensor's missing entries and *observed_res belong to the returned factors. *iters = iterations run.
 * Returns 1 if it stopped on tol, 0 otherwise, <0 on error. The mask must stay unchanged meanwhile. */
int ppals_cp_em(ppals_cp *s, const void *mask, const int64_t *box_lo, const int64_t *box_len,
                const int64_t *strides, void *stream, const ppals_cp_opts *o, int inner_sweeps,
                int *iters, double *observed_res);

/* ---- CP with element weights (the N-way toolbox's parafac(..., Weights); MILES; maximum-likelihood
 * PARAFAC): min sum_e h_e (x_e - m_e)^2 by Kiers' majorization (Kiers 1997) ----
 * With weights scaled to 0 <= h <= 1 and the current model m0, the working tensor z = m0 + h (x - m0)
 * satisfies  sum h (x - m)^2 <= sum (z - m)^2 + sum h (1 - h) (x - m0)^2  for every m, with equality at
 * m = m0: any ordinary sweep on Z (constrained and shaped ones, both schedules, lambda > 0) cannot raise the
 * weighted loss. For h in {0, 1} this is the EM imputation above.
 *
 * `data` and `weights` are two views of the SAME box of the GLOBAL tensor, each given exactly as the source of
 * ppals_tensor_import_device: both of element type `dtype` (PPALS_F32 or PPALS_F64), each with its own
 * strides >= 0 in elements (0 broadcasts: a per-variable weight vector is a view with one non-zero stride),
 * NULL strides = dense over the box, first index fastest.
 *
 * ppals_cp_wls_device: one majorization step. For every element of the box in this rank's leading-mode rows,
 * m the fp64 model [[W_0..W_{N-1}]] of the current factors (products and sums on the fp64 matrix cores),
 * x and h the view values widened to fp64, the value stored is
 *     h >= 1:            z = x                  loss contribution (x - m)^2
 *     h <= 0 or NaN:     z = m                  0; x is not used and may be NaN or Inf
 *     0 < h < 1:         z = fma(h, x - m, m)   h (x - m)^2
 * rounded once to the storage type, as ppals_tensor_import_device rounds an fp64 source. Elements outside
 * the box and other ranks' rows are untouched. The model sum is formed with the rank steps in the order the
 * imputation uses (4-wide fp64 MFMA steps, k ascending): with weights in {0, 1} and `data` holding the
 * tensor's own stored values, the resident tensor after the call equals, BIT FOR BIT, the tensor after
 * ppals_cp_impute_device with the corresponding mask from the same state (the mask laid out as `data`:
 * the unit-stride mode of the first side view leads the second mode group in both calls).
 *   weighted_sq == NULL: the host does not block; ordered on `stream` as the imputation is (the views may be
 *     changed by work queued on `stream` after the call).
 *   weighted_sq != NULL: *weighted_sq = the sum of the loss contributions over the box, formed in fp64 from
 *     x and m (it never sees the storage type) in a fixed order (the same state gives the same bits), summed
 *     over the ranks by one scalar all-reduce; the call returns when it is on the host.
 * The call bumps the tensor's generation like an imputation; factors, Grams and gradients do not change.
 * Refused before anything is launched or allocated:
 *   PPALS_ERR_ARG: a NULL pointer for either view; a dtype other than F32 / F64; any check
 *     ppals_tensor_check_device_view makes of an import source, made of both views (the message starts with
 *     the function's name and says which view failed);
 *   PPALS_ERR_UNSUPPORTED: BF16 storage (a bf16 rounding of z is coarser than the h (x - m) correction it
 *     carries, so the majorization no longer holds); R > 128 (the factor tile is kept in LDS); a back end
 *     without device views ("no device views", after the arithmetic checks, as for the imputation).
 * A multi-start session's inner engine is refused the way the imputation refuses it. */
int ppals_cp_wls_device(ppals_cp *s, const void *data, const void *weights, int dtype,
                        const int64_t *box_lo, const int64_t *box_len,
                        const int64_t *data_strides, const int64_t *weight_strides,
                        void *stream, double *weighted_sq /* may be NULL */);
/* Weighted CP: iteration k is a step followed by ppals_cp_sweeps_dt(inner_sweeps, o->lambda). The looks
 * (iterations 0, resprint, 2 resprint, ...), the last step on the way out, *iters and
 * *weighted_res = sqrt(loss) are those of ppals_cp_em. Stop rules at a look: weighted residual <= o->tol:
 * returns 1; from the second look on, prev - cur <= rel_change * prev: returns 2 (noisy data never reaches
 * an absolute tolerance; rel_change = 0 turns this rule off); o->maxiter or o->timelimit (agreed across
 * ranks): returns 0. <0 on error: the refusals of ppals_cp_wls_device, and inner_sweeps < 1 or
 * rel_change < 0 (PPALS_ERR_ARG). Both views must stay unchanged for the duration. */
int ppals_cp_wls(ppals_cp *s, const void *data, const void *weights, int dtype,
                 const int64_t *box_lo, const int64_t *box_len,
                 const int64_t *data_strides, const int64_t *weight_strides, void *stream,
                 const ppals_cp_opts *o, int inner_sweeps, double rel_change,
                 int *iters, double *weighted_res);

/* ---- Robust CP: Huber's loss by majorization (Huber 1964; Kiers 1997) ----
 * For data with gross outliers (scatter lines, dead pixels, spikes) of which neither a noise estimate nor a
 * mask is known: min L_c(m) = sum_e h_e rho_c(x_e - m_e), rho_c(r) = r^2 for |r| <= c and c (2 |r| - c)
 * otherwise (Huber's function scaled so that its quadratic part is the plain sum of squares; c = +inf is the
 * weighted loss above). With the current model m0, r0 = x - m0 and omega = min(1, c / |r0|),
 * rho_c(r) <= omega r^2 + (rho_c(r0) - omega r0^2) for every r, with equality at r0; Kiers' step with the
 * weight h omega <= 1 gives the working tensor z = m0 + h clip(x - m0, -c, c) and
 * L_c(m) <= sum (z - m)^2 + const(m0), equality at m0: any ordinary sweep on Z cannot raise L_c.
 *
 * ppals_cp_huber_device: one such step. Views, checks, box semantics, stream ordering, the generation bump
 * and the refusals are those of ppals_cp_wls_device; `weights` may be NULL (h = 1 everywhere; weight_strides is
 * then ignored), which is how robust fits are usually run and reads one view less. Per element, m the fp64
 * model formed as the weighted step forms it, x and h widened to fp64:
 *     !(h > 0) (h <= 0 or NaN):              z = m                  loss 0; x is not looked at
 *     d = x - m, a = |d|, !(a > c), h >= 1:  z = x                  d^2
 *     same, 0 < h < 1:                       z = fma(h, d, m)       h d^2
 *     a > c, dc = copysign(c, d), h >= 1:    z = m + dc             c (2 a - c)        counts as clipped
 *     same, 0 < h < 1:                       z = fma(h, dc, m)      h c (2 a - c)      counts as clipped
 * rounded once to the storage type. A NaN x lands in the !(a > c) rows and propagates as in the weighted step;
 * an infinite x under h > 0 and finite c is stored as m +- c and makes the loss infinite.
 *   huber_loss == NULL and clipped == NULL: the host does not block. Otherwise *huber_loss = L_c and
 *   *clipped = the number of clipped elements over the box, each formed in a fixed order (the same state gives
 *   the same bits) and summed over the ranks; the call returns when they are on the host.
 * With weights and c = +inf the resident tensor and the returned loss equal, BIT FOR BIT, those of
 * ppals_cp_wls_device from the same state; with weights == NULL and c = +inf the tensor equals an import of
 * `data`. PPALS_ERR_ARG in addition for !(c > 0) (zero, negative, NaN). */
int ppals_cp_huber_device(ppals_cp *s, const void *data, const void *weights /* NULL: h = 1 everywhere */,
                          int dtype, const int64_t *box_lo, const int64_t *box_len,
                          const int64_t *data_strides, const int64_t *weight_strides /* ignored if weights NULL */,
                          double c, void *stream, double *huber_loss /* may be NULL */,
                          int64_t *clipped /* may be NULL */);
/* Robust CP at a FIXED c: ppals_cp_wls with the Huber step in the weighted step's place; looks, stop rules,
 * return codes, the last step on the way out and *iters are those of ppals_cp_wls, *robust_res = sqrt(L_c).
 * The argument errors are those of ppals_cp_wls, and !(c > 0). (c is not re-estimated inside: that would break
 * the monotone descent. Stage it outside: some plain sweeps, c from the residual quantile below, a run; c
 * again from the robust fit's residuals, a second run.) */
int ppals_cp_robust(ppals_cp *s, const void *data, const void *weights, int dtype, const int64_t *box_lo,
                    const int64_t *box_len, const int64_t *data_strides, const int64_t *weight_strides,
                    void *stream, double c, const ppals_cp_opts *o, int inner_sweeps, double rel_change,
                    int *iters, double *robust_res /* sqrt(L_c) */);
/* A quantile of the absolute residuals |x - m| of the current factors over the box, without materialising the
 * residual: what the threshold c is chosen from (1.345 x 1.4826 x the median is the usual choice). Reads the
 * session's factors and the views only: no resident tensor is read and nothing is written, so every storage
 * type is accepted (BF16 too) and session and tensor are left bit for bit.
 * Over the elements of the box with h > 0 (all of them if weights == NULL), a_e = (float)|x_e - m_e|: the fp64
 * difference rounded to nearest fp32, every NaN one canonical NaN that sorts after +inf. *count = n, the number
 * of such elements; k = min(n - 1, max(0, ceil(p n) - 1)) in fp64; *value = the k-th smallest a_e (0-based)
 * widened to double; n = 0: *value = NaN, PPALS_OK. Exact (a radix select on integer counts): the result
 * does not depend on the launch geometry. The call waits for the result.
 * PPALS_ERR_ARG: p outside [0, 1] or NaN, NULL value, and the view checks of ppals_cp_huber_device;
 * PPALS_ERR_UNSUPPORTED: R > 128, a context of more than one rank, a back end without device views. */
int ppals_cp_abs_residual_quantile(ppals_cp *s, const void *data, const void *weights /* may be NULL */, int dtype,
                                   const int64_t *box_lo, const int64_t *box_len, const int64_t *data_strides,
                                   const int64_t *weight_strides, void *stream, double p,
                                   double *value, int64_t *count);

/* ---- PARAFAC2 (Harshman 1972; Kiers, ten Berge & Bro 1999): direct fitting ----
 * A CP model whose profiles in mode 0 may differ from slice to slice as long as their cross product stays the
 * same: chromatography with retention-time shifts, batch processes, EEG with varying latencies. The data is a
 * device view X of extents I x J x K, mode 0 the shifting mode, mode 2 the slices, X_k = X[:, :, k]:
 *     X_k ~ P_k B D_k A^T,   P_k (I x R) with orthonormal columns, B (R x R), A (J x R), D_k = diag(C[k, :]).
 * With the compressed tensor Y (R x J x K), Y_k = P_k^T X_k, [[B, A, C]] is a rank-R CP model of Y and
 *     ||X - model||^2 = (||X||^2 - ||Y||^2) + ||Y - [[B, A, C]]||^2 = lost_sq + (the inner session's residual)^2.
 * The object owns Y (stored as `storage_dtype`, PPALS_F32 or PPALS_F64), an ordinary ppals_cp session of rank R
 * on it (mode 0 = B, mode 1 = A, mode 2 = C), the projections P and the step's scratch (2 I R K doubles).
 *
 * ppals_parafac2_create: refused before anything is allocated — PPALS_ERR_ARG for R < 2, R > 64 (the Jacobi of
 * the slice polar factors keeps its R x R system in LDS), R > min(I, J), extents < 1, a bad dtype;
 * PPALS_ERR_UNSUPPORTED for PPALS_BF16 storage, a context of more than one rank (Y's leading mode is R and cannot
 * be sharded usefully) and a back end without device views. Initial state: B = I_R, C = 1,
 * A = ppals_fill_uniform_host(J R values, seed 1, offset 0) in [0, 1), every P_k the first R identity columns,
 * Y zero.
 * ppals_parafac2_cp: the inner session, BORROWED: use it for ppals_cp_set_factors / get_factors (the blocks
 * B, A, C in this order), set_mode_constraints, set_mode_shapes, set_schedule, sweeps, residual, leverages,
 * core consistency and ppals_cp_fms. NEVER pass it to ppals_cp_destroy: ppals_parafac2_destroy destroys it, the
 * tensor and the buffers. Mode 0 (B) must stay PPALS_MODE_FREE: the step and the driver refuse with
 * PPALS_ERR_ARG otherwise. */
int ppals_parafac2_create(ppals_ctx *ctx, int64_t I, int64_t J, int64_t K, int R, int storage_dtype,
                          ppals_parafac2 **out);
void ppals_parafac2_destroy(ppals_parafac2 *p);
ppals_cp *ppals_parafac2_cp(ppals_parafac2 *p);
/* The compressed tensor Y (R x J x K, r fastest), BORROWED like the session: for ppals_tensor_download,
 * ppals_tensor_export_device and ppals_tensor_norm. Never destroy it, and do not write to it: the step owns its
 * contents. */
ppals_tensor *ppals_parafac2_tensor(ppals_parafac2 *p);
/* One projection step from the inner session's current B, A, C. For every slice k:
 *   Q_k = X_k A D_k B^T                         first pass over X, elements widened to fp64
 *   P_k = Q_k (Q_k^T Q_k)^(-1/2)                the Gram route in fp64 under the rule of the orthonormal mode
 *       update: a converged Jacobi, every eigenvalue theta positive and finite and
 *       theta_min > theta_max * PPALS_ORTHO_MIN_RATIO; a slice that fails it KEEPS ITS PREVIOUS P_k and counts
 *       in *failed (an all-zero slice is such a slice: ordinary input, not an error)
 *   Y_k = P_k^T X_k                             second pass over X, rounded once to the storage type and written
 *       into the resident tensor; the tensor's generation is bumped, the session's factors do not change.
 * `data`: device memory of the context's device, `dtype` PPALS_F32 or PPALS_F64, `strides` in elements for the
 * modes (0, 1, 2), NULL = dense with the first index fastest. The pointer (not NULL, aligned to its element
 * size, device memory) and the range (the view's span inside its allocation) are checked as
 * ppals_tensor_check_device_view checks an import source: PPALS_ERR_ARG. strides[0] != 1 or slices that
 * overlap (a zero stride, aliased elements): PPALS_ERR_UNSUPPORTED — permute so that the shifting mode comes
 * first and make the tensor contiguous. Padded slices (strides[1] > I, strides[2] > strides[1] J) are fine.
 * Every refusal comes before any launch and leaves tensor, session and projections unchanged.
 * The reads of X wait for the work `stream` holds so far, and work queued on `stream` later waits for them.
 *   lost_sq == NULL and failed == NULL: the host does not block. Otherwise *lost_sq = sum x^2 - sum y^2, both
 *   sums in fp64 before the rounding of Y and in a fixed order (the same state gives the same bits), *failed =
 *   the number of slices that kept their P_k, and the call returns when they are on the host.
 * The number of launches does not depend on I, J, K, R. */
int ppals_parafac2_step_device(ppals_parafac2 *p, const void *data, int dtype, const int64_t *strides /* or NULL */,
                               void *stream, double *lost_sq /* may be NULL */, int *failed /* may be NULL */);
/* Direct fitting: iteration k is a step followed by inner_sweeps exact sweeps of the inner session at o->lambda,
 * with the looks, stop rules, return codes (1: tol, 2: rel_change), the last step on the way out and *iters of
 * ppals_cp_wls. The quantity looked at is lost_sq + residual^2, the residual the inner session's taken after the
 * step (one pass over the small Y); *res is its square root, ||X - model||. A sweep lowers the second term and
 * leaves the first, a step minimises the total over the P_k: the loss never rises. Argument errors: those of
 * ppals_cp_wls (NULL o, inner_sweeps < 1, rel_change < 0 or NaN, o->maxiter < 0) and of the step. */
int ppals_parafac2_run(ppals_parafac2 *p, const void *data, int dtype, const int64_t *strides, void *stream,
                       const ppals_cp_opts *o, int inner_sweeps, double rel_change, int *iters, double *res);
/* The projections: P_host receives I R K doubles, P_k column-major at I R k (a ragged object, below: R N doubles,
 * P_k with leading dimension rows[k] at R o_k — for equal rows the same layout); the device pointer (same layout)
 * stays the object's and is valid until ppals_parafac2_destroy; it is written by work on the engine stream. */
int ppals_parafac2_projections(ppals_parafac2 *p, double *P_host);
int ppals_parafac2_projections_device(ppals_parafac2 *p, const double **P);

/* ---- PARAFAC2 on slices of unequal length (batch processes of different duration, runs cut at different points) ----
 * Slice k is rows[k] x J; N = sum_k rows[k], o_k = sum_{l<k} rows[l]. The model, the compressed tensor Y (R x J x K),
 * the inner session, the loss identity and the driver are those above; only P_k (rows[k] x R) differs in size.
 * The object owns Y, the session, P and the step's scratch of R N doubles each (P_k column-major with leading
 * dimension rows[k] at R o_k), T, the outputs and the small device tables of the step (rows, row offsets, the
 * map from row tiles to slices, the view of the last step). A step on zero-padded slices of equal length gives
 * the same fit but reads the padding twice and holds max_k rows[k] K rows.
 *
 * ppals_parafac2_create_ragged: refused before anything is allocated — PPALS_ERR_ARG for NULL rows, K < 1 or
 * J < 1, R outside [2, 64], R > J, a rows[k] < R (the message names the first such k), a bad dtype;
 * PPALS_ERR_UNSUPPORTED as ppals_parafac2_create. The initial state is that of ppals_parafac2_create: every P_k the
 * first R identity columns. ppals_parafac2_cp, _tensor, _destroy and _projections_device serve both kinds of
 * object; ppals_parafac2_step_device and ppals_parafac2_run refuse a ragged object, and the two entry points below
 * an equal-length one, with PPALS_ERR_ARG. */
int ppals_parafac2_create_ragged(ppals_ctx *ctx, int64_t K, const int64_t *rows /* K */, int64_t J, int R,
                                 int storage_dtype, ppals_parafac2 **out);
/* The slice lengths, for both kinds of object (an equal-length object answers I for every slice), and their sum. */
int ppals_parafac2_rows(ppals_parafac2 *p, int64_t *rows /* K */, int64_t *total /* may be NULL */);
/* The step of ppals_parafac2_step_device on a ragged object. X_k[i, j] = data[offsets[k] + i + col_strides[k] j],
 * in elements, unit stride in i. offsets == NULL: the slices packed one after another, offsets[k] = J o_k;
 * col_strides == NULL: col_strides[k] = rows[k]. The stacked N x J column-major matrix is offsets[k] = o_k,
 * col_strides[k] = N. Padded slices and gaps are fine; the step only reads, so spans that overlap are not refused.
 * PPALS_ERR_ARG, before any launch, copy or allocation: an equal-length object, NULL data, a dtype other than
 * PPALS_F32 / PPALS_F64, a pointer not aligned to its element size or not device memory, an offsets[k] < 0, a
 * col_strides[k] < rows[k], a union of the slices' spans that does not lie inside the pointer's allocation, mode 0
 * of the inner session not PPALS_MODE_FREE. Semantics, *lost_sq, *failed, the ordering against `stream` and "the
 * host does not block when both outputs are NULL" are those of ppals_parafac2_step_device, with one exception: the
 * offsets and strides travel to the device when they differ from the last step's, and that copy waits for the
 * engine stream. The sums run in the orders of the equal-length step: equal rows on the dense layout give its
 * bits. The number of launches does not depend on K, the rows, J or R. */
int ppals_parafac2_step_ragged_device(ppals_parafac2 *p, const void *data, int dtype,
                                      const int64_t *offsets /* K, or NULL */,
                                      const int64_t *col_strides /* K, or NULL */, void *stream,
                                      double *lost_sq /* may be NULL */, int *failed /* may be NULL */);
/* The driver of ppals_parafac2_run on the ragged step: the same looks, stop rules, return codes and errors. */
int ppals_parafac2_run_ragged(ppals_parafac2 *p, const void *data, int dtype, const int64_t *offsets,
                              const int64_t *col_strides, void *stream, const ppals_cp_opts *o, int inner_sweeps,
                              double rel_change, int *iters, double *res);

/* ---- N-PLS regression (multilinear PLS: Bro, J. Chemometrics 10 (1996) 47-61; `npls` of the N-way toolbox) ----
 * X is a resident tensor of any order N >= 2, `mode` its sample mode with I = lens[mode] samples; Y is I x M on
 * the host, column-major. The caller has centred both (ppals_tensor_center for X). Component f has one unit weight
 * vector for every mode off the sample mode, W_f their outer product (laid out like a sample's slice), scores
 * t_f = (X - sum_{g<f} t_g o W_g) . W_f, response weights q_f (unit) and u_f = Y_res q_f; the inner relation
 * B[0..f, f] = (T^T T)^-1 T^T u_f is upper triangular (the scores of N-PLS are not orthogonal), and
 * Y_res = Y - T B Q^T. W_f is the best rank-one approximation, by alternating power iterations from the fibres
 * through the entry of largest magnitude, of Z = sum_m q_m Z_m, Z_m the deflated tensor contracted with column m of
 * Y_res; q is iterated from the column of Y_res with the largest sum of squares. Signs: the entry of largest
 * magnitude of every weight vector but the last is positive, the last makes <Z, W> positive.
 *
 * The tensor is NEVER WRITTEN and nothing of its size is allocated: the deflated tensor is not formed. A component
 * reads X twice (a contraction with the M columns of Y_res, a slice inner product with W_f); the working set is
 * M + 2 arrays of a slice's size in fp64. Elements are widened to fp64 as stored, sums are fp64 in a fixed
 * order: the same state gives the same bits. The calls read the primary resident layout, are ordered after the
 * work queued on the engine stream, bump no generation and disturb no session. They return with the results on
 * the host.
 *
 * Refusals come before anything is launched or allocated and the message starts with the function's name:
 * PPALS_ERR_ARG for NULL or dead handles, `mode` outside [0, N), M < 1, F < 1 or F > I, a non-finite Y, bad options
 * (a negative or NaN tolerance, a cap below 1), ncomp outside [1, components fitted], Xnew of another order or with
 * other extents off the sample mode; PPALS_ERR_UNSUPPORTED for a context of more than one rank.
 *
 * A zero or non-finite Z ends the fit with the components so far (possibly none): not an error, ppals_npls_dims
 * tells. status[f]: bit 0 the power iterations ran into hopm_max, bit 1 the loop over q into inner_max. */
typedef struct ppals_npls ppals_npls; /* a fitted N-PLS model: host arrays only, no reference to X or the context */
typedef struct {
  double hopm_tol; /* the power iterations stop when no weight entry moved by more than this (1e-12) */
  int hopm_max;    /* ... or after this many rounds (500) */
  double inner_tol; /* the loop over q (M > 1) stops when no entry of q moved by more than this (1e-12) */
  int inner_max;    /* ... or after this many rounds (200) */
} ppals_npls_opts;
enum {
  PPALS_NPLS_T = 0,      /* I x F   scores of X */
  PPALS_NPLS_U = 1,      /* I x F   scores of Y */
  PPALS_NPLS_Q = 2,      /* M x F   response weights, unit columns */
  PPALS_NPLS_B = 3,      /* F x F   inner relation, upper triangular */
  PPALS_NPLS_SSX = 4,    /* F       1 - ||X - sum_{g<=f} t_g o W_g||^2 / ||X||^2, from ||X||^2 - 2 sum t_g.s_g +
                                    sum (t_g.t_h) <W_g, W_h> at no pass: a difference, it loses digits when the
                                    residual is tiny */
  PPALS_NPLS_SSY = 5,    /* F       1 - ||Y_res||^2 / ||Y||^2 */
  PPALS_NPLS_STATUS = 6, /* F       the status bits, as doubles */
  PPALS_NPLS_W = 16      /* + k: lens x F, the weights of the k-th mode off the sample mode, k in [0, N - 1) */
};
/* opts == NULL: the defaults above. F counts the components wanted; all arrays below have the fitted number. */
int ppals_npls_fit(ppals_tensor *X, int mode, const double *Y, int M, int F, const ppals_npls_opts *opts,
                   ppals_npls **out);
void ppals_npls_destroy(ppals_npls *m);
/* any pointer may be NULL; lens: `order` extents, those of the training tensor */
int ppals_npls_dims(const ppals_npls *m, int *order, int *mode, int64_t *lens, int *M, int *wanted, int *fitted);
/* `what` as above, column-major; *n receives the number of doubles, out == NULL only asks for it */
int ppals_npls_get(const ppals_npls *m, int what, double *out, int64_t *n);
/* Yhat (Inew x M) from the first ncomp components, for a tensor of the model's order and extents off the sample
 * mode and any Inew: ONE pass over Xnew gives all raw scores, the rest is on the host. Tnew: Inew x ncomp. */
int ppals_npls_predict(const ppals_npls *m, ppals_tensor *Xnew, int ncomp, double *Yhat, double *Tnew /* may be NULL */);
/* The two tensor passes on their own, host pointers, the tensor viewed as [L, I, T] around `mode` (first index
 * fastest): Z[l,t,c] = sum_i X[l,i,t] U[i,c] (U: I x C, Z: L T C doubles) and S[i,c] = sum_{l,t} X[l,i,t] W[l,t,c]
 * (W: L T C, S: I x C). Column c has the bits of that column computed alone. Refusals as above (C < 1 too). */
int ppals_tensor_contract_mode(ppals_tensor *t, int mode, const double *U, int C, double *Z);
int ppals_tensor_slice_inner(ppals_tensor *t, int mode, const double *W, int C, double *S);
/* The same two passes for U or W of many columns: arguments, host pointers, layouts and refusals are those of the
 * two calls above, the message starts with the new name. The columns travel together, up to 64 a read of the
 * tensor, and products and sums run on the fp64 matrix cores wherever that was measured not to lose to the two
 * passes above (L == 1 with I >= 32 and more than 4 columns; L >= 16 with more than 32 columns for the contraction,
 * more than 8 for the slice inner product); otherwise the call goes through those. Results are DETERMINISTIC (two calls
 * give the same bits, every sum runs in an order fixed by the storage type, L, I, T and the number of columns, no
 * atomics) and WITHIN THE SAME ERROR BOUNDS as the narrow calls, but they are NOT BIT-EQUAL to them, and a column
 * need not have the bits of that column computed alone. */
int ppals_tensor_contract_columns(ppals_tensor *t, int mode, const double *U, int C, double *Z);
int ppals_tensor_slice_inner_columns(ppals_tensor *t, int mode, const double *W, int C, double *S);

/* ---- N-PLS cross-validation (leave-segments-out; `ncrossreg` of the N-way toolbox) ----
 * segment[i] in [0, S) names the segment of sample i. For every segment s the model is fitted on all samples
 * OUTSIDE s, with exactly the conventions of the fit above (the start of q, the rank-one rule and its start, the
 * signs, the triangular inner relation, the stops, the status bits), and predicts the samples of s:
 *   Ycv[i, :, f]   (I x M x F, column-major) the prediction of sample i from the first f + 1 components of the fit
 *                  without segment[i];
 *   press[f, m]    (F x M, column-major, may be NULL) = sum_i (Ycv[i, m, f] - Y[i, m])^2;
 *   fitted[s]      (S, may be NULL) the components the fit without s reached; a fit that ends early (zero or
 *                  non-finite Z) repeats its last prediction in its later columns of Ycv, and with no component
 *                  they hold the training mean of Y (0 if center == 0);
 *   status[s, f]   (S x F, column-major, may be NULL) the status bits of component f of the fit without s, 0 where
 *                  none was fitted;
 *   x_passes       (may be NULL) the shared passes over X: 2 F ceil(S / G) when no fit ends early (a pass of up
 *                  to 64 columns is one read of X on the wide routes; where the rule of the _columns calls sends
 *                  it through the narrow passes it reads X once per 4 columns).
 * center == 1: every fit centres X across the sample mode and Y on ITS OWN training samples, and the training mean
 * of Y is added back to the predictions; the caller passes the tensor as it is (one already centred by the centring
 * call gives the same result up to rounding). center == 0: nothing is centred.
 *
 * The tensor is NEVER WRITTEN OR COPIED, no reduced or re-centred tensor is formed, no generation moves and live
 * sessions are undisturbed: a fit leaves a segment out by zeroing its rows in the columns of Y_res that are
 * contracted with X; the columns of Y_res sum to zero over the training samples, so the contraction with the
 * centred tensor is the contraction with X; the centred scores are the raw scores less their training mean; and the
 * raw scores of the held-out samples come out of the same pass as the training scores. The fits run in groups of G
 * that share every pass, G the largest count with G M <= 64 columns and G (M + 2) fp64 slices within 2 GiB: one
 * contraction of G M columns and one slice inner product of G columns per component, through the passes of
 * the two _columns calls above; the rest is small work per fit and host arithmetic. Deterministic: the same
 * state gives the same bits.
 *
 * Refusals come before anything is launched or allocated, the message starts with "ppals_npls_crossval: ":
 * PPALS_ERR_ARG for NULL or dead handles, NULL Y, segment or Ycv, `mode` outside [0, N), M < 1, F < 1, S < 2 or
 * S > I, a label outside [0, S) or an empty segment, F larger than (the smallest training set) - center, center
 * other than 0 or 1, a non-finite Y, bad options (as the fit defines them); PPALS_ERR_UNSUPPORTED for a context of
 * more than one rank. */
int ppals_npls_crossval(ppals_tensor *X, int mode, const double *Y, int M, int F,
                        const int32_t *segment /* I entries in [0, S) */, int S, int center /* 0 or 1 */,
                        const ppals_npls_opts *opts /* or NULL */, double *Ycv /* I x M x F, column-major */,
                        double *press /* F x M, may be NULL */, int *fitted /* S, may be NULL */,
                        int *status /* S x F, may be NULL */, int64_t *x_passes /* may be NULL */);

/* ---- Tucker with missing entries (TensorLy's tucker(mask=...)): imputation and an EM driver ----
 * The contracts of ppals_cp_impute_device / ppals_cp_em with a Tucker session in the CP session's place:
 * the same PPALS_U8 mask view (a box of the GLOBAL tensor, strides >= 0, 0 broadcasts, NULL = dense, a byte
 * of 0 = MISSING), the same checks before anything is launched (PPALS_ERR_ARG, the message starts with
 * "ppals_tucker_impute_device: " / "ppals_tucker_em: "), each rank rewriting its own leading-mode rows.
 * A non-zero mask byte leaves the element bit for bit as it is; a zero byte replaces it with the fp64 model
 * core x_0 W_0 ... x_{N-1} W_{N-1} (products and sums on the fp64 matrix cores) rounded once to the
 * storage type (F32 or F64), of exactly the factors and core ppals_tucker_get_factors would return now:
 * the call first takes the path of ppals_tucker_export_model_device (deferred eigen-checks settled, pending
 * rotations applied), with the same effect on the session as that call. Unlike the CP call it may
 * therefore WAIT FOR THE DEVICE even with observed_sq == NULL; the stores themselves are ordered on
 * `stream` as the model export's are.
 *   observed_sq != NULL: *observed_sq = sum of (V - model)^2 over the OBSERVED elements of the box, V as
 *     stored, in fp64, in a fixed order (per-workgroup sums in order, the slabs of a large box in order,
 *     one scalar all-reduce over the ranks): the same state gives the same bits.
 * The call bumps the tensor's generation (once, if any of the box lies in this rank's rows): every session
 * on the tensor rebuilds its other layouts and drops tree nodes, the multi-sweep state and PP operators at
 * its next read. Factors and core do not change; elements outside the box and other ranks' rows are
 * untouched. The session keeps the operand buffers it shares with the model export. A REFUSED call (any
 * PPALS_ERR_ARG above, or PPALS_ERR_UNSUPPORTED on a back end without device views) returns before the
 * session is touched: nothing is settled, rotated or allocated. */
int ppals_tucker_impute_device(ppals_tucker *s, const void *mask, const int64_t *box_lo,
                               const int64_t *box_len, const int64_t *strides, void *stream,
                               double *observed_sq /* may be NULL */);
/* EM for Tucker with missing entries: iteration k is an imputation followed by
 * ppals_tucker_sweeps_dt(inner_sweeps). The looks (iterations 0, resprint, 2 resprint, ...), the stop rules
 * (observed residual <= o->tol at a look; o->maxiter; o->timelimit, agreed across ranks), the last
 * imputation on the way out, *iters, *observed_res and the return value are those of ppals_cp_em. Uses
 * tol, timelimit, maxiter and resprint of the options; lambda has no meaning here and is ignored, like the
 * rest. inner_sweeps >= 1 (else PPALS_ERR_ARG). The start is the factors and core the session holds at
 * the call: the usual one is ppals_tucker_hosvd on the tensor with its missing entries set to zero. */
int ppals_tucker_em(ppals_tucker *s, const void *mask, const int64_t *box_lo, const int64_t *box_len,
                    const int64_t *strides, void *stream, const ppals_cp_opts *o, int inner_sweeps,
                    int *iters, double *observed_res);

#ifdef __cplusplus
}
#endif
#endif
