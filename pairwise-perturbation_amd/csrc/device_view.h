// device_view.h — strided views of device memory for ppals_tensor_import_device / _export_device
// (include/ppals.h): the half of the argument checks that is plain arithmetic, and the copy plan the
// kernels of kernels_io.hip.h walk. Header-only and free of HIP, so that the host stand-in
// (tests/hostsim) and a CPU test driver compile it with g++; the pointer queries and the launches sit
// behind Ops::device_ptr_info / Ops::copy_view (ops.h).
//
// A view is a box of the GLOBAL tensor, box_lo[i] <= index_i < box_lo[i] + box_len[i], whose element
// (j_0, ..., j_{N-1}) (box-relative) sits at ptr + sum_i j_i * stride_i elements. The resident shard of
// a rank is dense, first index fastest, rows [row0, row0 + l0) of the leading mode.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>

#if defined(__HIPCC__)
#define DV_HD __host__ __device__
#define DV_UNROLL _Pragma("unroll")
#else
#define DV_HD
#define DV_UNROLL
#endif

namespace ppals {

constexpr int DV_MAX_ORDER = 8;  // = PPALS_MAX_ORDER
// element types of a view (the PPALS_F32 / F64 / F16 / BF16 / U8 codes); U8: the bytes of a mask view
// (ppals_cp_impute_device, dv_check_args with mask = true), never a source or destination of tensor values
enum ViewDType { DV_F32 = 0, DV_F64 = 1, DV_F16 = 2, DV_BF16 = 3, DV_U8 = 4 };
enum ViewDir { DV_IMPORT = 0, DV_EXPORT = 1 };
// (a) streaming copy-convert along a mode that is unit-stride in the view and fastest in the shard,
// (b) 64 x 64 LDS tiles between the shard's fastest modes and the view's unit-stride mode,
// (c) per-element gather (the view has no unit-stride mode: correct, not fast)
enum ViewKind { DV_EMPTY = 0, DV_STREAM = 1, DV_TILE = 2, DV_GATHER = 3 };

inline int dv_elem_size(int dt) { return dt == DV_F32 ? 4 : dt == DV_F64 ? 8 : dt == DV_U8 ? 1 : 2; }
inline bool dv_dtype_ok(int dir, int dt) {
  return dt == DV_F32 || dt == DV_F64 || (dir == DV_IMPORT && (dt == DV_F16 || dt == DV_BF16));
}

// checked int64 arithmetic: false on overflow
inline bool dv_mul(int64_t a, int64_t b, int64_t *o) { return !__builtin_mul_overflow(a, b, o); }
inline bool dv_add(int64_t a, int64_t b, int64_t *o) { return !__builtin_add_overflow(a, b, o); }

// bytes a view covers from its first element: (sum_i (len_i - 1) * stride_i + 1) * esize, 0 for an
// empty box. false: it does not fit in int64.
inline bool dv_span_bytes(int order, const int64_t *len, const int64_t *stride, int esize,
                          int64_t *out) {
  for (int i = 0; i < order; i++)
    if (len[i] == 0) {
      *out = 0;
      return true;
    }
  int64_t last = 0;
  for (int i = 0; i < order; i++) {
    int64_t t;
    if (!dv_mul(len[i] - 1, stride[i], &t) || !dv_add(last, t, &last)) return false;
  }
  return dv_add(last, 1, &last) && dv_mul(last, esize, out);
}

// [ptr, ptr + span) inside the allocation [base, base + size)
inline bool dv_in_allocation(uint64_t ptr, int64_t span, uint64_t base, uint64_t size) {
  if (span < 0 || ptr < base) return false;
  const uint64_t off = ptr - base;
  return off <= size && (uint64_t)span <= size - off;
}

// an export destination must not write one element twice: every mode of extent > 1 has a positive
// stride and, in order of increasing stride, each stride lies beyond the last element of the modes
// before it: stride[k+1] > sum_{m<=k} (len[m] - 1) * stride[m]. (That admits every layout the plainer
// stride[k+1] >= stride[k] * len[k] admits, and stepped views such as x.permute(...)[::2, 1:7].)
inline bool dv_no_self_overlap(int order, const int64_t *len, const int64_t *stride) {
  int idx[DV_MAX_ORDER], m = 0;
  for (int i = 0; i < order; i++) {
    if (len[i] == 0) return true;  // nothing is written
    if (len[i] > 1) {
      if (stride[i] <= 0) return false;
      idx[m++] = i;
    }
  }
  std::sort(idx, idx + m, [&](int a, int b) { return stride[a] < stride[b]; });
  int64_t reach = 0;  // the last offset of the modes before k + 1
  for (int k = 0; k + 1 < m; k++) {
    int64_t t;
    if (!dv_mul(len[idx[k]] - 1, stride[idx[k]], &t) || !dv_add(reach, t, &reach)) return false;
    if (stride[idx[k + 1]] <= reach) return false;
  }
  return true;
}

// a view with its defaults resolved
struct ViewArgs {
  int dir = DV_IMPORT, order = 0, dtype = DV_F32, esize = 4;
  int64_t lo[DV_MAX_ORDER], len[DV_MAX_ORDER], stride[DV_MAX_ORDER];
  int64_t span = 0;  // bytes, dv_span_bytes
};

// Every check that needs no pointer query. box_lo / box_len NULL: the whole tensor; strides NULL:
// dense over the box, first index fastest. false: *err says why (the C ABI returns PPALS_ERR_ARG).
// mask: the view is the mask of an imputation, read like an import source, its only type DV_U8.
inline bool dv_check_args(int dir, int order, const int64_t *glens, int dtype, const int64_t *box_lo,
                          const int64_t *box_len, const int64_t *strides, ViewArgs *a,
                          std::string *err, bool mask = false) {
  if (dir != DV_IMPORT && dir != DV_EXPORT) return *err = "direction must be 0 (import) or 1 (export)", false;
  if (mask) {
    if (dir != DV_IMPORT || dtype != DV_U8) return *err = "a mask view is read, as PPALS_U8", false;
  } else if (!dv_dtype_ok(dir, dtype))
    return *err = dir == DV_IMPORT ? "bad source dtype (PPALS_F32, F64, F16 or BF16)"
                                   : "bad destination dtype (PPALS_F32 or F64)",
           false;
  if (order < 1 || order > DV_MAX_ORDER) return *err = "bad tensor order", false;
  if ((box_lo == nullptr) != (box_len == nullptr))
    return *err = "box_lo and box_len must both be given or both be NULL", false;
  a->dir = dir;
  a->order = order;
  a->dtype = dtype;
  a->esize = dv_elem_size(dtype);
  for (int i = 0; i < order; i++) {
    a->lo[i] = box_lo ? box_lo[i] : 0;
    a->len[i] = box_len ? box_len[i] : glens[i];
    if (a->lo[i] < 0 || a->len[i] < 0 || a->lo[i] > glens[i] || a->len[i] > glens[i] - a->lo[i])
      return *err = "box mode " + std::to_string(i) + " [" + std::to_string(a->lo[i]) + ", +" +
                    std::to_string(a->len[i]) + ") outside the extent " + std::to_string(glens[i]),
             false;
  }
  for (int i = 0; i < order; i++) {
    if (strides) {
      a->stride[i] = strides[i];
    } else if (i == 0) {
      a->stride[i] = 1;
    } else if (!dv_mul(a->stride[i - 1], a->len[i - 1], &a->stride[i])) {
      return *err = "dense strides overflow int64", false;
    }
    if (a->stride[i] < 0) return *err = "negative stride in mode " + std::to_string(i), false;
  }
  if (!dv_span_bytes(order, a->len, a->stride, a->esize, &a->span))
    return *err = "the view's byte span overflows int64", false;
  if (dir == DV_EXPORT && !dv_no_self_overlap(order, a->len, a->stride))
    return *err = "the export destination overlaps itself (a zero stride on an extent > 1, or "
                  "aliased elements)",
           false;
  return true;
}

// The copy plan: the box cut to this rank's rows, extents of 1 dropped, neighbouring modes merged
// where both sides are contiguous across them. Plan mode 0 is the shard's fastest.
struct ViewPlan {
  int kind = DV_EMPTY;
  int nd = 0;  // plan modes
  int fk = 0;  // DV_TILE: the plan mode where the view has unit stride (>= 1)
  int64_t n[DV_MAX_ORDER] = {};
  int64_t vs[DV_MAX_ORDER] = {};  // view strides (elements)
  int64_t rs[DV_MAX_ORDER] = {};  // shard strides (elements)
  int64_t voff = 0, roff = 0;     // offsets of the first element from ptr / from the shard's start
  int64_t count = 0;              // elements this rank copies
};

inline ViewPlan dv_plan(const ViewArgs &a, const int64_t *glens, int64_t row0, int64_t l0) {
  ViewPlan p;
  const int64_t r_lo = std::max(a.lo[0], row0), r_hi = std::min(a.lo[0] + a.len[0], row0 + l0);
  if (r_hi <= r_lo) return p;
  for (int i = 1; i < a.order; i++)
    if (a.len[i] == 0) return p;
  int64_t n[DV_MAX_ORDER], rsf[DV_MAX_ORDER];
  rsf[0] = 1;
  for (int i = 1; i < a.order; i++) rsf[i] = rsf[i - 1] * (i == 1 ? l0 : glens[i - 1]);
  p.voff = (r_lo - a.lo[0]) * a.stride[0];
  p.roff = r_lo - row0;
  n[0] = r_hi - r_lo;
  for (int i = 1; i < a.order; i++) {
    p.roff += a.lo[i] * rsf[i];
    n[i] = a.len[i];
  }
  p.count = 1;
  for (int i = 0; i < a.order; i++) {
    p.count *= n[i];
    if (n[i] == 1) continue;
    const int k = p.nd - 1;
    if (k >= 0 && a.stride[i] == p.vs[k] * p.n[k] && rsf[i] == p.rs[k] * p.n[k]) {
      p.n[k] *= n[i];
    } else {
      p.n[p.nd] = n[i];
      p.vs[p.nd] = a.stride[i];
      p.rs[p.nd] = rsf[i];
      p.nd++;
    }
  }
  if (p.nd == 0) {  // one element
    p.nd = 1;
    p.n[0] = 1;
    p.vs[0] = p.rs[0] = 1;
  }
  if (p.vs[0] == 1) {
    p.kind = DV_STREAM;
    return p;
  }
  for (int k = 1; k < p.nd; k++)
    if (p.vs[k] == 1) {
      p.kind = DV_TILE;
      p.fk = k;
      return p;
    }
  p.kind = DV_GATHER;
  return p;
}

// Index decoding shared by the kernels and the CPU test: plan modes [m0, m1) of a flat index idx
// (first fastest) added to the view / shard offsets. Unrolled, so the plan's arrays are read at
// constant indices (a kernel argument indexed at run time would be copied to scratch).
DV_HD inline void dv_decode(const ViewPlan &p, int m0, int m1, int64_t idx, int64_t &v, int64_t &r) {
  DV_UNROLL
  for (int m = 0; m < DV_MAX_ORDER; m++)
    if (m >= m0 && m < m1) {
      const int64_t q = idx / p.n[m], c = idx - q * p.n[m];
      v += c * p.vs[m];
      r += c * p.rs[m];
      idx = q;
    }
}
// DV_TILE: the tile grid. Rows of a tile run over the flattened plan modes [0, fk) ("A", the shard's
// fast side), columns over plan mode fk ("B", unit-stride in the view), tiles over the other modes.
constexpr int DV_TILE_DIM = 64;
DV_HD inline void dv_tile_grid(const ViewPlan &p, int64_t *FA, int64_t *tA, int64_t *tB,
                               int64_t *tiles) {
  int64_t fa = 1, b = 1, nb = 1;
  DV_UNROLL
  for (int m = 0; m < DV_MAX_ORDER; m++) {
    if (m < p.fk) fa *= p.n[m];
    if (m == p.fk) b = p.n[m];
    if (m > p.fk && m < p.nd) nb *= p.n[m];
  }
  *FA = fa;
  *tA = (fa + DV_TILE_DIM - 1) / DV_TILE_DIM;
  *tB = (b + DV_TILE_DIM - 1) / DV_TILE_DIM;
  *tiles = *tA * *tB * nb;
}

// ---- a decomposition's model stored through a view (ppals_cp/tucker_export_model_device,
// kernels_model.hip.h). The box of a checked export view cut to this rank's rows: per mode its global
// lo / extent, view and shard strides, and the offsets of its first element from the view pointer and
// from the shard's start. false: this rank writes nothing.
struct ModelBox {
  int order = 0;
  int64_t lo[DV_MAX_ORDER] = {}, len[DV_MAX_ORDER] = {}, vs[DV_MAX_ORDER] = {}, rs[DV_MAX_ORDER] = {};
  int64_t voff = 0, roff = 0;
};
inline bool dv_model_box(const ViewArgs &a, const int64_t *glens, int64_t row0, int64_t l0,
                         ModelBox *b) {
  const int64_t r_lo = std::max(a.lo[0], row0), r_hi = std::min(a.lo[0] + a.len[0], row0 + l0);
  if (r_hi <= r_lo) return false;
  b->order = a.order;
  b->voff = (r_lo - a.lo[0]) * a.stride[0];
  b->roff = r_lo - row0;
  for (int i = 0; i < a.order; i++) {
    if (a.len[i] == 0) return false;
    b->lo[i] = i == 0 ? r_lo : a.lo[i];
    b->len[i] = i == 0 ? r_hi - r_lo : a.len[i];
    b->vs[i] = a.stride[i];
    b->rs[i] = i == 0 ? 1 : b->rs[i - 1] * (i == 1 ? l0 : glens[i - 1]);
    if (i > 0) b->roff += a.lo[i] * b->rs[i];
  }
  return true;
}
// modes of the box flattened into one index, the first listed fastest
struct ModelGroup {
  int n = 0;
  int64_t count = 1;
  int64_t len[DV_MAX_ORDER] = {}, vs[DV_MAX_ORDER] = {}, rs[DV_MAX_ORDER] = {};
  int mode[DV_MAX_ORDER] = {};
  void add(const ModelBox &b, int m) {
    mode[n] = m;
    len[n] = b.len[m];
    vs[n] = b.vs[m];
    rs[n] = b.rs[m];
    count *= b.len[m];
    n++;
  }
  // the offset of flat index i is i itself (under view strides vs, or shard strides rs)
  static bool unit(int n, const int64_t *len, const int64_t *st) {
    int64_t want = 1;
    for (int i = 0; i < n; i++) {
      if (len[i] > 1 && st[i] != want) return false;
      want *= len[i];
    }
    return true;
  }
  bool view_unit() const { return unit(n, len, vs); }
  bool shard_unit() const { return unit(n, len, rs); }
};
// dst[voff + offA(a) + offB(b)] = sum_k Q[a + ldq*k] * P[(b % pL) + pLK*(b / pL) + pL*k] (the residual:
// V[roff + rA(a) + rB(b)] minus the sum), a over group A (the view's fast side), b over group B
struct ModelPlan {
  ModelGroup ga, gb;
  int64_t voff = 0, roff = 0;
  int64_t ldq = 0, pL = 1, pLK = 0;
};
// The imputation (ppals_cp_impute_device, Ops::model_impute): the stores go to the SHARD, predicated on
// the bytes of a mask view, so the two sides change places for the kernel: its "view" is the shard
// (group A along the shard's fast side) and the side it reads, coalesced or through LDS, is the mask.
inline ModelPlan dv_model_swapped(ModelPlan mp) {
  for (int i = 0; i < mp.ga.n; i++) std::swap(mp.ga.rs[i], mp.ga.vs[i]);
  for (int i = 0; i < mp.gb.n; i++) std::swap(mp.gb.rs[i], mp.gb.vs[i]);
  std::swap(mp.roff, mp.voff);
  return mp;
}
// The weighted step (ppals_cp_wls_device, Ops::model_wls) reads TWO side views of one box beside the shard
// it rewrites: the data (the plan's vs / voff, as an export view's) and the weights, which a ModelSide
// carries: per mode of each group its stride, and the offset of the first element, cut to the rank's rows
// exactly as dv_model_box cuts the first view. `w` must be a checked view of the same box as the one `b`
// was cut from (same lo and len): only its strides differ.
struct ModelSide {
  ModelGroup ga, gb;  // len / mode as the plan's groups; vs = the second view's strides (rs unused, 0)
  int64_t off = 0;
};
inline ModelSide dv_model_side(const ViewArgs &w, const ModelBox &b, const ModelPlan &mp) {
  ModelSide s;
  s.off = (b.lo[0] - w.lo[0]) * w.stride[0];
  auto fill = [&](const ModelGroup &g, ModelGroup &o) {
    o.n = g.n;
    o.count = g.count;
    for (int i = 0; i < g.n; i++) {
      o.mode[i] = g.mode[i];
      o.len[i] = g.len[i];
      o.vs[i] = w.stride[g.mode[i]];
      o.rs[i] = 0;
    }
  };
  fill(mp.ga, s.ga);
  fill(mp.gb, s.gb);
  return s;
}
// How a side view is read by the weighted step: with the lane index along a (in the store pass) when it is
// unit-stride in A's fastest mode, or has no unit-stride run along b to prefer; otherwise with the lane
// index along b, through LDS. sa / sb: the view's strides in the first mode of group A / B (0 if the
// group is empty). A stride of 0 is a broadcast: every lane reads one address, either way.
inline bool dv_side_along_a(int64_t sa, int64_t sb) { return sa == 1 || sb != 1; }
// The second pass of the two-pass residual, view -= model: "V" is the view itself (its offsets in place
// of the shard's), after the tensor export has filled it.
inline ModelPlan dv_model_rmw(ModelPlan mp) {
  for (int i = 0; i < mp.ga.n; i++) mp.ga.rs[i] = mp.ga.vs[i];
  for (int i = 0; i < mp.gb.n; i++) mp.gb.rs[i] = mp.gb.vs[i];
  mp.roff = mp.voff;
  return mp;
}

}  // namespace ppals
