// kernels_fms.hip.h — the factor congruence behind the factor match score (Ops::factor_congruence,
// CpEngine::congruence): the cross products a_i^T b_i of two column sets in every mode on the fp64 matrix
// cores, with the column sums of squares of both sides, and the finishing pass that turns them into
// Phi, w_a and w_b. Two launches whatever the order, the number of starts and the extents. All fp64, no
// atomics: every sum is added in an order fixed by the extents alone.
#pragma once
#include "kernels_small.hip.h"

namespace ppals {

constexpr int FMS_CH = 32;           // rows of one staged chunk
constexpr int FMS_LD = FMS_CH + 2;   // doubles between two staged columns: 68 banks, 16 lanes on 16 bank pairs
constexpr int FMS_MAXC = 128;        // columns a side (Ops::kCongruenceMaxCols)
constexpr int FMS_MAXSLAB = 32;      // workgroups of one mode at the most
// LDS of k_fms_cross at 128 + 128 columns: 256 * 34 * 8 = 69 632 B of the 160 KB, two workgroups a CU
inline size_t fms_lds_bytes(int cap, int cbp, bool same) {
  return sizeof(double) * (size_t)FMS_LD * (size_t)(same ? cap : cap + cbp);
}

// By value, as a kernel argument. The rows of mode i are cut into chunks of FMS_CH; workgroup g serves
// mode i for slab0[i] <= g < slab0[i + 1] and there the cps[i] consecutive chunks from (g - slab0[i]) cps[i].
struct FmsArgs {
  const double *a[MAX_ORDER], *b[MAX_ORDER];
  int64_t lda[MAX_ORDER], ldb[MAX_ORDER];
  int64_t rows_a[MAX_ORDER], rows_b[MAX_ORDER];
  int slab0[MAX_ORDER + 1];
  int cps[MAX_ORDER];
  int N, Ca, Cb, same;  // same: b is a (one staging serves both operands)
  unsigned mask;        // bit i: mode i is compared (its cross product is formed)
};
// One workgroup's partial, Cap = 16 ceil(Ca / 16), Cbp likewise:
//   [ cross[q + Cbp * p]  (Cap * Cbp) | sum of squares of a's columns (Cap) | of b's columns (Cbp) ]
__host__ __device__ inline int64_t fms_part_stride(int cap, int cbp) { return (int64_t)cap * cbp + cap + cbp; }

// Workgroup g walks its chunks in order. A chunk of a (and of b unless same) is loaded with 32 consecutive
// lanes down a column — rows past the side's extent in this mode and columns past Ca / Cb enter as zeros —
// and staged column by column in LDS. Wave w owns the 16 x 16 output tiles (ta, tb), ta in {w, w + 4}, all
// tb, and adds 8 k-steps of v_mfma_f64_16x16x4_f64 per chunk to them: A operand a[row k0 + (lane >> 4),
// column 16 ta + (lane & 15)], B operand b[row k0 + (lane >> 4), column 16 tb + (lane & 15)], D at
// (p = 16 ta + (lane >> 4) + 4 reg, q = 16 tb + (lane & 15)) — the maps of kernels_model.hip.h. Thread t
// adds the squares of column t of a (t < 128) or t - 128 of b from LDS in row order. Every mode gets its
// sums of squares; only a compared mode gets its cross product.
// dynamic LDS: fms_lds_bytes
__global__ __launch_bounds__(256) void k_fms_cross(FmsArgs A, double *__restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) double lds_fms[];
  const int g = blockIdx.x, tid = threadIdx.x;
  int mode = 0;
  while (mode + 1 < A.N && g >= A.slab0[mode + 1]) mode++;
  const int slab = g - A.slab0[mode];
  const int nta = (A.Ca + 15) >> 4, ntb = (A.Cb + 15) >> 4;
  const int cap = 16 * nta, cbp = 16 * ntb;
  const int64_t ra = A.rows_a[mode], rb = A.rows_b[mode];
  const int64_t rmax = ra > rb ? ra : rb;
  const int64_t r_begin = (int64_t)slab * A.cps[mode] * FMS_CH;
  int64_t r_end = r_begin + (int64_t)A.cps[mode] * FMS_CH;
  if (r_end > rmax) r_end = rmax;
  const bool cross = (A.mask >> mode) & 1u;
  const double *__restrict__ ga = A.a[mode];
  const double *__restrict__ gb = A.b[mode];
  const int64_t lda = A.lda[mode], ldb = A.ldb[mode];
  double *As = lds_fms;
  double *Bs = A.same ? As : As + cap * FMS_LD;
  const int wave = tid >> 6, lane = tid & 63, j16 = lane & 15, g4 = lane >> 4;

  f64x4 acc[2][8];
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int tb = 0; tb < 8; tb++) acc[i][tb] = f64x4{0.0, 0.0, 0.0, 0.0};
  double ss = 0.0;
  const int sc = tid & 127;                         // the column whose squares this thread adds
  const double *Ss = tid < 128 ? As : Bs;
  const bool s_on = sc < (tid < 128 ? cap : cbp);

  for (int64_t r0 = r_begin; r0 < r_end; r0 += FMS_CH) {
    __syncthreads();  // the chunk before this one has been read
    for (int e = tid; e < cap * FMS_CH; e += 256) {
      const int r = e & (FMS_CH - 1), c = e / FMS_CH;
      const int64_t row = r0 + r;
      As[c * FMS_LD + r] = (c < A.Ca && row < ra) ? ga[row + lda * c] : 0.0;
    }
    if (!A.same)
      for (int e = tid; e < cbp * FMS_CH; e += 256) {
        const int r = e & (FMS_CH - 1), c = e / FMS_CH;
        const int64_t row = r0 + r;
        Bs[c * FMS_LD + r] = (c < A.Cb && row < rb) ? gb[row + ldb * c] : 0.0;
      }
    __syncthreads();
    if (s_on) {
#pragma unroll 8
      for (int r = 0; r < FMS_CH; r++) {
        const double v = Ss[sc * FMS_LD + r];
        ss += v * v;
      }
    }
    if (cross) {
#pragma unroll 2
      for (int k0 = 0; k0 < FMS_CH; k0 += 4) {
        double av[2];
#pragma unroll
        for (int i = 0; i < 2; i++) {
          const int ta = wave + 4 * i;
          av[i] = ta < nta ? As[(16 * ta + j16) * FMS_LD + k0 + g4] : 0.0;
        }
#pragma unroll
        for (int tb = 0; tb < 8; tb++) {
          if (tb < ntb) {
            const double bv = Bs[(16 * tb + j16) * FMS_LD + k0 + g4];
#pragma unroll
            for (int i = 0; i < 2; i++)
              if (wave + 4 * i < nta) acc[i][tb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[i], bv, acc[i][tb], 0, 0, 0);
          }
        }
      }
    }
  }

  double *out = part + (int64_t)g * fms_part_stride(cap, cbp);
  if (cross) {
#pragma unroll
    for (int i = 0; i < 2; i++) {
      const int ta = wave + 4 * i;
      if (ta >= nta) continue;
#pragma unroll
      for (int tb = 0; tb < 8; tb++) {
        if (tb >= ntb) continue;
#pragma unroll
        for (int r = 0; r < 4; r++) out[(16 * tb + j16) + (int64_t)cbp * (16 * ta + g4 + 4 * r)] = acc[i][tb][r];
      }
    }
  }
  if (s_on) out[(int64_t)cap * cbp + (tid < 128 ? sc : cap + sc)] = ss;
}

// The finishing pass. Every workgroup first adds, slab by slab in slab order, the sums of squares of all
// columns of both sides in every mode and keeps the norms in LDS (N (Ca + Cb) sums of at most FMS_MAXSLAB
// terms: cheaper than a launch of their own). Then one thread per entry (p, q), q fastest across the lanes
// as the partials are stored: per compared mode the slabs' cross products added in slab order, divided by
// both norms, multiplied over the modes; a norm that is not a positive finite number in a compared mode
// makes the entry 0. Workgroup 0 writes w_a and w_b, the products of the norms over ALL modes.
__global__ __launch_bounds__(256) void k_fms_finish(FmsArgs A, const double *__restrict__ part,
                                                    double *__restrict__ Phi, double *__restrict__ wa,
                                                    double *__restrict__ wb) {
  __shared__ double nrm[MAX_ORDER * 2 * FMS_MAXC];  // [mode][a: 0 .. 127 | b: 128 .. 255]
  const int tid = threadIdx.x;
  const int cap = 16 * ((A.Ca + 15) >> 4), cbp = 16 * ((A.Cb + 15) >> 4);
  const int64_t stride = fms_part_stride(cap, cbp);
  const int nc = A.Ca + A.Cb;
  for (int item = tid; item < A.N * nc; item += blockDim.x) {
    const int mode = item / nc, c = item % nc;
    const int64_t at = (int64_t)cap * cbp + (c < A.Ca ? c : cap + (c - A.Ca));
    double s = 0.0;
    for (int sl = A.slab0[mode]; sl < A.slab0[mode + 1]; sl++) s += part[sl * stride + at];
    nrm[mode * 2 * FMS_MAXC + (c < A.Ca ? c : FMS_MAXC + (c - A.Ca))] = sqrt(s);
  }
  __syncthreads();
  const double dmax = 1.79769313486231570e308;
  const int64_t total = (int64_t)A.Ca * A.Cb;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + tid; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int q = (int)(e % A.Cb), p = (int)(e / A.Cb);
    double phi = 1.0;
    bool bad = false;
    for (int mode = 0; mode < A.N; mode++) {
      if (!((A.mask >> mode) & 1u)) continue;
      const double x = nrm[mode * 2 * FMS_MAXC + p], y = nrm[mode * 2 * FMS_MAXC + FMS_MAXC + q];
      if (!(x > 0.0) || !(x <= dmax) || !(y > 0.0) || !(y <= dmax)) {
        bad = true;
        continue;
      }
      double dot = 0.0;
      for (int sl = A.slab0[mode]; sl < A.slab0[mode + 1]; sl++) dot += part[sl * stride + q + (int64_t)cbp * p];
      phi *= (dot / x) / y;
    }
    Phi[p + (int64_t)A.Ca * q] = bad ? 0.0 : phi;
  }
  if (blockIdx.x == 0)
    for (int c = tid; c < nc; c += blockDim.x) {
      double w = 1.0;
      for (int mode = 0; mode < A.N; mode++)
        w *= nrm[mode * 2 * FMS_MAXC + (c < A.Ca ? c : FMS_MAXC + (c - A.Ca))];
      if (c < A.Ca)
        wa[c] = w;
      else
        wb[c - A.Ca] = w;
    }
}

}  // namespace ppals
