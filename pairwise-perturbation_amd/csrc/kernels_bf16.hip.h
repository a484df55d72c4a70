// kernels_bf16.hip.h — the tensor scans of a bf16-stored tensor (PPALS_BF16).
//
//   out[.., n] = sum_k V[.., k, ..] * B[k, n]      V: bf16, B = Khatri-Rao product (fp64 factors)
//
// A value stored in bf16 is exact, so the only rounding left is in the Khatri-Rao operand. It is
// split into three bf16 pieces, B = hi + mid + lo (bf16_split3: ~24 significant bits, what the fp32
// path keeps of it), and every piece is multiplied on v_mfma_f32_16x16x32_bf16: a bf16 x bf16
// product is exact in fp32, so the products are as exact as those of v_mfma_f32_16x16x4_f32 on an
// fp32 tensor, on a pipe 16x faster. fp32 partial sums are flushed into fp64 registers every
// BF16_FLUSH k-blocks: no fp32 chain holds more than 64 products of one piece (the f32 path's bound).
//
// MFMA operand roles (16x16x32 bf16, cdna_hip_programming.md §3):
//   A[i = lane&15][k = 8*(lane>>4) + e]  <- Khatri-Rao piece      (i = output column n)
//   B[k = 8*(lane>>4) + e][j = lane&15]  <- tensor value          (j = a tensor row)
//   D[i][j]: lane holds column j = lane&15 and rows i = 4*(lane>>4) + reg
// A lane needs 8 CONSECUTIVE reduction indices of one tensor row. In the suffix layout a 16-byte
// load gives 8 consecutive rows at ONE reduction index, so a lane loads 8 reduction indices x 8 rows
// (eight 16-byte buffer loads) and transposes the 8 x 8 block of 16-bit values in its registers
// (two-input byte permutes, 4 per B operand); each B operand then feeds 3 * NT MFMAs.
//
// Packed operand (k_krp_pack_bf16), one 16-byte load per lane and piece:
//   packed[(((((blk*NT + nt)*3 + p)*4 + g)*16 + n)*8 + e] = piece_p(KRP[32*blk + 8*g + e][16*nt + n])
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bf16.h"

namespace ppals {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef unsigned int bf16_u32x4 __attribute__((ext_vector_type(4)));

constexpr int BF16_KB = 32;     // reduction indices per k-block (one MFMA)
constexpr int BF16_FLUSH = 2;   // k-blocks between fp32 -> fp64 flushes: 64 products per piece
// n-tiles of 16 result columns per launch: ONE, so R columns take ceil(R / 16) passes. The two-tile
// instantiation needs 292 registers (8 rows x 2 tiles of fp32 + fp64 accumulators beside the 8 x 8
// tensor block): one wave per SIMD, measured at 0.10 of the HBM peak on configs[3] against 0.60 for
// one tile at the headline (profiles/bf16_bench.md, "Above 16 columns")
constexpr int BF16_MAX_NT = 1;

__global__ void k_krp_pack_bf16(uint16_t *__restrict__ P, int nblk, int NT, KrpArgs a, int64_t J,
                                int col0, int ncols) {
  const int64_t total = (int64_t)nblk * NT * 4 * 16 * 8;  // one entry per (blk, nt, g, n, e)
  for (int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t0 < total;
       t0 += (int64_t)gridDim.x * blockDim.x) {
    int64_t t = t0;
    const int e = (int)(t % 8);
    t /= 8;
    const int n = (int)(t % 16);
    t /= 16;
    const int g = (int)(t % 4);
    t /= 4;
    const int nt = (int)(t % NT);
    const int64_t blk = t / NT;
    const int64_t j = blk * BF16_KB + 8 * g + e;
    const int c = 16 * nt + n;
    double v = 0.0;
    if (j < J && c < ncols) {
      v = 1.0;
      int64_t rem = j;
      for (int f = 0; f < a.nf; f++) {
        const int64_t jf = rem % a.rows[f];
        rem /= a.rows[f];
        v *= a.ptr[f][jf + a.ld[f] * (col0 + c)];
      }
    }
    uint16_t hi, mid, lo;
    bf16_split3(v, &hi, &mid, &lo);
    const int64_t base = ((blk * NT + nt) * 3) * 512 + (g * 16 + n) * 8 + e;
    P[base] = hi;
    P[base + 512] = mid;
    P[base + 1024] = lo;
  }
}

// Suffix scan (K1 / batched single-mode TTM) of a bf16 tensor:
//   out[mo(m) + n*out_nstride + batch*out_batch_stride] = sum_k V[m + M*k + batch*M*K] * B[k,n]
// grid: n_mtiles * nsplit * batch workgroups of 256 threads = 4 waves (block id = mtile + n_mtiles *
// (split + nsplit * batch)); a wave owns 128 consecutive rows (lane j16: rows 8*j16 .. 8*j16+7), lane
// group g the reduction indices 8g .. 8g+7 of every k-block of its split (k-blocks [split *
// kb_per_split, ...): the partial sums of a split land at out_split_stride, k_slab_reduce adds them).
// Every tensor byte is read once, by 16-byte buffer loads whose descriptor ends at the last valid
// column of the block (a partial block reads zeros there, and the packed operand is zero too).
// Padded layouts (row_ld > 0) store compact rows (scan_row_map). BIG: a k-block spans 2^31 bytes or
// more (32 * M * 2: M >= 2^25 rows, configs[3]'s 400^3), past 32-bit buffer offsets — 16-byte global
// loads with 64-bit addresses instead, the columns past K read as zeros by predication.
// Preconditions (launcher): M % 8 == 0, M >= 8, V 16-byte aligned, the packed operand < 2^31 bytes.
template <int NT, bool NTS, bool BIG>
__global__ __launch_bounds__(256) void k_scan_suffix_bf16(
    const uint16_t *__restrict__ V, int64_t M, int64_t K, const uint16_t *__restrict__ P, int n_mtiles,
    int nsplit, int kb_per_split, int nkb, double *__restrict__ out, int64_t out_nstride,
    int64_t out_split_stride, int64_t out_batch_stride, int ncols, int out32, int64_t row_ld,
    int64_t row_valid) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, j16 = lane & 15;
  unsigned bid = blockIdx.x;
  const int mtile = (int)(bid % (unsigned)n_mtiles);
  bid /= (unsigned)n_mtiles;
  const int split = (int)(bid % (unsigned)nsplit);
  const int64_t batch = bid / (unsigned)nsplit;
  const int kb0 = split * kb_per_split, kb1 = min(nkb, kb0 + kb_per_split);
  const int64_t m0 = ((int64_t)mtile * 4 + wave) * 128;
  if (m0 >= M) return;  // wave-uniform
  const int64_t m = m0 + 8 * j16;
  const int64_t m_ld = min(m, M - 8);  // lanes past the edge re-read a valid row, store nothing
  const uint16_t *vb = V + batch * M * K;
  const int64_t block_bytes = (int64_t)BF16_KB * M * 2;
  const int64_t total_bytes = K * M * 2;
  const int voff = BIG ? 0 : (int)(((int64_t)8 * g * M + m_ld) * 2);
  const int ustep = BIG ? 0 : (int)(M * 2);
  const __amdgpu_buffer_rsrc_t rsrcP = __builtin_amdgcn_make_buffer_rsrc(
      (void *)P, 0, (int)((int64_t)nkb * NT * 3 * 1024), 0x00020000);
  const int voffP = (g * 16 + j16) * 16;

  f32x4 acc[8][NT];
  double acc64[8][NT][4];
#pragma unroll
  for (int jj = 0; jj < 8; jj++)
#pragma unroll
    for (int nt = 0; nt < NT; nt++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        acc[jj][nt][r] = 0.f;
        acc64[jj][nt][r] = 0.0;
      }
  for (int kc = kb0; kc < kb1; kc += BF16_FLUSH) {
    const int ke = min(kb1, kc + BF16_FLUSH);
    for (int kb = kc; kb < ke; kb++) {
      bf16_u32x4 cv[8];  // cv[u]: rows m .. m+7 at reduction index 32 kb + 8 g + u
      if constexpr (BIG) {
        const int64_t k0 = (int64_t)kb * BF16_KB + 8 * g;
        const uint16_t *p0 = vb + k0 * M + m_ld;
#pragma unroll
        for (int u = 0; u < 8; u++) {
          const bf16_u32x4 z = {0u, 0u, 0u, 0u};
          cv[u] = k0 + u < K ? __builtin_nontemporal_load(reinterpret_cast<const bf16_u32x4 *>(p0 + u * M)) : z;
        }
      } else {
        const int64_t boff = (int64_t)kb * block_bytes;
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            (void *)((const char *)vb + boff), 0, (int)min(total_bytes - boff, block_bytes), 0x00020000);
#pragma unroll
        for (int u = 0; u < 8; u++)
          cv[u] = __builtin_bit_cast(bf16_u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, u * ustep, 2));
      }
      bf16x8_t ab[NT][3];
#pragma unroll
      for (int nt = 0; nt < NT; nt++)
#pragma unroll
        for (int p = 0; p < 3; p++)
          ab[nt][p] = __builtin_bit_cast(
              bf16x8_t, __builtin_amdgcn_raw_buffer_load_b128(rsrcP, voffP, ((kb * NT + nt) * 3 + p) * 1024, 0));
#pragma unroll
      for (int jj = 0; jj < 8; jj++) {
        // row jj's 8 reduction indices: dword w = (index 2w, index 2w+1), low half first
        bf16_u32x4 bw;
#pragma unroll
        for (int w = 0; w < 4; w++) {
          const unsigned a0 = cv[2 * w][jj >> 1], a1 = cv[2 * w + 1][jj >> 1];
          bw[w] = (jj & 1) ? __builtin_amdgcn_perm(a1, a0, 0x07060302u)
                           : __builtin_amdgcn_perm(a1, a0, 0x05040100u);
        }
        const bf16x8_t bv = __builtin_bit_cast(bf16x8_t, bw);
#pragma unroll
        for (int nt = 0; nt < NT; nt++)
#pragma unroll
          for (int p = 2; p >= 0; p--)  // smallest piece first
            acc[jj][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ab[nt][p], bv, acc[jj][nt], 0, 0, 0);
      }
    }
#pragma unroll
    for (int jj = 0; jj < 8; jj++)
#pragma unroll
      for (int nt = 0; nt < NT; nt++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          acc64[jj][nt][r] += (double)acc[jj][nt][r];
          acc[jj][nt][r] = 0.f;
        }
  }
  const ScanRowMap rm = scan_row_map<8>(m, M, row_ld, row_valid);
  if (rm.nvalid <= 0) return;
  const int64_t obase = split * out_split_stride + batch * out_batch_stride;
#pragma unroll
  for (int nt = 0; nt < NT; nt++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int n = 16 * nt + 4 * g + r;
      if (n >= ncols) continue;
      const int64_t idx = obase + (int64_t)n * out_nstride + rm.mo;
      // a lane's 8 rows are consecutive: 16-byte stores where they are aligned (NTS: non-temporal,
      // a result too large for the Infinity Cache — the rule of the fp32 kernels)
      if (out32 && rm.nvalid == 8 && ((uintptr_t)(reinterpret_cast<float *>(out) + idx) & 15) == 0) {
        float *o = reinterpret_cast<float *>(out) + idx;
#pragma unroll
        for (int h = 0; h < 2; h++) {
          const f32x4 v = {(float)acc64[4 * h][nt][r], (float)acc64[4 * h + 1][nt][r],
                           (float)acc64[4 * h + 2][nt][r], (float)acc64[4 * h + 3][nt][r]};
          if constexpr (NTS)
            __builtin_nontemporal_store(v, reinterpret_cast<f32x4 *>(o + 4 * h));
          else
            *reinterpret_cast<f32x4 *>(o + 4 * h) = v;
        }
      } else if (!out32 && rm.nvalid == 8 && ((uintptr_t)(out + idx) & 15) == 0) {
#pragma unroll
        for (int h = 0; h < 4; h++) {
          const f64x2 v = {acc64[2 * h][nt][r], acc64[2 * h + 1][nt][r]};
          if constexpr (NTS)
            __builtin_nontemporal_store(v, reinterpret_cast<f64x2 *>(out + idx + 2 * h));
          else
            *reinterpret_cast<f64x2 *>(out + idx + 2 * h) = v;
        }
      } else {
#pragma unroll
        for (int jj = 0; jj < 8; jj++)
          if (jj < rm.nvalid) scan_store(out, idx + jj, acc64[jj][nt][r], out32);
      }
    }
}

// Every other shape (unaligned rows, fewer than 8 rows, misaligned base): one thread per kept
// (row l, batch t), fp64 products against the plain fp64 Khatri-Rao matrix B (J x ncols):
//   out[mo(l) + out_tstride*t + out_rstride*n] = sum_j V[l + L*(j + J*t)] * B[j + J*n]
template <int NC>
__global__ __launch_bounds__(256) void k_scan_bf16_rows(const uint16_t *__restrict__ V, int64_t L, int64_t J,
                                                        int64_t T, const double *__restrict__ B, int ncols,
                                                        double *__restrict__ out, int64_t out_tstride,
                                                        int64_t out_rstride, int out32, int64_t row_ld,
                                                        int64_t row_valid) {
  const int64_t total = L * T;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t l = e % L, t = e / L;
    const ScanRowMap rm = scan_row_map<1>(l, L, row_ld, row_valid);
    if (rm.nvalid == 0) continue;
    double acc[NC];
#pragma unroll
    for (int n = 0; n < NC; n++) acc[n] = 0.0;
    const uint16_t *v = V + l + L * J * t;
    for (int64_t j = 0; j < J; j++) {
      const double x = (double)bf16_bits_to_float(v[L * j]);
#pragma unroll
      for (int n = 0; n < NC; n++)
        if (n < ncols) acc[n] += x * B[j + J * n];
    }
#pragma unroll
    for (int n = 0; n < NC; n++)
      if (n < ncols) scan_store(out, rm.mo + out_tstride * t + out_rstride * n, acc[n], out32);
  }
}

// The prefix form (L == 1): one wave per column t (grid-stride), its lanes striding over the contiguous reduction
// index j (coalesced), fp64 products, partial sums combined by a fixed butterfly (deterministic):
//   out[out_tstride*t + out_rstride*n] = sum_j V[j + J*t] * B[j + J*n]
template <int NC>
__global__ __launch_bounds__(256) void k_scan_bf16_prefix(const uint16_t *__restrict__ V, int64_t J, int64_t T,
                                                          const double *__restrict__ B, int ncols,
                                                          double *__restrict__ out, int64_t out_tstride,
                                                          int64_t out_rstride, int out32) {
  const int lane = threadIdx.x & 63;
  for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < T; t += (int64_t)gridDim.x * 4) {
  double acc[NC];
#pragma unroll
  for (int n = 0; n < NC; n++) acc[n] = 0.0;
  const uint16_t *v = V + J * t;
  for (int64_t j = lane; j < J; j += 64) {
    const double x = (double)bf16_bits_to_float(v[j]);
#pragma unroll
    for (int n = 0; n < NC; n++)
      if (n < ncols) acc[n] += x * B[j + J * n];
  }
#pragma unroll
  for (int n = 0; n < NC; n++) {
    if (n >= ncols) continue;
    double s = acc[n];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) scan_store(out, out_tstride * t + out_rstride * n, s, out32);
  }
  }
}

}  // namespace ppals
