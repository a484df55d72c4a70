// kernels_pack.hip.h — the lossless resident copies of an fp32 tensor that k_scan_suffix_pk (28 bits
// per element, 3.5 bytes) and k_scan_suffix_pk2 (26 bits, 3.25 bytes) read (kernels_scan.hip.h).
//
// The copy is made for ONE scan shape [L rows, J reduced, T batches] and is stored block-major in that
// scan's own unit. A BLOCK is what one workgroup of the one-n-tile fp32 buffer-load scan consumes per
// iteration: 4 waves x 64 rows x 16 reduction indices of one (batch, row tile, k-block), in the
// kernel's lane mapping — lane (g, j16) of wave w holds rows 256*tile + 64*w + 4*j16 .. +3 of the
// reduction indices 16*kb + 4*u + g, u = 0..3 (k-quad u).
//
// An element is stored as the low 24 bits of its fp32 word and a code c; the word is
//   ((base + c) << 24) | low24            base: one byte per block, the smallest top byte in it
// so a block qualifies when the top bytes (sign + upper seven exponent bits) of its elements span at
// most 16 consecutive values; a layout is packed only if EVERY block qualifies (the pre-pass reports
// the largest spread). The per-lane arithmetic of both formats is pack_codec.h.
//
// FORMAT 28. Bytes of a block (PACK_BLOCK_BYTES = 14336 when whole):
//   [0, 2048)                  code plane: 8 bytes per thread (wave*512 + lane*8): dword 0 serves
//                              quads 0 (even nibbles) and 1 (odd nibbles), dword 1 quads 2 and 3;
//                              nibble pair jj of a dword belongs to the lane's row jj
//   [2048 + 3072*u, + 3072)    k-quad u: 12 bytes per thread (wave*768 + lane*12) = three dwords;
//                              dword i holds the low 24 bits of row i in its low bytes and byte i of
//                              row 3's low part on top
// so each load instruction of a wave (one b64, four b96) reads one contiguous run. The quads of a
// short last k-block that lie entirely beyond J are not stored: the tile simply ends, and the
// scan's buffer descriptor makes them read as zero. The blocks of a tile are consecutive in k, the
// tiles consecutive in the kernel's tile order (row tile fastest, then batch); rows beyond L in the
// last row tile of a batch and indices beyond J inside a stored quad hold low part 0, code 0 (the
// scan never stores those rows, and the packed Khatri-Rao operand is zero at those indices).
// One side word per block, base replicated into its four bytes, sits in a side array.
//
// FORMAT 26. The same blocks, quads, tile order and tails; the code plane is half as large
// (PACK26_BLOCK_BYTES = 13312 when whole):
//   [0, 1024)                  code plane: one dword per thread (wave*256 + lane*4); byte jj holds the
//                              LOW two code bits of the lane's row jj, quad u at bits 2u..2u+1
//   [1024 + 3072*u, + 3072)    k-quad u, as above
// A block whose top bytes spread over 4..15 (an ESCAPE block) keeps its quads and low code bits where
// they always lie — block addresses stay arithmetic — and the UPPER two code bits of every element,
// in the same dword arrangement, in an escape plane of 1024 bytes in a side buffer, at the block's
// escape ordinal. Ordinals count the escape blocks in block order (k_pk_side_words: a prefix sum, no
// atomic counter, so the same tensor always gives the same bytes). The side word is
// base | (ordinal + 1) << 8; upper 24 bits zero: no escape plane, the scan reads zeros for it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ops.h"

namespace ppals {

typedef unsigned int pk_u32;
typedef pk_u32 pk_u32x2 __attribute__((ext_vector_type(2)));

// the 16 fp32 words of (block gid, thread tid) in the scan's lane mapping; absent ones flagged
struct PkLane {
  pk_u32 e[4][4];
  bool ok[4][4];
};
__device__ inline PkLane pk_gather(const float *__restrict__ V, int64_t L, int64_t J, int n_mtiles, int nkb,
                                   int64_t gid, int tid) {
  const int lane = tid & 63, wave = tid >> 6, g = lane >> 4, j16 = lane & 15;
  const int64_t tile = gid / nkb;
  const int kb = (int)(gid % nkb);
  const int64_t mtile = tile % n_mtiles, batch = tile / n_mtiles;
  const int64_t m = (mtile * 4 + wave) * 64 + 4 * j16;
  PkLane r;
#pragma unroll
  for (int u = 0; u < 4; u++) {
    const int64_t k = (int64_t)kb * 16 + 4 * u + g;
#pragma unroll
    for (int jj = 0; jj < 4; jj++) {
      r.ok[u][jj] = k < J && m + jj < L;
      r.e[u][jj] = r.ok[u][jj] ? __float_as_uint(V[(batch * J + k) * L + m + jj]) : 0u;
    }
  }
  return r;
}

// pre-pass, one workgroup per block: bases[gid] = the block's smallest top byte, with bit 8 set if
// the block would need an escape plane in format 26 (provisional: k_pk_side_words finishes the
// word); stats[0] = the largest (max - min) of any block, stats[1] = the number of escape blocks —
// an integer maximum and an integer count, so the order of the atomic updates does not matter;
// nothing a scan reads is accumulated atomically
__global__ __launch_bounds__(256) void k_pk_prepass(const float *__restrict__ V, int64_t L, int64_t J,
                                                    int n_mtiles, int nkb, pk_u32 *__restrict__ bases,
                                                    int *__restrict__ stats) {
  __shared__ int smn[256], smx[256];
  const int64_t gid = blockIdx.x;
  const PkLane r = pk_gather(V, L, J, n_mtiles, nkb, gid, threadIdx.x);
  int mn = 255, mx = 0;
#pragma unroll
  for (int u = 0; u < 4; u++)
#pragma unroll
    for (int jj = 0; jj < 4; jj++)
      if (r.ok[u][jj]) {
        const int t = (int)(r.e[u][jj] >> 24);
        mn = min(mn, t);
        mx = max(mx, t);
      }
  smn[threadIdx.x] = mn;
  smx[threadIdx.x] = mx;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      smn[threadIdx.x] = min(smn[threadIdx.x], smn[threadIdx.x + s]);
      smx[threadIdx.x] = max(smx[threadIdx.x], smx[threadIdx.x + s]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    mn = smn[0];
    mx = smx[0];
    if (mx < mn) mn = mx = 0;
    const bool escape = mx - mn >= PACK26_WINDOW;
    bases[gid] = (pk_u32)mn | (escape ? 0x100u : 0u);
    atomicMax(stats, mx - mn);
    if (escape) atomicAdd(stats + 1, 1);
  }
}

// the side words of format `fmt` from the pre-pass's provisional ones, in place. ONE workgroup:
// thread t owns the blocks [t*per, (t+1)*per), counts its escape flags, the counts are summed in
// thread order (an exclusive prefix sum through shared memory), and the thread numbers its escape
// blocks from there — ordinals in block order, the same on every run.
__global__ __launch_bounds__(1024) void k_pk_side_words(pk_u32 *__restrict__ bases, int64_t nblocks, int fmt) {
  __shared__ unsigned int cnt[1024];
  const int64_t per = (nblocks + 1023) / 1024;
  const int64_t b0 = min(nblocks, (int64_t)threadIdx.x * per), b1 = min(nblocks, b0 + per);
  unsigned int mine = 0;
  if (fmt == PACK_FMT26)
    for (int64_t b = b0; b < b1; b++) mine += (bases[b] >> 8) & 1u;
  cnt[threadIdx.x] = mine;
  __syncthreads();
  for (int s = 1; s < 1024; s <<= 1) {  // inclusive scan, two barriers per step
    const unsigned int add = (int)threadIdx.x >= s ? cnt[threadIdx.x - s] : 0u;
    __syncthreads();
    cnt[threadIdx.x] += add;
    __syncthreads();
  }
  unsigned int ordinal = cnt[threadIdx.x] - mine;
  for (int64_t b = b0; b < b1; b++) {
    const pk_u32 w = bases[b];
    const bool escape = (w >> 8) & 1u;
    bases[b] = pk_side_word(fmt, w & 0xffu, escape, ordinal);
    ordinal += escape ? 1u : 0u;
  }
}

// the copy itself (after a pre-pass whose spread is below PACK_WINDOW, and k_pk_side_words<FMT>), one
// workgroup per block
template <int FMT>
__global__ __launch_bounds__(256) void k_pk_pack(const float *__restrict__ V, int64_t L, int64_t J, int n_mtiles,
                                                 int nkb, int64_t tile_bytes, const pk_u32 *__restrict__ bases,
                                                 char *__restrict__ out, char *__restrict__ esc) {
  const int64_t gid = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const PkLane r = pk_gather(V, L, J, n_mtiles, nkb, gid, tid);
  const pk_u32 side = bases[gid], base = side & 0xffu;
  const int64_t tile = gid / nkb;
  const int kb = (int)(gid % nkb);
  char *blk = out + tile * tile_bytes + (int64_t)kb * pack_block_bytes(FMT);
  pk_u32 cw[2] = {0u, 0u};
#pragma unroll
  for (int u = 0; u < 4; u++) {
    pk_u32 e[4];
#pragma unroll
    for (int jj = 0; jj < 4; jj++) {
      e[jj] = r.ok[u][jj] ? r.e[u][jj] : base << 24;  // absent: low part 0, code 0
      if constexpr (FMT == PACK_FMT26)
        pk26_put(cw[0], cw[1], u, jj, (e[jj] >> 24) - base);
      else
        pk28_put(cw, u, jj, (e[jj] >> 24) - base);
    }
    if ((int64_t)kb * 16 + 4 * u < J) {
      pk_u32 *q = reinterpret_cast<pk_u32 *>(blk + pack_code_bytes(FMT) + u * PACK_QUAD_BYTES + pk_quad_offset(wave, lane));
      pk_u32 qw[3];
      pk_quad_encode(e, qw);
#pragma unroll
      for (int i = 0; i < 3; i++) q[i] = qw[i];
    }
  }
  if constexpr (FMT == PACK_FMT26) {
    *reinterpret_cast<pk_u32 *>(blk + pk_code_offset(FMT, wave, lane)) = cw[0];
    if (side >> 8)  // (block-uniform) the escape plane of this block, at its ordinal
      *reinterpret_cast<pk_u32 *>(esc + (int64_t)((side >> 8) - 1u) * PACK26_ESC_BYTES +
                                  pk_code_offset(FMT, wave, lane)) = cw[1];
  } else {
    *reinterpret_cast<pk_u32x2 *>(blk + pk_code_offset(FMT, wave, lane)) = pk_u32x2{cw[0], cw[1]};
  }
}

}  // namespace ppals
