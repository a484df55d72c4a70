// pack_codec.h — the per-lane arithmetic of the packed twins (kernels_pack.hip.h writes them,
// k_scan_suffix_pk / k_scan_suffix_pk2 in kernels_scan.hip.h read them), in ONE definition that
// compiles for the device and for the host (tests/pack26_shim): codes <-> code words, fp32 words <->
// the three dwords of a k-quad, and the sizes of a tile in either format.
//
// A lane of a block holds, per k-quad u = 0..3, the four fp32 words of its rows jj = 0..3. A word is
//   (base + code) << 24 | low24          base: the block's smallest top byte, code = 0..15
// Format 28 keeps a 4-bit code per element: two code dwords per lane, dword u>>1, nibble 2*jj + (u&1).
// Format 26 keeps the low two code bits in ONE code dword per lane — byte jj = row jj, quad u at bits
// 2u..2u+1 — and the upper two code bits, in the same arrangement, in the lane's dword of the
// block's escape plane; a block whose codes all fit two bits has no escape plane (reads as zero).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PPALS_PK_HD __host__ __device__ inline
#else
#define PPALS_PK_HD inline
#endif

namespace ppals {

constexpr int PACK_FMT28 = 28, PACK_FMT26 = 26;
constexpr int PACK_QUAD_BYTES = 3072;                        // 256 lanes x three dwords
constexpr int PACK_CODE_BYTES = 2048, PACK26_CODE_BYTES = 1024;  // 256 lanes x two / one dword
constexpr int PACK_BLOCK_BYTES = PACK_CODE_BYTES + 4 * PACK_QUAD_BYTES;      // 14336
constexpr int PACK26_BLOCK_BYTES = PACK26_CODE_BYTES + 4 * PACK_QUAD_BYTES;  // 13312
constexpr int PACK26_ESC_BYTES = 1024;                       // escape plane of one block
constexpr int PACK_WINDOW = 16;   // top bytes of a block must span fewer values than this
constexpr int PACK26_WINDOW = 4;  // ... and fewer than this for a block without an escape plane
constexpr int64_t PACK26_MAX_ESCAPES = (1 << 24) - 1;        // ordinal + 1 fits the side word's upper 24 bits

// (constexpr: callable on either side, and a compile-time constant where the format is one)
constexpr int pack_code_bytes(int fmt) { return fmt == PACK_FMT26 ? PACK26_CODE_BYTES : PACK_CODE_BYTES; }
constexpr int pack_block_bytes(int fmt) { return fmt == PACK_FMT26 ? PACK26_BLOCK_BYTES : PACK_BLOCK_BYTES; }
// bytes of one (row tile, batch): whole blocks, then the code plane and the quads of a short last
// k-block that reach below J
PPALS_PK_HD int64_t pack_tile_bytes(int fmt, int64_t J) {
  const int64_t kfull = J / 16, rem = J - kfull * 16;
  return kfull * pack_block_bytes(fmt) + (rem ? pack_code_bytes(fmt) + (rem + 3) / 4 * PACK_QUAD_BYTES : 0);
}

// byte offsets of thread (wave, lane) inside a block: its code word(s) in the code plane (the same
// offset serves its dword of a format-26 escape plane), and its three dwords inside a k-quad
PPALS_PK_HD int pk_code_offset(int fmt, int wave, int lane) {
  return fmt == PACK_FMT26 ? wave * 256 + lane * 4 : wave * 512 + lane * 8;
}
PPALS_PK_HD int pk_quad_offset(int wave, int lane) { return wave * 768 + lane * 12; }

// Which format a twin gets. mode: PPALS_PACK_LAYOUT (1: 28 bits, 2: 26 bits, anything else: the
// rule — 26 bits while escape blocks are at most 1/16 of the blocks, above that less than 15/16 of
// the saving is left). spread: largest (max - min) top byte of a block. 0: the twin is refused.
PPALS_PK_HD int pack_choose_format(int mode, int spread, int64_t escapes, int64_t blocks) {
  if (spread < 0 || spread >= PACK_WINDOW) return 0;
  const bool ordinals_fit = escapes < PACK26_MAX_ESCAPES;
  if (mode == 1) return PACK_FMT28;
  if (mode == 2) return ordinals_fit ? PACK_FMT26 : 0;
  return ordinals_fit && escapes * 16 <= blocks ? PACK_FMT26 : PACK_FMT28;
}

// the block's side word. Format 28: base in all four bytes. Format 26: base | (escape ordinal + 1) << 8,
// upper 24 bits zero: no escape plane.
PPALS_PK_HD uint32_t pk_side_word(int fmt, uint32_t base, bool escape, uint32_t ordinal) {
  if (fmt == PACK_FMT26) return base | (escape ? (ordinal + 1u) << 8 : 0u);
  return base * 0x01010101u;
}

// v_perm_b32(hi, lo, sel): result byte i is picked by selector byte i — 0..3: that byte of lo,
// 4..7: that byte of hi, 0x0c: zero. (The host form knows the selectors this file uses and, of the
// hardware's others, 0x0d..0xff = 0xff and 8..11 = sign fill of a 16-bit half.)
PPALS_PK_HD uint32_t pk_perm(uint32_t hi, uint32_t lo, uint32_t sel) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_perm(hi, lo, sel);
#else
  const uint64_t both = ((uint64_t)hi << 32) | lo;
  uint32_t r = 0;
  for (int i = 0; i < 4; i++) {
    const uint32_t s = (sel >> (8 * i)) & 0xffu;
    uint32_t b;
    if (s < 8) b = (uint32_t)(both >> (8 * s)) & 0xffu;
    else if (s < 12) b = ((both >> (16 * (s - 8) + 15)) & 1u) ? 0xffu : 0u;
    else if (s == 12) b = 0u;
    else b = 0xffu;
    r |= b << (8 * i);
  }
  return r;
#endif
}

// ---- the k-quad: words e[0..3] of rows 0..3 <-> three dwords (low 24 bits of rows 0..2, byte i of
// row 3's low part on top of dword i); the top bytes travel as codes
PPALS_PK_HD void pk_quad_encode(const uint32_t e[4], uint32_t q[3]) {
  for (int i = 0; i < 3; i++) q[i] = (e[i] & 0xffffffu) | (((e[3] >> (8 * i)) & 0xffu) << 24);
}
// tops: the four top bytes (base + code), byte jj = row jj
PPALS_PK_HD void pk_quad_decode(uint32_t tops, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t e[4]) {
  e[0] = pk_perm(tops, w0, 0x04020100u);
  e[1] = pk_perm(tops, w1, 0x05020100u);
  e[2] = pk_perm(tops, w2, 0x06020100u);
  e[3] = pk_perm(w1, w0, 0x0c0c0703u) |  // w0.b3, w1.b3, 0, 0
         pk_perm(tops, w2, 0x07030c0cu);  // 0, 0, w2.b3, tops.b3
}

// ---- format 28: cw[2], code 0..15 of (quad u, row jj)
PPALS_PK_HD void pk28_put(uint32_t cw[2], int u, int jj, uint32_t code) {
  cw[u >> 1] |= code << (8 * jj + 4 * (u & 1));
}
// (base + code <= 255 in every byte: no carries) basew: base in all four bytes
PPALS_PK_HD uint32_t pk28_tops(uint32_t cw0, uint32_t cw1, int u, uint32_t basew) {
  const uint32_t cw = (u >> 1) ? cw1 : cw0;
  return (((u & 1) ? cw >> 4 : cw) & 0x0f0f0f0fu) + basew;
}

// ---- format 26: cw the code dword, ew the lane's dword of the escape plane
PPALS_PK_HD void pk26_put(uint32_t &cw, uint32_t &ew, int u, int jj, uint32_t code) {
  cw |= (code & 3u) << (8 * jj + 2 * u);
  ew |= (code >> 2) << (8 * jj + 2 * u);
}
PPALS_PK_HD uint32_t pk26_tops(uint32_t cw, int u, uint32_t basew) {
  return ((cw >> (2 * u)) & 0x03030303u) + basew;
}
// the upper code bits of quad u, in place (bits 2..3 of every byte), to be added to pk26_tops
PPALS_PK_HD uint32_t pk26_escape(uint32_t ew, int u) {
  return (u == 0 ? ew << 2 : ew >> (2 * u - 2)) & 0x0c0c0c0cu;
}

}  // namespace ppals
