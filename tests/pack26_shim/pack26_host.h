// tests/pack26_shim/pack26_host.h — TEST INFRASTRUCTURE: one block of a packed twin written and read
// back on the host with the product's own per-lane arithmetic (csrc/pack_codec.h), thread by thread
// as k_pk_pack writes it and the packed scan reads it.
#pragma once
#include <stdint.h>
#include <string.h>

#include "pack_codec.h"

namespace p26 {
using namespace ppals;

// words[tid][u][jj]: the fp32 words of thread tid (top byte = base + code). block: pack_block_bytes(fmt)
// bytes; plane: PACK26_ESC_BYTES (format 26; all zero for a block without escape codes).
inline void pack_block(int fmt, const uint32_t *words, uint32_t base, uint8_t *block, uint8_t *plane) {
  for (int tid = 0; tid < 256; tid++) {
    const int lane = tid & 63, wave = tid >> 6;
    uint32_t cw[2] = {0u, 0u};
    for (int u = 0; u < 4; u++) {
      const uint32_t *e = words + (tid * 4 + u) * 4;
      for (int jj = 0; jj < 4; jj++) {
        if (fmt == PACK_FMT26) pk26_put(cw[0], cw[1], u, jj, (e[jj] >> 24) - base);
        else pk28_put(cw, u, jj, (e[jj] >> 24) - base);
      }
      uint32_t q[3];
      pk_quad_encode(e, q);
      memcpy(block + pack_code_bytes(fmt) + u * PACK_QUAD_BYTES + pk_quad_offset(wave, lane), q, sizeof q);
    }
    if (fmt == PACK_FMT26) {
      memcpy(block + pk_code_offset(fmt, wave, lane), &cw[0], 4);
      memcpy(plane + pk_code_offset(fmt, wave, lane), &cw[1], 4);
    } else {
      memcpy(block + pk_code_offset(fmt, wave, lane), cw, 8);
    }
  }
}

inline void unpack_block(int fmt, const uint8_t *block, const uint8_t *plane, uint32_t base, uint32_t *words) {
  const uint32_t basew = base * 0x01010101u;
  for (int tid = 0; tid < 256; tid++) {
    const int lane = tid & 63, wave = tid >> 6;
    uint32_t cw[2] = {0u, 0u};
    if (fmt == PACK_FMT26) {
      memcpy(&cw[0], block + pk_code_offset(fmt, wave, lane), 4);
      memcpy(&cw[1], plane + pk_code_offset(fmt, wave, lane), 4);
    } else {
      memcpy(cw, block + pk_code_offset(fmt, wave, lane), 8);
    }
    for (int u = 0; u < 4; u++) {
      uint32_t q[3];
      memcpy(q, block + pack_code_bytes(fmt) + u * PACK_QUAD_BYTES + pk_quad_offset(wave, lane), sizeof q);
      const uint32_t tops = fmt == PACK_FMT26 ? pk26_tops(cw[0], u, basew) + pk26_escape(cw[1], u)
                                              : pk28_tops(cw[0], cw[1], u, basew);
      pk_quad_decode(tops, q[0], q[1], q[2], words + (tid * 4 + u) * 4);
    }
  }
}

}  // namespace p26
