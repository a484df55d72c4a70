// tests/pack26_shim/pack26_shim.cpp — TEST INFRASTRUCTURE: a C surface over csrc/pack_codec.h for
// tests/test_pack26_codec_cpu.py (host only: no kernel, no device).
#include "pack26_host.h"

extern "C" {
void p26_pack_block(int fmt, const uint32_t *words, uint32_t base, uint8_t *block, uint8_t *plane) {
  p26::pack_block(fmt, words, base, block, plane);
}
void p26_unpack_block(int fmt, const uint8_t *block, const uint8_t *plane, uint32_t base, uint32_t *words) {
  p26::unpack_block(fmt, block, plane, base, words);
}
uint32_t p26_perm(uint32_t hi, uint32_t lo, uint32_t sel) { return ppals::pk_perm(hi, lo, sel); }
int64_t p26_tile_bytes(int fmt, int64_t J) { return ppals::pack_tile_bytes(fmt, J); }
int p26_block_bytes(int fmt) { return ppals::pack_block_bytes(fmt); }
int p26_choose_format(int mode, int spread, int64_t escapes, int64_t blocks) {
  return ppals::pack_choose_format(mode, spread, escapes, blocks);
}
uint32_t p26_side_word(int fmt, uint32_t base, int escape, uint32_t ordinal) {
  return ppals::pk_side_word(fmt, base, escape != 0, ordinal);
}
}
