// tests/pack26_shim/pack26_selfcheck.cpp — TEST INFRASTRUCTURE: the codec round trip of
// tests/test_pack26_codec_cpu.py as a stand-alone program, for a build with host sanitizers
// (make selfcheck). Every lane position and quad, every code (0..3 without an escape plane, 0..15
// with one, 0..15 in format 28), bases 0, 1, 127, 240: encode, decode, same words. Exit status 0: all did.
#include <stdio.h>
#include <vector>

#include "pack26_host.h"

int main() {
  using namespace ppals;
  const uint32_t bases[4] = {0u, 1u, 127u, 240u};
  std::vector<uint32_t> in(256 * 16), out(256 * 16);
  std::vector<uint8_t> block(PACK_BLOCK_BYTES), plane(PACK26_ESC_BYTES);
  long checked = 0, bad = 0;
  uint32_t rng = 12345u;
  for (int fmt : {PACK_FMT26, PACK_FMT28})
    for (uint32_t base : bases)
      for (uint32_t code = 0; code < 16; code++)
        for (int rot = 0; rot < 2; rot++) {  // rot 1: another code at every position (code + position)
          for (int i = 0; i < 256 * 16; i++) {
            rng = rng * 1664525u + 1013904223u;
            const uint32_t c = rot ? (code + (uint32_t)i) & 15u : code;
            in[i] = ((base + c) << 24) | (rng >> 8);
          }
          std::fill(block.begin(), block.end(), 0);
          std::fill(plane.begin(), plane.end(), 0);
          p26::pack_block(fmt, in.data(), base, block.data(), plane.data());
          if (fmt == PACK_FMT26 && !rot && code < 4)
            for (uint8_t b : plane) bad += b != 0;  // codes below 4 leave no escape bits
          p26::unpack_block(fmt, block.data(), plane.data(), base, out.data());
          for (int i = 0; i < 256 * 16; i++, checked++) bad += in[i] != out[i];
        }
  for (int64_t J : {1, 4, 9, 16, 17, 40, 200})
    bad += pack_tile_bytes(PACK_FMT28, J) - pack_tile_bytes(PACK_FMT26, J) != (J + 15) / 16 * 1024;
  printf("pack26 selfcheck: %ld words round-tripped, %ld mismatches\n", checked, bad);
  return bad ? 1 : 0;
}
