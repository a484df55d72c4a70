// bf16.h — the bfloat16 storage type of the resident tensor (PPALS_BF16) and the arithmetic the CPU
// tests check: the rounding of a stored value and the three-piece split of a Khatri-Rao operand.
// HIP-free: every function is __host__ __device__ under hipcc and plain C++ elsewhere.
//
// Rounding (what torch does for float64 -> bfloat16): fp64 -> fp32 round-to-nearest-even, then
// fp32 -> bf16 round-to-nearest-even. The double rounding is part of the contract: 1 + 2^-8 + 2^-30
// becomes 1.0, not 1 + 2^-7. NaN stays a (quiet) NaN, +-inf stay infinite, fp32 subnormals round
// like every other value. On the device the second step is the hardware cast (v_cvt_pk_bf16_f32 on
// gfx950); on the host it is the integer form of the same rounding.
//
// Split: an fp64 value x = hi + mid + lo + e, each piece a bf16 value, |e| <= 2^-24 |x| (for x
// whose pieces stay in the normal range). A bf16 x bf16 product is exact in fp32, so a tensor
// stored in bf16 contracted against (hi, mid, lo) on the bf16 matrix cores sees the operand to
// ~24 significant bits, as the fp32 path sees its fp32-rounded operand.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PPALS_HD __host__ __device__ inline
#else
#define PPALS_HD inline
#endif

namespace ppals {

PPALS_HD float bf16_bits_to_float(uint16_t b) {
  const uint32_t u = (uint32_t)b << 16;
  float f;
  __builtin_memcpy(&f, &u, 4);
  return f;
}

// fp32 -> bf16 bits, round to nearest even (NaN -> quiet NaN of the same sign)
PPALS_HD uint16_t bf16_bits_from_float(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
  // (opaque to the optimiser: it would otherwise fuse an fp64 -> fp32 -> bf16 chain into ONE
  // rounding of the fp64 value, which is not what torch stores)
  __asm__ volatile("" : "+v"(f));
  const __bf16 h = (__bf16)f;
  uint16_t b;
  __builtin_memcpy(&b, &h, 2);
  return b;
#else
  uint32_t u;
  __builtin_memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x0040u);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
#endif
}

// fp64 -> bf16 bits: fp64 -> fp32 (RNE) -> bf16 (RNE)
PPALS_HD uint16_t bf16_bits_from_double(double d) { return bf16_bits_from_float((float)d); }

// the three bf16 pieces of x: hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid); the
// differences are exact in fp64
PPALS_HD void bf16_split3(double x, uint16_t *hi, uint16_t *mid, uint16_t *lo) {
  *hi = bf16_bits_from_double(x);
  const double r1 = x - (double)bf16_bits_to_float(*hi);
  *mid = bf16_bits_from_double(r1);
  const double r2 = r1 - (double)bf16_bits_to_float(*mid);
  *lo = bf16_bits_from_double(r2);
}

// The tensor element type of PPALS_BF16 storage: 2 bytes, trivially constructible (it lives in LDS
// tiles), converting like the float / double casts the kernels already write: (bf16s)x rounds,
// (double)v and (float)v widen exactly.
struct bf16s {
  uint16_t u;
  bf16s() = default;
  PPALS_HD explicit bf16s(double d) : u(bf16_bits_from_double(d)) {}
  PPALS_HD explicit bf16s(float f) : u(bf16_bits_from_float(f)) {}
  PPALS_HD explicit operator float() const { return bf16_bits_to_float(u); }
  PPALS_HD explicit operator double() const { return (double)bf16_bits_to_float(u); }
};
static_assert(sizeof(bf16s) == 2, "bf16s is two bytes");

}  // namespace ppals

#undef PPALS_HD
