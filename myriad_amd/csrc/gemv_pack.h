// The stream order of the decode step's packed weight copies, shared by their writers (gemv.hip: mh_gemv_pack /
// mh_gemv_pack_fp8; lora_merge.hip: the merged q / v LoRA copies), so every writer produces the same bytes.
#pragma once
#include "common.h"

// waves per workgroup of the packed kernels: 8 when N / 16 workgroups under-fill the chip, else 4 (gemv.hip's launch rule,
// without the env knob)
static inline int gv_packed_nw(int N) { return ((N + 15) / 16 < 512) ? 8 : 4; }

// fp32 -> OCP e4m3fn code, round to nearest even; |x| <= 448, not NaN
__device__ __forceinline__ unsigned f32_to_e4m3fn(float x) {
  const unsigned u = __float_as_uint(x), sign = (u >> 24) & 0x80u, a = u & 0x7fffffffu;
  if (a < 0x3c800000u)                                              // |x| < 2^-6: subnormal codes m * 2^-9 (m = 8 is 2^-6)
    return sign | (unsigned)rintf(__uint_as_float(a) * 512.f);      // exact scaling, rintf rounds half to even
  const unsigned r = (a + 0x7ffffu + ((a >> 20) & 1u)) >> 20;       // 3 mantissa bits, half to even (a carry bumps the exponent)
  return sign | (r - (120u << 3));                                  // rebias 127 -> 7
}
