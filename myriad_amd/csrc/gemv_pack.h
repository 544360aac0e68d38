// The stream order of the decode step's packed weight copies, shared by their writers (gemv.hip: mh_gemv_pack /
// mh_gemv_pack_fp8 / mh_gemv_pack_fp4; lora_merge.hip: the merged q / v LoRA copies), so every writer produces the same bytes.
#pragma once
#include "common.h"

// waves per workgroup of the packed kernels: 8 when N / 16 workgroups under-fill the chip, else 4 (gemv.hip's launch rule)
static inline int gv_packed_nw(int N) { return ((N + 15) / 16 < 512) ? 8 : 4; }

// The layout of a packed copy of W [N, K] whose steps are kstep deep (64: bf16 and fp8, 128: fp4): `blocks` column blocks of 16
// rows, each split over nw waves of `per` steps (the last wave's tail past K is zero padding), a step being 1024 elements;
// per4: the scale dwords of a wave's fp4 steps, four steps each.  Every packer, element count and launcher takes it from here.
struct GvLayout { int nw, per, per4, blocks; };
static inline GvLayout gv_layout(int N, int K, int kstep) {
  GvLayout L;
  L.nw = gv_packed_nw(N);
  L.per = (K / kstep + L.nw - 1) / L.nw;
  L.per4 = (L.per + 3) / 4;
  L.blocks = (N + 15) / 16;
  return L;
}

// fp32 -> OCP e4m3fn code, round to nearest even; |x| <= 448, not NaN
__device__ __forceinline__ unsigned f32_to_e4m3fn(float x) {
  const unsigned u = __float_as_uint(x), sign = (u >> 24) & 0x80u, a = u & 0x7fffffffu;
  if (a < 0x3c800000u)                                              // |x| < 2^-6: subnormal codes m * 2^-9 (m = 8 is 2^-6)
    return sign | (unsigned)rintf(__uint_as_float(a) * 512.f);      // exact scaling, rintf rounds half to even
  const unsigned r = (a + 0x7ffffu + ((a >> 20) & 1u)) >> 20;       // 3 mantissa bits, half to even (a carry bumps the exponent)
  return sign | (r - (120u << 3));                                  // rebias 127 -> 7
}

// MXFP4 (OCP microscaling, e2m1 codes, 32 weights per block): the scale byte of a block whose largest |w| has the biased bf16
// exponent field E (0 for a zero or subnormal maximum): floor(log2 amax) - emax(e2m1), clamped below at 2 so that every
// code * 2^(b-127) is zero or a normal bf16; at most 252
__device__ __forceinline__ int mxfp4_scale_byte(int E) { return E - 2 > 2 ? E - 2 : 2; }

// bf16 bits of a finite w -> e2m1 code (sign | magnitude index into {0, 0.5, 1, 1.5, 2, 3, 4, 6}) of w / 2^(b-127): nearest, ties
// to the even code, saturated at +-6, the sign bit copied (zeros included).  Integer arithmetic on the bits: no fp32 mode bears
// on it.  |w| = sig * 2^(max(e,1) - 134), so 4 |w| / X = sig / 2^n with n = b + 5 - max(e,1) >= 3 (b is the block's scale byte,
// so e - b <= 2); the code is the number of midpoints 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5 passed, a tie passing only towards
// an even code.
__device__ __forceinline__ unsigned bf16_to_e2m1(unsigned bits, int b) {
  const int a = bits & 0x7fff, e = a >> 7;
  const int sig = e ? (128 | (a & 127)) : (a & 127);
  const int n = b + 5 - (e ? e : 1);
  unsigned code = 0;
  if (n <= 8)                                                        // sig < 256: from n = 9 on, 4 |w| / X < 1/2 and the code is 0
    code = (sig > (1 << n)) + (sig >= (3 << n)) + (sig > (5 << n)) + (sig >= (7 << n)) + (sig > (10 << n)) + (sig >= (14 << n)) +
           (sig > (20 << n));
  return ((bits >> 12) & 8u) | code;
}
