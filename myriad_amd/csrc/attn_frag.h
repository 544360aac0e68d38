// MFMA operand fragments out of row-major bf16 LDS images (row stride RS elements), shared by attn_seq.hip and attn_full.hip,
// and the fp32 -> bf16 packing of an accumulator pair into a B operand (attention.hip too).  lr = lane & 15, lg = lane >> 4.
#pragma once
#include "common.h"

typedef __attribute__((address_space(3))) short4_t lds_short4_t;

// A operand of the X^T.Y products: X is a key-major (row-major) LDS image, the operand row is column d = 16*jd + lr
// of X and its 8 reduction elements are rows {32c + 4g + r} U {32c + 16 + 4g + r}.  ds_read_b64_tr_b16: lane i of a
// 16-lane group addresses row (i >> 2), columns 4*(i & 3).. of a [4][16] block and receives column i of that block
// (tools/micro/tr_probe.hip).
template <int RS>
__device__ __forceinline__ short8_t lds_frag_tr(const bf16_t* img, int jd, int c, int lr, int lg) {
  const bf16_t* p = img + (32 * c + 4 * lg + (lr >> 2)) * RS + 16 * jd + 4 * (lr & 3);
  const short4_t a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_short4_t*)p);
  const short4_t b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_short4_t*)(p + 16 * RS));
  return (short8_t){a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}
// A operand of the X.Y^T products: row 16*j + lr of the image, k-chunk kk*32 + lg*8
template <int RS>
__device__ __forceinline__ short8_t lds_frag_rm(const bf16_t* img, int j, int kk, int lr, int lg) {
  return *reinterpret_cast<const short8_t*>(img + (16 * j + lr) * RS + kk * 32 + lg * 8);
}
__device__ __forceinline__ short8_t pack8(const float4_t& a, const float4_t& b) {
  return (short8_t){(short)f2bf(a[0]), (short)f2bf(a[1]), (short)f2bf(a[2]), (short)f2bf(a[3]),
                    (short)f2bf(b[0]), (short)f2bf(b[1]), (short)f2bf(b[2]), (short)f2bf(b[3])};
}
