// The 64 x 64 tile geometry of the tiled attention kernels (attention.hip, attn_ragged.hip): LDS image strides and the MFMA
// A-operand fragments read out of them.  lr = lane & 15, lg = lane >> 4.
#pragma once
#include "attn_frag.h"

#define TQ 64
#define TK 64

template <int DP>
struct Lds {
  static constexpr int ROW = DP + 8;   // row-major tile row stride (elements)
  static constexpr int TROW = TK + 8;  // transposed tile row stride (elements)
  static constexpr int RM_BYTES = 64 * ROW * 2;
  static constexpr int TR_BYTES = DP * TROW * 2;
};

// A-operand fragment from a row-major tile: row = 16*j + (lane&15), k-chunk (kk*4 + lane>>4)
template <int DP>
__device__ __forceinline__ short8_t frag_rm(const bf16_t* lds, int j, int kk, int lr, int lg) {
  return *reinterpret_cast<const short8_t*>(lds + (16 * j + lr) * Lds<DP>::ROW + kk * 32 + lg * 8);
}
// A-operand fragment from a transposed tile: row d = 16*jd + (lane&15); reduction elements
// {32c+4g+r} U {32c+16+4g+r}, r=0..3 -- matches the register order of a packed S^T / S accumulator pair.
template <int DP>
__device__ __forceinline__ short8_t frag_tr(const bf16_t* lds, int jd, int c, int lr, int lg) {
  const bf16_t* p = lds + (16 * jd + lr) * Lds<DP>::TROW + 32 * c + 4 * lg;
  const short4_t a = *reinterpret_cast<const short4_t*>(p);
  const short4_t b = *reinterpret_cast<const short4_t*>(p + 16);
  return (short8_t){a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}

#define NEG_INF (-__builtin_inff())
