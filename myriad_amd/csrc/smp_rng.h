// What the token sampler (sample.hip) and the beam sampler (beam_sample.hip) share: Philox4x32-10, the order-preserving
// fp32 <-> u32 map of the radix select, and the wave / block prefix sums over SNT threads.
#pragma once
#include "common.h"

#define SNT 1024                // threads per row
#define SNW (SNT / 64)
#define MH_SAMPLE_CAP 1024      // most candidates the sort takes; a larger tied top-k set is reported (kept = -1 / the overflow flag)

// ---------------------------------------------------------------------------------------------------- Philox4x32-10
__device__ __forceinline__ void philox4x32_10(unsigned c[4], unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c[0];
    const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c[2];
    const unsigned hi0 = (unsigned)(p0 >> 32), lo0 = (unsigned)p0, hi1 = (unsigned)(p1 >> 32), lo1 = (unsigned)p1;
    c[0] = hi1 ^ c[1] ^ k0;
    c[1] = lo1;
    c[2] = hi0 ^ c[3] ^ k1;
    c[3] = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

// order-preserving fp32 <-> u32 map: a > b (floats) <=> key(a) > key(b) (unsigned), and a == b <=> key(a) == key(b): -0.0 takes
// +0.0's key (a test of its bits, which no float identity the compiler may fold can undo), so the two zeros are one value for
// the threshold, the tie set and the sort.  smp_unkey gives +0.0 back for either.  NaN has no place in the order: a sign-clear
// NaN keys above +inf, a sign-set one below -inf, so callers map NaN away first (smp_key_draw, or the beam sampler's w == w).
#define SMP_KEY_NINF 0x007fffffu  // smp_key(-inf)
__device__ __forceinline__ unsigned smp_key(float f) {
  unsigned u = __float_as_uint(f);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// the key a logit draws with: NaN of either sign (exponent all ones, mantissa non-zero) is -inf
__device__ __forceinline__ unsigned smp_key_draw(float f) {
  return (__float_as_uint(f) & 0x7fffffffu) > 0x7f800000u ? SMP_KEY_NINF : smp_key(f);
}
__device__ __forceinline__ float smp_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// inclusive prefix sum over the 64 lanes of a wave
template <typename T>
__device__ __forceinline__ T smp_wave_scan(T v) {
  const int l = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T n = __shfl_up(v, o, 64);
    if (l >= o) v += n;
  }
  return v;
}
// inclusive prefix sum over the block (thread order); `wsum` is SNW entries of LDS
template <typename T>
__device__ __forceinline__ T smp_block_scan(T v, T* wsum) {
  v = smp_wave_scan(v);
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  __syncthreads();
  if (l == 63) wsum[w] = v;
  __syncthreads();
  T base = 0;
  for (int i = 0; i < w; ++i) base += wsum[i];
  return v + base;
}
