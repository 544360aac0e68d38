// The arithmetic of the one-query attention kernels, written once: attn_decode_kernel (attention.hip), attn_decode_draft_kernel,
// one_row_attention (attn_ragged.hip), attn_decode_split_kernel and attn_decode_split_draft_kernel with their merge launches.
// The product needs these to agree to the bit (a drafted row must equal the one-row step, a one-row prefill segment the token
// step, the split view itself across its forms); they do because each expression below exists once.  A kernel keeps its own grid,
// LDS layout, exits and barriers, and decides which rows it reads and writes; what differs inside a shared piece comes in as a
// template parameter or a callable that inlines away.  No function here knows which kernel calls it.
// Every operand order, every 0.f / 0u for a masked key and the place of `* scale` are part of the contract: the build contracts
// a * b + c (-ffp-contract=fast), so regrouping an expression changes bits.  Which product of the rotation's a * b + c * d is
// fused is the optimiser's choice and moved with the code around it, so rope_pair spells its two fused multiply-adds out, in the
// form these kernels always compiled to.  The sums s += q k and o += p v have one contraction only; they stay expressions (the
// builtin costs attn_decode_kernel two VGPRs), and o0 | o1 must be the caller's plain locals: handed elements of an array, the
// vectoriser packs the products apart from the sums and they are no longer fused.
#pragma once
#include "common.h"

#define OQ_WAVES 16            // waves that deal the keys of a (row, head) among themselves in the unsplit kernels
#define OQ_SPLIT_THREADS 256   // the split kernels: four waves per chunk
#define OQ_SPLIT_PSTRIDE 132   // floats per (row, head, chunk) partial record: o[128] | m | l | 2 pad (16-byte aligned records)

// One rotate-half pair, x1 c - x2 s and x2 c + x1 s, each one product rounded and one FMA -- the form rope_kernel
// (elementwise.hip) compiles to, written out so that the bits do not depend on what the optimiser makes of the code around the call.
__device__ __forceinline__ void rope_pair(float x1, float x2, float c, float s, float& lo, float& hi) {
#pragma clang fp contract(off)
  lo = __builtin_fmaf(x1, c, -(x2 * s));
  hi = __builtin_fmaf(x2, c, x1 * s);
}
// Rotary of one 4-pair item (modeling_llama.py:186-195): elements e[0..3] and e[half..half+3] of a head row, which are its
// dims i .. i+3 and i+half .. i+half+3, at position pos of the [max_pos, half] tables cs | sn; fp32 rotate-half, one rounding to
// bf16.  Where oa | ob go is the caller's business.
__device__ __forceinline__ void oq_rope4(const bf16_t* e, int half, const float* cs, const float* sn, int pos, int i, short4_t& oa,
                                         short4_t& ob) {
  const float4_t c4 = *reinterpret_cast<const float4_t*>(cs + (size_t)pos * half + i);
  const float4_t s4 = *reinterpret_cast<const float4_t*>(sn + (size_t)pos * half + i);
  const short4_t a = *reinterpret_cast<const short4_t*>(e);
  const short4_t bb = *reinterpret_cast<const short4_t*>(e + half);
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    float lo, hi;
    rope_pair(bf2f((bf16_t)a[t]), bf2f((bf16_t)bb[t]), c4[t], s4[t], lo, hi);
    oa[t] = (short)f2bf(lo);
    ob[t] = (short)f2bf(hi);
  }
}

// One key's score: 16 lanes share the key, 8 dims each (qf is the lane's slice of q * scale); every one of them gets the sum.
__device__ __forceinline__ float oq_score(const float (&qf)[8], short8_t kv) {
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) s += qf[e] * bf2f((bf16_t)kv[e]);
  s += __shfl_xor(s, 1, 64);
  s += __shfl_xor(s, 2, 64);
  s += __shfl_xor(s, 4, 64);
  s += __shfl_xor(s, 8, 64);
  return s;
}

// Scores of keys 0 .. len-1 into sc, `wave`'s share of OQ_WAVES: 4 keys per wave and pass, 64 per workgroup pass, two passes'
// loads in flight.  key(j, j0) loads this lane's 16 bytes of key j; j0 (uniform) is the first key of the pass pair.
template <class Key>
__device__ __forceinline__ void oq_scores(float* sc, const float (&qf)[8], bool dim_ok, int len, int wave, int lane, Key key) {
  const int sub = lane & 15, kq = lane >> 4;
  for (int j0 = 0; j0 < len; j0 += 2 * OQ_WAVES * 4) {
    short8_t kv[2];
    int jj[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      jj[u] = j0 + u * OQ_WAVES * 4 + wave * 4 + kq;
      kv[u] = (short8_t){0, 0, 0, 0, 0, 0, 0, 0};
      if (jj[u] < len && dim_ok) kv[u] = key(jj[u], j0);
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const float s = oq_score(qf, kv[u]);
      if (sub == 0 && jj[u] < len) sc[jj[u]] = s;
    }
  }
}

// Softmax statistics of n scores, one wave for itself: lane-stride max, lane-stride sum of e^(s - mx).  KEEP: the weight
// e^(s - mx) replaces the score (a caller that reads each weight more than once).
template <bool KEEP = false>
__device__ __forceinline__ void oq_softmax_stats(float* sc, int n, int lane, float& mx, float& sum) {
  mx = -INFINITY;
  for (int j = lane; j < n; j += 64) mx = fmaxf(mx, sc[j]);
  mx = wave_max(mx);
  sum = 0.f;
  for (int j = lane; j < n; j += 64) {
    const float w = __expf(sc[j] - mx);
    sum += w;
    if (KEEP) sc[j] = w;
  }
  sum = wave_sum(sum);
}

// N value rows j, j + OQ_WAVES, ... and their weights, the loads issued together.  TAIL: a key at or past len gives a zero
// weight and a zero value.  v(j) loads the lane's two dims of value row j.
template <int N, bool TAIL, class V>
__device__ __forceinline__ void oq_pv_load(const float* sc, float mx, int len, int j, bool own, V v, unsigned (&vv)[N],
                                           float (&pj)[N]) {
#pragma unroll
  for (int u = 0; u < N; ++u) {
    const int jk = j + OQ_WAVES * u;
    const bool ok = !TAIL || jk < len;
    vv[u] = (own && ok) ? v(jk) : 0u;
    pj[u] = ok ? __expf(sc[jk] - mx) : 0.f;
  }
}
template <int N>
__device__ __forceinline__ void oq_pv_add(const unsigned (&vv)[N], const float (&pj)[N], float& o0, float& o1) {
#pragma unroll
  for (int u = 0; u < N; ++u) {
    o0 += pj[u] * bf2f((bf16_t)(vv[u] & 0xffffu));
    o1 += pj[u] * bf2f((bf16_t)(vv[u] >> 16));
  }
}
// o = sum_j p_j V[j] over wave's keys wave, wave + OQ_WAVES, ...: eight row loads in flight, then a remainder of up to seven
// issued together.  A group of eight whose last key lies below `plain_below` (uniform over the wave) loads with vplain, which
// need not handle any other key; everything else with v.
template <class VPlain, class V>
__device__ __forceinline__ void oq_pv(const float* sc, float mx, int len, int wave, bool own, int plain_below, VPlain vplain, V v,
                                      float& o0, float& o1) {
  o0 = 0.f, o1 = 0.f;
  int j = wave;
  for (; j + 7 * OQ_WAVES < len; j += 8 * OQ_WAVES) {
    unsigned vv[8];
    float pj[8];
    if (j + 7 * OQ_WAVES < plain_below) oq_pv_load<8, false>(sc, mx, len, j, own, vplain, vv, pj);
    else oq_pv_load<8, false>(sc, mx, len, j, own, v, vv, pj);
    oq_pv_add(vv, pj, o0, o1);
  }
  unsigned vv[7];
  float pj[7];
  oq_pv_load<7, true>(sc, mx, len, j, own, v, vv, pj);
  oq_pv_add(vv, pj, o0, o1);
}
template <class V>
__device__ __forceinline__ void oq_pv(const float* sc, float mx, int len, int wave, bool own, V v, float& o0, float& o1) {
  oq_pv(sc, mx, len, wave, own, len, v, v, o0, o1);     // one source for every key: the test folds into the loop's own
}

// The OQ_WAVES partial outputs of part[w][128] summed in wave order, normalised and stored as two bf16 at dst (one wave's work).
__device__ __forceinline__ void oq_sum_store(const float* part, int lane, float sum, int len, bf16_t* dst) {
  const float inv = len > 0 ? 1.f / sum : 0.f;
  float r0 = 0.f, r1 = 0.f;
#pragma unroll
  for (int w = 0; w < OQ_WAVES; ++w) {
    r0 += part[w * 128 + 2 * lane];
    r1 += part[w * 128 + 2 * lane + 1];
  }
  *reinterpret_cast<unsigned*>(dst) = pack_bf2(r0 * inv, r1 * inv);
}

// Split view, one wave: a chunk's record from the four waves' partial outputs po[w * wstride + d], summed in fixed order.
__device__ __forceinline__ void oq_split_record(float* rec, const float* po, int wstride, int lane, bool own, float mx, float sum) {
  if (own) {
    const float* a = po + 2 * lane;
    rec[2 * lane] = ((a[0] + a[wstride]) + a[2 * wstride]) + a[3 * wstride];
    rec[2 * lane + 1] = ((a[1] + a[wstride + 1]) + a[2 * wstride + 1]) + a[3 * wstride + 1];
  }
  if (lane == 0) {
    rec[128] = mx;
    rec[129] = sum;
  }
}
// Split view, one wave: merge the nc chunk records at rec in chunk order, o = sum_c e^(m_c - M) o_c / sum_c e^(m_c - M) l_c,
// and store the lane's two bf16 of the D-wide head row `orow`.
__device__ __forceinline__ void oq_split_merge(const float* rec, int nc, int lane, int D, bf16_t* orow) {
  float M = -INFINITY;
  for (int c = 0; c < nc; ++c) M = fmaxf(M, rec[(size_t)c * OQ_SPLIT_PSTRIDE + 128]);
  float L = 0.f, o0 = 0.f, o1 = 0.f;
  const bool own = 2 * lane < D;
  for (int c = 0; c < nc; ++c) {
    const float* r = rec + (size_t)c * OQ_SPLIT_PSTRIDE;
    const float w = __expf(r[128] - M);
    L += w * r[129];
    if (own) {
      o0 += w * r[2 * lane];
      o1 += w * r[2 * lane + 1];
    }
  }
  if (own) {
    const float inv = nc > 0 ? 1.f / L : 0.f;
    *reinterpret_cast<unsigned*>(orow + 2 * lane) = pack_bf2(o0 * inv, o1 * inv);
  }
}

// ---- host side
static inline int oq_split_chunk(int chunk) { return chunk == 0 ? 128 : chunk; }
static inline bool oq_split_chunk_ok(int ch) { return ch == 128 || ch == 256 || ch == 512; }

// The K-row step entries' pointer, stride and alignment rules (qkv [G*K, ld_qkv], cache rows [k | v], out [G*K, ldo]); `nrow`
// may be null unless `rows`.  false: MH_ERR_ARG.
static inline bool oq_step_args_ok(const void* qkv, long ld_qkv, const void* cache, long cache_bstride, long ld_cache,
                                   const int* pos, const int* live, const int* nrow, bool rows, const float* cos_tab,
                                   const float* sin_tab, const void* out, long ldo, int G, int K, int H, int D) {
  if (!qkv || !cache || !pos || !live || !cos_tab || !sin_tab || !out || (rows && !nrow)) return false;
  if (ld_qkv % 8 || ld_cache % 8 || cache_bstride % 8 || ldo % 4 || ld_qkv < 3L * H * D || ld_cache < 2L * H * D ||
      ldo < (long)H * D)
    return false;
  if ((uintptr_t)qkv % 16 || (uintptr_t)cache % 16 || (uintptr_t)cos_tab % 16 || (uintptr_t)sin_tab % 16 || (uintptr_t)out % 8 ||
      (uintptr_t)pos % 4 || (uintptr_t)live % 4 || (uintptr_t)nrow % 4)
    return false;
  return (long)G * K * H <= 0x7fffffffL;
}
