// Split-KV decode attention (one query per (batch, head) over a long KV cache): the chat session's token step.
//
// attn_decode_kernel (attention.hip) runs ONE workgroup per (b, h): at batch 1 that is 32 workgroups on 256 CUs, each
// streaming its head's whole K|V history alone.  Here the keys are cut into chunks of CH: grid (ceil(T_cap / CH), B*H), every
// workgroup scores its chunk, and writes the chunk's softmax statistics and un-normalised output (m, l, o[D]) in fp32; a
// second, small launch merges the chunks of a (b, h) in chunk order and writes bf16 o.  Fixed order everywhere: the result is
// the same bits from run to run.
//
// Same contract as mh_attn_decode_rope, except that q is NOT rotated in place: many workgroups read the one q, so each rotates
// it in registers (same arithmetic: fp32 rotate-half, one rounding to bf16, then * scale).  The workgroup whose chunk holds
// row pos_dev[0] writes the new cache row [k | v] (bits as mh_attn_decode_rope writes them) and uses its LDS copy of that key
// and value for its own scores: no workgroup reads a row another one writes in the same launch.  kv_len lives in device memory,
// so one launch replays from a hipGraph while the context grows; a chunk that starts at or after kv_len[b] exits at once.
//
// ROWS (mh_attn_decode_rope_split_rows, the decode slots' form): per-row state as in mh_attn_decode_rope_rows.  Row b appends at
// cache row pos[b] (its rotary position too) instead of the shared pos_dev[0], and a row with live[b] == 0 is skipped: its chunk
// workgroups exit before they touch qkv, the cache or the partials, and the merge writes a zero out row without reading a
// record.  live[b] is uniform over a workgroup, so the exit is a scalar branch.  Everything per (row, head) -- chunking, score
// and softmax order, the four-wave sum, the in-order merge -- is the ROWS = false code, so a live row has the bits of
// mh_attn_decode_rope_split at B = 1 on that row with pos_dev[0] = pos[b].  One difference from the non-split rows kernel: that
// one rotates q in place in qkv, this one leaves qkv alone (nothing downstream reads q after the attention).
//
// The arithmetic is attn_one_query.h's, which attn_decode_split_draft.hip (the K-row verify step of draft decoding on this view)
// calls per row too.
#include "attn_one_query.h"

struct SplitParams {
  const bf16_t* qkv;
  long ld_qkv;
  bf16_t* cache;
  long cache_bs, ld_cache;
  const int* pos;
  const int* pos_dev;
  const int* kv_len;
  const int* live;
  const float* cs;
  const float* sn;
  float* part;
  bf16_t* out;
  long ldo;
  int B, H, D, T_cap, nch;
  float scale;
};

template <int CH, bool ROWS>
__global__ __launch_bounds__(OQ_SPLIT_THREADS) void attn_decode_split_kernel(SplitParams p) {
  __shared__ float sc[CH];                 // chunk scores
  __shared__ float po[4][128];             // per-wave partial outputs
  __shared__ float qs[128];                // rotated q (bf16-rounded) * scale
  __shared__ bf16_t knew[128], vnew[128];  // the new row's k (rotated) and v, owner chunk only
  const int c = blockIdx.x, bh = blockIdx.y;
  const int b = bh / p.H, h = bh % p.H;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int D = p.D, W = p.H * D;
  if (ROWS && p.live[b] == 0) return;              // idle slot: nothing read, nothing written
  int len = p.kv_len[b];
  len = len < p.T_cap ? len : p.T_cap;
  const int j0 = c * CH;
  const int prow = ROWS ? p.pos[b] : p.pos_dev[0];
  const bool owner = prow >= j0 && prow < j0 + CH && prow < p.T_cap;
  if (j0 >= len && !owner) return;
  const int n = len - j0 < CH ? len - j0 : CH;   // keys of this chunk (<= 0: the owner of a row past kv_len[b])

  // rotary (modeling_llama.py:186-195): q always, k | v of the new token by the owner only
  const int half = D >> 1, items = half >> 2;
  const bf16_t* src = p.qkv + (size_t)b * p.ld_qkv;
  bf16_t* crow = p.cache + (size_t)b * p.cache_bs + (size_t)prow * p.ld_cache;
  if (tid < 2 * items) {
    const int which = tid / items, i = (tid % items) * 4;
    if (which == 0 || owner) {
      const bf16_t* e = src + which * W + h * D + i;
      const int ps = p.pos[b];
      short4_t oa, ob;
      oq_rope4(e, half, p.cs, p.sn, ps, i, oa, ob);
      if (which == 0) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          qs[i + t] = bf2f((bf16_t)oa[t]) * p.scale;
          qs[i + half + t] = bf2f((bf16_t)ob[t]) * p.scale;
        }
      } else {
        *reinterpret_cast<short4_t*>(crow + h * D + i) = oa;
        *reinterpret_cast<short4_t*>(crow + h * D + i + half) = ob;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          knew[i + t] = (bf16_t)oa[t];
          knew[i + half + t] = (bf16_t)ob[t];
        }
      }
    }
  } else if (owner && tid < 2 * items + (D >> 3)) {
    const int cc = (tid - 2 * items) * 8;
    const short8_t v8 = *reinterpret_cast<const short8_t*>(src + 2 * W + h * D + cc);
    *reinterpret_cast<short8_t*>(crow + W + h * D + cc) = v8;
#pragma unroll
    for (int t = 0; t < 8; ++t) vnew[cc + t] = (bf16_t)v8[t];
  }
  __syncthreads();
  if (n <= 0) return;                            // the owner of a row no query of this batch row attends to

  const bf16_t* kp = p.cache + (size_t)b * p.cache_bs + (size_t)j0 * p.ld_cache + h * D;
  const bf16_t* vp = kp + W;
  const int lrow = prow - j0;                    // the new row inside this chunk (owner), else out of [0, CH)

  // phase 1: scores.  16 lanes per key (8 dims each), 16 keys per 256-thread pass, 8 passes' loads in flight
  const int sub = lane & 15, kq = lane >> 4;
  const bool dim_ok = sub * 8 < D;
  float qf[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) qf[e] = dim_ok ? qs[sub * 8 + e] : 0.f;
  constexpr int PASSES = CH / 16, UNR = PASSES < 8 ? PASSES : 8;
  for (int u0 = 0; u0 < PASSES; u0 += UNR) {
    short8_t kv[UNR];
    int jj[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      jj[u] = (u0 + u) * 16 + wave * 4 + kq;
      kv[u] = (short8_t){0, 0, 0, 0, 0, 0, 0, 0};
      if (jj[u] < n && jj[u] != lrow && dim_ok) kv[u] = *reinterpret_cast<const short8_t*>(kp + (size_t)jj[u] * p.ld_cache + sub * 8);
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      if (jj[u] == lrow && dim_ok) kv[u] = *reinterpret_cast<const short8_t*>(knew + sub * 8);
      const float s = oq_score(qf, kv[u]);
      if (sub == 0 && jj[u] < n) sc[jj[u]] = s;
    }
  }
  __syncthreads();
  // phase 2: the chunk's softmax statistics (every wave for itself)
  float mx, sum;
  oq_softmax_stats(sc, n, lane, mx, sum);
  // phase 3: o = sum_j p_j V[j]; lane owns dims 2*lane, 2*lane+1; wave w takes keys w, w+4, ...; 8 row loads in flight
  float o0 = 0.f, o1 = 0.f;
  const bool own = 2 * lane < D;
  for (int j = wave; j < n; j += 32) {
    unsigned vv[8];
    float pj[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int jr = j + 4 * u;
      const bool ok = jr < n;
      vv[u] = 0u;
      if (own && ok) vv[u] = jr == lrow ? *reinterpret_cast<const unsigned*>(vnew + 2 * lane)
                                        : *reinterpret_cast<const unsigned*>(vp + (size_t)jr * p.ld_cache + 2 * lane);
      pj[u] = ok ? __expf(sc[jr] - mx) : 0.f;
    }
    oq_pv_add(vv, pj, o0, o1);
  }
  po[wave][2 * lane] = o0;
  po[wave][2 * lane + 1] = o1;
  __syncthreads();
  if (wave == 0) oq_split_record(p.part + ((size_t)bh * p.nch + c) * OQ_SPLIT_PSTRIDE, &po[0][0], 128, lane, own, mx, sum);
}

// merge the chunks of one (b, h) in chunk order: o = sum_c e^(m_c - M) o_c / sum_c e^(m_c - M) l_c
template <int CH, bool ROWS>
__global__ __launch_bounds__(64) void attn_decode_combine_kernel(SplitParams p) {
  const int bh = blockIdx.x, b = bh / p.H, h = bh % p.H, lane = threadIdx.x;
  if (ROWS && p.live[b] == 0) {                    // idle slot: a zero row, no partial record read
    if (2 * lane < p.D) *reinterpret_cast<unsigned*>(p.out + (size_t)b * p.ldo + h * p.D + 2 * lane) = 0u;
    return;
  }
  int len = p.kv_len[b];
  len = len < p.T_cap ? len : p.T_cap;
  const int nc = len > 0 ? (len + CH - 1) / CH : 0;
  oq_split_merge(p.part + (size_t)bh * p.nch * OQ_SPLIT_PSTRIDE, nc, lane, p.D, p.out + (size_t)b * p.ldo + h * p.D);
}

extern "C" long mh_attn_decode_split_ws_floats(int B, int H, int T_cap, int chunk) {
  const int ch = oq_split_chunk(chunk);
  if (B <= 0 || H <= 0 || T_cap <= 0 || !oq_split_chunk_ok(ch)) return -1;
  return (long)B * H * ((T_cap + ch - 1) / ch) * OQ_SPLIT_PSTRIDE;
}

template <int CH, bool ROWS>
static int launch_split(const SplitParams& p, hipStream_t s) {
  hipLaunchKernelGGL((attn_decode_split_kernel<CH, ROWS>), dim3(p.nch, p.B * p.H), dim3(OQ_SPLIT_THREADS), 0, s, p);
  MH_CHECK_LAUNCH();
  hipLaunchKernelGGL((attn_decode_combine_kernel<CH, ROWS>), dim3(p.B * p.H), dim3(64), 0, s, p);
  MH_CHECK_LAUNCH();
  return MH_OK;
}

// the two entries: pos_dev (one shared cache row) for ROWS = false, live (per-row state) for ROWS = true
template <bool ROWS>
static int split_entry(const void* qkv, long ld_qkv, void* cache, long cache_bstride, long ld_cache, const int* pos, const int* pos_dev,
                       const int* kv_len, const int* live, const float* cos_tab, const float* sin_tab, void* out, long ldo,
                       float* partials, long partials_floats, int B, int H, int D, int T_cap, int chunk, float scale,
                       hipStream_t stream) {
  if (B <= 0) return MH_OK;
  if (!qkv || !cache || !pos || !(ROWS ? live : pos_dev) || !kv_len || !cos_tab || !sin_tab || !out || !partials || H <= 0)
    return MH_ERR_ARG;
  if (D % 8 || D <= 0 || D > 128 || (D >> 1) % 4 || ld_qkv % 8 || ld_cache % 8 || cache_bstride % 8 || ldo % 4 || T_cap <= 0 ||
      T_cap > 8192 || ld_qkv < 3L * H * D || ld_cache < 2L * H * D || ldo < (long)H * D)
    return MH_ERR_ARG;
  const long need = mh_attn_decode_split_ws_floats(B, H, T_cap, chunk);
  if (need < 0 || partials_floats < need) return MH_ERR_ARG;
  const int ch = oq_split_chunk(chunk);
  SplitParams p = {};
  p.qkv = (const bf16_t*)qkv; p.ld_qkv = ld_qkv; p.cache = (bf16_t*)cache; p.cache_bs = cache_bstride; p.ld_cache = ld_cache;
  p.pos = pos; p.pos_dev = pos_dev; p.kv_len = kv_len; p.live = live; p.cs = cos_tab; p.sn = sin_tab; p.part = partials;
  p.out = (bf16_t*)out; p.ldo = ldo; p.B = B; p.H = H; p.D = D; p.T_cap = T_cap; p.nch = (T_cap + ch - 1) / ch; p.scale = scale;
  if (ch == 256) return launch_split<256, ROWS>(p, stream);
  if (ch == 512) return launch_split<512, ROWS>(p, stream);
  return launch_split<128, ROWS>(p, stream);
}

extern "C" int mh_attn_decode_rope_split(const void* qkv, long ld_qkv, void* cache, long cache_bstride, long ld_cache, const int* pos,
                                         const int* pos_dev, const int* kv_len, const float* cos_tab, const float* sin_tab, void* out,
                                         long ldo, float* partials, long partials_floats, int B, int H, int D, int T_cap, int chunk,
                                         float scale, hipStream_t stream) {
  return split_entry<false>(qkv, ld_qkv, cache, cache_bstride, ld_cache, pos, pos_dev, kv_len, nullptr, cos_tab, sin_tab, out, ldo,
                            partials, partials_floats, B, H, D, T_cap, chunk, scale, stream);
}

extern "C" int mh_attn_decode_rope_split_rows(const void* qkv, long ld_qkv, void* cache, long cache_bstride, long ld_cache,
                                              const int* pos, const int* kv_len, const int* live, const float* cos_tab,
                                              const float* sin_tab, void* out, long ldo, float* partials, long partials_floats, int B,
                                              int H, int D, int T_cap, int chunk, float scale, hipStream_t stream) {
  return split_entry<true>(qkv, ld_qkv, cache, cache_bstride, ld_cache, pos, nullptr, kv_len, live, cos_tab, sin_tab, out, ldo,
                           partials, partials_floats, B, H, D, T_cap, chunk, scale, stream);
}
