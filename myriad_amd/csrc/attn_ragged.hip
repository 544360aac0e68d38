// Packed prefill of several decode slots (llama.py LlamaHIP._prefill_packed): causal self-attention over R sequences of
// different lengths packed row-wise into one qkv matrix, with the rotary embedding and the KV-cache write fused in.
//
// Per segment (row0, len, slot) the one launch does what the prefill branch of _decode_block does in three on that segment as a
// B = 1 batch -- mh_rope_inplace on q and k, mh_copy3d_bf16 of k | v into the cache, mh_attn_fwd(causal) -- and its bits:
//   * the rotation is rope_kernel's arithmetic (fp32 rotate-half, one rounding to bf16), applied while loading: q into the
//     lane's B-operand registers, k into the LDS tile; qkv itself is only read;
//   * the attention is attn_fwd_kernel's: 64-query tiles, 64-key tiles in ascending order, the same MFMA order and the same
//     online-softmax updates (no bias, no dropout, no LSE);
//   * a query of a segment sees that segment's keys only: the key loop runs over the segment's own rows.
// Grid (ceil(max len / 64), R * H).  The workgroup whose query tile IS the key tile it stages (the diagonal tile, the last of
// its causal loop) also stores that tile's rotated k and v rows to cache[slot]; every key tile below len has exactly one such
// workgroup, so each cache row is written once and no workgroup reads the cache.  A workgroup whose query tile lies past its
// segment's len leaves before the first barrier on a workgroup-uniform branch.
//
// mh_attn_prefill_ragged_past (the PAST = true form of the kernel) is the same pass on top of a cached prefix: a segment is
// (row0, len, slot, past), its len rows are the NEW rows of a request whose keys 0 .. past-1 lie in cache[slot] already (rotated
// k | v, as every writer of these caches leaves them), and the bits are those of the prefill branch of _decode_block with that
// `past` (mh_attn_fwd(causal) with Sq = len over Sk = past + len keys, q_off = past).  The key loop runs over ABSOLUTE 64-key
// tiles from key 0: a staged row below past is copied from the cache, a row at or above it is qkv row key - past, rotated while
// loading; with past % 64 != 0 one tile mixes both.  No workgroup reads a cache row >= past, so workgroups need no order and
// nothing stale in the slot is seen.  New cache row past + c is written by the workgroup whose query tile owns chunk row c (that
// key always lies in its causal range), exactly once; rows below past and at or above past + len are never written.
// A segment of one row takes one_row_attention below, as mh_attn_fwd takes the decode kernel for Sq == 1.
//
// mh_attn_prefill_ragged_shared (PAST and SHARED) is the _past pass for segments that continue the SAME cached prefix: several
// segments may name one slot, with equal or different past, and the cache is only read.  The _past form reads no cache row
// >= past and takes every key at or above past from qkv (the one-row path from LDS), so its cache stores feed nothing in the
// launch: the flag drops them and changes nothing else, and a segment's out rows have the bits _past gives it alone.
#include "attn_tile.h"
#include "attn_one_query.h"

#include <algorithm>
#include <vector>

struct RaggedParams {
  const bf16_t* qkv;    // [M, ld_qkv] = [q | k | v], pre-rotary
  const int* pos;       // [M] rotary position of each packed row
  const int* seg;       // [R, 3] (row0, len, slot); the PAST form [R, 4] (row0, len, slot, past)
  bf16_t* cache;        // [n_slots][T_cap][ld_cache] rows [k | v]
  const float* cs;      // [max_pos, D / 2]
  const float* sn;
  bf16_t* o;            // [M, ldo]
  long ld_qkv, cache_bs, ld_cache, ldo;
  int M, H, D, n_slots, T_cap, max_pos;
  float scale;
  int lds_bytes;        // PAST form: the launch's dynamic LDS, which a one-row segment's scores must fit
};

// Eight rotated elements, head columns [c, c + 8), of the head starting at `head` (c % 8 == 0 and (D / 2) % 8 == 0, so the
// eight lie in one half): rope_kernel's expressions element by element (rope_pair, attn_one_query.h), out[c] = x[c] cos -
// x[c + half] sin in the first half, out[c] = x[c] cos + x[c - half] sin in the second.
__device__ __forceinline__ short8_t rope8(const bf16_t* head, int c, int half, const float* cs_row, const float* sn_row) {
  const bool first = c < half;
  const int i = first ? c : c - half;
  const short8_t a = *reinterpret_cast<const short8_t*>(head + i);
  const short8_t b = *reinterpret_cast<const short8_t*>(head + i + half);
  const float4_t c0 = *reinterpret_cast<const float4_t*>(cs_row + i), c1 = *reinterpret_cast<const float4_t*>(cs_row + i + 4);
  const float4_t s0 = *reinterpret_cast<const float4_t*>(sn_row + i), s1 = *reinterpret_cast<const float4_t*>(sn_row + i + 4);
  short8_t out;
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    const float x1 = bf2f((bf16_t)a[t]), x2 = bf2f((bf16_t)b[t]);
    const float cv = t < 4 ? c0[t & 3] : c1[t & 3], sv = t < 4 ? s0[t & 3] : s1[t & 3];
    float lo, hi;
    rope_pair(x1, x2, cv, sv, lo, hi);
    out[t] = (short)f2bf(first ? lo : hi);
  }
  return out;
}

// A segment of ONE new row on top of `past` cached keys.  mh_attn_fwd sends Sq == 1 (Sk <= 8192) to attn_decode_kernel
// (attention.hip), not to the tile kernel, so the bits the prefill branch of _decode_block gives such a segment are that kernel's:
// fp32 throughout, 16 lanes per key for the scores, every wave its own softmax statistics, the keys dealt round-robin to 16 waves
// for P.V (eight at a time, then a remainder of seven) and the 16 partial outputs summed in wave order.  Both call that arithmetic
// in attn_one_query.h; each of this workgroup's 4 waves takes 4 of the OQ_WAVES shares in turn, and the scores' LDS is reused for
// the partial outputs.  The new row's rotated k and its v are written to cache row `past` (not with SHARED, which writes no cache
// row) and kept in LDS: key `past` is read from there, so no cache row >= past is read here either.
// ONE_ROW_MAX_KEYS is mh_attn_fwd's Sq == 1 rule (Sk <= 8192): a change there must be made here too.
#define ONE_ROW_MAX_KEYS 8192
__host__ __device__ __forceinline__ int one_row_score_floats(int keys) {
  const int n = (keys + 63) & ~63;
  return n > OQ_WAVES * 128 ? n : OQ_WAVES * 128;
}
template <bool SHARED>
__device__ __forceinline__ void one_row_attention(const RaggedParams& p, char* smem, const bf16_t* xb, bf16_t* cb, int row, int past,
                                                  int h) {
  const int tid = threadIdx.x, lane = tid & 63, rw = tid >> 6;
  const int D = p.D, half = D >> 1, W = p.H * D, len = past + 1;
  float* sc = reinterpret_cast<float*>(smem);
  bf16_t* krow = reinterpret_cast<bf16_t*>(smem + (size_t)one_row_score_floats(len) * 4);
  bf16_t* vrow = krow + 128;
  int ps = p.pos[row];
  ps = ps < 0 ? 0 : (ps < p.max_pos ? ps : p.max_pos - 1);
  const float* cs_row = p.cs + (size_t)ps * half;
  const float* sn_row = p.sn + (size_t)ps * half;
  if (tid < (D >> 3)) {
    const short8_t v = rope8(xb + W, tid * 8, half, cs_row, sn_row);
    *reinterpret_cast<short8_t*>(krow + tid * 8) = v;
    if (!SHARED) *reinterpret_cast<short8_t*>(cb + (long)past * p.ld_cache + tid * 8) = v;
  } else if (tid >= 64 && tid - 64 < (D >> 3)) {
    const int c = (tid - 64) * 8;
    const short8_t v = *reinterpret_cast<const short8_t*>(xb + 2 * W + c);
    *reinterpret_cast<short8_t*>(vrow + c) = v;
    if (!SHARED) *reinterpret_cast<short8_t*>(cb + (long)past * p.ld_cache + W + c) = v;
  }
  __syncthreads();
  const bf16_t* kp = cb;
  const bf16_t* vp = cb + W;
  // phase 1: scores
  const int sub = lane & 15;
  float qf[8];
  const bool dim_ok = sub * 8 < D;
  {
    short8_t qv = {0, 0, 0, 0, 0, 0, 0, 0};
    if (dim_ok) qv = rope8(xb, sub * 8, half, cs_row, sn_row);
#pragma unroll
    for (int e = 0; e < 8; ++e) qf[e] = bf2f((bf16_t)qv[e]) * p.scale;
  }
  for (int i = 0; i < 4; ++i)
    oq_scores(sc, qf, dim_ok, len, rw * 4 + i, lane, [&](int j, int) {
      return j < past ? *reinterpret_cast<const short8_t*>(kp + (size_t)j * p.ld_cache + sub * 8)
                      : *reinterpret_cast<const short8_t*>(krow + sub * 8);
    });
  __syncthreads();
  // phase 2: softmax statistics (the same in every wave)
  float mx, sum;
  oq_softmax_stats(sc, len, lane, mx, sum);
  // phase 3: o = sum_j p_j V[j]; lane owns dims 2*lane, 2*lane+1; share w takes keys w, w+16, ...
  const bool own = 2 * lane < D;
  float po0[4], po1[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float o0, o1;
    oq_pv(sc, mx, len, rw * 4 + i, own, [&](int j) {
      return j < past ? *reinterpret_cast<const unsigned*>(vp + (size_t)j * p.ld_cache + 2 * lane)
                      : *reinterpret_cast<const unsigned*>(vrow + 2 * lane);
    }, o0, o1);
    po0[i] = o0;
    po1[i] = o1;
  }
  __syncthreads();                                 // every wave is done with the scores: their LDS takes the partial outputs
  float* part = sc;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    part[(rw * 4 + i) * 128 + 2 * lane] = po0[i];
    part[(rw * 4 + i) * 128 + 2 * lane + 1] = po1[i];
  }
  __syncthreads();
  if (rw == 0 && own) oq_sum_store(part, lane, sum, len, p.o + (long)row * p.ldo + h * D + 2 * lane);
}

template <int DP, bool PAST, bool SHARED>
__global__ __launch_bounds__(256) void attn_prefill_ragged_kernel(RaggedParams p) {
  static_assert(PAST || !SHARED, "the shared form reads a prefix: it is a PAST form");
  constexpr int SW = PAST ? 4 : 3;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* Ks = reinterpret_cast<bf16_t*>(smem);
  bf16_t* Vt = reinterpret_cast<bf16_t*>(smem + Lds<DP>::RM_BYTES);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, lg = lane >> 4;
  const int sg = blockIdx.y / p.H, h = blockIdx.y % p.H;
  const int row0 = p.seg[SW * sg], len = p.seg[SW * sg + 1], slot = p.seg[SW * sg + 2];
  const int past = PAST ? p.seg[SW * sg + 3] : 0;                // keys 0 .. past-1 are cache[slot]'s rows
  const int q0 = blockIdx.x * TQ;
  // the host entry validated its copy of the table; the same bounds again on the device's (all uniform over the workgroup), so
  // that no table can index outside qkv, o or the cache
  if (row0 < 0 || len <= 0 || len > p.T_cap || (long)row0 + len > p.M || slot < 0 || slot >= p.n_slots) return;
  if (PAST && (past < 0 || past > p.T_cap - len)) return;
  if (q0 >= len) return;
  const int D = p.D, half = D >> 1, W = p.H * D;
  const int qi = q0 + wave * 16 + lr;  // this lane's query row within the segment
  const bf16_t* xb = p.qkv + (long)row0 * p.ld_qkv + h * D;   // the segment's rows, this head's q columns
  bf16_t* cb = p.cache + (long)slot * p.cache_bs + h * D;
  if (PAST && len == 1 && past < ONE_ROW_MAX_KEYS) {            // mh_attn_fwd's own rule for Sq == 1: the decode kernel's bits
    if (one_row_score_floats(past + 1) * 4 + 512 > p.lds_bytes) return;   // workgroup-uniform, like every test above
    one_row_attention<SHARED>(p, smem, xb, cb, row0, past, h);
    return;
  }
  const int kv_end = past + (len < q0 + TQ ? len : q0 + TQ);  // causal: keys 0 .. the tile's last query (absolute keys)

  short8_t qf[DP / 32];
  {
    int ps = qi < len ? p.pos[row0 + qi] : 0;
    ps = ps < 0 ? 0 : (ps < p.max_pos ? ps : p.max_pos - 1);  // a position outside the table is the caller's error, never a fault
#pragma unroll
    for (int kk = 0; kk < DP / 32; ++kk) {
      const int col = kk * 32 + lg * 8;
      qf[kk] = (short8_t){0, 0, 0, 0, 0, 0, 0, 0};
      if (qi < len && col < D)
        qf[kk] = rope8(xb + (long)qi * p.ld_qkv, col, half, p.cs + (size_t)ps * half, p.sn + (size_t)ps * half);
    }
  }

  float4_t acc[DP / 16];
#pragma unroll
  for (int jd = 0; jd < DP / 16; ++jd) acc[jd] = (float4_t){0.f, 0.f, 0.f, 0.f};
  float m = NEG_INF, lsum = 0.f;
  constexpr int CH = DP / 8;

  for (int k0 = 0; k0 < kv_end; k0 += TK) {
    const bool diag = k0 == q0;
    // this workgroup stores chunk row c; the shared form stores none
    const auto own = [&](int c) { return SHARED ? false : PAST ? (c >= q0 && c < q0 + TQ) : diag; };
    __syncthreads();
    // K tile, rotated, row-major (stage_rowmajor's image); rows >= past + len are zero-filled.  Key k0 + row is chunk row c =
    // key - past; this workgroup stores the rows of its own query tile (without a prefix: the diagonal tile, k0 == q0)
    for (int idx = threadIdx.x; idx < 64 * CH; idx += 256) {
      const int row = idx / CH, ch = idx - row * CH;
      const int c = k0 + row - past;
      short8_t v = (short8_t){0, 0, 0, 0, 0, 0, 0, 0};
      if (PAST && c < 0) {
        if (ch * 8 < D) v = *reinterpret_cast<const short8_t*>(cb + (long)(k0 + row) * p.ld_cache + ch * 8);
      } else if (c < len && ch * 8 < D) {
        int ps = p.pos[row0 + c];
        ps = ps < 0 ? 0 : (ps < p.max_pos ? ps : p.max_pos - 1);
        v = rope8(xb + (long)c * p.ld_qkv + W, ch * 8, half, p.cs + (size_t)ps * half, p.sn + (size_t)ps * half);
        if (own(c)) *reinterpret_cast<short8_t*>(cb + (long)(k0 + row) * p.ld_cache + ch * 8) = v;
      }
      *reinterpret_cast<short8_t*>(Ks + row * Lds<DP>::ROW + ch * 8) = v;
    }
    // V tile, transposed (stage_transposed's image)
    for (int idx = threadIdx.x; idx < 64 * CH; idx += 256) {
      const int row = idx & 63, ch = idx >> 6;
      const int c = k0 + row - past;
      short8_t v = (short8_t){0, 0, 0, 0, 0, 0, 0, 0};
      if (PAST && c < 0) {
        if (ch * 8 < D) v = *reinterpret_cast<const short8_t*>(cb + (long)(k0 + row) * p.ld_cache + W + ch * 8);
      } else if (c < len && ch * 8 < D) {
        v = *reinterpret_cast<const short8_t*>(xb + (long)c * p.ld_qkv + 2 * W + ch * 8);
        if (own(c)) *reinterpret_cast<short8_t*>(cb + (long)(k0 + row) * p.ld_cache + W + ch * 8) = v;
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) Vt[(ch * 8 + e) * Lds<DP>::TROW + row] = (bf16_t)v[e];
    }
    __syncthreads();
    float4_t s[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s[j] = (float4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < DP / 32; ++kk)
        s[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_rm<DP>(Ks, j, kk, lr, lg), qf[kk], s[j], 0, 0, 0);
    }
    float tmax = NEG_INF;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = k0 + 16 * j + 4 * lg + r;
        const bool ok = key < past + len && key <= past + qi && qi < len;
        const float val = s[j][r] * p.scale;
        s[j][r] = ok ? val : NEG_INF;
        tmax = fmaxf(tmax, s[j][r]);
      }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
    const float m_new = fmaxf(m, tmax);
    const float alpha = (m_new == NEG_INF) ? 1.f : __expf(m - m_new);
    float psum = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e = (m_new == NEG_INF) ? 0.f : __expf(s[j][r] - m_new);
        s[j][r] = e;
        psum += e;
      }
    lsum = lsum * alpha + psum;
    m = m_new;
    const short8_t pb0 = pack8(s[0], s[1]), pb1 = pack8(s[2], s[3]);
#pragma unroll
    for (int jd = 0; jd < DP / 16; ++jd) {
      acc[jd] *= alpha;
      acc[jd] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_tr<DP>(Vt, jd, 0, lr, lg), pb0, acc[jd], 0, 0, 0);
      acc[jd] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_tr<DP>(Vt, jd, 1, lr, lg), pb1, acc[jd], 0, 0, 0);
    }
  }
  lsum += __shfl_xor(lsum, 16, 64);
  lsum += __shfl_xor(lsum, 32, 64);
  if (qi < len) {
    const float inv = lsum > 0.f ? 1.f / lsum : 0.f;
    bf16_t* ob = p.o + (long)(row0 + qi) * p.ldo + h * D;
#pragma unroll
    for (int jd = 0; jd < DP / 16; ++jd) {
      const int d = jd * 16 + lg * 4;
      if (d < D) {
        uint2 pk;
        pk.x = pack_bf2(acc[jd][0] * inv, acc[jd][1] * inv);
        pk.y = pack_bf2(acc[jd][2] * inv, acc[jd][3] * inv);
        *reinterpret_cast<uint2*>(ob + d) = pk;
      }
    }
  }
}

template <int DP, bool PAST, bool SHARED = false>
static int launch_ragged(RaggedParams p, int tiles, int R, hipStream_t s) {
  size_t sh = Lds<DP>::RM_BYTES + Lds<DP>::TR_BYTES;         // <= 35,840 bytes: no opt-in needed
  if (PAST && (size_t)p.lds_bytes > sh) sh = p.lds_bytes;    // a one-row segment's scores: <= 33,280 bytes
  p.lds_bytes = (int)sh;
  hipLaunchKernelGGL((attn_prefill_ragged_kernel<DP, PAST, SHARED>), dim3(tiles, R * p.H), dim3(256), sh, s, p);
  MH_CHECK_LAUNCH();
  return MH_OK;
}

// All entries: `sw` = 3 or 4 ints per segment (without / with `past`); `shared` (sw = 4 only): segments may name one slot
// several times and the cache is only read.
static int prefill_ragged(int sw, bool shared, const void* qkv, long ld_qkv, const int* pos, const int* seg, const int* seg_host,
                          int R, void* cache, long cache_bstride, long ld_cache, int n_slots, int T_cap, const float* cos_tab,
                          const float* sin_tab, int max_pos, void* out, long ldo, int M, int H, int D, float scale,
                          hipStream_t stream) {
  if (R == 0) return MH_OK;
  if (R < 0 || M <= 0 || H <= 0 || n_slots <= 0 || T_cap <= 0 || max_pos <= 0) return MH_ERR_ARG;
  if (D <= 0 || D % 16 || D > 128) return MH_ERR_UNSUPPORTED;
  if (!qkv || !pos || !seg || !seg_host || !cache || !cos_tab || !sin_tab || !out) return MH_ERR_ARG;
  const long W = (long)H * D;
  if (ld_qkv < 3 * W || ld_qkv % 8 || ld_cache < 2 * W || ld_cache % 8 || cache_bstride % 8 || ldo < W || ldo % 4 ||
      cache_bstride < (long)T_cap * ld_cache || (long)R * H > 65535)
    return MH_ERR_ARG;
  if ((uintptr_t)qkv % 16 || (uintptr_t)cache % 16 || (uintptr_t)cos_tab % 16 || (uintptr_t)sin_tab % 16 || (uintptr_t)out % 8)
    return MH_ERR_ARG;
  // the segment table: 0 < len <= T_cap, 0 <= slot < n_slots, rows inside [0, M), slots distinct (unless `shared`), segments
  // disjoint; with a prefix 0 <= past and past + len <= T_cap
  std::vector<std::pair<long, long>> rows(R);
  std::vector<int> slots(R);
  int max_len = 0, one_row_lds = 0;
  for (int i = 0; i < R; ++i) {
    const int row0 = seg_host[sw * i], len = seg_host[sw * i + 1], slot = seg_host[sw * i + 2];
    if (len <= 0 || len > T_cap || slot < 0 || slot >= n_slots || row0 < 0 || (long)row0 + len > M) return MH_ERR_ARG;
    if (sw == 4) {
      const int past = seg_host[sw * i + 3];
      if (past < 0 || past > T_cap - len) return MH_ERR_ARG;
      if (len == 1 && past < ONE_ROW_MAX_KEYS) one_row_lds = std::max(one_row_lds, one_row_score_floats(past + 1) * 4 + 512);
    }
    rows[i] = {row0, (long)row0 + len};
    slots[i] = slot;
    max_len = std::max(max_len, len);
  }
  std::sort(rows.begin(), rows.end());
  std::sort(slots.begin(), slots.end());
  for (int i = 1; i < R; ++i)
    if (rows[i].first < rows[i - 1].second || (!shared && slots[i] == slots[i - 1])) return MH_ERR_ARG;

  RaggedParams p = {};
  p.qkv = (const bf16_t*)qkv; p.pos = pos; p.seg = seg; p.cache = (bf16_t*)cache; p.cs = cos_tab; p.sn = sin_tab;
  p.o = (bf16_t*)out;
  p.ld_qkv = ld_qkv; p.cache_bs = cache_bstride; p.ld_cache = ld_cache; p.ldo = ldo;
  p.M = M; p.H = H; p.D = D; p.n_slots = n_slots; p.T_cap = T_cap; p.max_pos = max_pos; p.scale = scale;
  p.lds_bytes = one_row_lds;
  const int tiles = (max_len + TQ - 1) / TQ;
  if (sw == 4 && shared) {
    if (D <= 64) return launch_ragged<64, true, true>(p, tiles, R, stream);
    if (D <= 96) return launch_ragged<96, true, true>(p, tiles, R, stream);
    return launch_ragged<128, true, true>(p, tiles, R, stream);
  }
  if (sw == 4) {
    if (D <= 64) return launch_ragged<64, true>(p, tiles, R, stream);
    if (D <= 96) return launch_ragged<96, true>(p, tiles, R, stream);
    return launch_ragged<128, true>(p, tiles, R, stream);
  }
  if (D <= 64) return launch_ragged<64, false>(p, tiles, R, stream);
  if (D <= 96) return launch_ragged<96, false>(p, tiles, R, stream);
  return launch_ragged<128, false>(p, tiles, R, stream);
}

extern "C" int mh_attn_prefill_ragged(const void* qkv, long ld_qkv, const int* pos, const int* seg, const int* seg_host, int R,
                                      void* cache, long cache_bstride, long ld_cache, int n_slots, int T_cap, const float* cos_tab,
                                      const float* sin_tab, int max_pos, void* out, long ldo, int M, int H, int D, float scale,
                                      hipStream_t stream) {
  return prefill_ragged(3, false, qkv, ld_qkv, pos, seg, seg_host, R, cache, cache_bstride, ld_cache, n_slots, T_cap, cos_tab,
                        sin_tab, max_pos, out, ldo, M, H, D, scale, stream);
}

// The same pass on top of a cached prefix: segment tables [R, 4] = (row0, len, slot, past).
extern "C" int mh_attn_prefill_ragged_past(const void* qkv, long ld_qkv, const int* pos, const int* seg, const int* seg_host,
                                           int R, void* cache, long cache_bstride, long ld_cache, int n_slots, int T_cap,
                                           const float* cos_tab, const float* sin_tab, int max_pos, void* out, long ldo, int M,
                                           int H, int D, float scale, hipStream_t stream) {
  return prefill_ragged(4, false, qkv, ld_qkv, pos, seg, seg_host, R, cache, cache_bstride, ld_cache, n_slots, T_cap, cos_tab,
                        sin_tab, max_pos, out, ldo, M, H, D, scale, stream);
}

// Several segments continuing the SAME cached prefix (the candidates of one prompt, LlamaDecode.score_continuations): the _past
// form's tables, but slots may repeat and the cache is only read -- the kernel's SHARED flag drops every cache store, the new
// rows' k | v are staged from qkv as before (the one-row path keeps them in LDS).  Per segment the out rows have the bits of
// mh_attn_prefill_ragged_past on that segment alone.
extern "C" int mh_attn_prefill_ragged_shared(const void* qkv, long ld_qkv, const int* pos, const int* seg, const int* seg_host,
                                             int R, const void* cache, long cache_bstride, long ld_cache, int n_slots, int T_cap,
                                             const float* cos_tab, const float* sin_tab, int max_pos, void* out, long ldo, int M,
                                             int H, int D, float scale, hipStream_t stream) {
  return prefill_ragged(4, true, qkv, ld_qkv, pos, seg, seg_host, R, const_cast<void*>(cache), cache_bstride, ld_cache, n_slots,
                        T_cap, cos_tab, sin_tab, max_pos, out, ldo, M, H, D, scale, stream);
}
