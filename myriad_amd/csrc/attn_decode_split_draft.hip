// K-row split-KV token-step attention (the verify step of draft-and-verify decoding on the split-KV view): row g*K + j of qkv is the
// token at position pos[g] + j of sequence g, and its out row and cache row carry the bits of the j-th of nrow[g] sequential
// mh_attn_decode_rope_split_rows launches at B = 1 with the same chunk, pos = pos[g] + j and kv_len = pos[g] + j + 1
// (tests/test_split_draft_kernels_gpu.py holds the two to the same bits).
//
// attn_decode_split.hip cuts the keys at fixed multiples of the chunk size, whatever kv_len is, so the K rows of a step share every
// chunk boundary.  One workgroup per (chunk, sequence, head) -- grid (ceil(T_cap / CH), G*H), not K times that -- loads each cached
// key and each cached value ONCE and serves the queries of all the group's rows; per row it calls what the one-row split kernel
// calls in attn_one_query.h, in its order: the key's score, the lane-stride statistics over the row's own n_j keys, the fixed
// four-wave sum, and in the merge launch the merge with nc_j = ceil((pos[g] + j + 1) / CH).  Phase 3 is this kernel's own loop (a
// value row is loaded once and meets every row's stored weight) in the one-row kernel's order: wave w's keys w, w + 4, ... in
// groups of 8.
//
// The rows depend on each other: row j sees the keys of rows 0 .. j-1 of the same launch.  No workgroup reads a cache row >= pos[g]
// (a stale row a rejected guess left there may hold anything): the workgroup rotates the k of the step rows whose position falls in
// its own chunk into LDS, with their v, and is the only one to write those cache rows.  The q of every row is rotated into LDS; qkv
// is not written (as in the split kernel, unlike attn_decode_draft.hip).  A key at or beyond a row's n_j contributes a zero weight
// AND a zero value to it, as in the one-row kernel.
#include "attn_one_query.h"

#define SD_MAX_K 8

struct SplitDraftParams {
  const bf16_t* qkv;    // [G*K, ld_qkv] = [q | k | v], only read
  bf16_t* cache;        // [G][T_cap][2W] rows [k | v]
  bf16_t* out;          // [G*K, ldo]
  const int* pos;       // [G] position of row 0 of the group
  const int* live;      // [G] 0 = the sequence is idle
  const int* nrow;      // [G] rows of the group that hold a token, 1 .. K; null (mh_attn_decode_rope_split_draft): all K
  const float* cs;
  const float* sn;
  float* part;
  long ld_qkv, cache_bs, ld_cache, ldo;
  int K, H, D, T_cap, nch;
  float scale;
};

// rows of group g this step serves: nrow[g] (or K), less those whose position would leave the cache; <= 0: none
__device__ __forceinline__ int sd_rows(const SplitDraftParams& p, int g, int p0) {
  int nr = p.nrow ? p.nrow[g] : p.K;
  nr = nr < p.K ? nr : p.K;
  return nr < p.T_cap - p0 ? nr : p.T_cap - p0;
}

// KT: K rounded up to 1, 2, 4 or 8 -- the rows a workgroup holds in registers
template <int CH, int KT>
__global__ __launch_bounds__(OQ_SPLIT_THREADS) void attn_decode_split_draft_kernel(SplitDraftParams p) {
  __shared__ float sc[KT][CH];               // chunk scores per row, then the un-normalised weights e^(s - m)
  __shared__ float po[4][KT][128];           // per-wave partial outputs
  __shared__ float qs[KT][128];              // rotated q (bf16-rounded) * scale
  __shared__ __align__(16) bf16_t knew[KT][128], vnew[KT][128];   // this chunk's step rows: k (rotated) and v, at index (row in group)
  __shared__ float smx[KT], ssum[KT];
  const int c = blockIdx.x, gh = blockIdx.y;
  const int g = gh / p.H, h = gh % p.H;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int D = p.D, W = p.H * D;
  // uniform over the workgroup, ahead of the first barrier: an idle sequence, no row inside the cache, a chunk past the last row
  if (p.live[g] == 0) return;
  const int p0 = p.pos[g];
  if (p0 < 0) return;
  const int nr = sd_rows(p, g, p0);
  const int j0 = c * CH;
  if (nr <= 0 || j0 >= p0 + nr) return;
  const int nmax = p0 + nr - j0 < CH ? p0 + nr - j0 : CH;       // keys of this chunk the last row sees
  const int lo = p0 - j0;                                       // chunk-local index of step row 0 (may be < 0 or >= CH)

  // rotary (the split kernel's block, one 4-pair item per thread and pass): q of every row; k | v of the rows this chunk owns
  {
    const int half = D >> 1, items = half >> 2, vitems = D >> 3;
    const int nrot = 2 * nr * items, total = nrot + nr * vitems;
    for (int t = tid; t < total; t += OQ_SPLIT_THREADS) {
      if (t < nrot) {
        const int which = t / (nr * items), r = (t / items) % nr, i = (t % items) * 4;
        const int pp = p0 + r;
        const bool mine = pp >= j0 && pp < j0 + CH;
        if (which == 0 || mine) {
          const bf16_t* e = p.qkv + (size_t)(g * p.K + r) * p.ld_qkv + which * W + h * D + i;
          short4_t oa, ob;
          oq_rope4(e, half, p.cs, p.sn, pp, i, oa, ob);
          if (which == 0) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              qs[r][i + u] = bf2f((bf16_t)oa[u]) * p.scale;
              qs[r][i + half + u] = bf2f((bf16_t)ob[u]) * p.scale;
            }
          } else {
            bf16_t* crow = p.cache + (size_t)g * p.cache_bs + (size_t)pp * p.ld_cache;
            *reinterpret_cast<short4_t*>(crow + h * D + i) = oa;
            *reinterpret_cast<short4_t*>(crow + h * D + i + half) = ob;
            *reinterpret_cast<short4_t*>(&knew[r][i]) = oa;
            *reinterpret_cast<short4_t*>(&knew[r][i + half]) = ob;
          }
        }
      } else {
        const int r = (t - nrot) / vitems, cc = ((t - nrot) % vitems) * 8;
        const int pp = p0 + r;
        if (pp >= j0 && pp < j0 + CH) {
          const short8_t v8 = *reinterpret_cast<const short8_t*>(p.qkv + (size_t)(g * p.K + r) * p.ld_qkv + 2 * W + h * D + cc);
          *reinterpret_cast<short8_t*>(p.cache + (size_t)g * p.cache_bs + (size_t)pp * p.ld_cache + W + h * D + cc) = v8;
          *reinterpret_cast<short8_t*>(&vnew[r][cc]) = v8;
        }
      }
    }
  }
  __syncthreads();

  const bf16_t* kp = p.cache + (size_t)g * p.cache_bs + (size_t)j0 * p.ld_cache + h * D;      // rows < p0 only
  const bf16_t* vp = kp + W;

  // phase 1: scores.  16 lanes per key (8 dims each), 16 keys per 256-thread pass; each key is loaded once and meets every row's q
  const int sub = lane & 15, kq = lane >> 4;
  const bool dim_ok = sub * 8 < D;
  float qf[KT][8];
#pragma unroll
  for (int r = 0; r < KT; ++r)
#pragma unroll
    for (int e = 0; e < 8; ++e) qf[r][e] = (dim_ok && r < nr) ? qs[r][sub * 8 + e] : 0.f;
  constexpr int PASSES = CH / 16, UNR = KT > 4 ? 4 : 8;
  for (int u0 = 0; u0 < PASSES && u0 * 16 < nmax; u0 += UNR) {
    short8_t kv[UNR];
    int jj[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      jj[u] = (u0 + u) * 16 + wave * 4 + kq;
      kv[u] = (short8_t){0, 0, 0, 0, 0, 0, 0, 0};
      if (jj[u] < nmax && jj[u] < lo && dim_ok) kv[u] = *reinterpret_cast<const short8_t*>(kp + (size_t)jj[u] * p.ld_cache + sub * 8);
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      if (jj[u] < nmax && jj[u] >= lo && dim_ok) kv[u] = *reinterpret_cast<const short8_t*>(&knew[jj[u] - lo][sub * 8]);
#pragma unroll
      for (int r = 0; r < KT; ++r) {
        if (r < nr) {
          const float s = oq_score(qf[r], kv[u]);
          if (sub == 0 && jj[u] <= lo + r) sc[r][jj[u]] = s;      // row r sees keys 0 .. pos[g] + r
        }
      }
    }
  }
  __syncthreads();
  // phase 2: each row's softmax statistics over its own n_r keys, in the one-row kernel's lane-stride order.  There every wave
  // computes the same two numbers for itself; here wave w does it for rows w and w + 4 and leaves the weights in place of the scores
  for (int r = wave; r < nr; r += 4) {
    const int n = lo + r + 1 < CH ? lo + r + 1 : CH;
    if (n <= 0) continue;
    float mx, sum;
    oq_softmax_stats<true>(sc[r], n, lane, mx, sum);
    if (lane == 0) {
      smx[r] = mx;
      ssum[r] = sum;
    }
  }
  __syncthreads();
  // phase 3: o_r = sum_j p_rj V[j]; lane owns dims 2*lane, 2*lane+1; wave w takes keys w, w+4, ...; each value row loaded once
  float o0[KT], o1[KT];
#pragma unroll
  for (int r = 0; r < KT; ++r) o0[r] = o1[r] = 0.f;
  const bool own = 2 * lane < D;
  for (int j = wave; j < nmax; j += 32) {
    unsigned vv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int jr = j + 4 * u;
      vv[u] = 0u;
      if (own && jr < nmax)
        vv[u] = jr >= lo ? *reinterpret_cast<const unsigned*>(&vnew[jr - lo][2 * lane])
                         : *reinterpret_cast<const unsigned*>(vp + (size_t)jr * p.ld_cache + 2 * lane);
    }
#pragma unroll
    for (int r = 0; r < KT; ++r) {
      const int n = lo + r + 1 < CH ? lo + r + 1 : CH;
      if (r < nr && j < n) {                       // the one-row kernel's loop ends at its own n
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int jr = j + 4 * u;
          const bool ok = jr < n;
          const float pj = ok ? sc[r][jr] : 0.f;
          const unsigned v = ok ? vv[u] : 0u;
          o0[r] += pj * bf2f((bf16_t)(v & 0xffffu));
          o1[r] += pj * bf2f((bf16_t)(v >> 16));
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < KT; ++r) {
    po[wave][r][2 * lane] = o0[r];
    po[wave][r][2 * lane + 1] = o1[r];
  }
  __syncthreads();
  for (int r = wave; r < nr; r += 4) {
    if (lo + r + 1 <= 0) continue;                 // the chunk starts past this row's keys: no record
    float* rec = p.part + (((size_t)(g * p.K + r) * p.H + h) * p.nch + c) * OQ_SPLIT_PSTRIDE;
    oq_split_record(rec, &po[0][r][0], KT * 128, lane, own, smx[r], ssum[r]);
  }
}

// attn_decode_combine_kernel's merge per (row, head)
template <int CH>
__global__ __launch_bounds__(64) void attn_decode_split_draft_combine_kernel(SplitDraftParams p) {
  const int bh = blockIdx.x, row = bh / p.H, h = bh % p.H, lane = threadIdx.x;
  const int g = row / p.K, jr0 = row - g * p.K;
  const int p0 = p.pos[g];
  if (p.live[g] == 0 || p0 < 0 || jr0 >= sd_rows(p, g, p0)) {      // no token in this row: a zero row, no partial record read
    if (2 * lane < p.D) *reinterpret_cast<unsigned*>(p.out + (size_t)row * p.ldo + h * p.D + 2 * lane) = 0u;
    return;
  }
  const int len = p0 + jr0 + 1;
  const int nc = (len + CH - 1) / CH;
  oq_split_merge(p.part + (size_t)bh * p.nch * OQ_SPLIT_PSTRIDE, nc, lane, p.D, p.out + (size_t)row * p.ldo + h * p.D);
}

extern "C" long mh_attn_decode_split_draft_ws_floats(int G, int K, int H, int T_cap, int chunk) {
  const int ch = oq_split_chunk(chunk);
  if (G <= 0 || K <= 0 || H <= 0 || T_cap <= 0 || !oq_split_chunk_ok(ch)) return -1;
  return (long)G * K * H * ((T_cap + ch - 1) / ch) * OQ_SPLIT_PSTRIDE;
}

template <int CH, int KT>
static int sd_launch(const SplitDraftParams& p, int G, hipStream_t s) {
  hipLaunchKernelGGL((attn_decode_split_draft_kernel<CH, KT>), dim3(p.nch, G * p.H), dim3(OQ_SPLIT_THREADS), 0, s, p);
  MH_CHECK_LAUNCH();
  hipLaunchKernelGGL((attn_decode_split_draft_combine_kernel<CH>), dim3(G * p.K * p.H), dim3(64), 0, s, p);
  MH_CHECK_LAUNCH();
  return MH_OK;
}

template <int CH>
static int sd_launch_k(const SplitDraftParams& p, int G, hipStream_t s) {
  if (p.K == 1) return sd_launch<CH, 1>(p, G, s);
  if (p.K == 2) return sd_launch<CH, 2>(p, G, s);
  if (p.K <= 4) return sd_launch<CH, 4>(p, G, s);
  return sd_launch<CH, 8>(p, G, s);
}

// G sequences of K consecutive token rows: see include/myriad_hip.h.  `nrow` null: every group has K rows.
static int split_draft_launch(const void* qkv, long ld_qkv, void* cache, long cache_bstride, long ld_cache, const int* pos,
                              const int* live, const int* nrow, bool rows, const float* cos_tab, const float* sin_tab, void* out,
                              long ldo, float* partials, long partials_floats, int G, int K, int H, int D, int T_cap, int chunk,
                              float scale, hipStream_t stream) {
  const int ch = oq_split_chunk(chunk);
  if (K < 1 || H <= 0 || T_cap <= 0 || T_cap > 8192 || !oq_split_chunk_ok(ch)) return MH_ERR_ARG;
  if (D <= 0 || D % 16 || D > 128 || K > SD_MAX_K) return MH_ERR_UNSUPPORTED;
  if (G <= 0) return MH_OK;                        // nothing to do: the answer says whether the shape is supported
  if (!oq_step_args_ok(qkv, ld_qkv, cache, cache_bstride, ld_cache, pos, live, nrow, rows, cos_tab, sin_tab, out, ldo, G, K, H, D))
    return MH_ERR_ARG;
  if (!partials || (uintptr_t)partials % 4 || (long)G * H > 65535L) return MH_ERR_ARG;
  const long need = mh_attn_decode_split_draft_ws_floats(G, K, H, T_cap, chunk);
  if (need < 0 || partials_floats < need) return MH_ERR_ARG;
  SplitDraftParams p;
  p.qkv = (const bf16_t*)qkv; p.cache = (bf16_t*)cache; p.out = (bf16_t*)out; p.pos = pos; p.live = live; p.nrow = nrow;
  p.cs = cos_tab; p.sn = sin_tab; p.part = partials; p.ld_qkv = ld_qkv; p.cache_bs = cache_bstride; p.ld_cache = ld_cache; p.ldo = ldo;
  p.K = K; p.H = H; p.D = D; p.T_cap = T_cap; p.nch = (T_cap + ch - 1) / ch; p.scale = scale;
  if (ch == 256) return sd_launch_k<256>(p, G, stream);
  if (ch == 512) return sd_launch_k<512>(p, G, stream);
  return sd_launch_k<128>(p, G, stream);
}

extern "C" int mh_attn_decode_rope_split_draft(const void* qkv, long ld_qkv, void* cache, long cache_bstride, long ld_cache,
                                               const int* pos, const int* live, const float* cos_tab, const float* sin_tab, void* out,
                                               long ldo, float* partials, long partials_floats, int G, int K, int H, int D, int T_cap,
                                               int chunk, float scale, hipStream_t stream) {
  return split_draft_launch(qkv, ld_qkv, cache, cache_bstride, ld_cache, pos, live, nullptr, false, cos_tab, sin_tab, out, ldo, partials,
                            partials_floats, G, K, H, D, T_cap, chunk, scale, stream);
}

// The decode slots' form: group g holds nrow[g] token rows (1 .. K); the rest of its K rows are skipped like an idle group's.
extern "C" int mh_attn_decode_rope_split_draft_rows(const void* qkv, long ld_qkv, void* cache, long cache_bstride, long ld_cache,
                                                    const int* pos, const int* live, const int* nrow, const float* cos_tab,
                                                    const float* sin_tab, void* out, long ldo, float* partials, long partials_floats,
                                                    int G, int K, int H, int D, int T_cap, int chunk, float scale,
                                                    hipStream_t stream) {
  return split_draft_launch(qkv, ld_qkv, cache, cache_bstride, ld_cache, pos, live, nrow, true, cos_tab, sin_tab, out, ldo, partials,
                            partials_floats, G, K, H, D, T_cap, chunk, scale, stream);
}
