// Beam search on the KV-cache decode path (HF GenerationMixin._beam_search, num_beams <= 8): the two device pieces of a beam
// step.  The host keeps the hypotheses; these kernels keep the per-step work off it.
//   beam_row_topk_kernel   one 1024-thread workgroup per logits row (V <= 32768, row in registers): logsumexp, the EOS ban,
//                          score = beam_score + log_softmax, then the row's top K = 2*nb candidates by (score desc, token asc).
//                          Every wave takes its own top K by K wave-wide arg-max rounds (no block barrier inside a round); the
//                          16 waves' 16*K survivors are ranked in LDS.  A row's top K holds every candidate of that row that can
//                          reach its item's top K, so the per-item merge needs nothing else.
//   beam_merge_kernel      one workgroup per batch item: ranks the item's rpi*K (<= 128) row survivors by (score desc, flat
//                          index asc), flat = row_in_item * V + token, and writes the item's top K -- the step's record.
//                          Optionally the step's pos / kvlen advance rides along (nothing in the step reads them after this).
//   beam_reorder_kv_kernel cache[r, p] = cache[src[r], p] for p in [*lo, *hi), every layer in one launch, in place: a thread owns
//                          one 16-byte cell (layer, item, position, columns) for all nb sibling rows of the item, loads every
//                          source row of that cell, then stores -- no cell is shared between threads, so no hazard; src, lo and
//                          hi are read from device memory so the launch can be captured in the token step's hipGraph.
// The three kernels are templates on ITEMS (the decode slots' beam groups, one request per item): every item then has its own
// live flag, generated count (which decides its EOS ban), position and reorder window in device memory, and an idle item's
// workgroups leave on a scalar branch.  ITEMS = false is the code above, unchanged.
#include "common.h"

#define BNT 1024                // threads per row (beam_row_topk_kernel)
#define BNW (BNT / 64)
#define BVPT 32                 // values per thread: V <= BNT * BVPT = 32768
#define BKMAX 16                // K = 2 * nb, nb <= 8

struct BeamCand { float s; int i; };

// a comes strictly before b: higher score, ties to the lower index (NaN scores are mapped to -inf before they get here)
__device__ __forceinline__ bool bm_before(float as, int ai, float bs, int bi) { return as > bs || (as == bs && ai < bi); }

__device__ __forceinline__ float bm_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float bm_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// scores [R] = each row's running beam score; part[R][K] = (score, token) of the row's top K
// ITEMS: rows row / nb * nb .. + nb - 1 are item g's; an idle item's rows leave before they load a logit (blockIdx is uniform: a
// scalar branch), a live one bans prm[1] while gen[g] < prm[0]
template <bool ITEMS>
__global__ __launch_bounds__(BNT) void beam_row_topk_kernel(const float* __restrict__ logits, long ldl,
                                                            const float* __restrict__ scores, float* __restrict__ part_s,
                                                            int* __restrict__ part_i, int V, int K, int ban_id, int nb,
                                                            const int* __restrict__ live, const int* __restrict__ gen,
                                                            const int* __restrict__ prm) {
  __shared__ float red[BNW];
  __shared__ float cs[BNW * BKMAX];
  __shared__ int ci[BNW * BKMAX];
  const long row = blockIdx.x;
  if (ITEMS) {
    const int g = blockIdx.x / nb;
    if (!live[g]) return;
    ban_id = gen[g] < prm[0] ? prm[1] : -1;
  }
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const float* x = logits + row * ldl;
  const float ninf = -__builtin_inff();

  float v[BVPT];
  float mx = ninf;
#pragma unroll
  for (int i = 0; i < BVPT; ++i) {
    const int j = i * BNT + tid;
    v[i] = j < V ? x[j] : ninf;
    mx = fmaxf(mx, v[i]);
  }
  // row max
  mx = bm_wave_max(mx);
  if (lane == 0) red[w] = mx;
  __syncthreads();
  mx = red[0];
#pragma unroll
  for (int i = 1; i < BNW; ++i) mx = fmaxf(mx, red[i]);
  __syncthreads();
  // sum of exp(x - max)
  float se = 0.f;
#pragma unroll
  for (int i = 0; i < BVPT; ++i) se += expf(v[i] - mx);      // -inf (padding, a -inf logit) contributes 0
  se = bm_wave_sum(se);
  if (lane == 0) red[w] = se;
  __syncthreads();
  se = 0.f;
#pragma unroll
  for (int i = 0; i < BNW; ++i) se += red[i];
  // log_softmax as torch forms it, (x - max) - log(sum), the ban after it (HF applies the processors to the log-probs), then
  // the running score of the beam
  const float ls = logf(se), bs = scores[row];
#pragma unroll
  for (int i = 0; i < BVPT; ++i) {
    const int j = i * BNT + tid;
    float s = bs + ((v[i] - mx) - ls);
    if (j == ban_id || !(s == s)) s = ninf;
    v[i] = s;
  }

  // per-wave top K: round k takes the best candidate strictly after round k-1's winner (thr) in (score desc, index asc)
  float ts = __builtin_inff();
  int ti = -1;
  for (int k = 0; k < K; ++k) {
    float bsc = ninf;
    int bi = 0x7fffffff;                                     // "none yet": any real candidate comes before it
#pragma unroll
    for (int i = 0; i < BVPT; ++i) {
      const int j = i * BNT + tid;
      if (j < V && bm_before(ts, ti, v[i], j) && bm_before(v[i], j, bsc, bi)) { bsc = v[i]; bi = j; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float os = __shfl_xor(bsc, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (bm_before(os, oi, bsc, bi)) { bsc = os; bi = oi; }
    }
    if (lane == 0) { cs[w * K + k] = bsc; ci[w * K + k] = bi; }
    ts = bsc;
    ti = bi;
  }
  __syncthreads();
  // rank the BNW * K wave survivors; the row's top K are those of rank < K.  Real candidates have distinct indices, so distinct
  // ranks.  The (-inf, 0x7fffffff) entries of waves that ran out all share ONE rank, the number of real survivors -- and that is
  // >= K, because a wave hands on min(K, its candidates) and the row has V >= K of them: none is written, every rank < K once
  const int n = BNW * K;
  for (int c = tid; c < n; c += BNT) {
    const float s = cs[c];
    const int i = ci[c];
    int rank = 0;
    for (int o = 0; o < n; ++o) rank += bm_before(cs[o], ci[o], s, i) ? 1 : 0;
    if (rank < K) {
      part_s[row * K + rank] = s;
      part_i[row * K + rank] = i;
    }
  }
}

// ITEMS (rpi = nb): an idle item records (0.0, -1) K times and keeps its state; a live one advances its own rows' pos / kvlen
// and its gen (which the row kernel, an earlier launch, has read)
template <bool ITEMS>
__global__ __launch_bounds__(128) void beam_merge_kernel(const float* __restrict__ part_s, const int* __restrict__ part_i,
                                                         float* __restrict__ out_s, int* __restrict__ out_i, int rpi, int V, int K,
                                                         int* __restrict__ pos, int* __restrict__ kvlen, int n_adv,
                                                         const int* __restrict__ live, int* __restrict__ gen) {
  __shared__ float cs[8 * BKMAX];
  __shared__ int ci[8 * BKMAX];
  const int b = blockIdx.x, tid = threadIdx.x, n = rpi * K;
  if (ITEMS && !live[b]) {
    if (tid < K) {
      out_s[(long)b * K + tid] = 0.f;
      out_i[(long)b * K + tid] = -1;
    }
    return;
  }
  if (tid < n) {
    const long src = (long)b * n + tid;                      // row b * rpi + tid / K, its rank tid % K
    cs[tid] = part_s[src];
    const int tok = part_i[src];
    ci[tid] = tok == 0x7fffffff ? tok : (tid / K) * V + tok;
  }
  __syncthreads();
  if (tid < n) {
    const float s = cs[tid];
    const int i = ci[tid];
    int rank = 0;
    for (int o = 0; o < n; ++o) rank += bm_before(cs[o], ci[o], s, i) ? 1 : 0;
    if (rank < K) {
      out_s[(long)b * K + rank] = s;
      out_i[(long)b * K + rank] = i;
    }
  }
  if (ITEMS) {
    if (tid < rpi) { pos[b * rpi + tid] += 1; kvlen[b * rpi + tid] += 1; }
    if (tid == 0) gen[b] += 1;
  } else if (b == 0 && pos && kvlen) {
    for (int r = tid; r < n_adv; r += blockDim.x) { pos[r] += 1; kvlen[r] += 1; }
  }
}

extern "C" int mh_beam_topk(const float* logits, long ldl, const float* scores, float* part_s, int* part_i, float* out_s, int* out_i,
                            int B, int rpi, int nb, int V, int ban_id, int* pos, int* kvlen, int n_adv, hipStream_t stream) {
  if (B <= 0) return MH_OK;
  if (!logits || !scores || !part_s || !part_i || !out_s || !out_i || V <= 0 || ldl < V) return MH_ERR_ARG;
  if (nb < 1 || nb > 8 || (rpi != 1 && rpi != nb) || V > BNT * BVPT || V < 2 * nb || n_adv < 0) return MH_ERR_UNSUPPORTED;
  const int K = 2 * nb;
  hipLaunchKernelGGL(beam_row_topk_kernel<false>, dim3(B * rpi), dim3(BNT), 0, stream, logits, ldl, scores, part_s, part_i, V, K,
                     ban_id, rpi, (const int*)nullptr, (const int*)nullptr, (const int*)nullptr);
  MH_CHECK_LAUNCH();
  hipLaunchKernelGGL(beam_merge_kernel<false>, dim3(B), dim3(128), 0, stream, part_s, part_i, out_s, out_i, rpi, V, K, pos, kvlen,
                     n_adv, (const int*)nullptr, (int*)nullptr);
  MH_CHECK_LAUNCH();
  return MH_OK;
}

extern "C" int mh_beam_topk_items(const float* logits, long ldl, const float* scores, float* part_s, int* part_i, float* out_s,
                                  int* out_i, int G, int nb, int V, const int* live, int* gen, const int* prm, int* pos, int* kvlen,
                                  hipStream_t stream) {
  if (G <= 0) return MH_OK;
  if (!logits || !scores || !part_s || !part_i || !out_s || !out_i || !live || !gen || !prm || !pos || !kvlen || V <= 0 || ldl < V)
    return MH_ERR_ARG;
  if (nb < 1 || nb > 8 || V > BNT * BVPT || V < 2 * nb) return MH_ERR_UNSUPPORTED;
  const int K = 2 * nb;
  hipLaunchKernelGGL(beam_row_topk_kernel<true>, dim3(G * nb), dim3(BNT), 0, stream, logits, ldl, scores, part_s, part_i, V, K, -1,
                     nb, live, (const int*)gen, prm);
  MH_CHECK_LAUNCH();
  hipLaunchKernelGGL(beam_merge_kernel<true>, dim3(G), dim3(128), 0, stream, part_s, part_i, out_s, out_i, nb, V, K, pos, kvlen, 0,
                     live, gen);
  MH_CHECK_LAUNCH();
  return MH_OK;
}

// ---------------------------------------------------------------------------------------------------- KV reorder
#define RKT 256                 // threads per workgroup: one 16-byte cell (8 bf16 columns) each
#define RKP 4                   // positions per workgroup

typedef __attribute__((ext_vector_type(4))) unsigned u32x4_t;

// grid (ceil(T_cap / RKP), ceil(C / (8 * RKT)), L * B); caches[l] = layer l's [B*nb, T_cap, C] bf16 base
// ITEMS: item b's window is [lo_p[b], hi_p[b]) and an item with live[b] == 0 is not touched
template <bool ITEMS>
__global__ __launch_bounds__(RKT) void beam_reorder_kv_kernel(bf16_t* const* __restrict__ caches, int B, int nb, long T_cap, int C,
                                                              const int* __restrict__ src, const int* __restrict__ lo_p,
                                                              const int* __restrict__ hi_p, const int* __restrict__ live) {
  const int l = blockIdx.z / B, b = blockIdx.z % B;
  if (ITEMS && !live[b]) return;
  const int lo = max(ITEMS ? lo_p[b] : *lo_p, 0);
  const long hi = min((long)(ITEMS ? hi_p[b] : *hi_p), T_cap);
  const long p0 = (long)blockIdx.x * RKP;
  if (p0 >= hi || p0 + RKP <= lo) return;                   // blocks outside [lo, hi) exit at once
  const int col = (blockIdx.y * RKT + threadIdx.x) * 8;
  if (col >= C) return;
  bf16_t* base = caches[l];
  const long r0 = (long)b * nb;
  int sr[8];
  bool any = false;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    sr[j] = j;                                               // identity: no copy
    if (j < nb) {
      const int s = src[r0 + j] - (int)r0;
      if (s >= 0 && s < nb) sr[j] = s;                       // a parent outside the item is ignored (never a cross-item write)
      any |= sr[j] != j;
    }
  }
  if (!any) return;
  for (long p = max(p0, (long)lo); p < min(p0 + RKP, hi); ++p) {
    u32x4_t val[8];
#pragma unroll
    for (int j = 0; j < 8; ++j)                              // every source value of the cell first ...
      if (j < nb && sr[j] != j) val[j] = *reinterpret_cast<const u32x4_t*>(base + ((r0 + sr[j]) * T_cap + p) * C + col);
#pragma unroll
    for (int j = 0; j < 8; ++j)                              // ... then the stores
      if (j < nb && sr[j] != j) *reinterpret_cast<u32x4_t*>(base + ((r0 + j) * T_cap + p) * C + col) = val[j];
  }
}

extern "C" int mh_beam_reorder_kv(void* const* caches, int L, int B, int nb, long T_cap, int C, const int* src, const int* lo,
                                  const int* hi, hipStream_t stream) {
  if (L <= 0 || B <= 0 || T_cap <= 0) return MH_OK;
  if (!caches || !src || !lo || !hi || C <= 0) return MH_ERR_ARG;
  if (nb < 1 || nb > 8 || (C % 8) != 0 || (long)L * B > 65535) return MH_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)((T_cap + RKP - 1) / RKP), (unsigned)((C + 8 * RKT - 1) / (8 * RKT)), (unsigned)(L * B));
  hipLaunchKernelGGL(beam_reorder_kv_kernel<false>, grid, dim3(RKT), 0, stream, (bf16_t* const*)caches, B, nb, T_cap, C, src, lo,
                     hi, (const int*)nullptr);
  MH_CHECK_LAUNCH();
  return MH_OK;
}

extern "C" int mh_beam_reorder_kv_items(void* const* caches, int L, int G, int nb, long T_cap, int C, const int* src, const int* lo,
                                        const int* hi, const int* live, hipStream_t stream) {
  if (L <= 0 || G <= 0 || T_cap <= 0) return MH_OK;
  if (!caches || !src || !lo || !hi || !live || C <= 0) return MH_ERR_ARG;
  if (nb < 1 || nb > 8 || (C % 8) != 0 || (long)L * G > 65535) return MH_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)((T_cap + RKP - 1) / RKP), (unsigned)((C + 8 * RKT - 1) / (8 * RKT)), (unsigned)(L * G));
  hipLaunchKernelGGL(beam_reorder_kv_kernel<true>, grid, dim3(RKT), 0, stream, (bf16_t* const*)caches, G, nb, T_cap, C, src, lo, hi,
                     live);
  MH_CHECK_LAUNCH();
  return MH_OK;
}
