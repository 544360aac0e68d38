// Beam-search multinomial sampling and the repetition penalty under beams (HF GenerationMixin._beam_search with do_sample=True:
// log_softmax -> RepetitionPenalty -> MinLength ban -> Temperature -> TopK -> TopP (min_tokens_to_keep = 2) -> + beam score ->
// multinomial(2 * nb) without replacement), as the selection pair of a beam step.  Drawing K items without replacement from
// softmax(acc) in draw order is taking the top K of acc + Gumbel noise (Plackett-Luce), so the step stays a top-K:
//   beam_sample_row_kernel   one 1024-thread workgroup per logits row (V <= 32768, row in registers, the layout and the
//                            logsumexp of beam_row_topk_kernel, so the log-probs are bit-equal to it): penalty on the log-probs
//                            of the ids in the row's seen bitmap, ban, w = lp * inv_temp, the k-th largest w by the sampler's radix
//                            select (ties kept), the top-p cut over the sorted candidates (the best two always stay), acc = w +
//                            score, key = acc + g, g = -log(-log(u)), u from Philox4x32-10 with counter (t, flat, item, 1); then
//                            the row's top K = 2 * nb by (key desc, token asc) as (key, acc, token).  Candidates that are out
//                            carry key = acc = -inf and still rank (by token), so a row always hands on K valid tokens.
//   beam_sample_merge_kernel one workgroup per item: ranks the nb * K survivors by (key desc, flat asc), writes (acc, flat) -- the
//                            step's record --, the keys when asked, the item's overflow flag, and carries the step / pos / kvlen
//                            advance.
//   beam_seen_update_kernel  seen[r] = seen[src[r]] | bit(ids[r]) in place: a thread owns one bitmap word for all nb sibling rows
//                            of an item, loads every source word, then stores (beam_reorder_kv_kernel's hazard argument).
// DRAW = false compiles the temperature, the cuts and the noise out: key = acc, deterministic beam search with the penalty.
// (inv_temp, top_p, top_k, penalty), the seed and the step counter are read from device memory, as in sample.hip.
// The three kernels are templates on ITEMS (the decode slots' beam groups, one request per group of nb rows, as in beam.hip): group
// g then has its own live flag, generated count gen[g] (its EOS ban and its Philox step) and seed[g] in device memory, the item
// field of its Philox counter is 0 -- it draws what it would draw alone at B = 1 --, and an idle group's workgroups leave on a
// scalar branch.  ITEMS = false is the code above, unchanged.
#include "common.h"
#include "smp_rng.h"

#define BSV 32                  // values per thread: V <= SNT * BSV = 32768
#define BSKMAX 16               // K = 2 * nb, nb <= 8

// a comes strictly before b: higher key, ties to the lower index (NaN keys are mapped to -inf before they get here)
__device__ __forceinline__ bool bs_before(float as, int ai, float bs, int bi) { return as > bs || (as == bs && ai < bi); }

__device__ __forceinline__ float bs_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float bs_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// part_k / part_a / part_i [R][K] = (key, acc, token) of the row's top K by key; part_f [R] = 1 when the row's tied top-k set
// passed MH_SAMPLE_CAP (the top-p cut was not applied: the host redoes the item)
// ITEMS: rows row / nb * nb .. + nb - 1 are group g's; an idle group's rows leave before they load a logit or a bitmap word
// (blockIdx is uniform: a scalar branch), a live one bans bprm[1] while gen[g] < bprm[0] and draws Philox step gen[g] + t_add of
// seed[g] with the counter's item field 0
template <bool DRAW, bool ITEMS>
__global__ __launch_bounds__(SNT) void beam_sample_row_kernel(const float* __restrict__ logits, long ldl, const float* __restrict__ scores,
                                                              const unsigned* __restrict__ seen, int W, float* __restrict__ part_k,
                                                              float* __restrict__ part_a, int* __restrict__ part_i,
                                                              int* __restrict__ part_f, int V, int nb, int K, int ban_id,
                                                              const float* __restrict__ prm, const unsigned long long* __restrict__ seed,
                                                              const int* __restrict__ step, int t_add,
                                                              const int* __restrict__ live, const int* __restrict__ gen,
                                                              const int* __restrict__ bprm) {
  if (ITEMS) {
    const int g = blockIdx.x / nb;
    if (!live[g]) return;
    ban_id = gen[g] < bprm[0] ? bprm[1] : -1;
    if (DRAW) {
      seed += g;
      step = gen + g;
    }
  }
  __shared__ float red[SNW];
  __shared__ float cs[SNW * BSKMAX], ca[SNW * BSKMAX];
  __shared__ int ci[SNW * BSKMAX];
  __shared__ unsigned hist[256];
  __shared__ unsigned sh_prefix, sh_rank;
  __shared__ int isum[SNW];
  __shared__ float fsum[SNW];
  __shared__ unsigned long long cand[MH_SAMPLE_CAP];
  __shared__ float cum[MH_SAMPLE_CAP];
  const long row = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float* x = logits + row * ldl;
  const float ninf = -__builtin_inff();

  // 1. log_softmax as beam_row_topk_kernel forms it: (x - max) - log(sum exp(x - max)), the same layout and summation order
  float v[BSV];
  float mx = ninf;
#pragma unroll
  for (int i = 0; i < BSV; ++i) {
    const int j = i * SNT + tid;
    v[i] = j < V ? x[j] : ninf;
    mx = fmaxf(mx, v[i]);
  }
  mx = bs_wave_max(mx);
  if (lane == 0) red[wv] = mx;
  __syncthreads();
  mx = red[0];
#pragma unroll
  for (int i = 1; i < SNW; ++i) mx = fmaxf(mx, red[i]);
  __syncthreads();
  float se = 0.f;
#pragma unroll
  for (int i = 0; i < BSV; ++i) se += expf(v[i] - mx);       // -inf (padding, a -inf logit) contributes 0
  se = bs_wave_sum(se);
  if (lane == 0) red[wv] = se;
  __syncthreads();
  se = 0.f;
#pragma unroll
  for (int i = 0; i < SNW; ++i) se += red[i];
  const float ls = logf(se), bsc = scores[row];
#pragma unroll
  for (int i = 0; i < BSV; ++i) {
    const float lp = (v[i] - mx) - ls;
    v[i] = lp == lp ? lp : ninf;                              // a NaN log-prob (a NaN or +inf logit in the row) is -inf
  }

  // 2. repetition penalty on the log-probs of the ids this hypothesis generated; 3. the EOS ban
  const float pen = seen ? prm[3] : 1.f;
  if (pen != 1.f) {
    const unsigned* sr = seen + row * W;
#pragma unroll
    for (int i = 0; i < BSV; ++i) {
      const int j = i * SNT + tid;
      if (j < V && ((sr[j >> 5] >> (j & 31)) & 1u)) v[i] = v[i] < 0.f ? v[i] * pen : v[i] / pen;
    }
  }
#pragma unroll
  for (int i = 0; i < BSV; ++i)
    if (i * SNT + tid == ban_id) v[i] = ninf;

  float a[BSV];                                               // acc; v becomes the key
  if (!DRAW) {
#pragma unroll
    for (int i = 0; i < BSV; ++i) {
      const float s = bsc + v[i];
      v[i] = s == s ? s : ninf;
      a[i] = v[i];
    }
    if (tid == 0) part_f[row] = 0;
  } else {
    // 4. temperature; 5. the k-th largest w by a 4-pass radix select over the ordered keys (sample_rows_kernel's), ties kept
    const float inv_temp = prm[0], top_p = prm[1];
    int k = (int)prm[2];
    k = k < 2 ? 2 : k;                                        // min_tokens_to_keep = 2 under beams
    k = k > V ? V : k;
#pragma unroll
    for (int i = 0; i < BSV; ++i) {
      const float w = __fmul_rn(v[i], inv_temp);
      v[i] = w == w ? w : ninf;
    }
    unsigned prefix = 0, rank = (unsigned)k;
#pragma unroll 1
    for (int pass = 0; pass < 4; ++pass) {
      const int shift = 24 - 8 * pass;
      const unsigned hmask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
      if (tid < 256) hist[tid] = 0;
      __syncthreads();
      // Log-probs share their top bits, so most lanes of a wave name the same two or three bins: up to four rounds of "one
      // lane adds the count of every lane in its bin" come first, and whoever is left after them adds for itself
#pragma unroll
      for (int i = 0; i < BSV; ++i) {
        const unsigned kv = smp_key(v[i]);                    // k <= V: the padding past V never holds the k-th value
        const bool in = i * SNT + tid < V && (kv & hmask) == prefix;
        const unsigned bin = (kv >> shift) & 255u;
        unsigned long long todo = __ballot(in);
        for (int r = 0; r < 4 && todo; ++r) {
          const int leader = __ffsll((long long)todo) - 1;
          const unsigned lb = __shfl(bin, leader, 64);
          const unsigned long long same = __ballot(in && bin == lb);
          if (lane == leader) atomicAdd(&hist[lb], (unsigned)__popcll(same));
          todo &= ~same;
        }
        if ((todo >> lane) & 1ull) atomicAdd(&hist[bin], 1u);
      }
      __syncthreads();
      if (tid < 64) {                     // lane l holds bins 255-4l .. 252-4l (largest first)
        unsigned c[4], s = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) { c[j] = hist[255 - 4 * tid - j]; s += c[j]; }
        unsigned before = smp_wave_scan(s) - s;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (before < rank && rank <= before + c[j]) {
            sh_prefix = prefix | ((unsigned)(255 - 4 * tid - j) << shift);
            sh_rank = rank - before;
          }
          before += c[j];
        }
      }
      __syncthreads();
      prefix = sh_prefix;
      rank = sh_rank;
    }
    const unsigned KEY_NINF = SMP_KEY_NINF;
    const unsigned thr = prefix;            // key of the k-th largest; every finite w with key >= thr is a candidate
    int mine = 0;
#pragma unroll
    for (int i = 0; i < BSV; ++i) {
      const unsigned kv = smp_key(v[i]);
      mine += (kv >= thr && kv > KEY_NINF) ? 1 : 0;
    }
    const int incl = smp_block_scan<int>(mine, isum);
    int n = 0;
#pragma unroll
    for (int i = 0; i < SNW; ++i) n += isum[i];
    const bool over = n > MH_SAMPLE_CAP;
    if (tid == 0) part_f[row] = over ? 1 : 0;

    // 6. top-p over the candidates sorted by (w desc, id asc): candidate i stays while its exclusive prefix mass is below
    //    top_p * total, the best two always; `cut` = the (key, ~id) word of the last one that stays.  Past the cap the cut is
    //    not applied (the flag asks the host to redo the item); with two candidates or fewer there is nothing to cut
    unsigned long long cut = 0ull;
    if (top_p < 1.f && !over && n > 2) {
      int o = incl - mine;
#pragma unroll
      for (int i = 0; i < BSV; ++i) {
        const unsigned kv = smp_key(v[i]);
        if (kv >= thr && kv > KEY_NINF) cand[o++] = ((unsigned long long)kv << 32) | (0xffffffffu - (unsigned)(i * SNT + tid));
      }
      int P = 1;
      while (P < n) P <<= 1;
      for (int i = n + tid; i < P; i += SNT) cand[i] = 0ull;    // below every candidate
      __syncthreads();
      for (int size = 2; size <= P; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
          if (tid < (P >> 1)) {
            const int lo = 2 * tid - (tid & (stride - 1)), hi = lo + stride;
            const bool desc = (lo & size) == 0;
            const unsigned long long ea = cand[lo], eb = cand[hi];
            if ((ea < eb) == desc) { cand[lo] = eb; cand[hi] = ea; }
          }
          __syncthreads();
        }
      const float vmax = smp_unkey((unsigned)(cand[0] >> 32));
      const float p = tid < n ? expf(smp_unkey((unsigned)(cand[tid] >> 32)) - vmax) : 0.f;
      const float c = smp_block_scan<float>(p, fsum);
      if (tid < n) cum[tid] = c;
      __syncthreads();
      const float total = cum[n - 1];
      const float excl = tid == 0 ? 0.f : (tid < n ? cum[tid - 1] : 0.f);
      int mk = __syncthreads_count(tid < n && excl < top_p * total);
      mk = mk < 2 ? 2 : mk;
      cut = cand[mk - 1];
    }

    // 7. acc = w + score for what stays; 8. key = acc + Gumbel noise from the candidate's own Philox stream
    const unsigned long long sd = *seed;
    const unsigned t = (unsigned)((step ? *step : 0) + t_add);
    const unsigned item = ITEMS ? 0u : (unsigned)(row / nb), base = (unsigned)(row % nb) * (unsigned)V;
#pragma unroll
    for (int i = 0; i < BSV; ++i) {
      const int j = i * SNT + tid;
      const unsigned kv = smp_key(v[i]);
      const bool in = kv >= thr && kv > KEY_NINF && ((((unsigned long long)kv << 32) | (0xffffffffu - (unsigned)j)) >= cut);
      float acc = ninf, key = ninf;
      if (in) {
        acc = __fadd_rn(v[i], bsc);
        acc = acc == acc ? acc : ninf;
        unsigned c[4] = {t, base + (unsigned)j, item, 1u};
        philox4x32_10(c, (unsigned)sd, (unsigned)(sd >> 32));
        const float u = ((float)(c[0] >> 9) + 0.5f) * (1.0f / 8388608.0f);      // exact in fp32, never 0 or 1
        key = acc + (-logf(-logf(u)));
        key = key == key ? key : ninf;
      }
      a[i] = acc;
      v[i] = key;
    }
  }

  // 9. per-wave top K by (key desc, token asc): round k takes the best candidate strictly after round k-1's winner
  float ts = __builtin_inff();
  int ti = -1;
  for (int k = 0; k < K; ++k) {
    float bk = ninf, ba = ninf;
    int bi = 0x7fffffff;                                     // "none yet": any real candidate comes before it
#pragma unroll
    for (int i = 0; i < BSV; ++i) {
      const int j = i * SNT + tid;
      if (j < V && bs_before(ts, ti, v[i], j) && bs_before(v[i], j, bk, bi)) { bk = v[i]; bi = j; ba = a[i]; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ok = __shfl_xor(bk, o, 64), oa = __shfl_xor(ba, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (bs_before(ok, oi, bk, bi)) { bk = ok; bi = oi; ba = oa; }
    }
    if (lane == 0) { cs[wv * K + k] = bk; ci[wv * K + k] = bi; ca[wv * K + k] = ba; }
    ts = bk;
    ti = bi;
  }
  __syncthreads();
  // rank the SNW * K wave survivors (beam_row_topk_kernel's argument: V >= K real candidates, so every rank < K is written once)
  const int n = SNW * K;
  for (int c = tid; c < n; c += SNT) {
    const float s = cs[c];
    const int i = ci[c];
    int rank = 0;
    for (int o = 0; o < n; ++o) rank += bs_before(cs[o], ci[o], s, i) ? 1 : 0;
    if (rank < K && i != 0x7fffffff) {
      part_k[row * K + rank] = s;
      part_a[row * K + rank] = ca[c];
      part_i[row * K + rank] = i;
    }
  }
}

// ITEMS: an idle group records (0.0, -1) K times and flag 0 and keeps its state; a live one advances its own rows' pos / kvlen and
// its gen (which the row kernel, an earlier launch, has read) -- or nothing when pos / kvlen are null (a refill's first pick)
template <bool ITEMS>
__global__ __launch_bounds__(128) void beam_sample_merge_kernel(const float* __restrict__ part_k, const float* __restrict__ part_a,
                                                                const int* __restrict__ part_i, const int* __restrict__ part_f,
                                                                float* __restrict__ out_s, int* __restrict__ out_i,
                                                                int* __restrict__ out_f, float* __restrict__ out_k, int nb, int V,
                                                                int K, int* __restrict__ step, int* __restrict__ pos,
                                                                int* __restrict__ kvlen, int n_adv,
                                                                const int* __restrict__ live, int* __restrict__ gen) {
  __shared__ float cs[8 * BSKMAX];
  __shared__ int ci[8 * BSKMAX];
  const int b = blockIdx.x, tid = threadIdx.x, n = nb * K;
  if (ITEMS && !live[b]) {
    if (tid < K) {
      out_s[(long)b * K + tid] = 0.f;
      out_i[(long)b * K + tid] = -1;
    }
    if (tid == 0) out_f[b] = 0;
    return;
  }
  float acc = 0.f;
  if (tid < n) {
    const long src = (long)b * n + tid;                      // row b * nb + tid / K, its rank tid % K
    cs[tid] = part_k[src];
    acc = part_a[src];
    ci[tid] = (tid / K) * V + part_i[src];
  }
  __syncthreads();
  if (tid < n) {
    const float s = cs[tid];
    const int i = ci[tid];
    int rank = 0;
    for (int o = 0; o < n; ++o) rank += bs_before(cs[o], ci[o], s, i) ? 1 : 0;
    if (rank < K) {
      out_s[(long)b * K + rank] = acc;
      out_i[(long)b * K + rank] = i;
      if (out_k) out_k[(long)b * K + rank] = s;
    }
  }
  if (tid == 0) {
    int f = 0;
    for (int j = 0; j < nb; ++j) f |= part_f[(long)b * nb + j];
    out_f[b] = f;
  }
  if (ITEMS) {
    if (pos && kvlen) {
      if (tid < nb) { pos[b * nb + tid] += 1; kvlen[b * nb + tid] += 1; }
      if (tid == 0) gen[b] += 1;
    }
  } else if (b == 0 && pos && kvlen) {
    for (int r = tid; r < n_adv; r += blockDim.x) { pos[r] += 1; kvlen[r] += 1; }
    if (tid == 0 && step) *step += 1;
  }
}

extern "C" int mh_beam_sample_topk(const float* logits, long ldl, const float* scores, const unsigned* seen, float* part_k,
                                   float* part_a, int* part_i, int* part_f, float* out_s, int* out_i, int* out_f, float* out_k, int B,
                                   int nb, int V, int ban_id, int draw, const float* params, const unsigned long long* seed, int* step,
                                   int t_add, int* pos, int* kvlen, int n_adv, hipStream_t stream) {
  if (B <= 0) return MH_OK;
  if (!logits || !scores || !part_k || !part_a || !part_i || !part_f || !out_s || !out_i || !out_f || V <= 0 || ldl < V) return MH_ERR_ARG;
  if ((draw && (!params || !seed)) || (seen && !params) || (!pos != !kvlen)) return MH_ERR_ARG;
  if (nb < 1 || nb > 8 || V > SNT * BSV || (V % 4) != 0 || V < 2 * nb || V < 3 || n_adv < 0) return MH_ERR_UNSUPPORTED;
  const int K = 2 * nb, W = (V + 31) / 32;
  if (draw)
    hipLaunchKernelGGL((beam_sample_row_kernel<true, false>), dim3(B * nb), dim3(SNT), 0, stream, logits, ldl, scores, seen, W, part_k,
                       part_a, part_i, part_f, V, nb, K, ban_id, params, seed, (const int*)step, t_add, (const int*)nullptr,
                       (const int*)nullptr, (const int*)nullptr);
  else
    hipLaunchKernelGGL((beam_sample_row_kernel<false, false>), dim3(B * nb), dim3(SNT), 0, stream, logits, ldl, scores, seen, W, part_k,
                       part_a, part_i, part_f, V, nb, K, ban_id, params, seed, (const int*)step, t_add, (const int*)nullptr,
                       (const int*)nullptr, (const int*)nullptr);
  MH_CHECK_LAUNCH();
  hipLaunchKernelGGL(beam_sample_merge_kernel<false>, dim3(B), dim3(128), 0, stream, part_k, part_a, part_i, part_f, out_s, out_i, out_f,
                     out_k, nb, V, K, step, pos, kvlen, n_adv, (const int*)nullptr, (int*)nullptr);
  MH_CHECK_LAUNCH();
  return MH_OK;
}

extern "C" int mh_beam_sample_topk_items(const float* logits, long ldl, const float* scores, const unsigned* seen, float* part_k,
                                         float* part_a, int* part_i, int* part_f, float* out_s, int* out_i, int* out_f, float* out_k,
                                         int G, int nb, int V, int draw, const float* params, const unsigned long long* seed,
                                         const int* live, int* gen, const int* bprm, int t_add, int* pos, int* kvlen,
                                         hipStream_t stream) {
  if (G <= 0) return MH_OK;
  if (!logits || !scores || !part_k || !part_a || !part_i || !part_f || !out_s || !out_i || !out_f || !live || !gen || !bprm || V <= 0 ||
      ldl < V)
    return MH_ERR_ARG;
  if ((draw && (!params || !seed)) || (seen && !params) || (!pos != !kvlen)) return MH_ERR_ARG;
  if (nb < 1 || nb > 8 || V > SNT * BSV || (V % 4) != 0 || V < 2 * nb || V < 3) return MH_ERR_UNSUPPORTED;
  const int K = 2 * nb, W = (V + 31) / 32;
  if (draw)
    hipLaunchKernelGGL((beam_sample_row_kernel<true, true>), dim3(G * nb), dim3(SNT), 0, stream, logits, ldl, scores, seen, W, part_k,
                       part_a, part_i, part_f, V, nb, K, -1, params, seed, (const int*)nullptr, t_add, live, (const int*)gen, bprm);
  else
    hipLaunchKernelGGL((beam_sample_row_kernel<false, true>), dim3(G * nb), dim3(SNT), 0, stream, logits, ldl, scores, seen, W, part_k,
                       part_a, part_i, part_f, V, nb, K, -1, params, seed, (const int*)nullptr, t_add, live, (const int*)gen, bprm);
  MH_CHECK_LAUNCH();
  hipLaunchKernelGGL(beam_sample_merge_kernel<true>, dim3(G), dim3(128), 0, stream, part_k, part_a, part_i, part_f, out_s, out_i, out_f,
                     out_k, nb, V, K, (int*)nullptr, pos, kvlen, 0, live, gen);
  MH_CHECK_LAUNCH();
  return MH_OK;
}

// ---------------------------------------------------------------------------------------------------- seen bitmaps
#define BST 256

// grid (ceil(W / BST), B): thread = one bitmap word of one item, for the item's nb rows
// ITEMS: a group with live[g] == 0 leaves before it reads a word (blockIdx.y is uniform: a scalar branch)
template <bool ITEMS>
__global__ __launch_bounds__(BST) void beam_seen_update_kernel(unsigned* __restrict__ seen, const int* __restrict__ src,
                                                               const long* __restrict__ ids, int nb, int W, int V,
                                                               const int* __restrict__ live) {
  if (ITEMS && !live[blockIdx.y]) return;
  const int w = blockIdx.x * BST + threadIdx.x;
  if (w >= W) return;
  const long r0 = (long)blockIdx.y * nb;
  unsigned val[8];
#pragma unroll
  for (int j = 0; j < 8; ++j)                                // every source word first ...
    if (j < nb) {
      int s = src[r0 + j] - (int)r0;
      if (s < 0 || s >= nb) s = j;                           // a parent outside the item is ignored (never a cross-item read)
      unsigned m = seen[(r0 + s) * W + w];
      const long id = ids[r0 + j];
      if (id >= 0 && id < V && (int)(id >> 5) == w) m |= 1u << (id & 31);
      val[j] = m;
    }
#pragma unroll
  for (int j = 0; j < 8; ++j)                                // ... then the stores
    if (j < nb) seen[(r0 + j) * W + w] = val[j];
}

extern "C" int mh_beam_seen_update(unsigned* seen, const int* src, const long* ids, int B, int nb, int V, hipStream_t stream) {
  if (B <= 0) return MH_OK;
  if (!seen || !src || !ids || V <= 0) return MH_ERR_ARG;
  if (nb < 1 || nb > 8 || B > 65535) return MH_ERR_UNSUPPORTED;
  const int W = (V + 31) / 32;
  hipLaunchKernelGGL(beam_seen_update_kernel<false>, dim3((W + BST - 1) / BST, B), dim3(BST), 0, stream, seen, src, ids, nb, W, V,
                     (const int*)nullptr);
  MH_CHECK_LAUNCH();
  return MH_OK;
}

extern "C" int mh_beam_seen_update_items(unsigned* seen, const int* src, const long* ids, int G, int nb, int V, const int* live,
                                         hipStream_t stream) {
  if (G <= 0) return MH_OK;
  if (!seen || !src || !ids || !live || V <= 0) return MH_ERR_ARG;
  if (nb < 1 || nb > 8 || G > 65535) return MH_ERR_UNSUPPORTED;
  const int W = (V + 31) / 32;
  hipLaunchKernelGGL(beam_seen_update_kernel<true>, dim3((W + BST - 1) / BST, G), dim3(BST), 0, stream, seen, src, ids, nb, W, V, live);
  MH_CHECK_LAUNCH();
  return MH_OK;
}
