// Device-side sampling for the KV-cache decode: HF's per-row logits-processor chain of `generate(do_sample=True, ...)`
// (transformers generation/utils.py `_get_logits_processor`: RepetitionPenalty -> MinLength -> Temperature -> TopK -> TopP ->
// multinomial) as two kernels, so a sampled token step stays one fixed hipGraph with one small device->host record, like greedy.
//   repetition_penalty_kernel  in place on fp32 logits: x = x * p if x < 0 else x / p for every id in the row's seen-token bitmap,
//                              after the token just fed in (prev_ids) was added to it.
//   sample_rows_kernel         one 1024-thread workgroup per row, row resident in registers (V <= 32768): ban, temperature, top-k
//                              threshold by a 4-pass radix select, the kept candidates (ties at the k-th value included, at most
//                              MH_SAMPLE_CAP) sorted in LDS by (logit desc, id asc), softmax, top-p cut, inverse-CDF draw.
//                              The two zeros are one value, a NaN logit is -inf for the draw, a +inf logit is drawn alone
//                              (the contract is mh_sample_rows' in include/myriad_hip.h).
// Random numbers: Philox4x32-10 (Salmon et al., SC'11), key = the 64-bit seed, counter = (t, 0, row, 0), u = (x0 >> 8) * 2^-24.
// The seed, the step counter and (inv_temp, top_p, top_k, penalty) are read from device memory: graph replays draw fresh numbers
// and a change of the knobs needs no re-capture.
// The decode-slot engine runs the same three launches in a per-row ("slots") form: row r has its own live flag, its own seed and its
// own generated-token count gen[r], which is both the Philox step of its next draw -- counter = (gen[r], 0, 0, 0), so a request's
// stream depends on (its seed, the token index) only, not on the slot it sits in or on its neighbours -- and what decides its EOS
// ban (gen[r] < min_length); min_length and eos_id follow the four knobs in `params` (six floats).  The uniform entry points are
// instances of the same bodies with the per-row reads compiled out.
#include "common.h"
#include "smp_rng.h"          // SNT / SNW / MH_SAMPLE_CAP, Philox4x32-10, the ordered keys and the prefix sums

struct SmpTop { float best; int idx; float second; };
__device__ __forceinline__ SmpTop smp_combine(const SmpTop& a, const SmpTop& b) {
  const bool take_b = (b.best > a.best) || (b.best == a.best && b.idx < a.idx);
  SmpTop o;
  o.best = take_b ? b.best : a.best;
  o.idx = take_b ? b.idx : a.idx;
  o.second = fmaxf(fmaxf(a.second, b.second), take_b ? a.best : b.best);
  return o;
}

// params = (inv_temp, top_p, top_k, penalty) f32 on the device; seed = one u64; step = the decode step counter (or null): t = *step + t_add.
// ROWS: the slot form -- params = (inv_temp, top_p, top_k, penalty, min_length, eos_id), seed[row] and gen[row] per row, t = gen[row],
// the ban is eos_id while gen[row] < min_length (ban_id, step and t_add are unused); a row with live[row] == 0 (live may be null:
// every row is live) leaves before the first barrier -- live[row] is uniform over the workgroup, one scalar branch -- and writes
// out = -1, margin = p_max = 0, kept = 0.  DRAW = false stops after the arg-max, margin and p_max: the greedy pick with the same
// per-row ban (kept, u_out and seed are not touched).
template <bool ROWS, bool DRAW>
__global__ __launch_bounds__(SNT) void sample_rows_kernel_t(const float* __restrict__ logits, long ldl, long* __restrict__ out,
                                                float* __restrict__ margin, float* __restrict__ pmax, int* __restrict__ kept,
                                                float* __restrict__ u_out, int V, int ban_id, const float* __restrict__ params,
                                                const unsigned long long* __restrict__ seed, const int* __restrict__ step, int t_add,
                                                const int* __restrict__ gen, const int* __restrict__ live) {
  __shared__ float sb[SNW], s2[SNW], red[SNW], fsum[SNW];
  __shared__ int si[SNW], isum[SNW];
  __shared__ unsigned hist[256];
  __shared__ unsigned sh_prefix, sh_rank;
  __shared__ float sh_u;
  __shared__ unsigned long long cand[MH_SAMPLE_CAP];
  __shared__ float cum[MH_SAMPLE_CAP];
  const long row = blockIdx.x;
  const int tid = threadIdx.x;
  const float* x = logits + row * ldl;
  const float ninf = -__builtin_inff();
  const float inv_temp = params[0], top_p = params[1];
  int k = (int)params[2];
  k = k < 1 ? 1 : (k > V ? V : k);
  if (ROWS) {
    if (live && !live[row]) {
      if (tid == 0) {
        out[row] = -1;
        margin[row] = 0.f;
        pmax[row] = 0.f;
        if (DRAW) kept[row] = 0;
      }
      return;
    }
    ban_id = gen[row] < (int)params[4] ? (int)params[5] : -1;
  }

  if (DRAW && tid == 0) {
    const unsigned long long sd = ROWS ? seed[row] : *seed;
    unsigned c[4] = {ROWS ? (unsigned)gen[row] : (unsigned)((step ? *step : 0) + t_add), 0u, ROWS ? 0u : (unsigned)row, 0u};
    philox4x32_10(c, (unsigned)sd, (unsigned)(sd >> 32));
    sh_u = (float)(c[0] >> 8) * (1.0f / 16777216.0f);
  }

  // 1. the row in registers (the layout of argmax_pmax_wide_kernel, so margin and p_max come out bit-equal to it), ban
  float4_t xv[8];
  const int t4 = tid * 4;
  SmpTop tp = {ninf, t4 < V ? t4 : 0, ninf};
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int j = (i * SNT + tid) * 4;
    xv[i] = (float4_t){ninf, ninf, ninf, ninf};
    if (j + 3 < V) xv[i] = *reinterpret_cast<const float4_t*>(x + j);
    else
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (j + e < V) xv[i][e] = x[j + e];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (j + e == ban_id) xv[i][e] = ninf;
      const float v = xv[i][e];
      if (v > tp.best) { tp.second = tp.best; tp.best = v; tp.idx = j + e; }
      else if (v > tp.second) tp.second = v;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    SmpTop q;
    q.best = __shfl_xor(tp.best, o, 64);
    q.idx = __shfl_xor(tp.idx, o, 64);
    q.second = __shfl_xor(tp.second, o, 64);
    tp = smp_combine(tp, q);
  }
  const int w = tid >> 6, l = tid & 63;
  if (l == 0) { sb[w] = tp.best; si[w] = tp.idx; s2[w] = tp.second; }
  __syncthreads();
  SmpTop all = {sb[0], si[0], s2[0]};
#pragma unroll
  for (int i = 1; i < SNW; ++i) all = smp_combine(all, (SmpTop){sb[i], si[i], s2[i]});
  {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) s += __expf((xv[i][e] - all.best) * inv_temp);
    s = block_sum<SNW>(s, red);
    if (tid == 0) {
      if (margin) margin[row] = all.best - all.second;
      if (pmax) pmax[row] = 1.f / s;
      if (!DRAW) out[row] = all.idx;
    }
  }
  if (!DRAW) return;
  if (all.best == __builtin_inff()) {     // a +inf logit takes all the mass: the arg-max (its lowest id), alone, whatever top_p is
    if (tid == 0) {
      out[row] = all.idx;
      kept[row] = 1;
      if (u_out) u_out[row] = sh_u;
    }
    return;
  }

  // 2. temperature (HF TemperatureLogitsWarper), then the k-th largest tempered logit: radix select over the ordered keys, 8 bits
  //    a pass from the top; past-V and banned entries are -inf, the smallest key, so they never move the k-th value of a row
  //    with k <= V.  A NaN logit is -inf here, and here only: xv, which margin and p_max were formed from, stays as loaded
  unsigned kv[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) kv[i][e] = smp_key_draw(xv[i][e] * inv_temp);
  unsigned prefix = 0, rank = (unsigned)k;
#pragma unroll 1
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    const unsigned hmask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if ((kv[i][e] & hmask) == prefix) atomicAdd(&hist[(kv[i][e] >> shift) & 255u], 1u);
    __syncthreads();
    if (tid < 64) {                       // lane l holds bins 255-4l .. 252-4l (largest first)
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
  const unsigned thr = prefix;            // key of the k-th largest; every finite logit with key >= thr is kept (ties included)

  // 3. gather the candidates, (key, ~id) in one u64 so that a descending sort is (logit desc, id asc)
  int mine = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) mine += (kv[i][e] >= thr && kv[i][e] > KEY_NINF) ? 1 : 0;
  const int incl = smp_block_scan<int>(mine, isum);
  int n = 0;
#pragma unroll
  for (int i = 0; i < SNW; ++i) n += isum[i];
  if (n == 0 || n > MH_SAMPLE_CAP) {      // tied top-k set past the cap (or nothing finite): the host draws this row
    if (tid == 0) {
      out[row] = all.idx;
      kept[row] = -1;
      if (u_out) u_out[row] = sh_u;
    }
    return;
  }
  int o = incl - mine;
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (kv[i][e] >= thr && kv[i][e] > KEY_NINF) {
        const unsigned id = (unsigned)((i * SNT + tid) * 4 + e);
        cand[o++] = ((unsigned long long)kv[i][e] << 32) | (0xffffffffu - id);
      }
  int P = 1;
  while (P < n) P <<= 1;
  for (int i = n + tid; i < P; i += SNT) cand[i] = 0ull;      // below every candidate
  __syncthreads();

  // 4. bitonic sort of the P <= 1024 entries, descending
  for (int size = 2; size <= P; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      if (tid < (P >> 1)) {
        const int lo = 2 * tid - (tid & (stride - 1)), hi = lo + stride;
        const bool desc = (lo & size) == 0;
        const unsigned long long a = cand[lo], b = cand[hi];
        if ((a < b) == desc) { cand[lo] = b; cand[hi] = a; }
      }
      __syncthreads();
    }

  // 5. softmax over the top-k set, top-p cut (keep i iff its exclusive prefix mass < top_p), inverse-CDF draw
  const float vmax = smp_unkey((unsigned)(cand[0] >> 32));
  if (vmax == __builtin_inff()) {         // a finite logit the temperature pushed to +inf: as a +inf logit, the first of the order
    if (tid == 0) {
      out[row] = (long)(0xffffffffu - (unsigned)(cand[0] & 0xffffffffull));
      kept[row] = 1;
      if (u_out) u_out[row] = sh_u;
    }
    return;
  }
  const float p = tid < n ? expf(smp_unkey((unsigned)(cand[tid] >> 32)) - vmax) : 0.f;
  const float c = smp_block_scan<float>(p, fsum);
  if (tid < n) cum[tid] = c;
  __syncthreads();
  const float total = cum[n - 1];
  const float excl = tid == 0 ? 0.f : (tid < n ? cum[tid - 1] : 0.f);
  int mk = __syncthreads_count(tid < n && (top_p >= 1.f || excl < top_p * total));
  mk = mk > 0 ? mk : 1;                   // the largest token is always kept (min_tokens_to_keep = 1)
  const float target = sh_u * cum[mk - 1];
  int sel = __syncthreads_count(tid < mk && cum[tid] <= target);
  sel = sel < mk ? sel : mk - 1;
  if (tid == 0) {
    out[row] = (long)(0xffffffffu - (unsigned)(cand[sel] & 0xffffffffull));
    kept[row] = mk;
    if (u_out) u_out[row] = sh_u;
  }
}

extern "C" int mh_sample_rows(const float* logits, long ldl, long* out, float* margin, float* pmax, int* kept, float* u_out, int R,
                              int V, int ban_id, const float* params, const unsigned long long* seed, const int* step, int t_add,
                              hipStream_t stream) {
  if (R <= 0) return MH_OK;
  if (!logits || !out || !kept || !params || !seed || V <= 0 || ldl < V) return MH_ERR_ARG;
  if (V > 8 * SNT * 4 || (ldl % 4) != 0 || ((uintptr_t)logits & 15)) return MH_ERR_UNSUPPORTED;
  hipLaunchKernelGGL((sample_rows_kernel_t<false, true>), dim3(R), dim3(SNT), 0, stream, logits, ldl, out, margin, pmax, kept, u_out, V,
                     ban_id, params, seed, step, t_add, (const int*)nullptr, (const int*)nullptr);
  MH_CHECK_LAUNCH();
  return MH_OK;
}

// The slot forms: what the uniform sampler refuses they refuse; margin and pmax are required (an idle row writes them).
static int slots_args(const float* logits, long ldl, int V) {
  if (V <= 0 || ldl < V) return MH_ERR_ARG;
  if (V > 8 * SNT * 4 || (ldl % 4) != 0 || ((uintptr_t)logits & 15)) return MH_ERR_UNSUPPORTED;
  return MH_OK;
}
extern "C" int mh_sample_rows_slots(const float* logits, long ldl, long* out, float* margin, float* pmax, int* kept, float* u_out, int R,
                                    int V, const float* params, const unsigned long long* seed, const int* gen, const int* live,
                                    hipStream_t stream) {
  if (R <= 0) return MH_OK;
  if (!logits || !out || !margin || !pmax || !kept || !params || !seed || !gen) return MH_ERR_ARG;
  if (const int e = slots_args(logits, ldl, V)) return e;
  hipLaunchKernelGGL((sample_rows_kernel_t<true, true>), dim3(R), dim3(SNT), 0, stream, logits, ldl, out, margin, pmax, kept, u_out, V, -1,
                     params, seed, (const int*)nullptr, 0, gen, live);
  MH_CHECK_LAUNCH();
  return MH_OK;
}
extern "C" int mh_argmax_pmax_rows_slots(const float* logits, long ldl, long* out, float* margin, float* pmax, int R, int V,
                                         const float* params, const int* gen, const int* live, hipStream_t stream) {
  if (R <= 0) return MH_OK;
  if (!logits || !out || !margin || !pmax || !params || !gen) return MH_ERR_ARG;
  if (const int e = slots_args(logits, ldl, V)) return e;
  hipLaunchKernelGGL((sample_rows_kernel_t<true, false>), dim3(R), dim3(SNT), 0, stream, logits, ldl, out, margin, pmax, (int*)nullptr,
                     (float*)nullptr, V, -1, params, (const unsigned long long*)nullptr, (const int*)nullptr, 0, gen, live);
  MH_CHECK_LAUNCH();
  return MH_OK;
}

// ---------------------------------------------------------------------------------------------------- repetition penalty
// HF RepetitionPenaltyLogitsProcessor on the generated tokens (generate(inputs_embeds=...) starts input_ids empty): each id once,
// however often it was generated.  The thread that owns the bitmap word of prev_ids[row] sets its bit, so no other thread races it.
// ROWS: the slot form, a row with live[row] == 0 changes neither its logits nor its bitmap.
template <bool ROWS>
__device__ __forceinline__ void repetition_penalty_body(float* __restrict__ logits, long ldl, unsigned* __restrict__ seen,
                                                        const long* __restrict__ prev_ids, int V, int W,
                                                        const float* __restrict__ penalty, const int* __restrict__ live) {
  const long row = blockIdx.x;
  if (ROWS && !live[row]) return;
  const float pen = *penalty;
  float* x = logits + row * ldl;
  unsigned* sr = seen + row * W;
  const long nid = prev_ids ? prev_ids[row] : -1;
  for (int w = threadIdx.x; w < W; w += blockDim.x) {
    unsigned m = sr[w];
    if (nid >= 0 && nid < V && (int)(nid >> 5) == w) {
      m |= 1u << (nid & 31);
      sr[w] = m;
    }
    while (m) {
      const int j = w * 32 + __builtin_ctz(m);
      m &= m - 1;
      if (j < V) {
        const float v = x[j];
        x[j] = v < 0.f ? v * pen : v / pen;
      }
    }
  }
}

__global__ __launch_bounds__(256) void repetition_penalty_kernel(float* __restrict__ logits, long ldl, unsigned* __restrict__ seen,
                                                                 const long* __restrict__ prev_ids, int V, int W,
                                                                 const float* __restrict__ penalty) {
  repetition_penalty_body<false>(logits, ldl, seen, prev_ids, V, W, penalty, nullptr);
}
__global__ __launch_bounds__(256) void repetition_penalty_slots_kernel(float* __restrict__ logits, long ldl, unsigned* __restrict__ seen,
                                                                       const long* __restrict__ prev_ids, int V, int W,
                                                                       const float* __restrict__ penalty, const int* __restrict__ live) {
  repetition_penalty_body<true>(logits, ldl, seen, prev_ids, V, W, penalty, live);
}

extern "C" int mh_repetition_penalty_rows(float* logits, long ldl, unsigned* seen, const long* prev_ids, int R, int V,
                                          const float* penalty, hipStream_t stream) {
  if (R <= 0) return MH_OK;
  if (!logits || !seen || !penalty || V <= 0 || ldl < V) return MH_ERR_ARG;
  hipLaunchKernelGGL(repetition_penalty_kernel, dim3(R), dim3(256), 0, stream, logits, ldl, seen, prev_ids, V, (V + 31) / 32, penalty);
  MH_CHECK_LAUNCH();
  return MH_OK;
}

extern "C" int mh_repetition_penalty_rows_slots(float* logits, long ldl, unsigned* seen, const long* prev_ids, int R, int V,
                                                const float* penalty, const int* live, hipStream_t stream) {
  if (R <= 0) return MH_OK;
  if (!logits || !seen || !penalty || !live || V <= 0 || ldl < V) return MH_ERR_ARG;
  hipLaunchKernelGGL(repetition_penalty_slots_kernel, dim3(R), dim3(256), 0, stream, logits, ldl, seen, prev_ids, V, (V + 31) / 32,
                     penalty, live);
  MH_CHECK_LAUNCH();
  return MH_OK;
}

// ---------------------------------------------------------------------------------------------------- end of a sampled step
// mh_decode_advance with one more record row: rec[4][R] f32 = (id, margin, p_max, kept) -- kept = -1 asks the host to draw the row.
__global__ void decode_advance_kept_kernel(const long* __restrict__ nxt, const float* __restrict__ margin, const float* __restrict__ pmax,
                                           const int* __restrict__ kept, float* __restrict__ rec, long* __restrict__ next_ids,
                                           int* __restrict__ step, int* __restrict__ pos, int* __restrict__ kvlen, int R) {
  for (int r = threadIdx.x; r < R; r += blockDim.x) {
    const long id = nxt[r];
    rec[r] = (float)id;
    rec[R + r] = margin[r];
    rec[2 * R + r] = pmax[r];
    rec[3 * R + r] = (float)kept[r];
    next_ids[r] = id;
    pos[r] += 1;
    kvlen[r] += 1;
  }
  if (threadIdx.x == 0) *step += 1;
}

extern "C" int mh_decode_advance_kept(const long* nxt, const float* margin, const float* pmax, const int* kept, float* rec, long* next_ids,
                                      int* step, int* pos, int* kvlen, int R, hipStream_t stream) {
  if (R <= 0) return MH_OK;
  if (!nxt || !margin || !pmax || !kept || !rec || !next_ids || !step || !pos || !kvlen) return MH_ERR_ARG;
  hipLaunchKernelGGL(decode_advance_kept_kernel, dim3(1), dim3(64), 0, stream, nxt, margin, pmax, kept, rec, next_ids, step, pos, kvlen,
                     R);
  MH_CHECK_LAUNCH();
  return MH_OK;
}

// The slot engine's form (mh_decode_advance_rows with the kept row and the per-row token count): a row with live[r] != 0 records
// (id, margin, p_max, kept), feeds its id back and advances pos, kvlen and gen; an idle row records (-1, 0, 0, 0) and keeps all its
// state.  kept may be null (the greedy pick has no kept set): the fourth record row is then 0.
__global__ void decode_advance_kept_rows_kernel(const long* __restrict__ nxt, const float* __restrict__ margin,
                                                const float* __restrict__ pmax, const int* __restrict__ kept, float* __restrict__ rec,
                                                long* __restrict__ next_ids, int* __restrict__ step, int* __restrict__ pos,
                                                int* __restrict__ kvlen, int* __restrict__ gen, const int* __restrict__ live, int R) {
  for (int r = threadIdx.x; r < R; r += blockDim.x) {
    if (live[r]) {
      const long id = nxt[r];
      rec[r] = (float)id;
      rec[R + r] = margin[r];
      rec[2 * R + r] = pmax[r];
      rec[3 * R + r] = kept ? (float)kept[r] : 0.f;
      next_ids[r] = id;
      pos[r] += 1;
      kvlen[r] += 1;
      gen[r] += 1;
    } else {
      rec[r] = -1.f;
      rec[R + r] = 0.f;
      rec[2 * R + r] = 0.f;
      rec[3 * R + r] = 0.f;
    }
  }
  if (threadIdx.x == 0) *step += 1;
}

extern "C" int mh_decode_advance_kept_rows(const long* nxt, const float* margin, const float* pmax, const int* kept, float* rec,
                                           long* next_ids, int* step, int* pos, int* kvlen, int* gen, const int* live, int R,
                                           hipStream_t stream) {
  if (R <= 0) return MH_OK;
  if (!nxt || !margin || !pmax || !rec || !next_ids || !step || !pos || !kvlen || !gen || !live) return MH_ERR_ARG;
  hipLaunchKernelGGL(decode_advance_kept_rows_kernel, dim3(1), dim3(64), 0, stream, nxt, margin, pmax, kept, rec, next_ids, step, pos,
                     kvlen, gen, live, R);
  MH_CHECK_LAUNCH();
  return MH_OK;
}
