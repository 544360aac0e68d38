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
#include "smp_rows.h"         // the sampler's row body

// The row body (smp_rows.h, shared with the verify step's sampler in draft_sample.hip) in its uniform and slot forms.
template <bool ROWS, bool DRAW>
__global__ __launch_bounds__(SNT) void sample_rows_kernel_t(const float* __restrict__ logits, long ldl, long* __restrict__ out,
                                                float* __restrict__ margin, float* __restrict__ pmax, int* __restrict__ kept,
                                                float* __restrict__ u_out, int V, int ban_id, const float* __restrict__ params,
                                                const unsigned long long* __restrict__ seed, const int* __restrict__ step, int t_add,
                                                const int* __restrict__ gen, const int* __restrict__ live) {
  sample_row_body<ROWS ? SMP_ROWS : SMP_UNIFORM, DRAW>(logits, ldl, out, margin, pmax, kept, u_out, V, ban_id, params, seed, step, t_add,
                                                       gen, live, nullptr, 1);
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
