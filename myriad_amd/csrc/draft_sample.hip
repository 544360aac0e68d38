// Draft-and-verify decoding under the per-row tail of the decode slots (the repetition penalty, the per-request EOS ban, the device
// sampler): the three launches that follow the logits of a verify step of G groups x K rows, K <= 8.  Row (g, j) is the token
// step of request g at token index gen[g] + j, so each launch works out for that row what the plain slot step would see there:
//   repetition_penalty_draft_kernel  the seen set of row (g, j) is the bitmap seen[g] plus the tokens fed in rows 0 .. j of the
//                                    group (ids_k[g*K .. g*K + j]); the bitmap itself is only read -- the K workgroups of a group
//                                    share it -- and mh_draft_accept_sampled_rows adds the tokens that stood.
//   sample_rows_draft_kernel         sample.hip's row body (smp_rows.h) with seed[g], t = gen[g] + j and the ban for that t: the
//                                    draw depends on (logits row, seed, t) only, so row j draws the token the plain step would draw
//                                    at that index, and a guess stands iff it equals that draw (exact replay, not rejection
//                                    sampling).
//   draft_accept_sampled_kernel      draft.hip's per-slot accept with the kept rule, the bitmap update and gen[g] += n_out.
#include "common.h"
#include "smp_rows.h"

#define DRAFT_MAX_K 8

// One 256-thread workgroup per row (g, j); thread t owns the bitmap words t, t + 256, ... of the row's seen set and the logits
// they name, so every id is penalised once however the bitmap and the extras overlap.
__global__ __launch_bounds__(256) void repetition_penalty_draft_kernel(float* __restrict__ logits, long ldl,
                                                                       const unsigned* __restrict__ seen,
                                                                       const long* __restrict__ ids_k, const int* __restrict__ nrow,
                                                                       const int* __restrict__ live, int K, int V, int W,
                                                                       const float* __restrict__ penalty) {
  const long row = blockIdx.x;
  const long g = row / K;
  const int j = (int)(row - g * K);
  if (!live[g] || j >= nrow[g]) return;
  const float pen = *penalty;
  float* x = logits + row * ldl;
  const unsigned* sr = seen + g * W;
  long extra[DRAFT_MAX_K];
#pragma unroll
  for (int e = 0; e < DRAFT_MAX_K; ++e) extra[e] = e <= j ? ids_k[g * K + e] : -1;
  for (int w = threadIdx.x; w < W; w += blockDim.x) {
    unsigned m = sr[w];
#pragma unroll
    for (int e = 0; e < DRAFT_MAX_K; ++e)
      if (extra[e] >= 0 && extra[e] < V && (int)(extra[e] >> 5) == w) m |= 1u << (extra[e] & 31);
    while (m) {
      const int i = w * 32 + __builtin_ctz(m);
      m &= m - 1;
      if (i < V) {
        const float v = x[i];
        x[i] = v < 0.f ? v * pen : v / pen;
      }
    }
  }
}

extern "C" int mh_repetition_penalty_draft_rows(float* logits, long ldl, const unsigned* seen, const long* ids_k, const int* nrow,
                                                const int* live, int G, int K, int V, const float* penalty, hipStream_t stream) {
  if (K < 1 || K > DRAFT_MAX_K) return MH_ERR_ARG;
  if (G <= 0) return MH_OK;
  if (!logits || !seen || !ids_k || !nrow || !live || !penalty || V <= 0 || ldl < V) return MH_ERR_ARG;
  hipLaunchKernelGGL(repetition_penalty_draft_kernel, dim3(G * K), dim3(256), 0, stream, logits, ldl, seen, ids_k, nrow, live, K, V,
                     (V + 31) / 32, penalty);
  MH_CHECK_LAUNCH();
  return MH_OK;
}

template <bool DRAW>
__global__ __launch_bounds__(SNT) void sample_rows_draft_kernel(const float* __restrict__ logits, long ldl, long* __restrict__ out,
                                                                float* __restrict__ margin, float* __restrict__ pmax,
                                                                int* __restrict__ kept, float* __restrict__ u_out, int V,
                                                                const float* __restrict__ params,
                                                                const unsigned long long* __restrict__ seed,
                                                                const int* __restrict__ gen, const int* __restrict__ live,
                                                                const int* __restrict__ nrow, int K) {
  sample_row_body<SMP_DRAFT, DRAW>(logits, ldl, out, margin, pmax, kept, u_out, V, -1, params, seed, nullptr, 0, gen, live, nrow, K);
}

extern "C" int mh_sample_rows_draft(const float* logits, long ldl, long* out, float* margin, float* pmax, int* kept, float* u_out,
                                    int G, int K, int V, const float* params, const unsigned long long* seed, const int* gen,
                                    const int* nrow, const int* live, int draw, hipStream_t stream) {
  if (K < 1 || K > DRAFT_MAX_K) return MH_ERR_ARG;
  if (G <= 0) return MH_OK;
  if (!logits || !out || !margin || !pmax || !params || !gen || !nrow || !live || (draw && (!kept || !seed))) return MH_ERR_ARG;
  if (V <= 0 || ldl < V) return MH_ERR_ARG;
  if (V > 8 * SNT * 4 || (ldl % 4) != 0 || ((uintptr_t)logits & 15)) return MH_ERR_UNSUPPORTED;
  if (draw)
    hipLaunchKernelGGL((sample_rows_draft_kernel<true>), dim3(G * K), dim3(SNT), 0, stream, logits, ldl, out, margin, pmax, kept, u_out,
                       V, params, seed, gen, live, nrow, K);
  else
    hipLaunchKernelGGL((sample_rows_draft_kernel<false>), dim3(G * K), dim3(SNT), 0, stream, logits, ldl, out, margin, pmax,
                       (int*)nullptr, (float*)nullptr, V, params, (const unsigned long long*)nullptr, gen, live, nrow, K);
  MH_CHECK_LAUNCH();
  return MH_OK;
}

// One 64-thread workgroup per group g.  rec[g] = 4K + 1 floats: the K picks, their margins, their p_max, their kept counts (0
// without `kept`), then n_out.  Thread 0 alone touches the group's bitmap, and no other workgroup of the launch reads it.
__global__ __launch_bounds__(64) void draft_accept_sampled_kernel(const long* __restrict__ nxt, const float* __restrict__ mar,
                                                                  const float* __restrict__ pmx, const int* __restrict__ kept,
                                                                  long* ids, long* __restrict__ next, const int* __restrict__ nguess,
                                                                  const int* __restrict__ live, const float* __restrict__ top_p,
                                                                  unsigned* __restrict__ seen, float* __restrict__ rec,
                                                                  int* __restrict__ pos, int* __restrict__ kvlen,
                                                                  int* __restrict__ gen, int* __restrict__ step, int K, int V, int W) {
  const int g = blockIdx.x, t = threadIdx.x;
  const long* nx = nxt + (size_t)g * K;
  const float* mr = mar + (size_t)g * K;
  const float* pm = pmx + (size_t)g * K;
  const int* kp = kept ? kept + (size_t)g * K : nullptr;
  long* id = ids + (size_t)g * K;
  float* r = rec + (size_t)g * (4 * K + 1);
  if (g == 0 && t == 0) *step += 1;              // once per launch, whether or not group 0 is live
  if (!live[g]) {                                // uniform over the workgroup, ahead of the barrier
    if (t < K) {
      r[t] = -1.f;
      r[K + t] = 0.f;
      r[2 * K + t] = 0.f;
      r[3 * K + t] = 0.f;
    }
    if (t == 0) r[4 * K] = 0.f;
    return;
  }
  const float tp = *top_p;                       // <= 0: no row needs a draw; looked at without `kept` only
  const int ng = min(max(nguess[g], 0), K - 1);
  int n = 1;                                     // every thread counts for itself: K <= 8 reads
  for (int j = 0; j < ng; ++j) {
    const bool host_draws = kp ? kp[j] < 0 : (tp > 0.f && !(pm[j] >= tp));
    if (host_draws || nx[j] != id[j + 1]) break;
    ++n;
  }
  if (t < K) {
    r[t] = (float)nx[t];
    r[K + t] = mr[t];
    r[2 * K + t] = pm[t];
    r[3 * K + t] = kp ? (float)kp[t] : 0.f;
  }
  __syncthreads();                               // every thread has read the guesses before ids[0] is replaced
  if (t == 0) {
    if (seen)                                    // the fed token and the confirmed guesses; the kept pick joins when it is fed
      for (int j = 0; j < n; ++j) {
        const long v = id[j];
        if (v >= 0 && v < V) seen[(size_t)g * W + (v >> 5)] |= 1u << (v & 31);
      }
    r[4 * K] = (float)n;
    id[0] = nx[n - 1];
    next[g] = nx[n - 1];
    const int np = pos[g] + n;
    pos[g] = np;
    kvlen[g] = np + 1;
    gen[g] += n;
  }
}

extern "C" int mh_draft_accept_sampled_rows(const long* nxt, const float* margin, const float* pmax, const int* kept, long* ids_k,
                                            long* next_ids, const int* nguess, const int* live, const float* top_p, unsigned* seen,
                                            float* rec, int* pos, int* kvlen, int* gen, int* step, int G, int K, int V,
                                            hipStream_t stream) {
  if (K < 1 || K > DRAFT_MAX_K) return MH_ERR_ARG;
  if (G <= 0) return MH_OK;
  if (!nxt || !margin || !pmax || !ids_k || !next_ids || !nguess || !live || !top_p || !rec || !pos || !kvlen || !gen || !step)
    return MH_ERR_ARG;
  if (seen && V <= 0) return MH_ERR_ARG;
  hipLaunchKernelGGL(draft_accept_sampled_kernel, dim3(G), dim3(64), 0, stream, nxt, margin, pmax, kept, ids_k, next_ids, nguess, live,
                     top_p, seen, rec, pos, kvlen, gen, step, K, V, (V + 31) / 32);
  MH_CHECK_LAUNCH();
  return MH_OK;
}
