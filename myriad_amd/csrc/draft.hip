// Draft-and-verify greedy decoding: the end of a K-row verify step (mh_draft_accept), after mh_argmax_pmax_rows over the K logit
// rows of each sequence.  Row j was fed ids[j] (ids[0] the last real token, ids[1..] guesses), so its pick nxt[j] is the true greedy
// token iff every earlier guess was right: the window keeps the leading rows whose pick confirms the next guess, plus the one token
// the last of them produces anyway.
//
// Rows of rejected guesses leave stale cache rows at pos' .. pos + K - 1 (pos' = the advanced position).  Nothing reads them: the
// next step is either a verify step, which overwrites rows pos' .. pos' + K - 1 and reads no cache row >= pos', or a plain one-row
// step, which overwrites row pos' and whose kvlen = pos' + 1 stops short of the rest.
#include "common.h"

#define DRAFT_MAX_K 8

// One 64-thread workgroup per sequence g.  rec[g] = 3K + 1 floats: the K picks, their margins, their p_max, then n_out.
__global__ __launch_bounds__(64) void draft_accept_kernel(const long* __restrict__ nxt, const float* __restrict__ mar,
                                                          const float* __restrict__ pmx, long* ids, const float* __restrict__ top_p,
                                                          float* __restrict__ rec, int* __restrict__ pos, int* __restrict__ kvlen,
                                                          int* __restrict__ step, int K) {
  const int g = blockIdx.x, t = threadIdx.x;
  const long* nx = nxt + (size_t)g * K;
  const float* mr = mar + (size_t)g * K;
  const float* pm = pmx + (size_t)g * K;
  long* id = ids + (size_t)g * K;
  float* r = rec + (size_t)g * (3 * K + 1);
  const float tp = *top_p;                       // <= 0: no row needs a draw
  int n = 1;                                     // every thread counts for itself: K <= 8 reads
  for (int j = 0; j < K - 1; ++j) {
    if (nx[j] != id[j + 1] || (tp > 0.f && !(pm[j] >= tp))) break;
    ++n;
  }
  if (t < K) {
    r[t] = (float)nx[t];
    r[K + t] = mr[t];
    r[2 * K + t] = pm[t];
  }
  __syncthreads();                               // every thread has read the guesses before ids[0] is replaced
  if (t == 0) {
    r[3 * K] = (float)n;
    id[0] = nx[n - 1];
    const int np = pos[g] + n;
    pos[g] = np;
    kvlen[g] = np + 1;
    if (g == 0) *step += 1;
  }
}

// The decode slots' form (mh_draft_accept_rows): group g is slot g, with its own live flag and its own count nguess[g] of real
// guesses behind the fed token.  Fillers past nguess[g] are never confirmed, an idle group records id -1 and changes nothing, and
// the kept pick also goes to next[g], the fed id of the plain S-row step, so that step can follow without a host copy.
__global__ __launch_bounds__(64) void draft_accept_rows_kernel(const long* __restrict__ nxt, const float* __restrict__ mar,
                                                               const float* __restrict__ pmx, long* ids, long* __restrict__ next,
                                                               const int* __restrict__ nguess, const int* __restrict__ live,
                                                               const float* __restrict__ top_p, float* __restrict__ rec,
                                                               int* __restrict__ pos, int* __restrict__ kvlen, int* __restrict__ step,
                                                               int K) {
  const int g = blockIdx.x, t = threadIdx.x;
  const long* nx = nxt + (size_t)g * K;
  const float* mr = mar + (size_t)g * K;
  const float* pm = pmx + (size_t)g * K;
  long* id = ids + (size_t)g * K;
  float* r = rec + (size_t)g * (3 * K + 1);
  if (g == 0 && t == 0) *step += 1;              // once per launch, whether or not group 0 is live
  if (!live[g]) {                                // uniform over the workgroup, ahead of the barrier
    if (t < K) {
      r[t] = -1.f;
      r[K + t] = 0.f;
      r[2 * K + t] = 0.f;
    }
    if (t == 0) r[3 * K] = 0.f;
    return;
  }
  const float tp = *top_p;                       // <= 0: no row needs a draw
  const int ng = min(max(nguess[g], 0), K - 1);
  int n = 1;                                     // every thread counts for itself: K <= 8 reads
  for (int j = 0; j < ng; ++j) {
    if (nx[j] != id[j + 1] || (tp > 0.f && !(pm[j] >= tp))) break;
    ++n;
  }
  if (t < K) {
    r[t] = (float)nx[t];
    r[K + t] = mr[t];
    r[2 * K + t] = pm[t];
  }
  __syncthreads();                               // every thread has read the guesses before ids[0] is replaced
  if (t == 0) {
    r[3 * K] = (float)n;
    id[0] = nx[n - 1];
    next[g] = nx[n - 1];
    const int np = pos[g] + n;
    pos[g] = np;
    kvlen[g] = np + 1;
  }
}

extern "C" int mh_draft_accept_rows(const long* nxt, const float* margin, const float* pmax, long* ids_k, long* next_ids,
                                    const int* nguess, const int* live, const float* top_p, float* rec, int* pos, int* kvlen,
                                    int* step, int G, int K, hipStream_t stream) {
  if (K < 1 || K > DRAFT_MAX_K) return MH_ERR_ARG;
  if (G <= 0) return MH_OK;
  if (!nxt || !margin || !pmax || !ids_k || !next_ids || !nguess || !live || !top_p || !rec || !pos || !kvlen || !step)
    return MH_ERR_ARG;
  hipLaunchKernelGGL(draft_accept_rows_kernel, dim3(G), dim3(64), 0, stream, nxt, margin, pmax, ids_k, next_ids, nguess, live, top_p,
                     rec, pos, kvlen, step, K);
  MH_CHECK_LAUNCH();
  return MH_OK;
}

extern "C" int mh_draft_accept(const long* nxt, const float* margin, const float* pmax, long* ids, const float* top_p, float* rec,
                               int* pos, int* kvlen, int* step, int G, int K, hipStream_t stream) {
  if (K < 1 || K > DRAFT_MAX_K) return MH_ERR_ARG;
  if (G <= 0) return MH_OK;
  if (!nxt || !margin || !pmax || !ids || !top_p || !rec || !pos || !kvlen || !step) return MH_ERR_ARG;
  hipLaunchKernelGGL(draft_accept_kernel, dim3(G), dim3(64), 0, stream, nxt, margin, pmax, ids, top_p, rec, pos, kvlen, step, K);
  MH_CHECK_LAUNCH();
  return MH_OK;
}
