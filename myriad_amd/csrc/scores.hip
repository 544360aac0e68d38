// Token log-probabilities of a decode step: the log-softmax, at temperature 1, of the logits row a pick was made from, at the
// picked id and at up to MH_SCORE_WATCH ids read from device memory (one captured graph serves every watch set).  Per row r:
//   out[0][r] = lse = m + log(sum_j exp(x_j - m)),  m = max_j x_j      (f32, fixed summation order)
//   out[1][r] = x[ids[r]] - lse
//   out[2 + w][r] = x[watch[w]] - lse                                  (0.0 for a watch slot outside [0, V))
// An idle row (live[r] == 0, or ids[r] < 0: what the slot engine's pick kernels leave for one) writes 0.0 to its ten entries and
// reads no logits.  Temperature, top-k, top-p and the EOS ban do not enter: they shape the pick, not the model's distribution.
// expf / logf are the accurate ones (1 ulp each), so the error bound of tests/token_scores_ref.py needs no fast-math term.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"

#define SCT 1024                // threads per row
#define SCW (SCT / 64)
#define MH_SCORE_WATCH 8

__device__ __forceinline__ bool score_idle(const long* __restrict__ ids, const int* __restrict__ live, float* __restrict__ out,
                                           long ldo, long row) {
  if ((live == nullptr || live[row] != 0) && ids[row] >= 0) return false;
  if (threadIdx.x < 2 + MH_SCORE_WATCH) out[threadIdx.x * ldo + row] = 0.f;
  return true;
}

// the ten entries of a live row from its lse; x[...] is read again from memory (one 4-byte load per entry)
__device__ __forceinline__ void score_write(const float* __restrict__ x, const long* __restrict__ ids, const int* __restrict__ watch,
                                            float* __restrict__ out, long ldo, long row, int V, float lse) {
  if (threadIdx.x == 0) {
    const long id = ids[row];
    out[row] = lse;
    out[ldo + row] = id < V ? x[id] - lse : 0.f;
  } else if (threadIdx.x <= MH_SCORE_WATCH) {
    const int w = threadIdx.x - 1, id = watch[w];
    out[(2 + w) * ldo + row] = (id >= 0 && id < V) ? x[id] - lse : 0.f;
  }
}

// the row in registers as 8 float4 per thread: the layout and conditions of argmax_pmax_wide_kernel (V <= 32768, ldl % 4 == 0,
// 16-byte aligned base); columns past V count as -inf and are never read
__global__ __launch_bounds__(SCT) void token_scores_wide_kernel(const float* __restrict__ logits, long ldl, const long* __restrict__ ids,
                                                                const int* __restrict__ watch, float* __restrict__ out, long ldo,
                                                                int V, const int* __restrict__ live) {
  __shared__ float red[SCW];
  const long row = blockIdx.x;
  if (score_idle(ids, live, out, ldo, row)) return;
  const float* x = logits + row * ldl;
  const float ninf = -__builtin_inff();
  float4_t xv[8];
  float m = ninf;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int j = (i * SCT + threadIdx.x) * 4;
    xv[i] = (float4_t){ninf, ninf, ninf, ninf};
    if (j + 3 < V) xv[i] = *reinterpret_cast<const float4_t*>(x + j);
    else
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (j + e < V) xv[i][e] = x[j + e];
#pragma unroll
    for (int e = 0; e < 4; ++e) m = fmaxf(m, xv[i][e]);
  }
  m = block_max<SCW>(m, red);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) s += expf(xv[i][e] - m);             // -inf (past V, or a -inf logit) adds exp(-inf) = 0
  s = block_sum<SCW>(s, red);
  score_write(x, ids, watch, out, ldo, row, V, m + logf(s));
}

// any V, stride and alignment: one workgroup strides over the row twice with 4-byte loads
__global__ __launch_bounds__(SCT) void token_scores_strided_kernel(const float* __restrict__ logits, long ldl,
                                                                   const long* __restrict__ ids, const int* __restrict__ watch,
                                                                   float* __restrict__ out, long ldo, int V,
                                                                   const int* __restrict__ live) {
  __shared__ float red[SCW];
  const long row = blockIdx.x;
  if (score_idle(ids, live, out, ldo, row)) return;
  const float* x = logits + row * ldl;
  float m = -__builtin_inff();
  for (int j = threadIdx.x; j < V; j += SCT) m = fmaxf(m, x[j]);
  m = block_max<SCW>(m, red);
  float s = 0.f;
  for (int j = threadIdx.x; j < V; j += SCT) s += expf(x[j] - m);
  s = block_sum<SCW>(s, red);
  score_write(x, ids, watch, out, ldo, row, V, m + logf(s));
}

extern "C" int mh_token_scores_rows(const float* logits, long ldl, const long* ids, const int* watch, float* out, long ldo, int R,
                                    int V, const int* live, hipStream_t stream) {
  if (!logits || !ids || !watch || !out || V < 1) return MH_ERR_ARG;
  if (R <= 0) return MH_OK;
  if (ldo < R) return MH_ERR_ARG;
  if (V <= 8 * SCT * 4 && (ldl % 4) == 0 && !((uintptr_t)logits & 15))
    hipLaunchKernelGGL(token_scores_wide_kernel, dim3(R), dim3(SCT), 0, stream, logits, ldl, ids, watch, out, ldo, V, live);
  else
    hipLaunchKernelGGL(token_scores_strided_kernel, dim3(R), dim3(SCT), 0, stream, logits, ldl, ids, watch, out, ldo, V, live);
  MH_CHECK_LAUNCH();
  return MH_OK;
}
