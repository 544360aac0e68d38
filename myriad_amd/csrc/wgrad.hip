// Weight gradients of a trainable Q-Former (freeze_qformer: False).
//
// K30 TN weight-gradient GEMM:  dW[N,K] (+)= dY^T . X  with dY [M,N] and X [M,K] row-major bf16, fp32 accumulation into a
// strided fp32 output.  Every other GEMM of the library is NT (C = A . B^T); a weight gradient through it needs both operands
// transposed into bf16 copies first.  Here the reduction runs over the ROWS of both operands: a workgroup stages 32 rows of
// dY (64 columns) and of X (64 columns) row-major in LDS, exactly as they come from HBM, and reads each MFMA operand column-wise
// through the gfx950 transpose read (ds_read_b64_tr_b16): lane (c, g) of a 16-lane group receives column c of 4 rows, so one
// 16x16x32 operand of 8 reduction rows per lane is two transposed reads.  The row set a lane holds is the same for the A (dY)
// and B (X) operands, which is all the reduction needs.
// Optional fused bias gradient dB[N] (+)= sum_m dY[m,:]: the workgroups of the first K tile sum the dY values they stage.
// Split M: when the tile count leaves the chip under-filled, grid.z splits the rows; each split writes its fp32 partial into a
// workspace and a second launch sums the splits in split order (bit-identical run to run).
//
// K31 LayerNorm parameter gradients: dgamma = sum_m dy * xhat, dbeta = sum_m dy, with xhat recomputed from the LayerNorm's
// input exactly as layernorm_bwd_kernel does.  Per-block partials over a fixed row range + a fixed-order reduce: deterministic.
#include "common.h"

#define TN_BN 64                 // dW rows (N) per workgroup
#define TN_BK 64                 // dW columns (K) per workgroup
#define TN_BM 32                 // reduction rows per step
#define TN_RS (TN_BK + 16)       // LDS image row stride (elements): 160 B, a multiple of the 8-B transposed-read alignment
typedef __attribute__((address_space(3))) short4_t tn_lds_s4;

// lane (lr, lg): column 16 jd + lr of image rows {4 lg .. 4 lg + 3} U {16 + 4 lg .. 16 + 4 lg + 3}.  Every lane of the wave
// takes part (EXEC all ones): rows past M were staged as zeros.
__device__ __forceinline__ short8_t tn_frag(const bf16_t* img, int jd, int lr, int lg) {
  const bf16_t* p = img + (4 * lg + (lr >> 2)) * TN_RS + 16 * jd + 4 * (lr & 3);
  const short4_t a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tn_lds_s4*)p);
  const short4_t b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tn_lds_s4*)(p + 16 * TN_RS));
  return (short8_t){a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}

// grid (K / 64, N / 64, splits), 256 threads.  Split z covers rows [z * rows_per, min(M, (z + 1) * rows_per)).
// splits == 1: out (+)= the product, bias (+)= the column sums.  splits > 1: ws[z][N][K] = the split's product, wsb[z][N] its sums.
__global__ __launch_bounds__(256) void gemm_tn_wgrad_kernel(const bf16_t* __restrict__ dy, long lddy, const bf16_t* __restrict__ x,
                                                            long ldx, float* out, long ldo, float* bias, float* ws, float* wsb,
                                                            int M, int N, int K, int rows_per, int accumulate) {
  __shared__ __attribute__((aligned(16))) bf16_t img[2][TN_BM * TN_RS];
  __shared__ float red[TN_BM][TN_BN + 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lg = lane >> 4;
  const int k0 = blockIdx.x * TN_BK, n0 = blockIdx.y * TN_BN, z = blockIdx.z;
  const int m0 = z * rows_per;
  const int m1 = min(M, m0 + rows_per);
  const bool want_bias = bias != nullptr && blockIdx.x == 0;
  const int srow = tid >> 3, scol = (tid & 7) * 8;            // staging role: one row, 8 columns of each operand
  float bsum[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) bsum[e] = 0.f;
  short8_t ry, rx;
  auto load_step = [&](int mb) {
    const int m = mb + srow;
    ry = rx = (short8_t){0, 0, 0, 0, 0, 0, 0, 0};
    if (m < m1) {
      ry = *reinterpret_cast<const short8_t*>(dy + (long)m * lddy + n0 + scol);
      rx = *reinterpret_cast<const short8_t*>(x + (long)m * ldx + k0 + scol);
    }
  };
  // wave w owns the 32 x 32 quadrant (n: 32 (w >> 1), k: 32 (w & 1)) as 2 x 2 MFMA tiles
  const int jn = (wave >> 1) * 2, jk = (wave & 1) * 2;
  float4_t acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = (float4_t){0.f, 0.f, 0.f, 0.f};
  if (m0 < m1) load_step(m0);
  for (int mb = m0; mb < m1; mb += TN_BM) {
    __syncthreads();                                          // the previous step's operand reads are done
    *reinterpret_cast<short8_t*>(&img[0][srow * TN_RS + scol]) = ry;
    *reinterpret_cast<short8_t*>(&img[1][srow * TN_RS + scol]) = rx;
    if (want_bias) {
#pragma unroll
      for (int e = 0; e < 8; ++e) bsum[e] += bf2f((bf16_t)ry[e]);
    }
    __syncthreads();
    if (mb + TN_BM < m1) load_step(mb + TN_BM);               // in flight under the products
    const short8_t a0 = tn_frag(img[0], jn, lr, lg), a1 = tn_frag(img[0], jn + 1, lr, lg);
    const short8_t b0 = tn_frag(img[1], jk, lr, lg), b1 = tn_frag(img[1], jk + 1, lr, lg);
    acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b0, acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b1, acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b0, acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b1, acc[1][1], 0, 0, 0);
  }
  // D of the 16x16x32 MFMA: lane (lr, lg), register e = row 4 lg + e (dW row n), column lr (dW column k)
  const bool direct = gridDim.z == 1;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int n = n0 + 16 * (jn + a) + 4 * lg + e, k = k0 + 16 * (jk + b) + lr;
        if (direct) {
          float* o = out + (long)n * ldo + k;
          *o = accumulate ? *o + acc[a][b][e] : acc[a][b][e];
        } else {
          ws[((long)z * N + n) * K + k] = acc[a][b][e];
        }
      }
  if (want_bias) {                                            // the 32 staging rows' sums of each column, in row order
#pragma unroll
    for (int e = 0; e < 8; ++e) red[srow][scol + e] = bsum[e];
    __syncthreads();
    if (tid < TN_BN) {
      float s = 0.f;
      for (int r = 0; r < TN_BM; ++r) s += red[r][tid];
      const int n = n0 + tid;
      if (direct)
        bias[n] = accumulate ? bias[n] + s : s;
      else
        wsb[(long)z * N + n] = s;
    }
  }
}

// out[n, k] (+)= sum_z ws[z][n][k] in split order; bias[n] (+)= sum_z wsb[z][n].  One thread per 4 columns.
__global__ void tn_split_reduce_kernel(const float* __restrict__ ws, const float* __restrict__ wsb, int splits, float* out,
                                       long ldo, float* bias, int N, int K, int accumulate) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long per_row = K >> 2;
  if (i < (long)N * per_row) {
    const int n = (int)(i / per_row), k = (int)(i - (long)n * per_row) * 4;
    float4_t s = *reinterpret_cast<const float4_t*>(ws + (long)n * K + k);
    for (int z = 1; z < splits; ++z) s += *reinterpret_cast<const float4_t*>(ws + ((long)z * N + n) * K + k);
    float* o = out + (long)n * ldo + k;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = accumulate ? o[e] + s[e] : s[e];
  }
  if (bias != nullptr && i < N) {
    float s = wsb[i];
    for (int z = 1; z < splits; ++z) s += wsb[(long)z * N + i];
    bias[i] = accumulate ? bias[i] + s : s;
  }
}

extern "C" long mh_gemm_tn_wgrad_ws_floats(int M, int N, int K, int splits) {
  if (splits <= 1) return 0;
  return (long)splits * N * ((long)K + 1);
}

// The split count the library picks for a shape: enough workgroups for two per CU (256 CUs), each split >= 128 rows.
extern "C" int mh_gemm_tn_wgrad_auto_splits(int M, int N, int K) {
  if (M <= 0 || N <= 0 || K <= 0) return 1;
  const long tiles = (long)(N / TN_BN) * (K / TN_BK);
  int s = 1;
  while (s < 8 && tiles * s < 512 && (long)(s * 2) * 128 <= M) s *= 2;
  return s;
}

extern "C" int mh_gemm_tn_wgrad(const void* dy, long lddy, const void* x, long ldx, float* out, long ldo, float* bias,
                                int M, int N, int K, int accumulate, int splits, float* ws, long ws_floats,
                                hipStream_t stream) {
  if (M < 0 || N <= 0 || K <= 0 || N % TN_BN || K % TN_BK || lddy % 8 || ldx % 8 || lddy < N || ldx < K || ldo < K)
    return MH_ERR_ARG;
  if (((uintptr_t)dy | (uintptr_t)x) & 15) return MH_ERR_ARG;
  if (splits <= 0) splits = mh_gemm_tn_wgrad_auto_splits(M, N, K);
  if (splits > 1 && (ws == nullptr || ws_floats < mh_gemm_tn_wgrad_ws_floats(M, N, K, splits))) return MH_ERR_ARG;
  // rows per split: a multiple of the 32-row step; trailing splits may be empty (their partials are zeros)
  int rows_per = (M + splits - 1) / splits;
  rows_per = (rows_per + TN_BM - 1) / TN_BM * TN_BM;
  if (rows_per == 0) rows_per = TN_BM;
  float* wsb = splits > 1 ? ws + (long)splits * N * K : nullptr;
  hipLaunchKernelGGL(gemm_tn_wgrad_kernel, dim3(K / TN_BK, N / TN_BN, splits), dim3(256), 0, stream, (const bf16_t*)dy, lddy,
                     (const bf16_t*)x, ldx, out, ldo, bias, ws, wsb, M, N, K, rows_per, accumulate);
  MH_CHECK_LAUNCH();
  if (splits > 1) {
    const long n4 = (long)N * (K / 4);
    hipLaunchKernelGGL(tn_split_reduce_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, stream, ws, wsb, splits, out,
                       ldo, bias, N, K, accumulate);
    MH_CHECK_LAUNCH();
  }
  return MH_OK;
}

// ---- K31 LayerNorm parameter gradients ----------------------------------------------------------------------------------
#define LNP_NT 256
#define LNP_NW 4
#define LNP_ROWS 16               // rows per partial block
#define LNP_IT 4                  // float4 chunks per thread: D <= 4096

// part[blk][0][D] = sum over the block's rows of dy * xhat, part[blk][1][D] = sum of dy.
__global__ __launch_bounds__(LNP_NT) void layernorm_param_partial_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                                         float* __restrict__ part, int M, int D, float eps,
                                                                         float p_out, unsigned long long seed_out) {
  __shared__ float red[LNP_NW];
  const int r0 = blockIdx.x * LNP_ROWS, r1 = min(M, r0 + LNP_ROWS);
  float4_t sg[LNP_IT], sb[LNP_IT];
#pragma unroll
  for (int c = 0; c < LNP_IT; ++c) sg[c] = sb[c] = (float4_t){0.f, 0.f, 0.f, 0.f};
  for (int row = r0; row < r1; ++row) {
    const float* xr = x + (size_t)row * D;
    const float* gr = dy + (size_t)row * D;
    float s = 0.f;                                            // mean and rstd as layernorm_bwd_kernel computes them
    for (int i = threadIdx.x * 4; i < D; i += LNP_NT * 4) {
      const float4_t v = *reinterpret_cast<const float4_t*>(xr + i);
      s += v[0] + v[1] + v[2] + v[3];
    }
    const float mean = block_sum<LNP_NW>(s, red) / D;
    float ss = 0.f;
    for (int i = threadIdx.x * 4; i < D; i += LNP_NT * 4) {
      const float4_t v = *reinterpret_cast<const float4_t*>(xr + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) ss += (v[e] - mean) * (v[e] - mean);
    }
    const float r = rsqrtf(block_sum<LNP_NW>(ss, red) / D + eps);
#pragma unroll
    for (int c = 0; c < LNP_IT; ++c) {
      const int i = threadIdx.x * 4 + c * LNP_NT * 4;
      if (i < D) {
        const float4_t v = *reinterpret_cast<const float4_t*>(xr + i);
        float4_t g = *reinterpret_cast<const float4_t*>(gr + i);
        if (p_out > 0.f) {                                    // dropout on the LayerNorm's output: the gradient it passed on
#pragma unroll
          for (int e = 0; e < 4; ++e)
            g[e] *= dropout_keep(seed_out, (unsigned long long)((long)row * D + i + e), p_out, 1.f / (1.f - p_out));
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          sg[c][e] += g[e] * ((v[e] - mean) * r);
          sb[c][e] += g[e];
        }
      }
    }
  }
  float* pg = part + (size_t)blockIdx.x * 2 * D;
#pragma unroll
  for (int c = 0; c < LNP_IT; ++c) {
    const int i = threadIdx.x * 4 + c * LNP_NT * 4;
    if (i < D) {
      *reinterpret_cast<float4_t*>(pg + i) = sg[c];
      *reinterpret_cast<float4_t*>(pg + D + i) = sb[c];
    }
  }
}

__global__ void layernorm_param_reduce_kernel(const float* __restrict__ part, int nblk, int D, float* dgamma, float* dbeta,
                                              int accumulate) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= D) return;
  float g = 0.f, b = 0.f;
  for (int k = 0; k < nblk; ++k) {                            // block order: fixed
    g += part[(size_t)k * 2 * D + i];
    b += part[(size_t)k * 2 * D + D + i];
  }
  dgamma[i] = accumulate ? dgamma[i] + g : g;
  dbeta[i] = accumulate ? dbeta[i] + b : b;
}

extern "C" long mh_layernorm_param_grads_ws_floats(int M, int D) {
  return (long)((M + LNP_ROWS - 1) / LNP_ROWS) * 2 * D;
}

extern "C" int mh_layernorm_param_grads(const float* dy, const float* x, float* dgamma, float* dbeta, int M, int D, float eps,
                                        int accumulate, float p_out, unsigned long long seed_out, float* ws, long ws_floats,
                                        hipStream_t stream) {
  if (M < 0 || D <= 0 || D % 4 || D > LNP_NT * 4 * LNP_IT || !(p_out >= 0.f && p_out < 1.f)) return MH_ERR_ARG;
  if (M == 0) {
    if (!accumulate) {
      if (hipMemsetAsync(dgamma, 0, sizeof(float) * D, stream) != hipSuccess) return MH_ERR_LAUNCH;
      if (hipMemsetAsync(dbeta, 0, sizeof(float) * D, stream) != hipSuccess) return MH_ERR_LAUNCH;
    }
    return MH_OK;
  }
  const int nblk = (M + LNP_ROWS - 1) / LNP_ROWS;
  if (ws == nullptr || ws_floats < mh_layernorm_param_grads_ws_floats(M, D)) return MH_ERR_ARG;
  hipLaunchKernelGGL(layernorm_param_partial_kernel, dim3(nblk), dim3(LNP_NT), 0, stream, dy, x, ws, M, D, eps,
                     p_out, seed_out);
  MH_CHECK_LAUNCH();
  hipLaunchKernelGGL(layernorm_param_reduce_kernel, dim3((D + 255) / 256), dim3(256), 0, stream, ws, nblk, D, dgamma, dbeta,
                     accumulate);
  MH_CHECK_LAUNCH();
  return MH_OK;
}
