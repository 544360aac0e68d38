// Hidden dropout of a trainable Q-Former (BERT's hidden_dropout_prob, train mode), fused into the LayerNorms around it:
//   embeddings      h = dropout(LN(q))                      (Qformer.py:106-107)   -> output mask
//   BertSelfOutput  y = dropout(z) + h,  h' = LN(y)          (Qformer.py:285-289)   -> input mask on z = x W^T + b
//   BertOutput      y = dropout(z) + h,  h' = LN(y)          (Qformer.py:370-374)
// The keep mask is the project's counter-based hash (common.h dropout_keep: keep = hash(seed, row * D + col)), regenerated in
// the backward, never stored.  The forward writes y (the LayerNorm input, saved for the backward); the backward writes the
// residual's gradient dL/dy unmasked in fp32 and the GEMM's gradient dL/dz = dL/dy * mask in bf16.
// mh_dropout_keep_mask writes the mask itself (tests feed it to a torch reference).
#include "common.h"

#define QD_NT 256
#define QD_NW 4

__device__ __forceinline__ float qd_keep(unsigned long long seed, long idx, float p) {
  return dropout_keep(seed, (unsigned long long)idx, p, 1.f / (1.f - p));
}

// one 256-thread workgroup per row
__global__ __launch_bounds__(QD_NT) void layernorm_fwd_dropout_kernel(const float* __restrict__ z, const float* __restrict__ res,
                                                                      const float* __restrict__ w, const float* __restrict__ b,
                                                                      float* x_out, bf16_t* y_bf, float* y_f, int D, float eps,
                                                                      float p_in, unsigned long long seed_in, float p_out,
                                                                      unsigned long long seed_out) {
  __shared__ float red[QD_NW];
  const long row = blockIdx.x;
  const float* zr = z + row * D;
  float s = 0.f;
  for (int i = threadIdx.x; i < D; i += QD_NT) {
    float x = zr[i];
    if (res) {
      x = x * qd_keep(seed_in, row * D + i, p_in) + res[row * D + i];
      if (x_out) x_out[row * D + i] = x;
    }
    s += x;
  }
  __syncthreads();                                   // x_out is re-read below by the threads that wrote it only
  const float mean = block_sum<QD_NW>(s, red) / D;
  const float* xr = res ? (x_out ? x_out + row * D : nullptr) : zr;
  float ss = 0.f;
  for (int i = threadIdx.x; i < D; i += QD_NT) {
    const float x = xr ? xr[i] : zr[i] * qd_keep(seed_in, row * D + i, p_in) + res[row * D + i];
    ss += (x - mean) * (x - mean);
  }
  const float r = rsqrtf(block_sum<QD_NW>(ss, red) / D + eps);
  for (int i = threadIdx.x; i < D; i += QD_NT) {
    const float x = xr ? xr[i] : zr[i] * qd_keep(seed_in, row * D + i, p_in) + res[row * D + i];
    float y = (x - mean) * r * w[i] + b[i];
    if (p_out > 0.f) y *= qd_keep(seed_out, row * D + i, p_out);
    if (y_bf) y_bf[row * D + i] = f2bf(y);
    if (y_f) y_f[row * D + i] = y;
  }
}

__global__ __launch_bounds__(QD_NT) void layernorm_bwd_dropout_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                                      const float* __restrict__ w, float* dx, bf16_t* dz_bf,
                                                                      int D, float eps, float p_in, unsigned long long seed_in,
                                                                      float p_out, unsigned long long seed_out) {
  __shared__ float red[QD_NW];
  const long row = blockIdx.x;
  const float* xr = x + row * D;
  const float* gr = dy + row * D;
  float s = 0.f;
  for (int i = threadIdx.x; i < D; i += QD_NT) s += xr[i];
  const float mean = block_sum<QD_NW>(s, red) / D;
  float ss = 0.f;
  for (int i = threadIdx.x; i < D; i += QD_NT) ss += (xr[i] - mean) * (xr[i] - mean);
  const float r = rsqrtf(block_sum<QD_NW>(ss, red) / D + eps);
  float sg = 0.f, sgx = 0.f;
  for (int i = threadIdx.x; i < D; i += QD_NT) {
    const float g = gr[i] * qd_keep(seed_out, row * D + i, p_out) * w[i];
    sg += g;
    sgx += g * (xr[i] - mean) * r;
  }
  sg = block_sum<QD_NW>(sg, red) / D;
  sgx = block_sum<QD_NW>(sgx, red) / D;
  for (int i = threadIdx.x; i < D; i += QD_NT) {
    const float g = gr[i] * qd_keep(seed_out, row * D + i, p_out) * w[i];
    const float o = r * (g - sg - (xr[i] - mean) * r * sgx);
    if (dx) dx[row * D + i] = o;
    if (dz_bf) dz_bf[row * D + i] = f2bf(o * qd_keep(seed_in, row * D + i, p_in));
  }
}

__global__ void dropout_keep_mask_kernel(float* out, long n, float p, unsigned long long seed) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    out[i] = qd_keep(seed, i, p);
}

extern "C" int mh_layernorm_fwd_dropout(const float* z, const float* res, const float* w, const float* b, float* x_out,
                                        void* y_bf16, float* y_f32, int M, int D, float eps, float p_in,
                                        unsigned long long seed_in, float p_out, unsigned long long seed_out,
                                        hipStream_t stream) {
  if (M <= 0) return MH_OK;
  if (D <= 0 || !(p_in >= 0.f && p_in < 1.f) || !(p_out >= 0.f && p_out < 1.f) || (res && !x_out)) return MH_ERR_ARG;
  hipLaunchKernelGGL(layernorm_fwd_dropout_kernel, dim3(M), dim3(QD_NT), 0, stream, z, res, w, b, x_out, (bf16_t*)y_bf16,
                     y_f32, D, eps, p_in, seed_in, p_out, seed_out);
  MH_CHECK_LAUNCH();
  return MH_OK;
}

extern "C" int mh_layernorm_bwd_dropout(const float* dy, const float* x, const float* w, float* dx, void* dz_bf16, int M, int D,
                                        float eps, float p_in, unsigned long long seed_in, float p_out,
                                        unsigned long long seed_out, hipStream_t stream) {
  if (M <= 0) return MH_OK;
  if (D <= 0 || !(p_in >= 0.f && p_in < 1.f) || !(p_out >= 0.f && p_out < 1.f)) return MH_ERR_ARG;
  hipLaunchKernelGGL(layernorm_bwd_dropout_kernel, dim3(M), dim3(QD_NT), 0, stream, dy, x, w, dx, (bf16_t*)dz_bf16, D, eps,
                     p_in, seed_in, p_out, seed_out);
  MH_CHECK_LAUNCH();
  return MH_OK;
}

extern "C" int mh_dropout_keep_mask(float* out, long n, float p, unsigned long long seed, hipStream_t stream) {
  if (n <= 0) return MH_OK;
  if (!(p >= 0.f && p < 1.f)) return MH_ERR_ARG;
  const long blocks = (n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096;
  hipLaunchKernelGGL(dropout_keep_mask_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, out, n, p, seed);
  MH_CHECK_LAUNCH();
  return MH_OK;
}
