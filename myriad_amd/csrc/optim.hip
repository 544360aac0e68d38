// K15: AdamW on the flat fp32 trainable-parameter buffer (reference runner_base.py:104-139: torch.optim.AdamW,
// betas (0.9, 0.999), eps 1e-8, decoupled weight decay 0.05 on the wd group / 0 on the no-wd group), with an
// optional bf16 shadow copy written in the same pass (the copy the next step's MFMA GEMMs read).
// HBM-bound: 28 B/param algorithmic (read p,g,m,v ; write p,m,v) + 2 B for the shadow.
#include "common.h"

__global__ void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                             float* __restrict__ v, bf16_t* __restrict__ shadow, long n4, float lr, float beta1,
                             float beta2, float omb1, float omb2, float eps, float wd, float bc1, float bc2_sqrt,
                             float gscale) {
  for (long it = blockIdx.x * (long)blockDim.x + threadIdx.x; it < n4; it += (long)gridDim.x * blockDim.x) {
    float4_t pp = *reinterpret_cast<const float4_t*>(p + it * 4);
    const float4_t gg = *reinterpret_cast<const float4_t*>(g + it * 4);
    float4_t mm = *reinterpret_cast<const float4_t*>(m + it * 4);
    float4_t vv = *reinterpret_cast<const float4_t*>(v + it * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float gr = gg[e] * gscale;
      pp[e] *= (1.f - lr * wd);
      mm[e] = beta1 * mm[e] + omb1 * gr;
      vv[e] = beta2 * vv[e] + omb2 * gr * gr;
      const float denom = sqrtf(vv[e]) / bc2_sqrt + eps;
      pp[e] -= (lr / bc1) * (mm[e] / denom);
    }
    *reinterpret_cast<float4_t*>(p + it * 4) = pp;
    *reinterpret_cast<float4_t*>(m + it * 4) = mm;
    *reinterpret_cast<float4_t*>(v + it * 4) = vv;
    if (shadow) {
      uint2 pk;
      pk.x = pack_bf2(pp[0], pp[1]);
      pk.y = pack_bf2(pp[2], pp[3]);
      *reinterpret_cast<uint2*>(shadow + it * 4) = pk;
    }
  }
}

// step is 1-based.  grad_scale multiplies the gradient first (e.g. 1/world after a sum all-reduce).
extern "C" int mh_adamw_step(float* p, const float* g, float* m, float* v, void* shadow_bf16, long n, double lr,
                             double beta1, double beta2, double eps, double weight_decay, int step, double grad_scale,
                             hipStream_t stream) {
  if (n <= 0) return MH_OK;
  if (n % 4 || step < 1) return MH_ERR_ARG;
  // bias corrections and (1-beta) in double on the host, like torch.optim.AdamW
  const float bc1 = (float)(1.0 - pow(beta1, (double)step));
  const float bc2s = (float)sqrt(1.0 - pow(beta2, (double)step));
  const float omb1 = (float)(1.0 - beta1), omb2 = (float)(1.0 - beta2);
  long grid = (n / 4 + 255) / 256;
  if (grid > 256 * 16) grid = 256 * 16;
  hipLaunchKernelGGL(adamw_kernel, dim3((int)grid), dim3(256), 0, stream, p, g, m, v, (bf16_t*)shadow_bf16, n / 4,
                     (float)lr, (float)beta1, (float)beta2, omb1, omb2, (float)eps, (float)weight_decay, bc1, bc2s,
                     (float)grad_scale);
  MH_CHECK_LAUNCH();
  return MH_OK;
}

// ---- gated form: torch.optim.AdamW skips a parameter whose .grad is None (no decay, no moment update, its own step
// count) -- what happens to a module that no rank used in a step (reference myriad.py:378: random prompt stage;
// runner_base.py:96-98 find_unused_parameters).  `used` is a device float (the module's use count summed over ranks by
// the gradient all-reduce it rides on), `steps` the device-resident number of updates applied to the module so far:
// nothing is read back by the host.  mh_adamw_gated updates one contiguous range if *used > 0 with step = *steps + 1;
// mh_adamw_bump then advances the counters of the used modules (launch it after the module's last range).
__global__ void adamw_gated_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                   float* __restrict__ v, long n4, float lr, double beta1_d, double beta2_d, float eps,
                                   float wd, float gscale, const float* __restrict__ used, const int* __restrict__ steps) {
  if (*used <= 0.f) return;
  // bias corrections and (1-beta) from the double betas, like mh_adamw_step and torch.optim.AdamW: taken from the fp32-rounded
  // betas instead, (1-beta2) would be off by 1.3e-5 relative at beta2 = 0.999 and every stored exp_avg_sq with it
  const double st = (double)(*steps + 1);
  const float bc1 = (float)(1.0 - pow(beta1_d, st));
  const float bc2_sqrt = (float)sqrt(1.0 - pow(beta2_d, st));
  const float omb1 = (float)(1.0 - beta1_d), omb2 = (float)(1.0 - beta2_d);
  const float beta1 = (float)beta1_d, beta2 = (float)beta2_d;
  for (long it = blockIdx.x * (long)blockDim.x + threadIdx.x; it < n4; it += (long)gridDim.x * blockDim.x) {
    float4_t pp = *reinterpret_cast<const float4_t*>(p + it * 4);
    const float4_t gg = *reinterpret_cast<const float4_t*>(g + it * 4);
    float4_t mm = *reinterpret_cast<const float4_t*>(m + it * 4);
    float4_t vv = *reinterpret_cast<const float4_t*>(v + it * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float gr = gg[e] * gscale;
      pp[e] *= (1.f - lr * wd);
      mm[e] = beta1 * mm[e] + omb1 * gr;
      vv[e] = beta2 * vv[e] + omb2 * gr * gr;
      const float denom = sqrtf(vv[e]) / bc2_sqrt + eps;
      pp[e] -= (lr / bc1) * (mm[e] / denom);
    }
    *reinterpret_cast<float4_t*>(p + it * 4) = pp;
    *reinterpret_cast<float4_t*>(m + it * 4) = mm;
    *reinterpret_cast<float4_t*>(v + it * 4) = vv;
  }
}
__global__ void adamw_bump_kernel(const float* __restrict__ used, int* __restrict__ steps, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && used[i] > 0.f) steps[i] += 1;
}

extern "C" int mh_adamw_gated(float* p, const float* g, float* m, float* v, long n, double lr, double beta1, double beta2,
                              double eps, double weight_decay, double grad_scale, const float* used, const int* steps,
                              hipStream_t stream) {
  if (n <= 0) return MH_OK;
  if (n % 4 || !used || !steps) return MH_ERR_ARG;
  long grid = (n / 4 + 255) / 256;
  if (grid > 256 * 16) grid = 256 * 16;
  hipLaunchKernelGGL(adamw_gated_kernel, dim3((int)grid), dim3(256), 0, stream, p, g, m, v, n / 4, (float)lr, beta1, beta2,
                     (float)eps, (float)weight_decay, (float)grad_scale, used, steps);
  MH_CHECK_LAUNCH();
  return MH_OK;
}
extern "C" int mh_adamw_bump(const float* used, int* steps, int n, hipStream_t stream) {
  if (n <= 0) return MH_OK;
  hipLaunchKernelGGL(adamw_bump_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, used, steps, n);
  MH_CHECK_LAUNCH();
  return MH_OK;
}

// ---- global gradient-norm clipping and the non-finite step guard (torch.nn.utils.clip_grad_norm_, norm_type 2; GradScaler's
// skipped step), on the device: the host never reads the norm.  Three pieces:
//   mh_grad_sumsq     sum of squares of one contiguous range of the gradient buffer, gated by the module's use flag like the
//                     AdamW; every product and partial sum in fp64 (a product of two fp32 values is exact there and a sum of
//                     finite fp32 squares cannot overflow, so "the sum is finite" is "every element read is finite"); one fp64
//                     partial per workgroup into a workspace slot, fixed reduction order, no atomics: the same input on the same
//                     grid gives the same bits.
//   mh_clip_finalize  one workgroup: adds the partials (and, sharded data parallel, the per-rank sums in rank order) and writes
//                     the control block ctl[4] = {s, norm, apply, skipped} (include/myriad_hip.h).
//   mh_adamw_gated_ctl / mh_adamw_bump_ctl   the gated AdamW and its counter bump reading the control block: nothing happens
//                     when apply == 0, else the gradient is multiplied once, by (float)s.
#define SUMSQ_BLOCK 256
#define SUMSQ_MAX_GRID (256 * 16)

// fixed-order sum of one value per thread of a 256-thread workgroup; the result is valid in thread 0
__device__ __forceinline__ double block_sum_f64(double acc, double* lds) {
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) lds[wave] = acc;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < SUMSQ_BLOCK / 64; ++w) t += lds[w];
  return t;
}

__global__ void __launch_bounds__(SUMSQ_BLOCK) grad_sumsq_kernel(const float* __restrict__ g, long n4,
                                                                 const float* __restrict__ used,
                                                                 double* __restrict__ partials) {
  __shared__ double lds[SUMSQ_BLOCK / 64];
  double acc = 0.0;
  if (*used > 0.f) {                                       // an unused module's range is not read: it contributes 0
    for (long it = blockIdx.x * (long)blockDim.x + threadIdx.x; it < n4; it += (long)gridDim.x * blockDim.x) {
      const float4_t gg = *reinterpret_cast<const float4_t*>(g + it * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double x = (double)gg[e];
        acc += x * x;
      }
    }
  }
  const double t = block_sum_f64(acc, lds);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

static inline long sumsq_grid(long n) {
  long grid = (n / 4 + SUMSQ_BLOCK - 1) / SUMSQ_BLOCK;
  return grid > SUMSQ_MAX_GRID ? SUMSQ_MAX_GRID : grid;
}
// workspace slots (fp64 partials) mh_grad_sumsq writes for a range of n elements
extern "C" long mh_grad_sumsq_slots(long n) { return n <= 0 ? 0 : sumsq_grid(n); }

extern "C" int mh_grad_sumsq(const float* g, long n, const float* used, double* partials, long slots, hipStream_t stream) {
  if (n < 0 || n % 4 || !used || (n > 0 && (!g || !partials))) return MH_ERR_ARG;
  if (n == 0) return MH_OK;
  const long grid = sumsq_grid(n);
  if (slots < grid) return MH_ERR_ARG;
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3((int)grid), dim3(SUMSQ_BLOCK), 0, stream, g, n / 4, used, partials);
  MH_CHECK_LAUNCH();
  return MH_OK;
}

// thread t adds its contiguous chunk of the partials in index order, thread 0 then the chunk sums in index order
__device__ __forceinline__ double partials_sum(const double* __restrict__ partials, long n, double* chunk) {
  const long per = (n + SUMSQ_BLOCK - 1) / SUMSQ_BLOCK;
  const long lo = threadIdx.x * per, hi = lo + per < n ? lo + per : n;
  double acc = 0.0;
  for (long i = lo; i < hi; ++i) acc += partials[i];
  chunk[threadIdx.x] = acc;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0)
    for (int c = 0; c < SUMSQ_BLOCK; ++c) t += chunk[c];
  return t;
}

// sharded data parallel: this rank's sum into its slot of the world-long vector, zeros into the others (the sum all-reduce
// that follows then leaves every rank's value in its slot, exactly)
__global__ void __launch_bounds__(SUMSQ_BLOCK) clip_rank_sum_kernel(const double* __restrict__ partials, long n,
                                                                    double* __restrict__ rank_sums, int world, int rank) {
  __shared__ double chunk[SUMSQ_BLOCK];
  const double t = partials_sum(partials, n, chunk);
  if (threadIdx.x == 0)
    for (int r = 0; r < world; ++r) rank_sums[r] = r == rank ? t : 0.0;
}

__global__ void __launch_bounds__(SUMSQ_BLOCK) clip_finalize_kernel(const double* __restrict__ partials, long n,
                                                                    const double* __restrict__ rank_sums, int world,
                                                                    double max_norm, double grad_scale, int guard,
                                                                    double* __restrict__ ctl) {
  __shared__ double chunk[SUMSQ_BLOCK];
  double sumsq = partials_sum(partials, n, chunk);
  if (threadIdx.x != 0) return;
  for (int r = 0; r < world; ++r) sumsq += rank_sums[r];
  const double norm = grad_scale * sqrt(sumsq);            // of the averaged gradient; in double it cannot overflow
  // clip_grad_norm_: coef = max_norm / (norm + 1e-6) clamped to 1; max_norm = +inf is "clipping off"
  double coef = 1.0;
  if (max_norm < HUGE_VAL) {
    coef = max_norm / (norm + 1e-6);
    if (coef > 1.0) coef = 1.0;
  }
  const double apply = (guard && !isfinite(sumsq)) ? 0.0 : 1.0;
  ctl[0] = (double)(float)(grad_scale * coef);             // rounded once: the AdamW's single multiplier of the raw gradient
  ctl[1] = norm;
  ctl[2] = apply;
  ctl[3] += 1.0 - apply;
}

extern "C" int mh_clip_rank_sum(const double* partials, long n_partials, double* rank_sums, int world, int rank,
                                hipStream_t stream) {
  if (n_partials < 0 || (n_partials > 0 && !partials) || !rank_sums || world < 1 || rank < 0 || rank >= world) return MH_ERR_ARG;
  hipLaunchKernelGGL(clip_rank_sum_kernel, dim3(1), dim3(SUMSQ_BLOCK), 0, stream, partials, n_partials, rank_sums, world, rank);
  MH_CHECK_LAUNCH();
  return MH_OK;
}

// max_norm: the clipping threshold, +inf for none; guard != 0: apply = 0 when the sum of squares is not finite.
// rank_sums[world] (NULL / 0: none) are added in rank order after the partials.
extern "C" int mh_clip_finalize(const double* partials, long n_partials, const double* rank_sums, int world, double max_norm,
                                double grad_scale, int guard, double* ctl, hipStream_t stream) {
  if (n_partials < 0 || (n_partials > 0 && !partials) || world < 0 || (world > 0 && !rank_sums) || !ctl) return MH_ERR_ARG;
  if (!(max_norm > 0.0)) return MH_ERR_ARG;                // also refuses a NaN
  hipLaunchKernelGGL(clip_finalize_kernel, dim3(1), dim3(SUMSQ_BLOCK), 0, stream, partials, n_partials, rank_sums, world,
                     max_norm, grad_scale, guard, ctl);
  MH_CHECK_LAUNCH();
  return MH_OK;
}

// adamw_gated_kernel with the control block in front: the same statements in the same order (the existing kernel keeps its
// code object unchanged), the gradient's one multiplier read from ctl[0]
__global__ void adamw_gated_ctl_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                       float* __restrict__ v, long n4, float lr, double beta1_d, double beta2_d, float eps,
                                       float wd, const float* __restrict__ used, const int* __restrict__ steps,
                                       const double* __restrict__ ctl) {
  if (ctl[2] == 0.0 || *used <= 0.f) return;               // a skipped step: no decay, no moment update
  const float gscale = (float)ctl[0];
  // bias corrections and (1-beta) from the double betas, like mh_adamw_step and torch.optim.AdamW: taken from the fp32-rounded
  // betas instead, (1-beta2) would be off by 1.3e-5 relative at beta2 = 0.999 and every stored exp_avg_sq with it
  const double st = (double)(*steps + 1);
  const float bc1 = (float)(1.0 - pow(beta1_d, st));
  const float bc2_sqrt = (float)sqrt(1.0 - pow(beta2_d, st));
  const float omb1 = (float)(1.0 - beta1_d), omb2 = (float)(1.0 - beta2_d);
  const float beta1 = (float)beta1_d, beta2 = (float)beta2_d;
  for (long it = blockIdx.x * (long)blockDim.x + threadIdx.x; it < n4; it += (long)gridDim.x * blockDim.x) {
    float4_t pp = *reinterpret_cast<const float4_t*>(p + it * 4);
    const float4_t gg = *reinterpret_cast<const float4_t*>(g + it * 4);
    float4_t mm = *reinterpret_cast<const float4_t*>(m + it * 4);
    float4_t vv = *reinterpret_cast<const float4_t*>(v + it * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float gr = gg[e] * gscale;
      pp[e] *= (1.f - lr * wd);
      mm[e] = beta1 * mm[e] + omb1 * gr;
      vv[e] = beta2 * vv[e] + omb2 * gr * gr;
      const float denom = sqrtf(vv[e]) / bc2_sqrt + eps;
      pp[e] -= (lr / bc1) * (mm[e] / denom);
    }
    *reinterpret_cast<float4_t*>(p + it * 4) = pp;
    *reinterpret_cast<float4_t*>(m + it * 4) = mm;
    *reinterpret_cast<float4_t*>(v + it * 4) = vv;
  }
}
__global__ void adamw_bump_ctl_kernel(const float* __restrict__ used, int* __restrict__ steps, int n,
                                      const double* __restrict__ ctl) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (ctl[2] != 0.0 && i < n && used[i] > 0.f) steps[i] += 1;
}

extern "C" int mh_adamw_gated_ctl(float* p, const float* g, float* m, float* v, long n, double lr, double beta1, double beta2,
                                  double eps, double weight_decay, const float* used, const int* steps, const double* ctl,
                                  hipStream_t stream) {
  if (n < 0 || n % 4 || !used || !steps || !ctl || (n > 0 && (!p || !g || !m || !v))) return MH_ERR_ARG;
  if (n == 0) return MH_OK;
  long grid = (n / 4 + 255) / 256;
  if (grid > 256 * 16) grid = 256 * 16;
  hipLaunchKernelGGL(adamw_gated_ctl_kernel, dim3((int)grid), dim3(256), 0, stream, p, g, m, v, n / 4, (float)lr, beta1, beta2,
                     (float)eps, (float)weight_decay, used, steps, ctl);
  MH_CHECK_LAUNCH();
  return MH_OK;
}
extern "C" int mh_adamw_bump_ctl(const float* used, int* steps, int n, const double* ctl, hipStream_t stream) {
  if (n <= 0) return MH_OK;
  if (!used || !steps || !ctl) return MH_ERR_ARG;
  hipLaunchKernelGGL(adamw_bump_ctl_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, used, steps, n, ctl);
  MH_CHECK_LAUNCH();
  return MH_OK;
}
