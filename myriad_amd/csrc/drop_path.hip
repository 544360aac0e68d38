// Stochastic depth (timm drop_path, scale_by_keep) for the trainable EVA ViT, reference eva_vit.py:162,173-176.
// A branch (attention or MLP) of a block runs only on the rows of the samples it keeps: its GEMMs see a COMPACT [K*N, *] matrix
// (K kept samples of N tokens each, in batch order).  These row kernels join the compact branch to the full [B*N, D] fp32 residual
// stream, one 256-thread workgroup per row like norm.hip:
//   forward : h_out = h + scale * y[compact row] (kept) | h (dropped, the same bits), then the next LayerNorm -> bf16, written
//             full or compact for the branch that reads it;
//   backward: dx = dres + LayerNorm backward of the compact dY (kept) | dres (dropped, the same bits), plus the bf16 scaled copy the
//             next branch's weight-gradient / dgrad GEMMs read, full or compact;
//   the LayerNorm's parameter gradients over the kept rows only (fixed order, no atomics: wgrad.hip's two-pass form);
//   a gather-scale cast for a gradient no kernel here produced.
// The sample -> compact-slot maps come from the HOST and travel in the kernel arguments (at most 64 samples): the launchers check
// range, uniqueness and count before anything is launched, so no kernel ever indexes with a map nobody looked at.
#include "common.h"

#define NT 256
#define NW 4
#define DP_MAXB 64

struct DpMap {
  int slot[DP_MAXB];          // sample -> compact sample index, or -1: not in the set
};

// slot == NULL: every sample, in order (K must be B).  Otherwise the kept samples must number the compact slots 0 .. K-1 exactly
// once each.  inv (optional): compact slot -> sample.
static int dp_build_map(const int* slot, int B, int K, DpMap* m, DpMap* inv) {
  if (B < 1 || B > DP_MAXB || K < 0 || K > B) return MH_ERR_ARG;
  bool seen[DP_MAXB];
  for (int i = 0; i < DP_MAXB; ++i) {
    m->slot[i] = -1;
    if (inv) inv->slot[i] = -1;
    seen[i] = false;
  }
  int n = 0;
  for (int b = 0; b < B; ++b) {
    const int s = slot ? slot[b] : b;
    if (s < -1 || s >= K) return MH_ERR_ARG;
    if (s < 0) continue;
    if (seen[s]) return MH_ERR_ARG;
    seen[s] = true;
    m->slot[b] = s;
    if (inv) inv->slot[s] = b;
    ++n;
  }
  return n == K ? MH_OK : MH_ERR_ARG;
}

// ---- forward: residual scatter (+ LayerNorm) ------------------------------------------------------------------------------
// The row stays in registers between the residual add and the norm (NIT float4 chunks a thread, D <= 8192).
template <int NIT>
__global__ __launch_bounds__(NT) void dp_residual_ln_kernel(const float* __restrict__ h, const float* __restrict__ y, DpMap in,
                                                            float scale, const float* __restrict__ w, const float* __restrict__ b,
                                                            DpMap out, float* __restrict__ h_out, bf16_t* __restrict__ xn, int N,
                                                            int D, float eps) {
  __shared__ float red[NW];
  const size_t row = blockIdx.x;
  const int smp = (int)(row / N), t = (int)(row - (size_t)smp * N);
  const int si = y ? in.slot[smp] : -1, so = xn ? out.slot[smp] : -1;      // uniform over the workgroup
  if (!h_out && so < 0) return;
  const float* hr = h + row * D;
  const float* yr = si >= 0 ? y + ((size_t)si * N + t) * D : nullptr;
  float4_t v[NIT];
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < NIT; ++c) {
    const int i = threadIdx.x * 4 + c * NT * 4;
    if (i < D) {
      float4_t x = *reinterpret_cast<const float4_t*>(hr + i);
      if (yr) {
        const float4_t u = *reinterpret_cast<const float4_t*>(yr + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] = __builtin_fmaf(scale, u[e], x[e]);
      }
      if (h_out) *reinterpret_cast<float4_t*>(h_out + row * D + i) = x;
      v[c] = x;
      s += x[0] + x[1] + x[2] + x[3];
    }
  }
  if (so < 0) return;
  const float mean = block_sum<NW>(s, red) / D;
  float ss = 0.f;
#pragma unroll
  for (int c = 0; c < NIT; ++c) {
    const int i = threadIdx.x * 4 + c * NT * 4;
    if (i < D) {
#pragma unroll
      for (int e = 0; e < 4; ++e) ss += (v[c][e] - mean) * (v[c][e] - mean);
    }
  }
  const float r = rsqrtf(block_sum<NW>(ss, red) / D + eps);
  bf16_t* xr = xn + ((size_t)so * N + t) * D;
#pragma unroll
  for (int c = 0; c < NIT; ++c) {
    const int i = threadIdx.x * 4 + c * NT * 4;
    if (i < D) {
      const float4_t g = *reinterpret_cast<const float4_t*>(w + i);
      const float4_t bb = *reinterpret_cast<const float4_t*>(b + i);
      float4_t o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = (v[c][e] - mean) * r * g[e] + bb[e];
      uint2 pk;
      pk.x = pack_bf2(o[0], o[1]);
      pk.y = pack_bf2(o[2], o[3]);
      *reinterpret_cast<uint2*>(xr + i) = pk;
    }
  }
}

// ---- backward: LayerNorm backward of the compact dY + scatter into the residual gradient ------------------------------------
// The kept rows use layernorm_bwd_kernel's expressions (norm.hip).  dx_bf (optional): bf16(out_scale * dx) of the samples in `out`,
// at their compact rows.
template <int NIT>
__global__ __launch_bounds__(NT) void dp_ln_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                       const float* __restrict__ w, const float* __restrict__ dres, DpMap in,
                                                       DpMap out, float out_scale, float* __restrict__ dx,
                                                       bf16_t* __restrict__ dx_bf, int N, int D, float eps) {
  __shared__ float red[NW];
  const size_t row = blockIdx.x;
  const int smp = (int)(row / N), t = (int)(row - (size_t)smp * N);
  const int si = in.slot[smp], so = dx_bf ? out.slot[smp] : -1;            // uniform over the workgroup
  bf16_t* br = so >= 0 ? dx_bf + ((size_t)so * N + t) * D : nullptr;
  if (si < 0) {                                                            // dropped: the residual gradient passes through
    for (int i = threadIdx.x * 4; i < D; i += NT * 4) {
      const float4_t d = *reinterpret_cast<const float4_t*>(dres + row * D + i);
      *reinterpret_cast<float4_t*>(dx + row * D + i) = d;
      if (br) {
        uint2 pk;
        pk.x = pack_bf2(out_scale * d[0], out_scale * d[1]);
        pk.y = pack_bf2(out_scale * d[2], out_scale * d[3]);
        *reinterpret_cast<uint2*>(br + i) = pk;
      }
    }
    return;
  }
  const float* xr = x + row * D;
  const float* gr = dy + ((size_t)si * N + t) * D;
  float4_t xv[NIT], gv[NIT];
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < NIT; ++c) {
    const int i = threadIdx.x * 4 + c * NT * 4;
    if (i < D) {
      xv[c] = *reinterpret_cast<const float4_t*>(xr + i);
      gv[c] = *reinterpret_cast<const float4_t*>(gr + i);
      const float4_t v = xv[c];
      s += v[0] + v[1] + v[2] + v[3];
    }
  }
  const float mean = block_sum<NW>(s, red) / D;
  float ss = 0.f;
#pragma unroll
  for (int c = 0; c < NIT; ++c) {
    const int i = threadIdx.x * 4 + c * NT * 4;
    if (i < D) {
      const float4_t v = xv[c];
#pragma unroll
      for (int e = 0; e < 4; ++e) ss += (v[e] - mean) * (v[e] - mean);
    }
  }
  const float r = rsqrtf(block_sum<NW>(ss, red) / D + eps);
  float sg = 0.f, sgx = 0.f;
#pragma unroll
  for (int c = 0; c < NIT; ++c) {
    const int i = threadIdx.x * 4 + c * NT * 4;
    if (i < D) {
      const float4_t v = xv[c];
      const float4_t g = gv[c];
      const float4_t ww = *reinterpret_cast<const float4_t*>(w + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float gg = g[e] * ww[e];
        sg += gg;
        sgx += gg * (v[e] - mean) * r;
      }
    }
  }
  sg = block_sum<NW>(sg, red) / D;
  sgx = block_sum<NW>(sgx, red) / D;
#pragma unroll
  for (int c = 0; c < NIT; ++c) {
    const int i = threadIdx.x * 4 + c * NT * 4;
    if (i < D) {
      const float4_t v = xv[c];
      const float4_t g = gv[c];
      const float4_t ww = *reinterpret_cast<const float4_t*>(w + i);
      const float4_t d = *reinterpret_cast<const float4_t*>(dres + row * D + i);
      float4_t o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        o[e] = r * (g[e] * ww[e] - sg - (v[e] - mean) * r * sgx);
        o[e] += d[e];
      }
      *reinterpret_cast<float4_t*>(dx + row * D + i) = o;
      if (br) {
        uint2 pk;
        pk.x = pack_bf2(out_scale * o[0], out_scale * o[1]);
        pk.y = pack_bf2(out_scale * o[2], out_scale * o[3]);
        *reinterpret_cast<uint2*>(br + i) = pk;
      }
    }
  }
}

// ---- bf16(scale * src) of the samples in `out`, at their compact rows ---------------------------------------------------------
__global__ __launch_bounds__(NT) void dp_gather_scale_kernel(const float* __restrict__ src, DpMap out, float scale,
                                                             bf16_t* __restrict__ dst, int N, int D) {
  const size_t row = blockIdx.x;
  const int smp = (int)(row / N), t = (int)(row - (size_t)smp * N);
  const int so = out.slot[smp];
  if (so < 0) return;
  bf16_t* br = dst + ((size_t)so * N + t) * D;
  for (int i = threadIdx.x * 4; i < D; i += NT * 4) {
    const float4_t d = *reinterpret_cast<const float4_t*>(src + row * D + i);
    uint2 pk;
    pk.x = pack_bf2(scale * d[0], scale * d[1]);
    pk.y = pack_bf2(scale * d[2], scale * d[3]);
    *reinterpret_cast<uint2*>(br + i) = pk;
  }
}

// ---- LayerNorm parameter gradients over the kept rows ------------------------------------------------------------------------
// layernorm_param_partial_kernel (wgrad.hip) over the COMPACT rows: a block sums 16 compact rows serially, the blocks are added in
// block order.  dy is compact, x is the full residual stream; kept: compact sample -> sample.
#define DPP_ROWS 16
#define DPP_IT 4                  // float4 chunks per thread: D <= 4096

__global__ __launch_bounds__(NT) void dp_ln_param_partial_kernel(const float* __restrict__ dy, const float* __restrict__ x, DpMap kept,
                                                                 float* __restrict__ part, int Mc, int N, int D, float eps) {
  __shared__ float red[NW];
  const int r0 = blockIdx.x * DPP_ROWS, r1 = min(Mc, r0 + DPP_ROWS);
  float4_t sg[DPP_IT], sb[DPP_IT];
#pragma unroll
  for (int c = 0; c < DPP_IT; ++c) sg[c] = sb[c] = (float4_t){0.f, 0.f, 0.f, 0.f};
  for (int row = r0; row < r1; ++row) {
    const int k = row / N, t = row - k * N;
    const float* xr = x + ((size_t)kept.slot[k] * N + t) * D;
    const float* gr = dy + (size_t)row * D;
    float s = 0.f;
    for (int i = threadIdx.x * 4; i < D; i += NT * 4) {
      const float4_t v = *reinterpret_cast<const float4_t*>(xr + i);
      s += v[0] + v[1] + v[2] + v[3];
    }
    const float mean = block_sum<NW>(s, red) / D;
    float ss = 0.f;
    for (int i = threadIdx.x * 4; i < D; i += NT * 4) {
      const float4_t v = *reinterpret_cast<const float4_t*>(xr + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) ss += (v[e] - mean) * (v[e] - mean);
    }
    const float r = rsqrtf(block_sum<NW>(ss, red) / D + eps);
#pragma unroll
    for (int c = 0; c < DPP_IT; ++c) {
      const int i = threadIdx.x * 4 + c * NT * 4;
      if (i < D) {
        const float4_t v = *reinterpret_cast<const float4_t*>(xr + i);
        const float4_t g = *reinterpret_cast<const float4_t*>(gr + i);
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
  for (int c = 0; c < DPP_IT; ++c) {
    const int i = threadIdx.x * 4 + c * NT * 4;
    if (i < D) {
      *reinterpret_cast<float4_t*>(pg + i) = sg[c];
      *reinterpret_cast<float4_t*>(pg + D + i) = sb[c];
    }
  }
}

__global__ void dp_ln_param_reduce_kernel(const float* __restrict__ part, int nblk, int D, float* dgamma, float* dbeta,
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

// ---- launchers ------------------------------------------------------------------------------------------------------------
static bool dp_dims_ok(int B, int N, int D) {
  return B >= 1 && N >= 1 && D >= 4 && D % 4 == 0 && D <= 8192 && (long)B * N <= 0x7fffffffL;
}

extern "C" int mh_drop_path_residual_layernorm(const float* h, const float* y, const int* slot_in, int K_in, float scale,
                                               const float* w, const float* b, const int* slot_out, int K_out, float* h_out,
                                               void* xn_bf16, int B, int N, int D, float eps, hipStream_t stream) {
  if (!dp_dims_ok(B, N, D) || !h) return MH_ERR_ARG;
  if (B > DP_MAXB) return MH_ERR_UNSUPPORTED;
  DpMap in, out;
  if (y) {
    if (!slot_in || !h_out || K_in < 1) return MH_ERR_ARG;
    if (dp_build_map(slot_in, B, K_in, &in, nullptr) != MH_OK) return MH_ERR_ARG;
  } else {
    if (K_in != 0 || dp_build_map(nullptr, B, B, &in, nullptr) != MH_OK) return MH_ERR_ARG;
  }
  if (xn_bf16) {
    if (!w || !b || K_out < 1) return MH_ERR_ARG;
    if (dp_build_map(slot_out, B, slot_out ? K_out : B, &out, nullptr) != MH_OK || (!slot_out && K_out != B)) return MH_ERR_ARG;
  } else {
    if (K_out != 0 || dp_build_map(nullptr, B, B, &out, nullptr) != MH_OK) return MH_ERR_ARG;
  }
  if (!h_out && !xn_bf16) return MH_ERR_ARG;
  if (h_out == h) return MH_ERR_ARG;
  const int M = B * N;
#define DPF_LAUNCH(NIT_)                                                                                                   \
  hipLaunchKernelGGL(dp_residual_ln_kernel<NIT_>, dim3(M), dim3(NT), 0, stream, h, y, in, scale, w, b, out, h_out,          \
                     (bf16_t*)xn_bf16, N, D, eps)
  if (D <= 2 * NT * 4) DPF_LAUNCH(2);
  else if (D <= 4 * NT * 4) DPF_LAUNCH(4);
  else DPF_LAUNCH(8);
#undef DPF_LAUNCH
  MH_CHECK_LAUNCH();
  return MH_OK;
}

extern "C" int mh_drop_path_layernorm_bwd(const float* dy, const float* x, const float* w, const float* dres, const int* slot_in,
                                          int K_in, const int* slot_out, int K_out, float out_scale, float* dx, void* dx_bf16,
                                          int B, int N, int D, float eps, hipStream_t stream) {
  if (!dp_dims_ok(B, N, D) || !dy || !x || !w || !dres || !dx || !slot_in || K_in < 1 || dx == dres) return MH_ERR_ARG;
  if (B > DP_MAXB) return MH_ERR_UNSUPPORTED;
  DpMap in, out;
  if (dp_build_map(slot_in, B, K_in, &in, nullptr) != MH_OK) return MH_ERR_ARG;
  if (dx_bf16) {
    if (K_out < 1 || (!slot_out && K_out != B)) return MH_ERR_ARG;
    if (dp_build_map(slot_out, B, K_out, &out, nullptr) != MH_OK) return MH_ERR_ARG;
  } else {
    if (K_out != 0 || dp_build_map(nullptr, B, B, &out, nullptr) != MH_OK) return MH_ERR_ARG;
  }
  const int M = B * N;
#define DPB_LAUNCH(NIT_)                                                                                                   \
  hipLaunchKernelGGL(dp_ln_bwd_kernel<NIT_>, dim3(M), dim3(NT), 0, stream, dy, x, w, dres, in, out, out_scale, dx,          \
                     (bf16_t*)dx_bf16, N, D, eps)
  if (D <= 2 * NT * 4) DPB_LAUNCH(2);
  else if (D <= 4 * NT * 4) DPB_LAUNCH(4);
  else DPB_LAUNCH(8);
#undef DPB_LAUNCH
  MH_CHECK_LAUNCH();
  return MH_OK;
}

extern "C" int mh_drop_path_gather_scale(const float* src, const int* slot_out, int K_out, float scale, void* dst_bf16, int B,
                                         int N, int D, hipStream_t stream) {
  if (!dp_dims_ok(B, N, D) || !src || !dst_bf16 || K_out < 1 || (!slot_out && K_out != B)) return MH_ERR_ARG;
  if (B > DP_MAXB) return MH_ERR_UNSUPPORTED;
  DpMap out;
  if (dp_build_map(slot_out, B, K_out, &out, nullptr) != MH_OK) return MH_ERR_ARG;
  hipLaunchKernelGGL(dp_gather_scale_kernel, dim3(B * N), dim3(NT), 0, stream, src, out, scale, (bf16_t*)dst_bf16, N, D);
  MH_CHECK_LAUNCH();
  return MH_OK;
}

extern "C" long mh_drop_path_param_grads_ws_floats(int K, int N, int D) {
  if (K < 0 || N < 0 || D < 0) return 0;
  return (((long)K * N + DPP_ROWS - 1) / DPP_ROWS) * 2 * D;
}

extern "C" int mh_drop_path_layernorm_param_grads(const float* dy, const float* x, const int* slot_in, int K_in, float* dgamma,
                                                  float* dbeta, int B, int N, int D, float eps, int accumulate, float* ws,
                                                  long ws_floats, hipStream_t stream) {
  if (!dp_dims_ok(B, N, D) || D > NT * 4 * DPP_IT || !dy || !x || !dgamma || !dbeta || !slot_in || K_in < 1) return MH_ERR_ARG;
  if (B > DP_MAXB) return MH_ERR_UNSUPPORTED;
  DpMap in, kept;
  if (dp_build_map(slot_in, B, K_in, &in, &kept) != MH_OK) return MH_ERR_ARG;
  if (!ws || ws_floats < mh_drop_path_param_grads_ws_floats(K_in, N, D)) return MH_ERR_ARG;
  const int Mc = K_in * N;
  const int nblk = (Mc + DPP_ROWS - 1) / DPP_ROWS;
  hipLaunchKernelGGL(dp_ln_param_partial_kernel, dim3(nblk), dim3(NT), 0, stream, dy, x, kept, ws, Mc, N, D, eps);
  MH_CHECK_LAUNCH();
  hipLaunchKernelGGL(dp_ln_param_reduce_kernel, dim3((D + 255) / 256), dim3(256), 0, stream, ws, nblk, D, dgamma, dbeta, accumulate);
  MH_CHECK_LAUNCH();
  return MH_OK;
}
