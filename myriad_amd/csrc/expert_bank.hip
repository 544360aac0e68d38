// K16b: the one-shot head against a per-class reference bank (vision_expert.py: one_shot_banked / forward_banked).
//   bank_sim_max     part[b, chunk, l] = max_j <q[b, l], bank[bank_off[b] + j]> over the bank rows j of one chunk   (one tap)
//   bank_sim_finish  sim = sum_t w * max_chunk part_t ; simmask = 1 - sim at h x h ; amap = 1 - bilinear_ac(sim) at S x S
// bank_sim_max is the NT product of attention's Q.K^T (both operands K-contiguous, v_mfma_f32_16x16x32_bf16, fp32 accumulation)
// with a row-max in place of the store: the [L, rows] score matrix lives in accumulators only.  A workgroup of four waves owns
// BK_QT = 64 query rows of one sample and one chunk of BK_CH = 128 bank rows of that sample's class; a wave owns 16 query rows
// against all 128 bank rows (8 accumulator fragments).  Orientation S^T = bank . Q^T as attn_seq.hip: the bank fragment is the A
// operand (its row on lane & 15), the query fragment the B operand, so a lane holds one query's scores against bank rows
// 16 j + 4 (lane >> 4) + r and the row-max is 32 in-lane fmaxf and two cross-lane steps.  Both tiles are staged through LDS in
// D slabs of BK_KS = 64 elements, two buffers: the next slab's global loads are issued before the current slab's MFMAs and
// written to the other buffer after them, one barrier per slab.  Rows are padded to BK_RS = 80 elements (160 B): the 16 lanes
// of a ds_read_b128 group then start on 16 different multiples of four banks.
// Every dot product is one accumulator chain over the k-steps 0, 32, 64, ... of D in ascending order, whatever the chunk, the
// sample, the batch or the class's place in the bank: the bits of a score depend on its two rows and D alone, and a max over
// chunks is exact, so how the rows are split into chunks cannot show in the result.
// Bank rows past bank_rows[b] inside the last tile are staged as copies of the class's last row (never the neighbouring
// class's memory) and their scores are replaced by -inf before the max.
#include "attn_frag.h"
#include "expert_map.h"

#define BK_NT 256
#define BK_QT 64
#define BK_CH 128
#define BK_KS 64
#define BK_RS 80
#define BK_TILE ((BK_CH + BK_QT) * BK_RS)           // one buffer: bank rows 0..127, then query rows 0..63
#define BK_LD ((BK_CH + BK_QT) * (BK_KS / 8) / BK_NT)   // 16-byte pieces a thread stages per slab (6)

__global__ __launch_bounds__(BK_NT) void bank_sim_max_kernel(const bf16_t* __restrict__ q, long q_row0, long q_sample_rows,
                                                             const bf16_t* __restrict__ bank, const int* __restrict__ bank_off,
                                                             const int* __restrict__ bank_rows, float* __restrict__ part, int L,
                                                             int D, int max_chunks) {
  __shared__ __attribute__((aligned(16))) bf16_t lds[2][BK_TILE];
  const int b = blockIdx.z, chunk = blockIdx.y, l0 = blockIdx.x * BK_QT;
  const int rows = bank_rows[b];                    // uniform: a scalar load, and the exit below a scalar branch
  const int r0 = chunk * BK_CH;
  if (r0 >= rows) return;
  const long off = bank_off[b];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, lg = lane >> 4;

  const bf16_t* src[BK_LD];
  int dst[BK_LD], col[BK_LD];
#pragma unroll
  for (int i = 0; i < BK_LD; ++i) {
    const int piece = tid + BK_NT * i, row = piece >> 3;
    col[i] = (piece & 7) * 8;
    dst[i] = row * BK_RS + col[i];
    if (row < BK_CH) {
      const int br = min(r0 + row, rows - 1);       // tail rows: the class's own last row, masked below
      src[i] = bank + (off + br) * (long)D + col[i];
    } else {
      const int ql = min(l0 + row - BK_CH, L - 1);  // tail rows: the sample's own last patch, never stored
      src[i] = q + ((long)b * q_sample_rows + q_row0 + ql) * (long)D + col[i];
    }
  }
  uint4 st[BK_LD];
#pragma unroll
  for (int i = 0; i < BK_LD; ++i) st[i] = make_uint4(0, 0, 0, 0);
  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < BK_LD; ++i)
      if (k0 + col[i] < D) st[i] = *reinterpret_cast<const uint4*>(src[i] + k0);   // D % 32 == 0: a piece is inside or outside
  };
  auto stage = [&](int buf) {
#pragma unroll
    for (int i = 0; i < BK_LD; ++i) *reinterpret_cast<uint4*>(&lds[buf][dst[i]]) = st[i];
  };

  float4_t acc[BK_CH / 16];
#pragma unroll
  for (int j = 0; j < BK_CH / 16; ++j) acc[j] = (float4_t){0.f, 0.f, 0.f, 0.f};
  const int nslab = (D + BK_KS - 1) / BK_KS;
  fetch(0);
  stage(0);
  __syncthreads();
  for (int s = 0; s < nslab; ++s) {
    const bool more = s + 1 < nslab;
    if (more) fetch((s + 1) * BK_KS);
    const bf16_t* bt = lds[s & 1];
    const bf16_t* qt = bt + BK_CH * BK_RS;
    const int steps = min(BK_KS, D - s * BK_KS) / 32;
    for (int kk = 0; kk < steps; ++kk) {
      const short8_t qf = lds_frag_rm<BK_RS>(qt, wave, kk, lr, lg);
#pragma unroll
      for (int j = 0; j < BK_CH / 16; ++j)
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lds_frag_rm<BK_RS>(bt, j, kk, lr, lg), qf, acc[j], 0, 0, 0);
    }
    if (more) stage((s + 1) & 1);                   // last read in iteration s - 1, before its barrier
    __syncthreads();
  }

  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < BK_CH / 16; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (r0 + 16 * j + 4 * lg + r < rows) m = fmaxf(m, acc[j][r]);
  m = fmaxf(m, __shfl_xor(m, 16, 64));
  m = fmaxf(m, __shfl_xor(m, 32, 64));
  const int l = l0 + 16 * wave + lr;
  if (lg == 0 && l < L) part[((long)b * max_chunks + chunk) * L + l] = m;
}

// part [T, B, max_chunks, L = h h]; one workgroup rebuilds its sample's sim plane in LDS (every workgroup of a sample computes
// the same L values from the same inputs in the same order) and then writes its share of the S x S map and the h x h mask.
__global__ __launch_bounds__(BK_NT) void bank_sim_finish_kernel(const float* __restrict__ part, const int* __restrict__ bank_rows,
                                                                float* __restrict__ sim, float* __restrict__ simmask,
                                                                float* __restrict__ amap, int T, int B, int max_chunks, int h,
                                                                int S, float w) {
  extern __shared__ __attribute__((aligned(16))) float plane[];
  const int b = blockIdx.y, L = h * h;
  const int nch = min((bank_rows[b] + BK_CH - 1) / BK_CH, max_chunks);   // never past the slots bank_sim_max was given
  for (int l = threadIdx.x; l < L; l += BK_NT) {
    float acc = 0.f;
    for (int t = 0; t < T; ++t) {
      const float* p = part + (((long)t * B + b) * max_chunks) * L + l;
      float m = -INFINITY;
      for (int c = 0; c < nch; ++c) m = fmaxf(m, p[(long)c * L]);
      acc += w * m;                                 // rowmax_skip_kernel's accumulation, taps in ascending order
    }
    plane[l] = acc;
    if (blockIdx.x == 0) sim[(long)b * L + l] = acc;
  }
  __syncthreads();
  const int nmap = S * S;
  const float dS = bilinear_ac_div(S), dh = bilinear_ac_div(h);
  for (int it = blockIdx.x * BK_NT + threadIdx.x; it < nmap + L; it += gridDim.x * BK_NT) {
    if (it < nmap) {
      const int oy = it / S, ox = it - oy * S;
      const float v = bilinear_ac_at(plane, h, h, oy, ox, dS, dS);
      amap[(long)b * nmap + it] = 1.f - v;
    } else {
      const int i = it - nmap, oy = i / h, ox = i - oy * h;
      const float v = bilinear_ac_at(plane, h, h, oy, ox, dh, dh);   // the identity resize, as bilinear_ac(sim, h, h) does it
      simmask[(long)b * L + i] = 1.f - v;
    }
  }
}

extern "C" int mh_bank_sim_chunk_rows(void) { return BK_CH; }

extern "C" int mh_bank_sim_max(const void* q, long q_row0, long q_sample_rows, const void* bank, const int* bank_off,
                               const int* bank_rows, float* part, int B, int L, int D, int max_chunks, hipStream_t stream) {
  if (!q || !bank || !bank_off || !bank_rows || !part) return MH_ERR_ARG;
  if (B < 1 || B > 65535 || L < 1 || D < 32 || (D % 32) != 0 || max_chunks < 1 || max_chunks > 65535) return MH_ERR_ARG;
  if (q_row0 < 0 || q_sample_rows < q_row0 + L) return MH_ERR_ARG;
  hipLaunchKernelGGL(bank_sim_max_kernel, dim3((L + BK_QT - 1) / BK_QT, max_chunks, B), dim3(BK_NT), 0, stream,
                     (const bf16_t*)q, q_row0, q_sample_rows, (const bf16_t*)bank, bank_off, bank_rows, part, L, D, max_chunks);
  MH_CHECK_LAUNCH();
  return MH_OK;
}

extern "C" int mh_bank_sim_finish(const float* part, const int* bank_rows, float* sim, float* simmask, float* amap, int T, int B,
                                  int max_chunks, int h, int S, float w, hipStream_t stream) {
  if (!part || !bank_rows || !sim || !simmask || !amap) return MH_ERR_ARG;
  if (T < 1 || B < 1 || B > 65535 || max_chunks < 1 || h < 1 || h > 128 || S < 1 || S > 4096) return MH_ERR_ARG;
  const int items = S * S + h * h;
  int slices = (items + BK_NT - 1) / BK_NT;
  if (slices > 32) slices = 32;
  hipLaunchKernelGGL(bank_sim_finish_kernel, dim3(slices, B), dim3(BK_NT), (size_t)h * h * sizeof(float), stream, part,
                     bank_rows, sim, simmask, amap, T, B, max_chunks, h, S, w);
  MH_CHECK_LAUNCH();
  return MH_OK;
}
