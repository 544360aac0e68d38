// K5 (decode): skinny-M GEMM  C[M<=16, N] = alpha * A[M,K] . B[N,K]^T (+bias) (+residual)  -- weight streaming.
//
// One decode token multiplies 1..16 activation rows by every frozen weight matrix (13.2 GB bf16 per token for
// Vicuna-7B, reference modeling_llama.py:184-231 with the KV cache): HBM-bound, 2.1 ms/token at 6.3 TB/s.  The
// 128x128 training tile starves here (N = 4096 gives 32 workgroups for 256 CUs and nothing hides HBM latency), so
// this kernel makes the WEIGHT stream the only thing that matters:
//   * a workgroup owns 16 output columns (16 weight rows), its 4 waves split K and are reduced through LDS at the
//     end  ->  N/16 workgroups (768 for qkv, 1376 for gate|up), ~1k waves streaming;
//   * every lane loads its weight fragment straight from global memory in MFMA B-operand layout (no LDS round
//     trip -- the operand is read once and never shared between waves).  The dot product does not care which k a
//     lane holds as long as both operands agree, so lane (row, lg) takes 32 CONTIGUOUS bytes (k = 16*lg .. +15 of a
//     64-deep step, two MFMAs): the four lanes of a row then cover one whole 128-B line per step instead of half of
//     one (the first version, 16 B per lane of a 32-deep step, measured 3.9-4.2 TB/s; superseded in round 1 and since removed);
//   * the activation rows (<= 16 x K bf16, L2-resident) are read as the A operand of v_mfma_f32_16x16x32_bf16, so
//     one MFMA retires 1 KiB of weights: the matrix pipe is idle-cheap and exact-fp32 accumulation comes for free.
//
// FP8 weight-only decode (opt-in, llama.py decode_fp8): the packed kernels (MODE 2 and gemv_pro_kernel) also take a copy of W
// as OCP e4m3fn codes q [N, K] with one fp32 scale s_n per output row (mh_gemv_pack_fp8: s_n = amax_n / 448, q = e4m3fn(W / s_n),
// round to nearest even, saturated to +-448).  Same k per lane as the bf16 copy: a lane's 16 B now hold all 16 k of a 64-deep
// step, so one wave-instruction still reads one contiguous KiB, which is twice the k-depth.  Each code is widened exactly to
// bf16 in registers (v_cvt_scalef32_pk_bf16_fp8, scale 1; every e4m3fn value, subnormals included, is a bf16 value) and fed to
// the same v_mfma_f32_16x16x32_bf16, so products and the fp32 accumulation are those of x . q exactly.  s_n is applied in the
// epilogue, once per output column, after the cross-wave sum and BEFORE alpha:  v = (sum_k x q * s_n) * alpha (+bias)(+res).
// Activations are never quantised.
//
// MXFP4 weight-only decode (opt-in, llama.py decode_fp4): a third packed copy, OCP microscaling e2m1 codes with one power-of-two
// scale byte per 32 consecutive k of a row (mh_gemv_pack_fp4; the format rule is in include/myriad_hip.h).  A wave's step is
// 128 deep: lane (lr, lg) holds k = 32*lg .. 32*lg+31 of it in 16 B, so one wave-instruction still reads one contiguous KiB
// and a lane needs exactly one scale byte per step.  The scale bytes of four consecutive steps of a lane share one dword, so a
// 16-step batch costs four scale loads beside its sixteen code loads.  Each pair of codes is widened to bf16 in registers by
// v_cvt_scalef32_pk_bf16_fp4 with the block scale 2^(b-127) as its scale operand -- exact, every code * scale is a normal bf16
// or zero -- and fed to four v_mfma_f32_16x16x32_bf16 per step: products and fp32 sums are those of x . dq(W), no epilogue scale.
//
// Structure.  The three decode kernels -- gemv_kernel<2> (16 rows), gemv_pro_kernel (16 rows, the operand built in LDS by a
// fused prologue) and gemv_wide_kernel (17..64 rows, G column blocks per workgroup) -- share
//   gv_load / gv_mfma, gv_mfma_fp4, gv_fp4_widen, fp8x8_to_bf16   one step of a lane, by weight type;
//   gv_fp4_load / gv_fp4_mfma   one batch of up to UNROLL fp4 steps (gemv_kernel<2> and gemv_pro_kernel).  The bf16 / fp8 batch
//                    loops of those two kernels and the wide kernel's batch keep their own text: folded into shared helpers they
//                    no longer compile to today's instruction streams;
//   gv_red_put / gv_red_finish / gv_finish   the cross-wave sum through LDS and the epilogue (fp8 row scale, alpha, bias,
//                    residual, store), one text for all three kernels and the row-major MODE 1.
// Host side: the twelve product entries {plain, RMSNorm, SiLU, wide} x {bf16, fp8, fp4} are one argument record (GvArgs) and one
// entry body (gv_entry) in front of the three launchers; the layout rule of the packed copies (waves, steps per wave, column
// blocks) is gv_layout in gemv_pack.h, shared with every packer and with lora_merge.hip.
#include "common.h"
#include "gemv_pack.h"
#include <type_traits>

typedef unsigned char fp8_t;                                        // one OCP e4m3fn code
struct fp4_t { unsigned char v; };                                  // two OCP e2m1 codes, the lower k in the low nibble
template <typename WT> constexpr bool gv_is_fp4 = false;
template <> constexpr bool gv_is_fp4<fp4_t> = true;
typedef __attribute__((ext_vector_type(4))) unsigned gv_u4_t;

// 8 e4m3fn codes (two dwords, k ascending from the low byte) -> 8 bf16 in MFMA operand order; exact
__device__ __forceinline__ short8_t fp8x8_to_bf16(unsigned a, unsigned b) {
  gv_u4_t r;
  r[0] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(a, 1.0f, false));
  r[1] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(a, 1.0f, true));
  r[2] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(b, 1.0f, false));
  r[3] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(b, 1.0f, true));
  return __builtin_bit_cast(short8_t, r);
}

// One lane's weight fragment of one 64-deep step of a packed copy (k = 16*lg .. 16*lg+15), by weight type: the load is
// issued early (raw bytes held in registers), the widening happens at the MFMA.  A step is 1024 elements of WT in both
// layouts: 2 KiB of bf16 as two KiB halves (w0, w1), 1 KiB of fp8 (all 16 codes in w0; w1 is not used).
template <typename WT>
__device__ __forceinline__ void gv_load(const WT* wp, size_t t, short8_t& w0, short8_t& w1) {
  if constexpr (sizeof(WT) == 1) {
    w0 = __builtin_nontemporal_load(reinterpret_cast<const short8_t*>(wp + t * 1024));
  } else {
    w0 = __builtin_nontemporal_load(reinterpret_cast<const short8_t*>(wp + t * 1024));
    w1 = __builtin_nontemporal_load(reinterpret_cast<const short8_t*>(wp + t * 1024 + 512));
  }
}
template <typename WT>
__device__ __forceinline__ float4_t gv_mfma(short8_t x0, short8_t x1, short8_t w0, short8_t w1, float4_t acc) {
  if constexpr (sizeof(WT) == 1) {
    const gv_u4_t q = __builtin_bit_cast(gv_u4_t, w0);
    w0 = fp8x8_to_bf16(q[0], q[1]);
    w1 = fp8x8_to_bf16(q[2], q[3]);
  }
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x0, w0, acc, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(x1, w1, acc, 0, 0, 0);
}

// 8 e2m1 codes (one dword, k ascending from the low nibble, one byte_sel each pair) times the block scale -> 8 bf16 in MFMA
// operand order; exact
__device__ __forceinline__ short8_t gv_fp4_widen(unsigned q, float sc) {
  gv_u4_t r;
  r[0] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, sc, 0));
  r[1] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, sc, 1));
  r[2] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, sc, 2));
  r[3] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, sc, 3));
  return __builtin_bit_cast(short8_t, r);
}
// One lane's 128-deep fp4 step: x = its 32 activations (k = 32*lg .. +31 of the step, global memory or LDS), q = its 32 codes,
// b = the block's scale byte.  Eight codes (one dword, one byte_sel each pair) make the B operand of one MFMA.
__device__ __forceinline__ float4_t gv_mfma_fp4(const bf16_t* x, short8_t q16, unsigned b, float4_t acc) {
  const gv_u4_t q = __builtin_bit_cast(gv_u4_t, q16);
  const float sc = __uint_as_float(b << 23);                        // 2^(b-127), b in 2..252
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const short8_t w = gv_fp4_widen(q[i], sc);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const short8_t*>(x + 8 * i), w, acc, 0, 0, 0);
  }
  return acc;
}
// One batch of fp4 steps of a wave: n <= UNROLL live steps starting at step t0 of the wave's range (a multiple of 4; FULL: n =
// UNROLL, no guards).  The load puts the raw codes (16 B per step) and the scale dwords (four steps each) in registers; the
// product walks the steps in order, x = the lane's activations at the batch's first step (128 elements per step).
template <int UNROLL, bool FULL>
__device__ __forceinline__ void gv_fp4_load(const fp4_t* wp, const unsigned* sp, int t0, int n, short8_t (&w)[UNROLL],
                                            unsigned (&sc)[UNROLL / 4]) {
#pragma unroll
  for (int u = 0; u < UNROLL; ++u)
    if (FULL || u < n) w[u] = __builtin_nontemporal_load(reinterpret_cast<const short8_t*>(wp + (size_t)(t0 + u) * 1024));
#pragma unroll
  for (int g = 0; g < UNROLL / 4; ++g)
    if (FULL || 4 * g < n) sc[g] = __builtin_nontemporal_load(sp + (size_t)(t0 / 4 + g) * 64);
}
template <int UNROLL, bool FULL>
__device__ __forceinline__ float4_t gv_fp4_mfma(const bf16_t* x, int n, const short8_t (&w)[UNROLL], const unsigned (&sc)[UNROLL / 4],
                                                float4_t acc) {
#pragma unroll
  for (int u = 0; u < UNROLL; ++u)
    if (FULL || u < n) acc = gv_mfma_fp4(x + u * 128, w[u], (sc[u >> 2] >> (8 * (u & 3))) & 0xffu, acc);
  return acc;
}

// The epilogue of one output element of all three kernels: v is the cross-wave sum (times the fp8 row scale)
__device__ __forceinline__ void gv_finish(float v, int m, int n, void* Cv, const float* bias, const float* res, int ldc, int ldr,
                                          int out_f32, float alpha) {
  v *= alpha;
  if (bias) v += bias[n];
  if (res) v += res[(size_t)m * ldr + n];
  if (out_f32) reinterpret_cast<float*>(Cv)[(size_t)m * ldc + n] = v;
  else reinterpret_cast<bf16_t*>(Cv)[(size_t)m * ldc + n] = f2bf(v);
}
// The cross-wave K reduction through LDS, red[wave][column block of the group][16 x 16].  D layout: row 4*lg + r, col lr.
// gv_red_put: a wave's partial sums of block g (a barrier follows).  gv_red_finish: element (ml, lr) of block g, summed over
// w = 0 .. NW-1 from 0.f, the fp8 row scale s_n first, then gv_finish.
template <int NW, int G>
__device__ __forceinline__ void gv_red_put(float (&red)[NW][G][16 * 16], int wave, int g, int lr, int lg, float4_t acc) {
#pragma unroll
  for (int r = 0; r < 4; ++r) red[wave][g][(4 * lg + r) * 16 + lr] = acc[r];
}
template <int NW, int G, bool F8>
__device__ __forceinline__ void gv_red_finish(const float (&red)[NW][G][16 * 16], int g, int ml, int lr, int m, int n, void* Cv,
                                              const float* bias, const float* res, int ldc, int ldr, int out_f32, float alpha,
                                              const float* wscale) {
  float v = 0.f;
#pragma unroll
  for (int w = 0; w < NW; ++w) v += red[w][g][ml * 16 + lr];
  if constexpr (F8) v *= wscale[n];              // the row scale s_n first, then alpha
  gv_finish(v, m, n, Cv, bias, res, ldc, ldr, out_f32, alpha);
}

// MODE 1: B row-major [N, ldb] (the M <= 16 path of mh_gemm_bf16_nt).  MODE 2: B as a packed copy (bf16, fp8 or fp4).
template <int MODE, int UNROLL, int GV_NW, typename WT = bf16_t>
__global__ __launch_bounds__(GV_NW * 64) void gemv_kernel(const bf16_t* __restrict__ A, const WT* __restrict__ B,
                                                          void* __restrict__ Cv, const float* __restrict__ bias,
                                                          const float* res, int M, int N, int K, int lda, int ldb,
                                                          int ldc, int ldr, int out_f32, float alpha,
                                                          const float* __restrict__ wscale = nullptr) {
  constexpr bool F4 = gv_is_fp4<WT>, F8 = sizeof(WT) == 1 && !F4;
  constexpr int KS = F4 ? 128 : 64;                                // k-depth of one step of the packed copy
  static_assert(MODE == 1 || MODE == 2, "row-major or the packed copy");
  static_assert(!(F8 || F4) || MODE == 2, "fp8 / fp4 weights come only as the packed copy");
  __shared__ float red[GV_NW][1][16 * 16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int n0 = blockIdx.x * 16;
  int nrow = n0 + lr;
  nrow = nrow < N ? nrow : N - 1;
  const int mrow = lr < M ? lr : M - 1;          // rows >= M duplicate the last row; their results are never stored
  float4_t acc = (float4_t){0.f, 0.f, 0.f, 0.f};
  if constexpr (MODE == 2) {
    // MODE 1's arithmetic on a pre-permuted weight copy (mh_gemv_pack): the bytes lane (lr, lg) of wave w needs at step t
    // sit at ((block * NW + w) * per + t) * 2 KiB + h * 1 KiB + lane * 16, so every wave-instruction reads one contiguous
    // KiB and a wave walks one contiguous region -- 6.8 TB/s against 5.8 TB/s for the row-strided order on a pure stream
    // (tools/micro/stream_pattern.hip), and bit-identical results (same k per lane, same reduction order).
    // The fp8 copy (mh_gemv_pack_fp8): ((block * NW + w) * per + t) * 1 KiB + lane * 16, one KiB per step.
    // The fp4 copy (mh_gemv_pack_fp4): the same KiB per step at twice the depth, steps counted in 128; the scale bytes come as
    // dwords from wscale: ((block * NW + w) * ceil(per / 4) + t / 4) * 256 B + lane * 4, byte t % 4.
    const bf16_t* xp = A + (size_t)mrow * lda + lg * (KS / 4);
    const int nsteps = K / KS;
    const int per = (nsteps + GV_NW - 1) / GV_NW;
    const WT* wp = B + ((size_t)blockIdx.x * GV_NW + wave) * per * 1024 + lane * (16 / sizeof(WT));
    int s = wave * per;
    const int s0 = s;
    const int s_end = (s + per) < nsteps ? (s + per) : nsteps;
    if constexpr (F4) {
      const unsigned* sp = reinterpret_cast<const unsigned*>(wscale) + ((size_t)blockIdx.x * GV_NW + wave) * ((per + 3) / 4) * 64 + lane;
      short8_t w[UNROLL];
      unsigned sc[UNROLL / 4];
      for (; s + UNROLL <= s_end; s += UNROLL) {
        gv_fp4_load<UNROLL, true>(wp, sp, s - s0, UNROLL, w, sc);
        acc = gv_fp4_mfma<UNROLL, true>(xp + (size_t)s * 128, UNROLL, w, sc, acc);
      }
      if (s < s_end) {                                 // remainder as one partial batch, same order
        gv_fp4_load<UNROLL, false>(wp, sp, s - s0, s_end - s, w, sc);
        acc = gv_fp4_mfma<UNROLL, false>(xp + (size_t)s * 128, s_end - s, w, sc, acc);
      }
    } else {
      for (; s + UNROLL <= s_end; s += UNROLL) {
        short8_t w0[UNROLL], w1[UNROLL], x0[UNROLL], x1[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
          const int k = (s + u) * 64;
          gv_load(wp, (size_t)(s - s0 + u), w0[u], w1[u]);
          x0[u] = *reinterpret_cast<const short8_t*>(xp + k);
          x1[u] = *reinterpret_cast<const short8_t*>(xp + k + 8);
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) acc = gv_mfma<WT>(x0[u], x1[u], w0[u], w1[u], acc);
      }
      if (s < s_end) {                                   // remainder as one partial batch (loads in flight together), same order
        const int rem = s_end - s;
        short8_t w0[UNROLL], w1[UNROLL], x0[UNROLL], x1[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u)
          if (u < rem) {
            const int k = (s + u) * 64;
            gv_load(wp, (size_t)(s - s0 + u), w0[u], w1[u]);
            x0[u] = *reinterpret_cast<const short8_t*>(xp + k);
            x1[u] = *reinterpret_cast<const short8_t*>(xp + k + 8);
          }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u)
          if (u < rem) acc = gv_mfma<WT>(x0[u], x1[u], w0[u], w1[u], acc);
      }
    }
  } else {
    // 64-deep steps, lane holds k = 16*lg .. 16*lg+15 (32 contiguous bytes); wave w owns the contiguous K quarter
    // [w*K/4, (w+1)*K/4) rounded to steps, so each wave walks 16 rows line by line
    const bf16_t* wp = B + (size_t)nrow * ldb + lg * 16;
    const bf16_t* xp = A + (size_t)mrow * lda + lg * 16;
    const int nsteps = K / 64;
    const int per = (nsteps + GV_NW - 1) / GV_NW;
    int s = wave * per;
    const int s_end = (s + per) < nsteps ? (s + per) : nsteps;
    for (; s + UNROLL <= s_end; s += UNROLL) {
      short8_t w0[UNROLL], w1[UNROLL], x0[UNROLL], x1[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const int k = (s + u) * 64;
        w0[u] = __builtin_nontemporal_load(reinterpret_cast<const short8_t*>(wp + k));
        w1[u] = __builtin_nontemporal_load(reinterpret_cast<const short8_t*>(wp + k + 8));
        x0[u] = *reinterpret_cast<const short8_t*>(xp + k);
        x1[u] = *reinterpret_cast<const short8_t*>(xp + k + 8);
      }
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x0[u], w0[u], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x1[u], w1[u], acc, 0, 0, 0);
      }
    }
    for (; s < s_end; ++s) {
      const int k = s * 64;
      const short8_t w0 = *reinterpret_cast<const short8_t*>(wp + k), w1 = *reinterpret_cast<const short8_t*>(wp + k + 8);
      const short8_t x0 = *reinterpret_cast<const short8_t*>(xp + k), x1 = *reinterpret_cast<const short8_t*>(xp + k + 8);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x0, w0, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x1, w1, acc, 0, 0, 0);
    }
  }
  // D layout: row m = 4*lg + r, col n = lr.  Cross-wave K reduction through LDS, then wave 0 finishes.
  gv_red_put(red, wave, 0, lr, lg, acc);         // one column block: wave 0 finishes it
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = 4 * lg + r, n = n0 + lr;
      if (m < M && n < N) gv_red_finish<GV_NW, 1, F8>(red, 0, m, lr, m, n, Cv, bias, res, ldc, ldr, out_f32, alpha, wscale);
    }
  }
}

// called from mh_gemm_bf16_nt for M <= 16 (no GELU epilogue on this path): 8 waves when N / 16 workgroups under-fill the chip
// (N = 4096, K = 11008: 4.12 vs 3.86 TB/s with 8 waves), else 4 -- gv_packed_nw, the rule of the packed copies
int mh_launch_gemv(const void* A, int lda, const void* B, int ldb, void* C, int ldc, int M, int N, int K,
                   const float* bias, const float* residual, int ldr, int out_f32, float alpha, hipStream_t stream) {
  const dim3 grid((N + 15) / 16);
#define GV_LAUNCH(NW)                                                                                                \
  hipLaunchKernelGGL((gemv_kernel<1, 8, NW>), grid, dim3(NW * 64), 0, stream, (const bf16_t*)A, (const bf16_t*)B, C, \
                     bias, residual, M, N, K, lda, ldb, ldc, ldr, out_f32, alpha)
  if (gv_packed_nw(N) == 8) GV_LAUNCH(8);
  else GV_LAUNCH(4);
#undef GV_LAUNCH
  MH_CHECK_LAUNCH();
  return MH_OK;
}

// ---- stream-ordered weight copy for decode (288 GB of HBM: a second, 13.5 GB copy of the frozen LLaMA weights is cheap) ----

__global__ void gemv_pack_kernel(const bf16_t* __restrict__ W, int ldb, int N, int K, bf16_t* __restrict__ out, int nw, int per,
                                 long chunks) {
  const int nsteps = K / 64;
  for (long c = blockIdx.x * (long)blockDim.x + threadIdx.x; c < chunks; c += (long)gridDim.x * blockDim.x) {
    const int lane = (int)(c & 63), h = (int)((c >> 6) & 1);
    long r = c >> 7;
    const int t = (int)(r % per); r /= per;
    const int q = (int)(r % nw);
    const long nb = r / nw;
    const int lr = lane & 15, lg = lane >> 4;
    long row = nb * 16 + lr;
    row = row < N ? row : N - 1;
    const int step = q * per + t;
    short8_t v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (step < nsteps) v = *reinterpret_cast<const short8_t*>(W + row * ldb + step * 64 + lg * 16 + h * 8);
    *reinterpret_cast<short8_t*>(out + c * 8) = v;
  }
}

extern "C" long mh_gemv_pack_elems(int N, int K) {
  if (N <= 0 || K <= 0 || (K % 64) != 0) return -1;
  const GvLayout L = gv_layout(N, K, 64);
  return (long)L.blocks * L.nw * L.per * 1024;
}

extern "C" int mh_gemv_pack(const void* W, int ldb, int N, int K, void* out, hipStream_t stream) {
  if (N <= 0 || K <= 0 || (K % 64) != 0 || (ldb % 8) != 0 || ((uintptr_t)W & 15) || ((uintptr_t)out & 15)) return MH_ERR_ARG;
  const GvLayout L = gv_layout(N, K, 64);
  const long chunks = (long)L.blocks * L.nw * L.per * 128;
  long grid = (chunks + 255) / 256;
  if (grid > 65536) grid = 65536;
  hipLaunchKernelGGL(gemv_pack_kernel, dim3((int)grid), dim3(256), 0, stream, (const bf16_t*)W, ldb, N, K, (bf16_t*)out, L.nw, L.per,
                     chunks);
  MH_CHECK_LAUNCH();
  return MH_OK;
}

// weights in flight per lane per batch: 8 steps of the bf16 copy (16 KiB per wave), 16 of the fp8 copy (the same 16 KiB)
// (the fp4 copy: 16 steps of twice the depth, again 16 KiB)
template <typename WT> struct GvUnroll { static constexpr int value = sizeof(WT) == 1 ? 16 : 8; };
template <typename WT> constexpr int gv_kstep = gv_is_fp4<WT> ? 128 : 64;

// ---- the product entries' host side: one argument record, one launcher per kernel, one entry body ---------------------------
// The arguments of a product entry.  A: the activations (bf16 rows; the fused forms: f32 rows h or bf16 gate|up rows), lda in
// elements; P / wscale: the packed copy and its fp8 row scales or fp4 scale bytes (null for bf16); norm_w / eps: RMSNorm only.
struct GvArgs {
  const void* A;
  long lda;                  // the fused forms' leading dimension is a long; the bf16-row forms get an int and pass one on
  const void* P;
  const void* wscale;
  void* C;
  int ldc, M, N, K;
  const float* bias;
  const float* residual;
  int ldr, out_f32;
  float alpha;
  hipStream_t stream;
  const float* norm_w = nullptr;
  float eps = 0.f;
};
// what is in front of the product.  GV_SILU / GV_RMSNORM are gemv_pro_kernel's PRO; GV_PLAIN and GV_WIDE never reach that kernel
enum { GV_PLAIN = 0, GV_SILU = 1, GV_RMSNORM = 2, GV_WIDE = 3 };

template <typename WT>
static int launch_gemv_packed(const GvArgs& a) {
  if (a.M > 16 || a.K <= 0 || (a.K % gv_kstep<WT>) != 0 || (a.lda % 8) != 0 || ((uintptr_t)a.A & 15) || ((uintptr_t)a.P & 15))
    return MH_ERR_ARG;
  constexpr int U = GvUnroll<WT>::value;
  const GvLayout L = gv_layout(a.N, a.K, gv_kstep<WT>);
#define GV_LAUNCH(NW)                                                                                                            \
  hipLaunchKernelGGL((gemv_kernel<2, U, NW, WT>), dim3(L.blocks), dim3(NW * 64), 0, a.stream, (const bf16_t*)a.A, (const WT*)a.P, \
                     a.C, a.bias, a.residual, a.M, a.N, a.K, (int)a.lda, 0, a.ldc, a.ldr, a.out_f32, a.alpha, (const float*)a.wscale)
  if (L.nw == 8) GV_LAUNCH(8);
  else GV_LAUNCH(4);
#undef GV_LAUNCH
  MH_CHECK_LAUNCH();
  return MH_OK;
}

// ---- fp8 (e4m3fn) weight-only copy: row scale, quantisation and the stream order in one kernel ----------------------------
// q [N, K] e4m3fn in mh_gemv_pack's order at one byte per weight: lane (lr, lg) of wave w reads at step t the 16 codes
// k = 64 t' + 16 lg .. +15 (t' = w * per + t) of row 16 * block + lr at ((block * NW + w) * per + t) * 1 KiB + lane * 16.
// One workgroup per 16-row block: the 16 threads of a row find amax_n, then s_n = amax_n / 448 (fp32, correctly rounded;
// 1 for an all-zero row) and q = e4m3fn(clamp(W / s_n, -448, 448)) rounded to nearest even -- torch's
// (W.float() / s[:, None]).clamp(-448, 448).to(torch.float8_e4m3fn), bit for bit.  Rows past N repeat row N - 1 (as the bf16
// copy); their results are never stored.
__global__ __launch_bounds__(256) void gemv_pack_fp8_kernel(const bf16_t* __restrict__ W, int ldb, int N, int K,
                                                            unsigned char* __restrict__ out, float* __restrict__ scale_out, int nw,
                                                            int per) {
  __shared__ float srow[16];
  const int tid = threadIdx.x, nb = blockIdx.x;
  {
    const int lr = tid >> 4, j = tid & 15;
    int row = nb * 16 + lr;
    row = row < N ? row : N - 1;
    float amax = 0.f;
    for (int k = j * 8; k < K; k += 128) {
      const short8_t v = *reinterpret_cast<const short8_t*>(W + (size_t)row * ldb + k);
#pragma unroll
      for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(bf2f((bf16_t)v[e])));
    }
#pragma unroll
    for (int o = 8; o >= 1; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o));   // the 16 lanes of one row
    if (j == 0) {
      const float sc = amax > 0.f ? amax / 448.0f : 1.0f;
      srow[lr] = sc;
      if (nb * 16 + lr < N) scale_out[nb * 16 + lr] = sc;
    }
  }
  __syncthreads();
  const int nsteps = K / 64, chunks = nw * per * 64;
  for (int c = tid; c < chunks; c += 256) {
    const int lane = c & 63, r = c >> 6;
    const int t = r % per, q = r / per;
    const int lr = lane & 15, lg = lane >> 4;
    int row = nb * 16 + lr;
    row = row < N ? row : N - 1;
    const int step = q * per + t;
    gv_u4_t o = {0u, 0u, 0u, 0u};
    if (step < nsteps) {
      const bf16_t* src = W + (size_t)row * ldb + step * 64 + lg * 16;
      const short8_t v0 = *reinterpret_cast<const short8_t*>(src), v1 = *reinterpret_cast<const short8_t*>(src + 8);
      const float sc = srow[lr];
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const float w = bf2f((bf16_t)(e < 8 ? v0[e] : v1[e - 8]));
        const float x = fminf(fmaxf(w / sc, -448.f), 448.f);
        o[e >> 2] |= f32_to_e4m3fn(x) << (8 * (e & 3));
      }
    }
    *reinterpret_cast<gv_u4_t*>(out + ((size_t)nb * chunks + c) * 16) = o;
  }
}

extern "C" long mh_gemv_pack_fp8_elems(int N, int K) { return mh_gemv_pack_elems(N, K); }   // bytes: one per bf16 element

extern "C" int mh_gemv_pack_fp8(const void* W, int ldb, int N, int K, void* q_out, float* scale_out, hipStream_t stream) {
  if (N <= 0 || K <= 0 || (K % 64) != 0 || (ldb % 8) != 0 || ldb < K || !scale_out || ((uintptr_t)W & 15) || ((uintptr_t)q_out & 15) ||
      ((uintptr_t)scale_out & 3))
    return MH_ERR_ARG;
  const GvLayout L = gv_layout(N, K, 64);
  hipLaunchKernelGGL(gemv_pack_fp8_kernel, dim3(L.blocks), dim3(256), 0, stream, (const bf16_t*)W, ldb, N, K, (unsigned char*)q_out,
                     scale_out, L.nw, L.per);
  MH_CHECK_LAUNCH();
  return MH_OK;
}

// ---- decode GEMV with the producer of its activation operand fused in (one launch instead of two per Linear) ---------------
// The single-token step runs ~290 launches of 3-25 us; the RMSNorm in front of the qkv / gate|up / lm_head products and the
// SiLU gate in front of the down projection are per-row elementwise work on <= 16 rows that every workgroup can redo for
// itself: the operand rows are built ONCE per workgroup into LDS (bf16, [M][K]) and the weight stream then runs exactly as
// gemv_kernel<2> (same k per lane, same reduction order: bit-identical to the two-launch form).
//   PRO 1 (SiLU gate, modeling_llama.py:139-140): A = gu [M, 2K] bf16 with gate / up interleaved in blocks of 128
//          (llama.py interleave_gate_up); operand = bf16(silu(g) * u), the expression of silu_mul_fwd_kernel.
//   PRO 2 (RMSNorm, modeling_llama.py:66-74): A = h [M, K] f32; operand = bf16(w * (h * rsqrt(mean(h^2) + eps))): the first
//          256 threads sum the squares in rmsnorm_fwd_kernel's order (thread t: elements 4t + 1024 j) and the block reduction
//          adds the same four wave sums first, so the scale and every operand element carry the same bits.
template <int UNROLL, int GV_NW, int PRO, typename WT = bf16_t>
__global__ __launch_bounds__(GV_NW * 64) void gemv_pro_kernel(const void* __restrict__ Ain, long lda, const WT* __restrict__ B,
                                                              void* __restrict__ Cv, const float* __restrict__ bias, const float* res,
                                                              int M, int N, int K, int ldc, int ldr, int out_f32, float alpha,
                                                              const float* __restrict__ norm_w, float eps,
                                                              const float* __restrict__ wscale = nullptr) {
  constexpr bool F4 = gv_is_fp4<WT>, F8 = sizeof(WT) == 1 && !F4;
  constexpr int KS = F4 ? 128 : 64;                                // k-depth of one step of the packed copy
  extern __shared__ __attribute__((aligned(16))) char gsm[];
  bf16_t* xs = reinterpret_cast<bf16_t*>(gsm);                  // [M][K] operand rows
  __shared__ float red[GV_NW][1][16 * 16];
  __shared__ float bred[GV_NW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int n0 = blockIdx.x * 16;
  const int nsteps = K / KS;
  const int per = (nsteps + GV_NW - 1) / GV_NW;
  const WT* wp = B + ((size_t)blockIdx.x * GV_NW + wave) * per * 1024 + lane * (16 / sizeof(WT));
  // fp4: this wave's scale dwords (gemv_kernel<2>); not read otherwise
  const unsigned* sp =
      F4 ? reinterpret_cast<const unsigned*>(wscale) + ((size_t)blockIdx.x * GV_NW + wave) * ((per + 3) / 4) * 64 + lane : nullptr;
  // The weight stream does not depend on the operand: the first UNROLL steps of it are put in flight BEFORE the rows are
  // built (every workgroup of a launch starts at the same time; without this the HBM pipe idles for the ~3 us the prologue
  // takes).  Vector loads retire in order, so what the prologue needs first -- the fp32 row and the norm weights -- is
  // requested ahead of the weights.
  int s = wave * per;
  const int s0 = s;
  const int s_end = (s + per) < nsteps ? (s + per) : nsteps;
  bool have = s + UNROLL <= s_end;
  short8_t w0[UNROLL], w1[UNROLL];
  unsigned sc[UNROLL / 4];                                      // fp4 only
  float4_t hv[4];                                               // PRO 2: K <= 4096 (checked by the launcher)
  if (PRO == 2 && tid < 256) {
    const float* xr = reinterpret_cast<const float*>(Ain);
    int c = 0;
    for (int i = tid * 4; i < K; i += 1024, ++c) hv[c] = *reinterpret_cast<const float4_t*>(xr + i);
  }
  if (have) {
    if constexpr (F4) gv_fp4_load<UNROLL, true>(wp, sp, 0, UNROLL, w0, sc);
    else {
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) gv_load(wp, (size_t)u, w0[u], w1[u]);
    }
  }
  if (PRO == 1) {
    const bf16_t* gu = reinterpret_cast<const bf16_t*>(Ain);
    const int per_row = K >> 3;
    for (int it = tid; it < M * per_row; it += GV_NW * 64) {
      const int m = it / per_row, c = (it - m * per_row) * 8;
      const long gc = (long)(c >> 7) * 256 + (c & 127);
      const short8_t g = *reinterpret_cast<const short8_t*>(gu + (size_t)m * lda + gc);
      const short8_t u = *reinterpret_cast<const short8_t*>(gu + (size_t)m * lda + gc + 128);
      short8_t o;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float gv = bf2f((bf16_t)g[e]), uv = bf2f((bf16_t)u[e]);
        o[e] = (short)f2bf(gv / (1.f + __expf(-gv)) * uv);
      }
      *reinterpret_cast<short8_t*>(xs + (size_t)m * K + c) = o;
    }
  } else {
    const float* h = reinterpret_cast<const float*>(Ain);
    for (int m = 0; m < M; ++m) {
      const float* xr = h + (size_t)m * lda;
      float ss = 0.f;
      int c = 0;
      if (tid < 256)
        for (int i = tid * 4; i < K; i += 1024, ++c) {
          if (m > 0) hv[c] = *reinterpret_cast<const float4_t*>(xr + i);
          ss += hv[c][0] * hv[c][0] + hv[c][1] * hv[c][1] + hv[c][2] * hv[c][2] + hv[c][3] * hv[c][3];
        }
      ss = block_sum<GV_NW>(ss, bred);                        // waves 4.. add exact zeros: the sum of rmsnorm_fwd_kernel
      const float r = rsqrtf(ss / K + eps);
      c = 0;
      if (tid < 256)
        for (int i = tid * 4; i < K; i += 1024, ++c) {
          const float4_t g = *reinterpret_cast<const float4_t*>(norm_w + i);   // queues behind the weights: they are needed first anyway
          uint2 pk;
          pk.x = pack_bf2(g[0] * (hv[c][0] * r), g[1] * (hv[c][1] * r));
          pk.y = pack_bf2(g[2] * (hv[c][2] * r), g[3] * (hv[c][3] * r));
          *reinterpret_cast<uint2*>(xs + (size_t)m * K + i) = pk;
        }
    }
  }
  __syncthreads();
  const int mrow = lr < M ? lr : M - 1;
  const bf16_t* xp = xs + (size_t)mrow * K + lg * (KS / 4);
  float4_t acc = (float4_t){0.f, 0.f, 0.f, 0.f};
  while (have) {
    if constexpr (F4) acc = gv_fp4_mfma<UNROLL, true>(xp + (size_t)s * 128, UNROLL, w0, sc, acc);
    else {
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const int k = (s + u) * 64;
        const short8_t x0 = *reinterpret_cast<const short8_t*>(xp + k), x1 = *reinterpret_cast<const short8_t*>(xp + k + 8);
        acc = gv_mfma<WT>(x0, x1, w0[u], w1[u], acc);
      }
    }
    s += UNROLL;
    have = s + UNROLL <= s_end;
    if (have) {
      if constexpr (F4) gv_fp4_load<UNROLL, true>(wp, sp, s - s0, UNROLL, w0, sc);
      else {
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) gv_load(wp, (size_t)(s - s0 + u), w0[u], w1[u]);
      }
    }
  }
  if (s < s_end) {
    // the remainder of this wave's K range (K = 11008: 22 steps = 2 batches + 6) as ONE partial batch: its loads fly together
    // instead of one load latency per step; same accumulation order
    const int rem = s_end - s;
    if constexpr (F4) {
      gv_fp4_load<UNROLL, false>(wp, sp, s - s0, rem, w0, sc);
      acc = gv_fp4_mfma<UNROLL, false>(xp + (size_t)s * 128, rem, w0, sc, acc);
    } else {
#pragma unroll
      for (int u = 0; u < UNROLL; ++u)
        if (u < rem) gv_load(wp, (size_t)(s - s0 + u), w0[u], w1[u]);
#pragma unroll
      for (int u = 0; u < UNROLL; ++u)
        if (u < rem) {
          const int k = (s + u) * 64;
          const short8_t x0 = *reinterpret_cast<const short8_t*>(xp + k), x1 = *reinterpret_cast<const short8_t*>(xp + k + 8);
          acc = gv_mfma<WT>(x0, x1, w0[u], w1[u], acc);
        }
    }
  }
  gv_red_put(red, wave, 0, lr, lg, acc);         // one column block: wave 0 finishes it
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = 4 * lg + r, n = n0 + lr;
      if (m < M && n < N) gv_red_finish<GV_NW, 1, F8>(red, 0, m, lr, m, n, Cv, bias, res, ldc, ldr, out_f32, alpha, wscale);
    }
  }
}

#define GV_PRO_LDS_MAX (64 * 1024)
#define GV_PRO_MAX_ROWS 2
template <int PRO, typename WT>
static int launch_gemv_pro(const GvArgs& a) {
  const int M = a.M, K = a.K;
  if (M > 16 || K <= 0 || (K % gv_kstep<WT>) != 0 || ((uintptr_t)a.A & 15) || ((uintptr_t)a.P & 15)) return MH_ERR_ARG;
  if (PRO == GV_SILU && ((K % 128) != 0 || (a.lda % 8) != 0 || a.lda < 2L * K)) return MH_ERR_ARG;
  if (PRO == GV_RMSNORM && (!a.norm_w || (K % 4) != 0 || (a.lda % 4) != 0)) return MH_ERR_ARG;
  if (PRO == GV_RMSNORM && K > 4096) return MH_ERR_UNSUPPORTED;
  const size_t sh = (size_t)M * K * 2;
  // every workgroup rebuilds all M rows: measured at batch 8 (decode, M = 8) the fused step costs 6.5 ms per token against
  // 4.1 ms with the separate launches, at batch 1 it saves 0.3 ms -- fused for up to GV_PRO_MAX_ROWS rows only
  if (sh > GV_PRO_LDS_MAX || M > GV_PRO_MAX_ROWS) return MH_ERR_UNSUPPORTED;        // the caller falls back to the two-launch form
  constexpr int U = GvUnroll<WT>::value;
  const GvLayout L = gv_layout(a.N, K, gv_kstep<WT>);
  static bool attr8 = false, attr4 = false;                   // once per instantiation, outside any stream capture
#define GV_LAUNCH(NW, attr)                                                                                                        \
  do {                                                                                                                             \
    if (!attr) { (void)hipFuncSetAttribute((const void*)gemv_pro_kernel<U, NW, PRO, WT>, hipFuncAttributeMaxDynamicSharedMemorySize, GV_PRO_LDS_MAX); attr = true; } \
    hipLaunchKernelGGL((gemv_pro_kernel<U, NW, PRO, WT>), dim3(L.blocks), dim3(NW * 64), sh, a.stream, a.A, a.lda, (const WT*)a.P, a.C, \
                       a.bias, a.residual, M, a.N, K, a.ldc, a.ldr, a.out_f32, a.alpha, a.norm_w, a.eps, (const float*)a.wscale);   \
  } while (0)
  if (L.nw == 8) GV_LAUNCH(8, attr8);
  else GV_LAUNCH(4, attr4);
#undef GV_LAUNCH
  MH_CHECK_LAUNCH();
  return MH_OK;
}

// ---- MXFP4 weight-only copy: block amax, scale byte, e2m1 codes and the stream order in one kernel --------------------------
// Codes: mh_gemv_pack's order at half a byte per weight and 128-deep steps: lane (lr, lg) of wave w reads at step t the 32 codes
// k = 128 t' + 32 lg .. +31 (t' = w * per + t, per = ceil(K / 128 / NW)) of row 16 * block + lr at
// ((block * NW + w) * per + t) * 1 KiB + lane * 16, byte j = codes of k + 2j (low nibble) and k + 2j + 1.
// Scale bytes: that lane's block at step t at ((block * NW + w) * ceil(per / 4) + t / 4) * 256 + lane * 4 + t % 4.
// Steps past K / 128 (and the bytes that pad a scale dword) are zero blocks: codes 0, scale byte 2.  Rows past N repeat row N - 1.
// One thread quantises one block: 64 B in, 16 B and one byte out (the rule: gemv_pack.h bf16_to_e2m1, include/myriad_hip.h).
__global__ __launch_bounds__(256) void gemv_pack_fp4_kernel(const bf16_t* __restrict__ W, int ldb, int N, int K,
                                                            unsigned char* __restrict__ out, unsigned char* __restrict__ scale_out,
                                                            int nw, int per) {
  const int nb = blockIdx.x, nsteps = K / 128, per4 = (per + 3) / 4;
  const int chunks = nw * per4 * 4 * 64;
  for (int c = threadIdx.x; c < chunks; c += 256) {
    const int lane = c & 63, r = c >> 6;
    const int t = r % (per4 * 4), q = r / (per4 * 4);
    const int lr = lane & 15, lg = lane >> 4;
    int row = nb * 16 + lr;
    row = row < N ? row : N - 1;
    const int step = q * per + t;
    int b = 2;
    gv_u4_t o = {0u, 0u, 0u, 0u};
    if (t < per && step < nsteps) {
      const bf16_t* src = W + (size_t)row * ldb + step * 128 + lg * 32;
      short8_t v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = *reinterpret_cast<const short8_t*>(src + 8 * i);
      int amax = 0;                                                  // of the magnitude bits: monotonic in |w| for finite w
#pragma unroll
      for (int e = 0; e < 32; ++e) {
        const int a = v[e >> 3][e & 7] & 0x7fff;
        amax = a > amax ? a : amax;
      }
      b = mxfp4_scale_byte(amax >> 7);
#pragma unroll
      for (int e = 0; e < 32; ++e) o[e >> 3] |= bf16_to_e2m1((unsigned short)v[e >> 3][e & 7], b) << (4 * (e & 7));
    }
    scale_out[((size_t)(nb * nw + q) * per4 + (t >> 2)) * 256 + lane * 4 + (t & 3)] = (unsigned char)b;
    if (t < per) *reinterpret_cast<gv_u4_t*>(out + (((size_t)(nb * nw + q) * per + t) * 64 + lane) * 16) = o;
  }
}

static bool gv_fp4_dims(int N, int K) { return N > 0 && K > 0 && (K % 128) == 0; }

extern "C" long mh_gemv_pack_fp4_elems(int N, int K) {
  if (!gv_fp4_dims(N, K)) return -1;
  const GvLayout L = gv_layout(N, K, 128);
  return (long)L.blocks * L.nw * L.per * 1024;
}

extern "C" long mh_gemv_pack_fp4_scale_elems(int N, int K) {
  if (!gv_fp4_dims(N, K)) return -1;
  const GvLayout L = gv_layout(N, K, 128);
  return (long)L.blocks * L.nw * L.per4 * 256;
}

extern "C" int mh_gemv_pack_fp4(const void* W, int ldb, int N, int K, void* q_out, void* scale_out, hipStream_t stream) {
  if (!gv_fp4_dims(N, K) || (ldb % 8) != 0 || ldb < K || !scale_out || ((uintptr_t)W & 15) || ((uintptr_t)q_out & 15) ||
      ((uintptr_t)scale_out & 3))
    return MH_ERR_ARG;
  const GvLayout L = gv_layout(N, K, 128);
  hipLaunchKernelGGL(gemv_pack_fp4_kernel, dim3(L.blocks), dim3(256), 0, stream, (const bf16_t*)W, ldb, N, K, (unsigned char*)q_out,
                     (unsigned char*)scale_out, L.nw, L.per);
  MH_CHECK_LAUNCH();
  return MH_OK;
}

// ---- 17 .. 64 rows on the same packed copies (the decode slots above 16 rows) ------------------------------------------------
// mh_gemv_packed_wide / _fp8_wide / _fp4_wide: C[M <= 64, N] on the copy their 16-row counterparts read, no new layout.
//
// Bit contract: row m of a wide launch carries the bits the 16-row kernel gives that row (any M, output type, bias, residual,
// alpha).  A row of v_mfma_f32_16x16x32_bf16 depends on its own A row only, so it is enough to keep, per output element, the
// K split over the gv_packed_nw(N) waves (per = ceil(nsteps / NW)), the step order inside a wave and the MFMA order inside a
// step (two; four for fp4), the cross-wave sum w = 0 .. NW-1 starting from 0.f, and the epilogue (fp8 row scale, alpha, bias,
// residual -- gv_finish, the 16-row kernels' own epilogue).  Which workgroup owns which columns is free, and is the design:
//
// A workgroup of the 16-row kernel reads all M x K activations from L2 for 16 columns.  Per workgroup that is M / 16 times its
// bf16 weight bytes (x2 for fp8, x4 for fp4), so at 64 rows the L2 side carries 4 / 8 / 16 times the HBM stream, against an L2
// rate of ~70 GB/s per CU (17-19 TB/s chip-wide) beside ~25 GB/s per CU of HBM: L2-bound from ~32 rows on bf16, earlier on the
// narrow copies.  The region of (column block b, wave w) is `per` contiguous KiB-steps at ((b * NW + w) * per) * 1024 elements,
// so a workgroup takes G ADJACENT column blocks: wave w walks its K range once, loads each activation fragment once per
// row tile and feeds it to the weight fragments of all G blocks.  Activation bytes per weight byte fall to M / (16 G).
//   VGPRs:  ceil(M/16) x G accumulator quads (64 registers at 64 rows, G = 4) + G x U x 8 weight registers of a batch of U steps
//           (x 4 for fp8) + ceil(M/16) x U x 8 activation registers.  The variants the rule launches, as compiled at 64 rows
//           (VGPRs, waves per SIMD under __launch_bounds__(.., 2)):  G = 1, U = 2: 76-82, 6;  G = 2, U = 2: 112-126, 4;
//           G = 4, U = 4, fp8: 220, 2;  G = 4, fp4 (4-step batches of codes, one scale dword each, the 128-deep activation
//           fragments loaded step by step): 211, 2;  G = 4, U = 4, bf16 (the lm-head alone): 256 with 9 registers (24 B per
//           lane) spilled to scratch, 2 -- the batch holds 128 weight + 128 activation registers beside 64 accumulators.  It
//           is kept because it measures faster than the spill-free U = 2 build (138-164 registers, 3 waves: 86.9 us on the
//           lm-head at 64 rows against 64.7); loading the bf16 activations step by step, as fp4 does, would remove the spill.
//   Workgroups: ceil(N / 16 / G).  N = 4096 has 256 column blocks, 12288 has 768, 22016 has 1376, 32000 has 2000: any G > 1
//           leaves CUs without a workgroup at N = 4096, which already under-fills the chip (hence its 8 waves).
//   LDS:    the cross-wave reduction goes one row tile at a time through red[NW][G][256] (32 KiB at NW = 8, G = 4); wave g
//           finishes column block g.
// Measured (MI355X, one product per launch, the weights rotated through 4-12 copies so that none is found in a cache, us per
// launch, best U of 2 / 4 steps per batch; the 16-row kernel at 16 rows for scale; G and U were build-time sweep settings,
// only the variants of the rule below are compiled in):
//                          16 rows |  32 rows: G=1    G=2    G=4 |  64 rows: G=1    G=2    G=4
//   bf16 qkv   12288x4096    23.7  |          32.5   28.3   36.1 |          52.0   39.5   43.3
//   bf16 wo     4096x4096    10.9  |          13.1   15.4   23.8 |          21.5   24.9   30.4
//   bf16 g|u   22016x4096    41.8  |          62.4   43.0   47.2 |         101.0   58.5   57.7
//   bf16 down  4096x11008    22.9  |          31.4   36.6   55.7 |          49.4   59.9   71.2
//   bf16 head  32000x4096    55.4  |          80.3   59.0   56.8 |         136.8   77.5   64.7
//   fp8  qkv                 18.5  |          27.7   21.2   21.8 |          52.1   37.3   30.5
//   fp8  wo                   7.9  |          11.9   12.9   18.7 |          20.6   22.4   26.5
//   fp8  g|u                 34.2  |          51.3   32.6   29.9 |          98.4   53.9   45.3
//   fp8  down                17.9  |          24.8   29.6   41.9 |          47.0   52.7   58.6
//   fp4  qkv                 16.2  |          31.3   24.6   16.0 |          49.1   44.3   29.0
//   fp4  wo                   7.5  |          13.3   14.4   16.4 |          19.9   25.2   28.0
//   fp4  g|u                 27.6  |          65.0   36.8   29.2 |         107.3   65.2   49.7
//   fp4  down                15.4  |          31.8   32.5   38.1 |          48.9   59.1   65.4
// So the L2 argument holds where there are column blocks to spare -- the plain "more accumulators" form (G = 1) is 1.3 to 2.2
// times slower than the grouped one on qkv, gate|up and the lm-head at 64 rows -- and loses to the workgroup count at N = 4096,
// where grouping halves the CUs at work and G = 1 wins by 14-35 %.  The rule (gv_wide_group): the largest G of 4, 2, 1 that
// still leaves 384 workgroups on the bf16 copy and 192 on the one-byte copies (their weight bytes per column block are a half
// and a quarter, so the shared activation read is worth more workgroups there), G = 1 when not even G = 2 does:
//   bf16: wo / down 1, qkv / gate|up 2, lm-head 4;   fp8, fp4: wo / down 1, qkv / gate|up 4.
// U = 4 steps per batch with G = 4 (16 KiB of bf16 weights in flight per wave, the 16-row kernel's figure; 64.7 against 86.9 us
// on the lm-head at 64 rows), 2 otherwise (no gain measured, more registers).  What is left on the table is N = 4096: down at 64 rows costs 2.2 times
// its 16-row launch, all of it the 1.4 MB of activations every one of its 256 workgroups reads.
// Rows past M in the last row tile duplicate row M - 1 and column blocks past the last one duplicate the last block; neither
// is stored.
template <int MT, int G, int UNROLL, int GV_NW, typename WT>
__global__ __launch_bounds__(GV_NW * 64, 2) void gemv_wide_kernel(const bf16_t* __restrict__ A, const WT* __restrict__ B,
                                                                  void* __restrict__ Cv, const float* __restrict__ bias,
                                                                  const float* res, int M, int N, int K, int lda, int ldc, int ldr,
                                                                  int out_f32, float alpha, const float* __restrict__ wscale) {
  constexpr bool F4 = gv_is_fp4<WT>, F8 = sizeof(WT) == 1 && !F4;
  constexpr int KS = F4 ? 128 : 64;
  static_assert(G <= GV_NW && (!F4 || UNROLL == 4), "wave g finishes block g; an fp4 batch is one scale dword");
  __shared__ float red[GV_NW][G][16 * 16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int nblocks = (N + 15) / 16, b0 = blockIdx.x * G;
  const int glive = nblocks - b0 < G ? nblocks - b0 : G;
  const int nsteps = K / KS;
  const int per = (nsteps + GV_NW - 1) / GV_NW;
  const bf16_t* xp[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int m = t * 16 + lr;
    xp[t] = A + (size_t)(m < M ? m : M - 1) * lda + lg * (KS / 4);
  }
  const WT* wp[G];
  const unsigned* sp[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const int b = g < glive ? b0 + g : nblocks - 1;
    wp[g] = B + ((size_t)b * GV_NW + wave) * per * 1024 + lane * (16 / sizeof(WT));
    sp[g] = F4 ? reinterpret_cast<const unsigned*>(wscale) + ((size_t)b * GV_NW + wave) * ((per + 3) / 4) * 64 + lane : nullptr;
  }
  float4_t acc[MT][G];
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int g = 0; g < G; ++g) acc[t][g] = (float4_t){0.f, 0.f, 0.f, 0.f};
  int s = wave * per;
  const int s0 = s;
  const int s_end = (s + per) < nsteps ? (s + per) : nsteps;
  // one batch of n <= UNROLL steps from step s (full: n = UNROLL, no guards): every load of the batch in flight, then the
  // products step by step
  auto batch = [&](auto full_c, int n) {
    constexpr bool FULL = decltype(full_c)::value;
    if constexpr (F4) {
      short8_t w[G][UNROLL];
      unsigned sc[G];
#pragma unroll
      for (int g = 0; g < G; ++g) {
#pragma unroll
        for (int u = 0; u < UNROLL; ++u)
          if (FULL || u < n) w[g][u] = __builtin_nontemporal_load(reinterpret_cast<const short8_t*>(wp[g] + (size_t)(s - s0 + u) * 1024));
        sc[g] = __builtin_nontemporal_load(sp[g] + (size_t)((s - s0) / 4) * 64);
      }
#pragma unroll
      for (int u = 0; u < UNROLL; ++u)
        if (FULL || u < n) {
          short8_t x[MT][4];
#pragma unroll
          for (int t = 0; t < MT; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) x[t][i] = *reinterpret_cast<const short8_t*>(xp[t] + (size_t)(s + u) * 128 + 8 * i);
#pragma unroll
          for (int g = 0; g < G; ++g) {
            const gv_u4_t q = __builtin_bit_cast(gv_u4_t, w[g][u]);
            const float scl = __uint_as_float(((sc[g] >> (8 * u)) & 0xffu) << 23);     // 2^(b-127), gv_mfma_fp4
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const short8_t r = gv_fp4_widen(q[i], scl);             // widened once, used by every row tile
#pragma unroll
              for (int t = 0; t < MT; ++t) acc[t][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x[t][i], r, acc[t][g], 0, 0, 0);
            }
          }
        }
    } else {
      short8_t w0[UNROLL][G], w1[UNROLL][G], x0[UNROLL][MT], x1[UNROLL][MT];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u)
        if (FULL || u < n) {
#pragma unroll
          for (int g = 0; g < G; ++g) gv_load(wp[g], (size_t)(s - s0 + u), w0[u][g], w1[u][g]);
#pragma unroll
          for (int t = 0; t < MT; ++t) {
            x0[u][t] = *reinterpret_cast<const short8_t*>(xp[t] + (size_t)(s + u) * 64);
            x1[u][t] = *reinterpret_cast<const short8_t*>(xp[t] + (size_t)(s + u) * 64 + 8);
          }
        }
#pragma unroll
      for (int u = 0; u < UNROLL; ++u)
        if (FULL || u < n) {
#pragma unroll
          for (int g = 0; g < G; ++g) {
            short8_t a = w0[u][g], b = w1[u][g];
            if constexpr (F8) {                                        // widened once, used by every row tile
              const gv_u4_t q = __builtin_bit_cast(gv_u4_t, a);
              a = fp8x8_to_bf16(q[0], q[1]);
              b = fp8x8_to_bf16(q[2], q[3]);
            }
            // each accumulator takes x0 . w0 before x1 . w1; the row tiles in between keep dependent MFMAs apart
#pragma unroll
            for (int t = 0; t < MT; ++t) acc[t][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x0[u][t], a, acc[t][g], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < MT; ++t) acc[t][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x1[u][t], b, acc[t][g], 0, 0, 0);
          }
        }
    }
  };
  for (; s + UNROLL <= s_end; s += UNROLL) batch(std::true_type{}, UNROLL);
  if (s < s_end) batch(std::false_type{}, s_end - s);
  // D layout: row m = 4*lg + r, col n = lr.  One row tile at a time through LDS; wave g finishes column block g.
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    if (t) __syncthreads();
#pragma unroll
    for (int g = 0; g < G; ++g) gv_red_put(red, wave, g, lr, lg, acc[t][g]);
    __syncthreads();
    if (wave < glive) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ml = 4 * lg + r, m = t * 16 + ml, n = (b0 + wave) * 16 + lr;
        if (m < M && n < N) gv_red_finish<GV_NW, G, F8>(red, wave, ml, lr, m, n, Cv, bias, res, ldc, ldr, out_f32, alpha, wscale);
      }
    }
  }
}

// One launch of the variant (row tiles, column group, waves).  Steps per batch: an fp4 batch is the four steps of one scale
// dword; bf16 / fp8 take 4 with groups of 4 and 2 otherwise (the header comment above).
template <int MT, int G, int NW, typename WT>
static void launch_gemv_wide_v(const dim3 grid, const GvArgs& a) {
  constexpr int U = gv_is_fp4<WT> || G == 4 ? 4 : 2;
  hipLaunchKernelGGL((gemv_wide_kernel<MT, G, U, NW, WT>), grid, dim3(NW * 64), 0, a.stream, (const bf16_t*)a.A, (const WT*)a.P, a.C,
                     a.bias, a.residual, a.M, a.N, a.K, (int)a.lda, a.ldc, a.ldr, a.out_f32, a.alpha, (const float*)a.wscale);
}

// column blocks per workgroup: the largest group that leaves min_wg workgroups (the header comment above)
static int gv_wide_group(int N, bool one_byte) {
  const int nblocks = (N + 15) / 16, min_wg = one_byte ? 192 : 384;
  return nblocks / 4 >= min_wg ? 4 : nblocks / 2 >= min_wg ? 2 : 1;
}

// The (G, NW) pairs the rule reaches -- only these are instantiated.  NW = 8 means fewer than 512 column blocks: G = 1, or 2 on
// the one-byte copies from 384 blocks.  NW = 4: bf16 G = 1 (512..767 blocks), 2, 4; one-byte G = 2 (512..767), 4.
template <int MT, typename WT>
static void launch_gemv_wide_mt(int G, bool nw8, const dim3 grid, const GvArgs& a) {
  constexpr bool ONE = sizeof(WT) == 1;
  if (nw8) {
    if constexpr (ONE) {
      if (G == 2) { launch_gemv_wide_v<MT, 2, 8, WT>(grid, a); return; }
    }
    launch_gemv_wide_v<MT, 1, 8, WT>(grid, a);
  } else if (G == 4) {
    launch_gemv_wide_v<MT, 4, 4, WT>(grid, a);
  } else if (ONE || G == 2) {
    launch_gemv_wide_v<MT, 2, 4, WT>(grid, a);
  } else {
    if constexpr (!ONE) launch_gemv_wide_v<MT, 1, 4, WT>(grid, a);
  }
}

template <typename WT>
static int launch_gemv_wide(const GvArgs& a) {
  if (a.M > 64) return MH_ERR_ARG;
  if (a.M <= 16) return launch_gemv_packed<WT>(a);
  if (a.K <= 0 || (a.K % gv_kstep<WT>) != 0 || (a.lda % 8) != 0 || ((uintptr_t)a.A & 15) || ((uintptr_t)a.P & 15)) return MH_ERR_ARG;
  const GvLayout L = gv_layout(a.N, a.K, gv_kstep<WT>);
  const int G = gv_wide_group(a.N, sizeof(WT) == 1), MT = (a.M + 15) / 16;
  const dim3 grid((L.blocks + G - 1) / G);
  if (MT == 2) launch_gemv_wide_mt<2, WT>(G, L.nw == 8, grid, a);
  else if (MT == 3) launch_gemv_wide_mt<3, WT>(G, L.nw == 8, grid, a);
  else launch_gemv_wide_mt<4, WT>(G, L.nw == 8, grid, a);
  MH_CHECK_LAUNCH();
  return MH_OK;
}

// ---- the twelve product entries: {plain, RMSNorm, SiLU, wide} x {bf16, fp8, fp4} ----------------------------------------------
// An empty product is MH_OK; a missing or misaligned scale pointer of a one-byte copy is MH_ERR_ARG, like every malformed
// argument, before any launch; MH_ERR_UNSUPPORTED is the fused forms' "run the two launches instead".
template <int FORM, typename WT>
static int gv_entry(const GvArgs& a) {
  if (a.M <= 0 || a.N <= 0) return MH_OK;
  if (sizeof(WT) == 1 && (!a.wscale || ((uintptr_t)a.wscale & 3))) return MH_ERR_ARG;
  if constexpr (FORM == GV_PLAIN) return launch_gemv_packed<WT>(a);
  else if constexpr (FORM == GV_WIDE) return launch_gemv_wide<WT>(a);
  else return launch_gemv_pro<FORM, WT>(a);
}

// C[M <= 16, N] = alpha * A . W^T (+bias) (+residual) with W given as its mh_gemv_pack copy
extern "C" int mh_gemv_packed(const void* A, int lda, const void* P, void* C, int ldc, int M, int N, int K, const float* bias,
                              const float* residual, int ldr, int out_f32, float alpha, hipStream_t stream) {
  return gv_entry<GV_PLAIN, bf16_t>({A, lda, P, nullptr, C, ldc, M, N, K, bias, residual, ldr, out_f32, alpha, stream});
}

// C[M <= 16, N] = alpha * rmsnorm(H; norm_w, eps) . W^T (+bias) (+residual), W as its mh_gemv_pack copy; H [M, K] f32.
// MH_ERR_UNSUPPORTED when M * K * 2 bytes of operand do not fit the kernel's LDS budget (64 KiB), above GV_PRO_MAX_ROWS rows and
// for K > 4096.
extern "C" int mh_gemv_packed_rmsnorm(const float* H, long ldh, const float* norm_w, float eps, const void* P, void* C, int ldc,
                                      int M, int N, int K, const float* bias, const float* residual, int ldr, int out_f32,
                                      float alpha, hipStream_t stream) {
  return gv_entry<GV_RMSNORM, bf16_t>({H, ldh, P, nullptr, C, ldc, M, N, K, bias, residual, ldr, out_f32, alpha, stream, norm_w, eps});
}

// C[M <= 16, N] = alpha * (silu(g) * u) . W^T (+bias) (+residual): gu [M, >= 2K] bf16, gate / up interleaved in blocks of 128.
extern "C" int mh_gemv_packed_silu(const void* gu, long ldgu, const void* P, void* C, int ldc, int M, int N, int K,
                                   const float* bias, const float* residual, int ldr, int out_f32, float alpha,
                                   hipStream_t stream) {
  return gv_entry<GV_SILU, bf16_t>({gu, ldgu, P, nullptr, C, ldc, M, N, K, bias, residual, ldr, out_f32, alpha, stream});
}

// C[M <= 64, N] on the same copy: up to 16 rows the 16-row kernel, above it gemv_wide_kernel; row m carries the 16-row bits
extern "C" int mh_gemv_packed_wide(const void* A, int lda, const void* P, void* C, int ldc, int M, int N, int K,
                                   const float* bias, const float* residual, int ldr, int out_f32, float alpha,
                                   hipStream_t stream) {
  return gv_entry<GV_WIDE, bf16_t>({A, lda, P, nullptr, C, ldc, M, N, K, bias, residual, ldr, out_f32, alpha, stream});
}

// the fp8 copy (q, s) of mh_gemv_pack_fp8: C = alpha * s_n * op(A) . q^T (+bias) (+residual); the same four forms, the same contract
extern "C" int mh_gemv_packed_fp8(const void* A, int lda, const void* Q, const float* scale, void* C, int ldc, int M, int N,
                                  int K, const float* bias, const float* residual, int ldr, int out_f32, float alpha,
                                  hipStream_t stream) {
  return gv_entry<GV_PLAIN, fp8_t>({A, lda, Q, scale, C, ldc, M, N, K, bias, residual, ldr, out_f32, alpha, stream});
}
extern "C" int mh_gemv_packed_fp8_rmsnorm(const float* H, long ldh, const float* norm_w, float eps, const void* Q,
                                          const float* scale, void* C, int ldc, int M, int N, int K, const float* bias,
                                          const float* residual, int ldr, int out_f32, float alpha, hipStream_t stream) {
  return gv_entry<GV_RMSNORM, fp8_t>({H, ldh, Q, scale, C, ldc, M, N, K, bias, residual, ldr, out_f32, alpha, stream, norm_w, eps});
}
extern "C" int mh_gemv_packed_fp8_silu(const void* gu, long ldgu, const void* Q, const float* scale, void* C, int ldc, int M,
                                       int N, int K, const float* bias, const float* residual, int ldr, int out_f32, float alpha,
                                       hipStream_t stream) {
  return gv_entry<GV_SILU, fp8_t>({gu, ldgu, Q, scale, C, ldc, M, N, K, bias, residual, ldr, out_f32, alpha, stream});
}
extern "C" int mh_gemv_packed_fp8_wide(const void* A, int lda, const void* Q, const float* scale, void* C, int ldc, int M, int N,
                                       int K, const float* bias, const float* residual, int ldr, int out_f32, float alpha,
                                       hipStream_t stream) {
  return gv_entry<GV_WIDE, fp8_t>({A, lda, Q, scale, C, ldc, M, N, K, bias, residual, ldr, out_f32, alpha, stream});
}

// the fp4 copy (codes, scale bytes) of mh_gemv_pack_fp4: C = alpha * op(A) . dq(W)^T (+bias) (+residual); the kernels take the scale
// stream through their wscale argument
extern "C" int mh_gemv_packed_fp4(const void* A, int lda, const void* Q, const void* scale, void* C, int ldc, int M, int N, int K,
                                  const float* bias, const float* residual, int ldr, int out_f32, float alpha, hipStream_t stream) {
  return gv_entry<GV_PLAIN, fp4_t>({A, lda, Q, scale, C, ldc, M, N, K, bias, residual, ldr, out_f32, alpha, stream});
}
extern "C" int mh_gemv_packed_fp4_rmsnorm(const float* H, long ldh, const float* norm_w, float eps, const void* Q,
                                          const void* scale, void* C, int ldc, int M, int N, int K, const float* bias,
                                          const float* residual, int ldr, int out_f32, float alpha, hipStream_t stream) {
  return gv_entry<GV_RMSNORM, fp4_t>({H, ldh, Q, scale, C, ldc, M, N, K, bias, residual, ldr, out_f32, alpha, stream, norm_w, eps});
}
extern "C" int mh_gemv_packed_fp4_silu(const void* gu, long ldgu, const void* Q, const void* scale, void* C, int ldc, int M,
                                       int N, int K, const float* bias, const float* residual, int ldr, int out_f32, float alpha,
                                       hipStream_t stream) {
  return gv_entry<GV_SILU, fp4_t>({gu, ldgu, Q, scale, C, ldc, M, N, K, bias, residual, ldr, out_f32, alpha, stream});
}
extern "C" int mh_gemv_packed_fp4_wide(const void* A, int lda, const void* Q, const void* scale, void* C, int ldc, int M, int N,
                                       int K, const float* bias, const float* residual, int ldr, int out_f32, float alpha,
                                       hipStream_t stream) {
  return gv_entry<GV_WIDE, fp4_t>({A, lda, Q, scale, C, ldc, M, N, K, bias, residual, ldr, out_f32, alpha, stream});
}
