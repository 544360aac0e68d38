// q / v LoRA merged into the decode step's copy of the frozen qkv weight (llama.py decode_merge_lora; PEFT merge_adapter).
//
// W [3D, D] bf16 holds the rows [q | k | v] (the frozen columns of the bordered wqkv_ext, leading dimension ldw); the fp32 masters
// are A_q | A_v [2r, D] (adjacent: LoraQV._aqv) and B_q, B_v [D, r]; s = alpha / r.  The merged matrix M is
//   q rows n < D:         M[n, k] = bf16(W[n, k] + s * acc),  acc = sum over j = 0 .. r-1, in that order, of B_q[n, j] * A_q[j, k]
//   k rows D <= n < 2D:   M[n, k] = W[n, k]
//   v rows n >= 2D:       the q rule with B_v[n - 2D] and A_v
// acc starts at 0; every product, every sum, s * acc and the final add are separate fp32 operations rounded to nearest even (no
// contraction into FMAs: tests/lora_merge_ref.py restates the rule in torch fp32 and gets the same bits), then one
// round-to-nearest-even to bf16.  A is read from the fp32 masters, not from the bf16 border of wqkv_ext.
//
// Three outputs, each written in one pass from W (no intermediate row-major copy): the row-major matrix (export, tests), the
// mh_gemv_pack stream order and the mh_gemv_pack_fp8 codes + row scales -- bit for bit what gemv_pack / gemv_pack_fp8 write for the
// row-major M.  One workgroup per 16-row block (a block lies in one of q / k / v: D % 64 == 0), thread (sub, lane) of a round
// computes E consecutive k of row 16 * block + lane % 16, exactly the 16 B (bf16: E = 8) or 16 codes (fp8: E = 16) that lane reads
// at one step of the packed copy, so the stores are the packed copy's contiguous KiBs.  A round's KC columns of the r rows of A
// it needs are staged in LDS (fp32, 4 to 16 KiB); the block's 16 rows of B sit in registers.  The fp8 copy makes two passes
// over the block, as gemv_pack_fp8_kernel: the amax of the merged bf16 rows, then the codes, recomputing the rank-r sums (a few
// FMAs' worth of VALU, no extra HBM traffic beyond the second read of the block's W rows).
#include "common.h"
#include "gemv_pack.h"

typedef __attribute__((ext_vector_type(4))) unsigned lm_u4_t;

template <int R, int E, int KC>
struct LmStage {
  __device__ static void load(float (*As)[KC], const float* __restrict__ A, int D, int k0, int tid) {
    // A [R, D] fp32 columns k0 .. k0 + KC - 1 -> As; columns past D read as 0 (the packed copies' zero steps)
    constexpr int V4 = R * KC / 4;
    for (int i = tid; i < V4; i += 256) {
      const int j = i / (KC / 4), c = (i % (KC / 4)) * 4;
      float4_t v = {0.f, 0.f, 0.f, 0.f};
      if (k0 + c < D) v = *reinterpret_cast<const float4_t*>(A + (size_t)j * D + k0 + c);
      *reinterpret_cast<float4_t*>(&As[j][c]) = v;
    }
  }
};

// E merged values (as fp32: each exactly a bf16 value) of one row at k .. k + E - 1; lora == false: W's own values.
// The library is built with -ffp-contract=fast, under which the backend fuses a multiply feeding an add into an FMA whatever the
// source says; an empty asm statement on each product (a pair of k, so the packed fp32 instructions stay) keeps every product
// rounded on its own, as the rule states.
typedef __attribute__((ext_vector_type(2))) float lm_f2_t;
__device__ __forceinline__ lm_f2_t lm_rounded(lm_f2_t x) {
  asm("" : "+v"(x));
  return x;
}

template <int R, int E, int KC>
__device__ __forceinline__ void lm_values(const bf16_t* __restrict__ wrow, int k, int kk, bool lora, const float (&b)[R],
                                          float s, const float (*As)[KC], float (&v)[E]) {
  short8_t w8[E / 8];
#pragma unroll
  for (int u = 0; u < E / 8; ++u) w8[u] = __builtin_nontemporal_load(reinterpret_cast<const short8_t*>(wrow + k + 8 * u));
#pragma unroll
  for (int e = 0; e < E; ++e) v[e] = bf2f((bf16_t)w8[e / 8][e % 8]);
  if (!lora) return;
#pragma unroll
  for (int e = 0; e < E; e += 2) {
    lm_f2_t acc = {0.f, 0.f};
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const lm_f2_t a2 = *reinterpret_cast<const lm_f2_t*>(&As[j][kk + e]);
      acc = acc + lm_rounded(b[j] * a2);
    }
    const lm_f2_t m = (lm_f2_t){v[e], v[e + 1]} + lm_rounded(s * acc);
    v[e] = bf2f(f2bf(m[0]));
    v[e + 1] = bf2f(f2bf(m[1]));
  }
}

// OUT 0: row-major bf16 out[3D, ldo]; 1: the mh_gemv_pack copy; 2: the mh_gemv_pack_fp8 codes (out) and row scales.
// Launch: grid (3D / 16, splits), 256 threads; rounds of KC columns are dealt to blockIdx.y (OUT 0 / 1) -- the fp8 copy needs
// whole rows for its amax and takes splits = 1.
template <int R, int OUT>
__global__ __launch_bounds__(256) void lora_merge_kernel(const bf16_t* __restrict__ W, int ldw, const float* __restrict__ Aqv,
                                                         const float* __restrict__ Bq, const float* __restrict__ Bv, int D,
                                                         float s, void* __restrict__ out, int ldo, float* __restrict__ scale_out,
                                                         int steps) {
  constexpr int E = OUT == 2 ? 16 : 8;           // k per thread and round: one lane's 16 B of a packed step
  constexpr int KC = 16 * E;                     // k per round: 4 sub-groups of 64 lanes x 4 lane groups (lg) x E
  __shared__ __attribute__((aligned(16))) float As[R][KC];
  __shared__ float red[256];
  __shared__ float srow[16];
  const int tid = threadIdx.x, nb = blockIdx.x;
  const int lane = tid & 63, sub = tid >> 6, lr = lane & 15, lg = lane >> 4;
  const int row0 = nb * 16, row = row0 + lr;
  const int part = row0 / D;                     // 0 q, 1 k, 2 v: block-uniform
  const bool lora = part != 1;
  const float* A = Aqv + (part == 2 ? (size_t)R * D : 0);
  float b[R];
  {
    const float* Bm = part == 2 ? Bv + (size_t)(row - 2 * D) * R : Bq + (size_t)row * R;
#pragma unroll
    for (int j = 0; j < R; ++j) b[j] = lora ? Bm[j] : 0.f;
  }
  // chunk-local column of this thread: bf16 sub = (step, half) of two 64-deep steps, fp8 sub = one of four steps
  const int kk = OUT == 2 ? sub * 64 + lg * 16 : (sub >> 1) * 64 + lg * 16 + (sub & 1) * 8;
  const bf16_t* wrow = W + (size_t)row * ldw;
  const int kend = OUT == 0 ? D : steps * 64;    // the packed copies run on through their zero steps

  if constexpr (OUT == 2) {
    float amax = 0.f;
    for (int k0 = 0; k0 < D; k0 += KC) {
      if (lora) {
        __syncthreads();
        LmStage<R, E, KC>::load(As, A, D, k0, tid);
        __syncthreads();
      }
      if (k0 + kk < D) {
        float v[E];
        lm_values<R, E, KC>(wrow, k0 + kk, kk, lora, b, s, As, v);
#pragma unroll
        for (int e = 0; e < E; ++e) amax = fmaxf(amax, fabsf(v[e]));
      }
    }
    red[tid] = amax;
    __syncthreads();
    if (tid < 16) {                                // the 16 threads of row tid: sub 0..3 x lg 0..3
      float m = 0.f;
      for (int i = 0; i < 16; ++i) m = fmaxf(m, red[(i >> 2) * 64 + (i & 3) * 16 + tid]);
      const float sc = m > 0.f ? m / 448.0f : 1.0f;
      srow[tid] = sc;
      scale_out[row0 + tid] = sc;
    }
    __syncthreads();
    const float sc = srow[lr];
    for (int k0 = 0; k0 < kend; k0 += KC) {
      if (lora) {
        __syncthreads();
        LmStage<R, E, KC>::load(As, A, D, k0, tid);
        __syncthreads();
      }
      const int k = k0 + kk, step = k >> 6;
      lm_u4_t o = {0u, 0u, 0u, 0u};
      if (k < D) {
        float v[E];
        lm_values<R, E, KC>(wrow, k, kk, lora, b, s, As, v);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const float x = fminf(fmaxf(v[e] / sc, -448.f), 448.f);
          o[e >> 2] |= f32_to_e4m3fn(x) << (8 * (e & 3));
        }
      }
      *reinterpret_cast<lm_u4_t*>((unsigned char*)out + (((size_t)nb * steps + step) * 64 + lane) * 16) = o;
    }
  } else {
    for (int k0 = blockIdx.y * KC; k0 < kend; k0 += gridDim.y * KC) {
      if (lora) {
        __syncthreads();
        LmStage<R, E, KC>::load(As, A, D, k0, tid);
        __syncthreads();
      }
      const int k = k0 + kk;
      if (OUT == 0 && k >= D) continue;
      short8_t o = {0, 0, 0, 0, 0, 0, 0, 0};
      if (k < D) {
        float v[E];
        lm_values<R, E, KC>(wrow, k, kk, lora, b, s, As, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (short)(__builtin_bit_cast(unsigned, v[e]) >> 16);   // v[e] is a bf16 value
      }
      if constexpr (OUT == 0) {
        *reinterpret_cast<short8_t*>((bf16_t*)out + (size_t)row * ldo + k) = o;
      } else {                                     // element ((block * steps + step) * 2 + half) * 512 + lane * 8
        const int step = k >> 6, half = (k >> 3) & 1;
        *reinterpret_cast<short8_t*>((bf16_t*)out + ((((size_t)nb * steps + step) * 2 + half) * 64 + lane) * 8) = o;
      }
    }
  }
}

static int lm_check(const void* W, int ldw, const float* Aqv, const float* Bq, const float* Bv, int D, int r, const void* out) {
  if (!W || !Aqv || !Bq || !Bv || !out) return MH_ERR_ARG;
  if (D <= 0 || (D % 64) != 0 || D > (1 << 20) || (r != 8 && r != 16) || ldw < D || (ldw % 8) != 0) return MH_ERR_ARG;
  if (((uintptr_t)W & 15) || ((uintptr_t)Aqv & 15) || ((uintptr_t)out & 15) || ((uintptr_t)Bq & 3) || ((uintptr_t)Bv & 3))
    return MH_ERR_ARG;
  return MH_OK;
}

template <int OUT>
static int lm_launch(const void* W, int ldw, const float* Aqv, const float* Bq, const float* Bv, int D, int r, float s, void* out,
                     int ldo, float* scale_out, hipStream_t stream) {
  const GvLayout L = gv_layout(3 * D, D, 64);
  const int N = 3 * D, steps = L.nw * L.per;
  const int KC = OUT == 2 ? 256 : 128;
  const int rounds = ((OUT == 0 ? D : steps * 64) + KC - 1) / KC;      // >= 1; a row-major round may be partial
  // up to 4 workgroups per row block when the blocks alone leave the CUs short of work (bf16 outputs only)
  int splits = OUT == 2 ? 1 : (N / 16 >= 2048 ? 1 : 4);
  splits = splits < rounds ? splits : rounds;
  const dim3 grid(N / 16, splits);
  if (r == 8)
    hipLaunchKernelGGL((lora_merge_kernel<8, OUT>), grid, dim3(256), 0, stream, (const bf16_t*)W, ldw, Aqv, Bq, Bv, D, s, out, ldo,
                       scale_out, steps);
  else
    hipLaunchKernelGGL((lora_merge_kernel<16, OUT>), grid, dim3(256), 0, stream, (const bf16_t*)W, ldw, Aqv, Bq, Bv, D, s, out, ldo,
                       scale_out, steps);
  MH_CHECK_LAUNCH();
  return MH_OK;
}

extern "C" int mh_lora_merge(const void* W, int ldw, const float* Aqv, const float* Bq, const float* Bv, int D, int r, float s,
                             void* out, int ldo, hipStream_t stream) {
  const int rc = lm_check(W, ldw, Aqv, Bq, Bv, D, r, out);
  if (rc != MH_OK) return rc;
  if (ldo < D || (ldo % 8) != 0) return MH_ERR_ARG;
  return lm_launch<0>(W, ldw, Aqv, Bq, Bv, D, r, s, out, ldo, nullptr, stream);
}

extern "C" int mh_lora_merge_pack(const void* W, int ldw, const float* Aqv, const float* Bq, const float* Bv, int D, int r, float s,
                                  void* out, hipStream_t stream) {
  const int rc = lm_check(W, ldw, Aqv, Bq, Bv, D, r, out);
  if (rc != MH_OK) return rc;
  return lm_launch<1>(W, ldw, Aqv, Bq, Bv, D, r, s, out, 0, nullptr, stream);
}

extern "C" int mh_lora_merge_pack_fp8(const void* W, int ldw, const float* Aqv, const float* Bq, const float* Bv, int D, int r,
                                      float s, void* q_out, float* scale_out, hipStream_t stream) {
  const int rc = lm_check(W, ldw, Aqv, Bq, Bv, D, r, q_out);
  if (rc != MH_OK) return rc;
  if (!scale_out || ((uintptr_t)scale_out & 3)) return MH_ERR_ARG;
  return lm_launch<2>(W, ldw, Aqv, Bq, Bv, D, r, s, q_out, 0, scale_out, stream);
}
