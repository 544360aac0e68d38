// K-row token-step attention for ONE sequence per group (draft-and-verify greedy decoding, mh_attn_decode_rope_draft): row
// g*K + j of qkv is the token at position pos[g] + j of sequence g.  Grid = G*K*H workgroups; workgroup (g, j, h) is
// attn_decode_kernel (attention.hip) for that row alone at position pos[g] + j; both call the arithmetic in attn_one_query.h, so
// the out row, the rotated q and the cache row carry the bits of K sequential mh_attn_decode_rope steps
// (tests/test_draft_kernels_gpu.py holds the two to the same bits).
//
// The K rows depend on each other: row j sees the keys of rows 0 .. j-1 of the same launch, whose cache rows sibling workgroups
// are writing.  No workgroup reads a cache row >= pos[g].  Instead workgroup j rotates the k of rows 0 .. j itself, from qkv
// (whose k and v columns nobody writes), into LDS -- the same fp32 rotate-half and the same one rounding to bf16 as the cache row
// gets -- and reads those rows' v straight from qkv.  Only workgroup j writes cache row pos[g] + j and only it rotates q of row j
// in place.  No grid-wide synchronisation.
#include "attn_one_query.h"

#define DRAFT_MAX_K 8
#define DRAFT_LDS_LIMIT (160 * 1024)             // gfx950: LDS per CU

struct DraftParams {
  bf16_t* qkv;          // [G*K, ld_qkv] = [q | k | v]
  bf16_t* cache;        // [G][T_cap][2W] rows [k | v]
  bf16_t* out;          // [G*K, ldo]
  const int* pos;       // [G] position of row 0 of the group
  const int* live;      // [G] 0 = the sequence is idle
  const int* nrow;      // [G] rows of the group that hold a token, 1 .. K; null (mh_attn_decode_rope_draft): all K
  const float* cs;
  const float* sn;
  long ld_qkv, cache_bs, ld_cache, ldo;
  int K, H, D, T_cap;
  float scale;
};

__global__ __launch_bounds__(OQ_WAVES * 64) void attn_decode_draft_kernel(DraftParams p) {
  extern __shared__ float dsm[];                 // [T_cap] scores, [OQ_WAVES][128] partial outputs, then [K][D] bf16 rotated k
  const int h = blockIdx.x % p.H, row = blockIdx.x / p.H, g = row / p.K, jr0 = row - g * p.K;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int D = p.D, W = p.H * D;
  const int p0 = p.pos[g];
  // uniform over the workgroup, ahead of the first barrier: an idle sequence, a row past the group's count (the decode slots'
  // form: a slot with fewer than K - 1 guesses), or a row whose position would leave the cache
  if (!p.live[g] || p0 < 0 || p0 > p.T_cap - 1 - jr0 || (p.nrow && jr0 >= p.nrow[g])) {
    if (wave == 0 && 2 * lane < D) *reinterpret_cast<unsigned*>(p.out + (size_t)row * p.ldo + h * D + 2 * lane) = 0u;
    return;
  }
  const int ps = p0 + jr0, len = ps + 1;         // this row's position; it sees keys 0 .. ps
  float* sc = dsm;
  float* part = dsm + ((p.T_cap + 63) & ~63);
  bf16_t* kr = reinterpret_cast<bf16_t*>(part + OQ_WAVES * 128);
  bf16_t* cbase = p.cache + (size_t)g * p.cache_bs;
  bf16_t* src = p.qkv + (size_t)row * p.ld_qkv;
  {
    // attn_decode_kernel's rotary block: `items` threads per rotated head row.  Head row 0 is this row's q (in place), head row
    // 1 + i the k of row i <= jr0 of this step at position p0 + i, into LDS; the own k also goes to the cache row, with the own v
    const int half = D >> 1, items = half >> 2;
    bf16_t* crow = cbase + (size_t)ps * p.ld_cache;
    if (tid < (jr0 + 2) * items) {
      const int r = tid / items, i = (tid % items) * 4;
      const int which = r == 0 ? 0 : 1, ri = r == 0 ? jr0 : r - 1;
      bf16_t* e = p.qkv + (size_t)(g * p.K + ri) * p.ld_qkv + which * W + h * D + i;
      short4_t oa, ob;
      oq_rope4(e, half, p.cs, p.sn, p0 + ri, i, oa, ob);
      if (r == 0) {
        *reinterpret_cast<short4_t*>(e) = oa;
        *reinterpret_cast<short4_t*>(e + half) = ob;
      } else {
        *reinterpret_cast<short4_t*>(kr + ri * D + i) = oa;
        *reinterpret_cast<short4_t*>(kr + ri * D + i + half) = ob;
        if (ri == jr0) {
          *reinterpret_cast<short4_t*>(crow + h * D + i) = oa;
          *reinterpret_cast<short4_t*>(crow + h * D + i + half) = ob;
        }
      }
    } else if (tid < (jr0 + 2) * items + (D >> 3)) {
      const int c = (tid - (jr0 + 2) * items) * 8;
      *reinterpret_cast<short8_t*>(crow + W + h * D + c) = *reinterpret_cast<const short8_t*>(src + 2 * W + h * D + c);
    }
    __syncthreads();                               // q and the LDS keys are read back below by other waves of this workgroup
  }
  const bf16_t* qp = src + h * D;
  const bf16_t* kp = cbase + h * D;                // cache rows < p0 only
  const bf16_t* vp = cbase + W + h * D;
  const bf16_t* vq = p.qkv + (size_t)(g * p.K) * p.ld_qkv + 2 * W + h * D;     // v of row i of this step: vq + i * ld_qkv
  // phase 1: scores
  const int sub = lane & 15;                     // 16 lanes per key, dims sub*8 .. +7
  float qf[8];
  const bool dim_ok = sub * 8 < D;
  {
    short8_t qv = {0, 0, 0, 0, 0, 0, 0, 0};
    if (dim_ok) qv = *reinterpret_cast<const short8_t*>(qp + sub * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) qf[e] = bf2f((bf16_t)qv[e]) * p.scale;
  }
  oq_scores(sc, qf, dim_ok, len, wave, lane, [&](int j, int j0) {
    if (j0 + 2 * OQ_WAVES * 4 <= p0 || j < p0)       // (the first test is uniform: a pass wholly below p0 has no select)
      return *reinterpret_cast<const short8_t*>(kp + (size_t)j * p.ld_cache + sub * 8);
    return *reinterpret_cast<const short8_t*>(kr + (j - p0) * D + sub * 8);
  });
  __syncthreads();
  // phase 2: softmax statistics (each wave for itself)
  float mx, sum;
  oq_softmax_stats(sc, len, lane, mx, sum);
  // phase 3: o = sum_j p_j V[j]; lane owns dims 2*lane, 2*lane+1; wave w takes keys w, w+OQ_WAVES, ...  A group of eight keys
  // below p0 (uniform over the wave) lies in the cache: the one-row kernel's loads
  float o0, o1;
  const bool own = 2 * lane < D;
  const auto vcache = [&](int j) { return *reinterpret_cast<const unsigned*>(vp + (size_t)j * p.ld_cache + 2 * lane); };
  oq_pv(sc, mx, len, wave, own, p0, vcache, [&](int j) {
    const bf16_t* vrow = j < p0 ? vp + (size_t)j * p.ld_cache : vq + (size_t)(j - p0) * p.ld_qkv;
    return *reinterpret_cast<const unsigned*>(vrow + 2 * lane);
  }, o0, o1);
  part[wave * 128 + 2 * lane] = o0;
  part[wave * 128 + 2 * lane + 1] = o1;
  __syncthreads();
  if (wave == 0 && own) oq_sum_store(part, lane, sum, len, p.out + (size_t)row * p.ldo + h * D + 2 * lane);
}

// LDS of one workgroup: T_cap scores (rounded up to 64) and OQ_WAVES x 128 partial outputs in fp32, K x D rotated keys in bf16.
static size_t draft_lds_bytes(int T_cap, int K, int D) {
  return (((size_t)T_cap + 63) & ~(size_t)63) * 4 + OQ_WAVES * 128 * 4 + (size_t)K * D * 2;
}

// G sequences of K consecutive token rows in one launch: see include/myriad_hip.h.  `nrow` null: every group has K rows.
static int draft_launch(void* qkv, long ld_qkv, void* cache, long cache_bstride, long ld_cache, const int* pos, const int* live,
                        const int* nrow, bool rows, const float* cos_tab, const float* sin_tab, void* out, long ldo, int G, int K,
                        int H, int D, int T_cap, float scale, hipStream_t stream) {
  if (K < 1 || H <= 0 || T_cap <= 0) return MH_ERR_ARG;
  if (D <= 0 || D % 16 || D > 128 || K > DRAFT_MAX_K) return MH_ERR_UNSUPPORTED;
  const size_t sh = draft_lds_bytes(T_cap, K, D);
  if (sh > DRAFT_LDS_LIMIT) return MH_ERR_UNSUPPORTED;
  if (G <= 0) return MH_OK;                        // nothing to do: the answer says whether the shape is supported
  if (!oq_step_args_ok(qkv, ld_qkv, cache, cache_bstride, ld_cache, pos, live, nrow, rows, cos_tab, sin_tab, out, ldo, G, K, H, D))
    return MH_ERR_ARG;
  // > 64 KiB of dynamic LDS needs an explicit opt-in; raised only when a launch needs more than any before it
  static size_t allowed = 48 * 1024;
  if (sh > allowed) {
    if (hipFuncSetAttribute((const void*)attn_decode_draft_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh) != hipSuccess)
      return MH_ERR_LAUNCH;
    allowed = sh;
  }
  DraftParams p;
  p.qkv = (bf16_t*)qkv; p.cache = (bf16_t*)cache; p.out = (bf16_t*)out; p.pos = pos; p.live = live; p.nrow = nrow; p.cs = cos_tab; p.sn = sin_tab;
  p.ld_qkv = ld_qkv; p.cache_bs = cache_bstride; p.ld_cache = ld_cache; p.ldo = ldo;
  p.K = K; p.H = H; p.D = D; p.T_cap = T_cap; p.scale = scale;
  hipLaunchKernelGGL(attn_decode_draft_kernel, dim3(G * K * H), dim3(OQ_WAVES * 64), sh, stream, p);
  MH_CHECK_LAUNCH();
  return MH_OK;
}

extern "C" int mh_attn_decode_rope_draft(void* qkv, long ld_qkv, void* cache, long cache_bstride, long ld_cache, const int* pos,
                                         const int* live, const float* cos_tab, const float* sin_tab, void* out, long ldo, int G,
                                         int K, int H, int D, int T_cap, float scale, hipStream_t stream) {
  return draft_launch(qkv, ld_qkv, cache, cache_bstride, ld_cache, pos, live, nullptr, false, cos_tab, sin_tab, out, ldo, G, K, H, D,
                      T_cap, scale, stream);
}

// The decode slots' form: group g holds nrow[g] token rows (1 .. K); the rest of its K rows are skipped like an idle group's.
extern "C" int mh_attn_decode_rope_draft_rows(void* qkv, long ld_qkv, void* cache, long cache_bstride, long ld_cache, const int* pos,
                                              const int* live, const int* nrow, const float* cos_tab, const float* sin_tab,
                                              void* out, long ldo, int G, int K, int H, int D, int T_cap, float scale,
                                              hipStream_t stream) {
  return draft_launch(qkv, ld_qkv, cache, cache_bstride, ld_cache, pos, live, nrow, true, cos_tab, sin_tab, out, ldo, G, K, H, D,
                      T_cap, scale, stream);
}
