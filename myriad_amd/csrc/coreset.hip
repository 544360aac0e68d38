// K16c: greedy k-centre (farthest-point) coreset selection over the rows of one class of the vision expert's reference bank
// (vision_expert.py: compact_references; the rule is DESIGN section 6).  Two kernels per selected row, enqueued back to back:
//   coreset_update  mind[i] = min(mind[i], dist2(i, sel[j])) for every row i of the class, mind[sel[j]] = -1, and one
//                   (value, lowest index) arg-max partial per workgroup
//   coreset_pick    one workgroup reduces the partials to sel[j + 1] / radius2[j + 1] (after the last update: cover2)
// The dependency between two iterations is the kernel boundary; the centre's index is read from sel[j] on the device, so the
// host enqueues the 2 n launches without waiting.  No float atomics: every value has one writer.
// coreset_update is a streaming read of the class's T x rows x D bf16 elements.  CS_GL = 16 lanes share a row: lane g of the
// group reads the 16-byte pieces g, g + 16, g + 32, ... of the row in every tap, a group's load is 256 contiguous bytes and a
// wave's is four of them.  A group owns CS_RPG = 4 rows and walks them together (four independent loads per lane and step, one
// LDS read of the centre's piece serves all four), a workgroup of 16 groups owns CS_ROWS = 64 consecutive rows.  The centre's
// T D bf16 values are staged in LDS once per workgroup.
// dist2 is one fp32 chain per lane -- taps ascending, the lane's pieces ascending, the eight elements of a piece ascending,
// each step acc = fma(x - c, x - c, acc) -- followed by the butterfly over the 16 lanes (xor 8, 4, 2, 1; a + b == b + a, so
// every lane ends with the same bits).  The order is a function of (D, T) alone: the bits of dist2 depend on its two rows
// only, not on rows, row0, the grid or the neighbouring classes.  Rows past the class's end inside the last workgroup are read
// as copies of the class's own last row (never the neighbouring class's memory) and take no part in mind or the arg-max.
// The arg-max order is total (larger value first, then the lower index), so the way it is split over lanes, waves and
// workgroups cannot show in the result.
#include "common.h"

#define CS_NT 256
#define CS_GL 16                                    // lanes that share a row
#define CS_RPG 4                                    // rows a lane group walks together
#define CS_ROWS (CS_NT / CS_GL * CS_RPG)            // rows of a workgroup (64)
#define CS_MAX_T 8
#define CS_MAX_TD 16384                             // staged centre: T D bf16 <= 32 KiB of LDS (T = 8, D = 2048)

struct CsTaps { const bf16_t* p[CS_MAX_T]; };
struct CsPart { float v; int i; };

__device__ __forceinline__ bool cs_better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

__device__ __forceinline__ float cs_piece(const uint4 x, const uint4 c, float acc) {
  const unsigned xs[4] = {x.x, x.y, x.z, x.w}, cs[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float d0 = __uint_as_float(xs[e] << 16) - __uint_as_float(cs[e] << 16);
    acc = __builtin_fmaf(d0, d0, acc);
    const float d1 = __uint_as_float(xs[e] & 0xffff0000u) - __uint_as_float(cs[e] & 0xffff0000u);
    acc = __builtin_fmaf(d1, d1, acc);
  }
  return acc;
}

__global__ __launch_bounds__(CS_NT) void coreset_update_kernel(const CsTaps taps, int T, long ld, int D, long row0, int rows,
                                                               int j, int start, int* sel,
                                                               float* __restrict__ radius2, float* __restrict__ mind,
                                                               CsPart* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) uint4 cen[];      // [T][D / 8]
  __shared__ CsPart wbest[CS_NT / 64];
  const int tid = threadIdx.x, P = D >> 3;
  const int c = j == 0 ? start : sel[j];            // uniform: a scalar load
  if (j == 0 && blockIdx.x == 0 && tid == 0) {
    sel[0] = start;
    radius2[0] = INFINITY;
  }
#pragma unroll
  for (int t = 0; t < CS_MAX_T; ++t)
    if (t < T) {
      const uint4* src = reinterpret_cast<const uint4*>(taps.p[t] + (row0 + c) * ld);
      for (int i = tid; i < P; i += CS_NT) cen[t * P + i] = src[i];
    }
  __syncthreads();

  const int grp = tid / CS_GL, gl = tid & (CS_GL - 1);
  const int base = blockIdx.x * CS_ROWS + grp * CS_RPG;
  long roff[CS_RPG];
#pragma unroll
  for (int r = 0; r < CS_RPG; ++r) roff[r] = (row0 + min(base + r, rows - 1)) * ld;   // tail: the class's own last row
  float acc[CS_RPG];
#pragma unroll
  for (int r = 0; r < CS_RPG; ++r) acc[r] = 0.f;
#pragma unroll
  for (int t = 0; t < CS_MAX_T; ++t)
    if (t < T) {
      const uint4* ct = cen + t * P;
      const uint4* x[CS_RPG];
#pragma unroll
      for (int r = 0; r < CS_RPG; ++r) x[r] = reinterpret_cast<const uint4*>(taps.p[t] + roff[r]);
#pragma unroll 2
      for (int i = gl; i < P; i += CS_GL) {
        uint4 v[CS_RPG];
#pragma unroll
        for (int r = 0; r < CS_RPG; ++r) v[r] = x[r][i];
        const uint4 cc = ct[i];
#pragma unroll
        for (int r = 0; r < CS_RPG; ++r) acc[r] = cs_piece(v[r], cc, acc[r]);
      }
    }
#pragma unroll
  for (int r = 0; r < CS_RPG; ++r)
#pragma unroll
    for (int o = CS_GL / 2; o > 0; o >>= 1) acc[r] += __shfl_xor(acc[r], o, 64);

  // lane r of a group finishes row base + r: every lane of the group holds the same four sums
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  float d = acc[0];
#pragma unroll
  for (int r = 1; r < CS_RPG; ++r) d = gl == r ? acc[r] : d;
  const int row = base + gl;
  if (gl < CS_RPG && row < rows) {
    float m = j == 0 ? d : fminf(mind[row], d);
    if (row == c) m = -1.f;
    mind[row] = m;
    bv = m;
    bi = row;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (cs_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }
  if ((tid & 63) == 0) { wbest[tid >> 6].v = bv; wbest[tid >> 6].i = bi; }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < CS_NT / 64; ++w)
      if (cs_better(wbest[w].v, wbest[w].i, bv, bi)) { bv = wbest[w].v; bi = wbest[w].i; }
    part[blockIdx.x].v = bv;
    part[blockIdx.x].i = bi;
  }
}

// jn < n: sel[jn] / radius2[jn] = the arg-max over the partials; jn == n (after the last update): cover2 = the maximum.
__global__ __launch_bounds__(CS_NT) void coreset_pick_kernel(const CsPart* __restrict__ part, int nwg, int jn, int n,
                                                             int* __restrict__ sel, float* __restrict__ radius2,
                                                             float* __restrict__ cover2) {
  __shared__ CsPart wbest[CS_NT / 64];
  const int tid = threadIdx.x;
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  for (int k = tid; k < nwg; k += CS_NT) {
    const float v = part[k].v;
    const int i = part[k].i;
    if (cs_better(v, i, bv, bi)) { bv = v; bi = i; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (cs_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }
  if ((tid & 63) == 0) { wbest[tid >> 6].v = bv; wbest[tid >> 6].i = bi; }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < CS_NT / 64; ++w)
      if (cs_better(wbest[w].v, wbest[w].i, bv, bi)) { bv = wbest[w].v; bi = wbest[w].i; }
    if (jn < n) {
      sel[jn] = bi;
      radius2[jn] = bv;
    } else {
      *cover2 = bv;
    }
  }
}

static inline long cs_groups(int rows) { return ((long)rows + CS_ROWS - 1) / CS_ROWS; }

extern "C" long mh_coreset_ws_bytes(int rows) { return rows < 1 ? -1 : cs_groups(rows) * (long)sizeof(CsPart); }

extern "C" int mh_coreset_select(const void* const* taps, int T, long ld, int D, long row0, int rows, int n, int start, int* sel,
                                 float* radius2, float* mind, float* cover2, void* ws, long ws_bytes, hipStream_t stream) {
  if (!taps || !sel || !radius2 || !mind || !cover2 || !ws) return MH_ERR_ARG;
  if (T < 1 || T > CS_MAX_T || D < 8 || (D % 8) != 0 || ld < D || (ld % 8) != 0 || row0 < 0) return MH_ERR_ARG;
  if (rows < 1 || n < 1 || n > rows || start < 0 || start >= rows) return MH_ERR_ARG;
  if (ws_bytes < mh_coreset_ws_bytes(rows) || ((uintptr_t)ws & 7) != 0) return MH_ERR_ARG;
  CsTaps tp;
  for (int t = 0; t < CS_MAX_T; ++t) {
    tp.p[t] = t < T ? (const bf16_t*)taps[t] : nullptr;
    if (t < T && (!taps[t] || ((uintptr_t)taps[t] & 15) != 0)) return MH_ERR_ARG;   // 16-byte loads
  }
  if ((long)T * D > CS_MAX_TD) return MH_ERR_UNSUPPORTED;
  const int nwg = (int)cs_groups(rows);
  const size_t lds = (size_t)T * D * sizeof(bf16_t);
  CsPart* part = (CsPart*)ws;
  for (int j = 0; j < n; ++j) {
    hipLaunchKernelGGL(coreset_update_kernel, dim3(nwg), dim3(CS_NT), lds, stream, tp, T, ld, D, row0, rows, j, start, sel,
                       radius2, mind, part);
    hipLaunchKernelGGL(coreset_pick_kernel, dim3(1), dim3(CS_NT), 0, stream, part, nwg, j + 1, n, sel, radius2, cover2);
    MH_CHECK_LAUNCH();                              // a failed launch ends the loop at once, not 2 n launches later
  }
  return MH_OK;
}
