// K17: streaming localisation metrics for anomaly maps (seg_metrics.py: SegMetrics.update; eval_protocol.seg_metrics_from_hist).
//   mask_components   8-connected components of binary masks [B, H, W]: labels (-1 on background, else the smallest linear index
//                     y W + x of the pixel's component), area (the component's pixel count at that root pixel, 0 elsewhere),
//                     n_regions [B]
//   seg_hist_update   hist [3, 2^20] int64 += per-key counts of the normal pixels (row 0), of the anomalous pixels (row 1) and
//                     floor(2^40 / area of its region) per anomalous pixel (row 2); counters [4] int64 += pixels, anomalous
//                     pixels, regions, non-finite scores
//
// mask_components: one workgroup per image, everything in LDS.  Under 8-connectivity the foreground pixels of one aligned 2 x 2
// block are always one component, so the union-find runs over blocks, not pixels (block-based union-find): nb = ceil(H/2) ceil(W/2)
// <= 20479 32-bit parents L[] with native ds atomics, where per-pixel labels of a 256 x 256 image would need 16-bit ones.
//   0  M[blk] = the block's 4-bit occupancy (bit 2 dy + dx), L[blk] = blk
//   1  every foreground block unites with its left / upper-left / upper / upper-right neighbour block where a pixel pair of the
//      two touches.  Block coordinates are checked, never linear indices, so x = W - 1 is no neighbour of x = 0 of the next row.
//   2  L[blk] = find(blk), then the occupancy moves into L's top four bits and M is freed
//   3  M[root] = min over the component's blocks of (their first pixel in raster order) << 16     (atomicMin)
//   4  M[root] += the block's pixel count, the component's first pixel left out: low half = area - 1 <= 65535
//   5  per pixel, coalesced: labels / area / the region count
// Termination: L[x] <= x always and every write lowers a parent (atomicMin, or the flattening store of an ancestor), so find()
// walks a strictly decreasing chain, and unite() repeats only after its atomicMin met a parent that another lane had lowered in
// between -- it then carries on from that smaller value.  Nothing waits for another lane or wave to act.
//
// seg_hist_update: the key of a score is the top 20 bits of the order-preserving transform of its fp32 bits (-0 -> +0; negative:
// all bits flipped; else the sign bit set), so a bf16 map is keyed exactly and an fp32 map keeps 11 mantissa bits.  Integer
// atomics only: the sums do not depend on arrival order.  aggregate = 1: the lanes of a wave that hold the same (row, key) are
// found with ballots and their leader adds once -- a flat background puts a whole wave on one bin; 0: one atomic per lane.
#include "common.h"

#define SM_NT 1024
#define SM_MAX_PIX 65536
#define SM_MAX_LDS (160 * 1024)
#define SH_NT 256
#define SH_BINS (1 << 20)

__device__ __forceinline__ unsigned sm_find(const volatile unsigned* L, unsigned a) {
  unsigned p = L[a];
  while (p != a) {          // p < a: strictly decreasing
    a = p;
    p = L[a];
  }
  return a;
}

__device__ __forceinline__ void sm_unite(unsigned* L, unsigned a, unsigned b) {
  bool done = false;
  while (!done) {
    a = sm_find(L, a);
    b = sm_find(L, b);
    if (a < b) {
      const unsigned old = atomicMin(&L[b], a);
      done = old == b;      // b was still a root: hooked.  Else someone lowered L[b] to old < b: go on with (a, old)
      b = old;
    } else if (b < a) {
      const unsigned old = atomicMin(&L[a], b);
      done = old == a;
      a = old;
    } else {
      done = true;
    }
  }
}

__global__ __launch_bounds__(SM_NT) void mask_components_kernel(const unsigned char* __restrict__ masks, int* __restrict__ labels,
                                                                int* __restrict__ area, int* __restrict__ n_regions, int H,
                                                                int W) {
  extern __shared__ unsigned sm_lds[];
  const int nbx = (W + 1) >> 1, nby = (H + 1) >> 1, nb = nbx * nby, N = H * W, tid = threadIdx.x;
  unsigned* L = sm_lds;
  unsigned* M = sm_lds + nb;
  unsigned* count = sm_lds + 2 * nb;
  const unsigned char* mk = masks + (long)blockIdx.x * N;

  if (tid == 0) *count = 0;
  for (int blk = tid; blk < nb; blk += SM_NT) {
    const int by = blk / nbx, bx = blk - by * nbx, y = 2 * by, x = 2 * bx;
    const bool xr = x + 1 < W, yd = y + 1 < H;
    const unsigned char* p = mk + y * W + x;
    unsigned pat = p[0] != 0;
    if (xr && p[1]) pat |= 2;
    if (yd && p[W]) pat |= 4;
    if (xr && yd && p[W + 1]) pat |= 8;
    M[blk] = pat;
    L[blk] = blk;
  }
  __syncthreads();

  for (int blk = tid; blk < nb; blk += SM_NT) {
    const unsigned pat = M[blk];
    if (!pat) continue;
    const int by = blk / nbx, bx = blk - by * nbx;
    if (bx > 0 && (pat & 5) && (M[blk - 1] & 10)) sm_unite(L, blk, blk - 1);
    if (by > 0) {
      if ((pat & 3) && (M[blk - nbx] & 12)) sm_unite(L, blk, blk - nbx);
      if (bx > 0 && (pat & 1) && (M[blk - nbx - 1] & 8)) sm_unite(L, blk, blk - nbx - 1);
      if (bx + 1 < nbx && (pat & 2) && (M[blk - nbx + 1] & 4)) sm_unite(L, blk, blk - nbx + 1);
    }
  }
  __syncthreads();

  for (int blk = tid; blk < nb; blk += SM_NT)
    if (M[blk]) L[blk] = sm_find(L, blk);   // a racing find() reads the old parent or the root: both are ancestors
  __syncthreads();
  for (int blk = tid; blk < nb; blk += SM_NT) {
    L[blk] |= M[blk] << 28;                 // nb < 2^28
    M[blk] = 0xFFFFFFFFu;
  }
  __syncthreads();

  for (int blk = tid; blk < nb; blk += SM_NT) {
    const unsigned v = L[blk], pat = v >> 28;
    if (!pat) continue;
    const int by = blk / nbx, bx = blk - by * nbx;
    const int first = (2 * by + ((pat & 3) ? 0 : 1)) * W + 2 * bx + (((pat & 3) ? (pat & 1) : (pat & 4)) ? 0 : 1);
    atomicMin(&M[v & 0x0FFFFFFFu], (unsigned)first << 16);
  }
  __syncthreads();

  for (int blk = tid; blk < nb; blk += SM_NT) {
    const unsigned v = L[blk], pat = v >> 28;
    if (!pat) continue;
    const int by = blk / nbx, bx = blk - by * nbx;
    const int first = (2 * by + ((pat & 3) ? 0 : 1)) * W + 2 * bx + (((pat & 3) ? (pat & 1) : (pat & 4)) ? 0 : 1);
    const unsigned root = v & 0x0FFFFFFFu;
    const unsigned n = __popc(pat) - ((M[root] >> 16) == (unsigned)first ? 1u : 0u);   // the high half is final since pass 3
    if (n) atomicAdd(&M[root], n);
  }
  __syncthreads();

  int* lab_out = labels + (long)blockIdx.x * N;
  int* area_out = area + (long)blockIdx.x * N;
  for (int i = tid; i < N; i += SM_NT) {
    const int y = i / W, x = i - y * W;
    const unsigned v = L[(y >> 1) * nbx + (x >> 1)];
    int lab = -1, ar = 0;
    if ((v >> (28 + 2 * (y & 1) + (x & 1))) & 1u) {
      const unsigned m = M[v & 0x0FFFFFFFu];
      lab = (int)(m >> 16);
      if (lab == i) {
        ar = (int)(m & 0xFFFFu) + 1;
        atomicAdd(count, 1u);
      }
    }
    lab_out[i] = lab;
    area_out[i] = ar;
  }
  __syncthreads();
  if (tid == 0) n_regions[blockIdx.x] = (int)*count;
}

__device__ __forceinline__ unsigned long long sh_wave_sum(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(SH_NT) void seg_hist_update_kernel(const void* __restrict__ maps, int maps_bf16,
                                                                const unsigned char* __restrict__ masks,
                                                                const int* __restrict__ labels, const int* __restrict__ area,
                                                                unsigned long long* __restrict__ hist,
                                                                unsigned long long* __restrict__ counters, long total, int N,
                                                                int aggregate) {
  const int lane = threadIdx.x & 63;
  unsigned n_pix = 0, n_pos = 0, n_reg = 0, n_bad = 0;      // wave-uniform
  for (long base = (long)blockIdx.x * SH_NT; base < total; base += (long)gridDim.x * SH_NT) {
    const long i = base + threadIdx.x;
    const bool in = i < total;
    unsigned u = 0;
    bool pos = false, root = false;
    unsigned long long w = 0;
    if (in) {
      u = maps_bf16 ? ((unsigned)reinterpret_cast<const bf16_t*>(maps)[i]) << 16 : reinterpret_cast<const unsigned*>(maps)[i];
      pos = masks[i] != 0;
      const long img = (i / N) * N;
      root = area[i] > 0;
      if (pos) {
        const int lab = labels[i];
        const int a = (unsigned)lab < (unsigned)N ? area[img + lab] : 0;     // labels / area are mask_components' outputs
        w = a > 0 ? (1ull << 40) / (unsigned)a : 0ull;
      }
    }
    if (u == 0x80000000u) u = 0;
    const bool finite = (u & 0x7F800000u) != 0x7F800000u;
    const unsigned key = ((u & 0x80000000u) ? ~u : (u | 0x80000000u)) >> 12;
    const bool live = in && finite;
    n_pix += __popcll(__ballot(in));
    n_pos += __popcll(__ballot(in && pos));
    n_reg += __popcll(__ballot(in && root));
    n_bad += __popcll(__ballot(in && !finite));
    if (!aggregate) {
      if (live) {
        atomicAdd(&hist[(pos ? SH_BINS : 0) + key], 1ull);
        if (pos) atomicAdd(&hist[2 * SH_BINS + key], w);
      }
      continue;
    }
    const unsigned kk = live ? ((pos ? SH_BINS : 0) | key) : 0xFFFFFFFFu;
    unsigned long long todo = __ballot(live);
    while (todo) {                                          // every turn retires its leader: at most 64 turns
      const int leader = __ffsll((long long)todo) - 1;
      const unsigned k = __shfl(kk, leader, 64);
      const bool mine = kk == k;
      const unsigned long long same = __ballot(mine);
      const unsigned n = __popcll(same);
      if (k & SH_BINS) {
        unsigned long long ws = mine ? w : 0ull;
        if (n > 1) ws = sh_wave_sum(ws);
        if (lane == leader) {
          atomicAdd(&hist[k], (unsigned long long)n);       // k = 2^20 + key: row 1
          atomicAdd(&hist[k + SH_BINS], ws);
        }
      } else if (lane == leader) {
        atomicAdd(&hist[k], (unsigned long long)n);
      }
      todo &= ~same;
    }
  }
  if (lane == 0) {
    if (n_pix) atomicAdd(&counters[0], (unsigned long long)n_pix);
    if (n_pos) atomicAdd(&counters[1], (unsigned long long)n_pos);
    if (n_reg) atomicAdd(&counters[2], (unsigned long long)n_reg);
    if (n_bad) atomicAdd(&counters[3], (unsigned long long)n_bad);
  }
}

// dynamic LDS of one mask_components workgroup, or -1 where the image is refused
extern "C" long mh_mask_components_lds_bytes(int H, int W) {
  if (H < 1 || W < 1 || (long)H * W > SM_MAX_PIX) return -1;
  const long nb = (long)((H + 1) / 2) * ((W + 1) / 2);
  const long bytes = (2 * nb + 1) * (long)sizeof(unsigned);
  return bytes > SM_MAX_LDS ? -1 : bytes;
}

extern "C" int mh_mask_components(const void* masks, int* labels, int* area, int* n_regions, int B, int H, int W,
                                  hipStream_t stream) {
  if (!masks || !labels || !area || !n_regions || B < 1) return MH_ERR_ARG;
  const long bytes = mh_mask_components_lds_bytes(H, W);
  if (bytes < 0) return MH_ERR_ARG;
  static long attr_bytes = 64 * 1024;     // what a kernel may ask for without the attribute
  if (bytes > attr_bytes) {
    if (hipFuncSetAttribute((const void*)mask_components_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) !=
        hipSuccess)
      return MH_ERR_LAUNCH;
    attr_bytes = bytes;
  }
  hipLaunchKernelGGL(mask_components_kernel, dim3(B), dim3(SM_NT), (size_t)bytes, stream, (const unsigned char*)masks, labels,
                     area, n_regions, H, W);
  MH_CHECK_LAUNCH();
  return MH_OK;
}

extern "C" int mh_seg_hist_update(long long* hist, long long* counters, const void* maps, int maps_bf16, const void* masks,
                                  const int* labels, const int* area, int B, int H, int W, int aggregate, hipStream_t stream) {
  if (!hist || !counters || !maps || !masks || !labels || !area || B < 1 || H < 1 || W < 1) return MH_ERR_ARG;
  if ((long)H * W > SM_MAX_PIX) return MH_ERR_ARG;
  const long total = (long)B * H * W;
  long blocks = (total + SH_NT - 1) / SH_NT;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(seg_hist_update_kernel, dim3((unsigned)blocks), dim3(SH_NT), 0, stream, maps, maps_bf16,
                     (const unsigned char*)masks, labels, area, (unsigned long long*)hist, (unsigned long long*)counters, total,
                     H * W, aggregate);
  MH_CHECK_LAUNCH();
  return MH_OK;
}
