// Master -> working-copy refresh of a trainable module's weight matrices (the EVA ViT with freeze_vit: False): from a row-major
// fp32 [R, C] master write, in ONE pass, the bf16 row-major copy W (row stride ld_dst >= C) and the bf16 transposed copy W^T
// [C, R] (row stride ld_t >= R) that the dgrad GEMMs read.  8 bytes of HBM traffic per weight (4 read, 2 + 2 written) where a
// cast followed by a transpose moves 10.  Batched: one launch walks a device-resident table of matrix descriptors, so the 156
// matrices of the 39-block ViT are one launch.  Only elements inside [R, C] are written: the zero padding of a wider
// destination (patch_w's K = 588 -> 640, a padded hidden width) is left alone.  Rounding is f2bf / pack_bf2, the conversion
// mh_cast_f32_to_bf16 and mh_transpose_to_bf16 use: same bits.
//
// Tile: 64 x 64, 256 threads.  Load: lane (g = t & 15, p = t >> 4) reads rows 2p, 2p + 1 (then 2p + 32, 2p + 33) at columns
// 4g .. 4g + 3 as two 16-byte loads; the 16 lanes of a row cover its 256 bytes.  Row-major store: 8 bytes per lane, the 16
// lanes of a row write one full 128-byte line.  Transposed copy through LDS: the lane packs (row 2p, row 2p + 1) of each of
// its four columns into one 32-bit word and stores it at T[column][p], T = [64][33] words.  The odd row stride puts the word
// of column c, pair p on bank (c + p) mod 32: a 32-lane half of a wave (g = 0..15, two p) lands on 16 banks twice, and a
// two-way ds_write_b32 costs no extra LDS cycle (MI355X: the instruction takes 4 cycles, the array 2 per 32 words).  Read-out:
// lane (j = t & 15, c = t >> 4 (+16, +32, +48)) takes words 2j, 2j + 1 of column c -- rows 4j .. 4j + 3 -- as two 32-bit
// reads: the 32 lanes of a half read columns c, c + 1 at banks (c + 2j) and (c + 1 + 2j') mod 32, which differ in parity: no
// conflict.  The 16 lanes of an output row store 8 bytes each: one full 128-byte line of W^T.
// The bank arithmetic above is derived from the documented LDS bank rules, not measured: no bank-conflict counter run was taken.
// What was measured is the whole launch (tools/vit_finetune_bench.py: 984 M weights in 1.40 ms, 5.6 TB/s of HBM traffic), far
// from any LDS limit: a tile costs about 256 LDS cycles against the ~4000 clocks its 32 KB of HBM traffic take per CU.
// Every block first finds its matrix by a binary search over the descriptor table: up to 8 dependent 4-byte global loads for the
// 156-matrix ViT (all L2 hits after the first wave of blocks), a latency each block pays once before its own loads.
#include "common.h"

struct MhRefreshDesc {          // 64 bytes; mh_refresh_bf16_pair_pack writes it, the kernel reads it
  const float* src;             // [R, C] row-major, contiguous
  bf16_t* dst;                  // [R, ld_dst] or null
  bf16_t* dst_t;                // [C, ld_t] or null
  long ld_dst, ld_t;
  int R, C;
  int tile0;                    // index of this matrix's first tile in the launch
  int tiles_c;                  // tiles per tile row: ceil(C / 64)
  int vec;                      // bit 0: 16-byte source loads, bit 1: 8-byte stores to dst, bit 2: 8-byte stores to dst_t
  int pad_;
};
static_assert(sizeof(MhRefreshDesc) == 64, "descriptor layout is part of the ABI (mh_refresh_bf16_pair_desc_bytes)");

#define RF_T 64
#define RF_LD 33

__global__ __launch_bounds__(256) void refresh_pair_kernel(const MhRefreshDesc* __restrict__ table, int n_desc) {
  __shared__ unsigned T[RF_T][RF_LD];
  // the matrix this tile belongs to: the last descriptor whose first tile is <= blockIdx.x (uniform across the block)
  int lo = 0, hi = n_desc - 1;
  const int tile = (int)blockIdx.x;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (table[mid].tile0 <= tile) lo = mid; else hi = mid - 1;
  }
  const MhRefreshDesc d = table[lo];
  const int local = tile - d.tile0;
  const int r0 = (local / d.tiles_c) * RF_T, c0 = (local % d.tiles_c) * RF_T;
  if (r0 >= d.R) return;                                       // a tile count larger than the table's matrices: nothing to do
  const int R = d.R, C = d.C;
  const int t = threadIdx.x;
  const bool need_t = d.dst_t != nullptr;
  {
    const int g = t & 15, c = c0 + 4 * g;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int p = (t >> 4) + 16 * it;                        // row pair inside the tile
      float v[2][4];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int r = r0 + 2 * p + h;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[h][e] = 0.f;
        if (r < R && c < C) {
          const float* s = d.src + (long)r * C + c;
          if ((d.vec & 1) && c + 3 < C) {
            const float4_t f = *reinterpret_cast<const float4_t*>(s);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[h][e] = f[e];
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (c + e < C) v[h][e] = s[e];
          }
          if (d.dst != nullptr) {
            bf16_t* o = d.dst + (long)r * d.ld_dst + c;
            if ((d.vec & 2) && c + 3 < C) {
              uint2 pk;
              pk.x = pack_bf2(v[h][0], v[h][1]);
              pk.y = pack_bf2(v[h][2], v[h][3]);
              *reinterpret_cast<uint2*>(o) = pk;
            } else {
#pragma unroll
              for (int e = 0; e < 4; ++e)
                if (c + e < C) o[e] = f2bf(v[h][e]);
            }
          }
        }
      }
      if (need_t) {
#pragma unroll
        for (int e = 0; e < 4; ++e) T[4 * g + e][p] = pack_bf2(v[0][e], v[1][e]);
      }
    }
  }
  if (!need_t) return;
  __syncthreads();
  {
    const int j = t & 15, r = r0 + 4 * j;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int ci = (t >> 4) + 16 * it, c = c0 + ci;
      if (c >= C || r >= R) continue;
      uint2 pk;
      pk.x = T[ci][2 * j];
      pk.y = T[ci][2 * j + 1];
      bf16_t* o = d.dst_t + (long)c * d.ld_t + r;
      if ((d.vec & 4) && r + 3 < R) {
        *reinterpret_cast<uint2*>(o) = pk;
      } else {
        const unsigned w[2] = {pk.x, pk.y};
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (r + e < R) o[e] = (bf16_t)(w[e >> 1] >> (16 * (e & 1)));
      }
    }
  }
}

extern "C" long mh_refresh_bf16_pair_desc_bytes(void) { return (long)sizeof(MhRefreshDesc); }

extern "C" long mh_refresh_bf16_pair_pack(void* host_table, int index, long first_tile, const float* src, void* dst, long ld_dst,
                                          void* dst_t, long ld_t, int R, int C) {
  if (host_table == nullptr || index < 0 || first_tile < 0 || src == nullptr || R <= 0 || C <= 0) return MH_ERR_ARG;
  if (((uintptr_t)host_table & 7) || ((uintptr_t)src & 3) || ((uintptr_t)dst & 1) || ((uintptr_t)dst_t & 1)) return MH_ERR_ARG;
  if (dst == nullptr && dst_t == nullptr) return MH_ERR_ARG;
  if (dst != nullptr && ld_dst < C) return MH_ERR_ARG;         // a destination row shorter than the source row
  if (dst_t != nullptr && ld_t < R) return MH_ERR_ARG;
  const long tiles_c = (C + RF_T - 1) / RF_T, tiles_r = (R + RF_T - 1) / RF_T;
  const long next = first_tile + tiles_c * tiles_r;
  if (next > 0x7fffffffL) return MH_ERR_ARG;
  MhRefreshDesc& d = reinterpret_cast<MhRefreshDesc*>(host_table)[index];
  d.src = src;
  d.dst = (bf16_t*)dst;
  d.dst_t = (bf16_t*)dst_t;
  d.ld_dst = dst != nullptr ? ld_dst : 0;
  d.ld_t = dst_t != nullptr ? ld_t : 0;
  d.R = R;
  d.C = C;
  d.tile0 = (int)first_tile;
  d.tiles_c = (int)tiles_c;
  d.vec = ((C % 4 == 0 && ((uintptr_t)src & 15) == 0) ? 1 : 0) |
          ((dst != nullptr && ld_dst % 4 == 0 && ((uintptr_t)dst & 7) == 0) ? 2 : 0) |
          ((dst_t != nullptr && ld_t % 4 == 0 && ((uintptr_t)dst_t & 7) == 0) ? 4 : 0);
  d.pad_ = 0;
  return next;
}

extern "C" int mh_refresh_bf16_pair(const void* dev_table, int n_desc, long total_tiles, hipStream_t stream) {
  if (n_desc == 0 && total_tiles == 0) return MH_OK;
  if (dev_table == nullptr || ((uintptr_t)dev_table & 15) || n_desc <= 0 || total_tiles <= 0 || total_tiles > 0x7fffffffL)
    return MH_ERR_ARG;
  if (total_tiles < n_desc) return MH_ERR_ARG;                 // every matrix has at least one tile
  hipLaunchKernelGGL(refresh_pair_kernel, dim3((unsigned)total_tiles), dim3(256), 0, stream,
                     (const MhRefreshDesc*)dev_table, n_desc);
  MH_CHECK_LAUNCH();
  return MH_OK;
}
