// The row body of the token sampler: one 1024-thread workgroup per logits row, the row resident in registers (the steps are listed
// at the top of sample.hip).  sample.hip instantiates it for the uniform and the slot forms, draft_sample.hip for the rows of a
// draft-and-verify step; the three differ only in where a row finds its seed, its Philox step t, its EOS ban and its live flag.
#pragma once
#include "smp_rng.h"

struct SmpTop { float best; int idx; float second; };
__device__ __forceinline__ SmpTop smp_combine(const SmpTop& a, const SmpTop& b) {
  const bool take_b = (b.best > a.best) || (b.best == a.best && b.idx < a.idx);
  SmpTop o;
  o.best = take_b ? b.best : a.best;
  o.idx = take_b ? b.idx : a.idx;
  o.second = fmaxf(fmaxf(a.second, b.second), take_b ? a.best : b.best);
  return o;
}

enum { SMP_UNIFORM = 0, SMP_ROWS = 1, SMP_DRAFT = 2 };

// SMP_UNIFORM: params = (inv_temp, top_p, top_k, penalty) f32 on the device; seed = one u64; step = the decode step counter (or
// null): t = *step + t_add, counter = (t, 0, row, 0).
// SMP_ROWS: the slot form -- params = (inv_temp, top_p, top_k, penalty, min_length, eos_id), seed[row] and gen[row] per row, t =
// gen[row], counter = (t, 0, 0, 0), the ban is eos_id while t < min_length (ban_id, step and t_add are unused); a row with
// live[row] == 0 (live may be null: every row is live) leaves before the first barrier -- live[row] is uniform over the workgroup,
// one scalar branch -- and writes out = -1, margin = p_max = 0, kept = 0.
// SMP_DRAFT: the slot form for groups of K rows -- row = g * K + j reads seed[g], t = gen[g] + j and live[g], and is idle as well
// when j >= nrow[g] (live and nrow are required).
// DRAW = false stops after the arg-max, margin and p_max: the greedy pick with the same per-row ban (kept, u_out and seed are not
// touched).
template <int MODE, bool DRAW>
__device__ __forceinline__ void sample_row_body(const float* __restrict__ logits, long ldl, long* __restrict__ out,
                                                float* __restrict__ margin, float* __restrict__ pmax, int* __restrict__ kept,
                                                float* __restrict__ u_out, int V, int ban_id, const float* __restrict__ params,
                                                const unsigned long long* __restrict__ seed, const int* __restrict__ step, int t_add,
                                                const int* __restrict__ gen, const int* __restrict__ live,
                                                const int* __restrict__ nrow, int K) {
  constexpr bool ROWS = MODE != SMP_UNIFORM;
  __shared__ float sb[SNW], s2[SNW], red[SNW], fsum[SNW];
  __shared__ int si[SNW], isum[SNW];
  __shared__ unsigned hist[256];
  __shared__ unsigned sh_prefix, sh_rank;
  __shared__ float sh_u;
  __shared__ unsigned long long cand[MH_SAMPLE_CAP];
  __shared__ float cum[MH_SAMPLE_CAP];
  const long row = blockIdx.x;
  const int tid = threadIdx.x;
  const float* x = logits + row * ldl;
  const float ninf = -__builtin_inff();
  const float inv_temp = params[0], top_p = params[1];
  int k = (int)params[2];
  k = k < 1 ? 1 : (k > V ? V : k);
  const long srow = MODE == SMP_DRAFT ? row / K : row;      // the row of the per-request state
  const int tj = MODE == SMP_DRAFT ? (int)(row - srow * K) : 0;
  if (ROWS) {
    if (MODE == SMP_DRAFT ? (!live[srow] || tj >= nrow[srow]) : (live && !live[row])) {
      if (tid == 0) {
        out[row] = -1;
        margin[row] = 0.f;
        pmax[row] = 0.f;
        if (DRAW) kept[row] = 0;
      }
      return;
    }
    ban_id = gen[srow] + tj < (int)params[4] ? (int)params[5] : -1;
  }

  if (DRAW && tid == 0) {
    const unsigned long long sd = ROWS ? seed[srow] : *seed;
    unsigned c[4] = {ROWS ? (unsigned)(gen[srow] + tj) : (unsigned)((step ? *step : 0) + t_add), 0u, ROWS ? 0u : (unsigned)row, 0u};
    philox4x32_10(c, (unsigned)sd, (unsigned)(sd >> 32));
    sh_u = (float)(c[0] >> 8) * (1.0f / 16777216.0f);
  }

  // 1. the row in registers (the layout of argmax_pmax_wide_kernel, so margin and p_max come out bit-equal to it), ban
  float4_t xv[8];
  const int t4 = tid * 4;
  SmpTop tp = {ninf, t4 < V ? t4 : 0, ninf};
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int j = (i * SNT + tid) * 4;
    xv[i] = (float4_t){ninf, ninf, ninf, ninf};
    if (j + 3 < V) xv[i] = *reinterpret_cast<const float4_t*>(x + j);
    else
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (j + e < V) xv[i][e] = x[j + e];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (j + e == ban_id) xv[i][e] = ninf;
      const float v = xv[i][e];
      if (v > tp.best) { tp.second = tp.best; tp.best = v; tp.idx = j + e; }
      else if (v > tp.second) tp.second = v;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    SmpTop q;
    q.best = __shfl_xor(tp.best, o, 64);
    q.idx = __shfl_xor(tp.idx, o, 64);
    q.second = __shfl_xor(tp.second, o, 64);
    tp = smp_combine(tp, q);
  }
  const int w = tid >> 6, l = tid & 63;
  if (l == 0) { sb[w] = tp.best; si[w] = tp.idx; s2[w] = tp.second; }
  __syncthreads();
  SmpTop all = {sb[0], si[0], s2[0]};
#pragma unroll
  for (int i = 1; i < SNW; ++i) all = smp_combine(all, (SmpTop){sb[i], si[i], s2[i]});
  {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) s += __expf((xv[i][e] - all.best) * inv_temp);
    s = block_sum<SNW>(s, red);
    if (tid == 0) {
      if (margin) margin[row] = all.best - all.second;
      if (pmax) pmax[row] = 1.f / s;
      if (!DRAW) out[row] = all.idx;
    }
  }
  if (!DRAW) return;
  if (all.best == __builtin_inff()) {     // a +inf logit takes all the mass: the arg-max (its lowest id), alone, whatever top_p is
    if (tid == 0) {
      out[row] = all.idx;
      kept[row] = 1;
      if (u_out) u_out[row] = sh_u;
    }
    return;
  }

  // 2. temperature (HF TemperatureLogitsWarper), then the k-th largest tempered logit: radix select over the ordered keys, 8 bits
  //    a pass from the top; past-V and banned entries are -inf, the smallest key, so they never move the k-th value of a row
  //    with k <= V.  A NaN logit is -inf here, and here only: xv, which margin and p_max were formed from, stays as loaded
  unsigned kv[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) kv[i][e] = smp_key_draw(xv[i][e] * inv_temp);
  unsigned prefix = 0, rank = (unsigned)k;
#pragma unroll 1
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    const unsigned hmask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if ((kv[i][e] & hmask) == prefix) atomicAdd(&hist[(kv[i][e] >> shift) & 255u], 1u);
    __syncthreads();
    if (tid < 64) {                       // lane l holds bins 255-4l .. 252-4l (largest first)
      unsigned c[4], s = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) { c[j] = hist[255 - 4 * tid - j]; s += c[j]; }
      unsigned before = smp_wave_scan(s) - s;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (before < rank && rank <= before + c[j]) {
          sh_prefix = prefix | ((unsigned)(255 - 4 * tid - j) << shift);
          sh_rank = rank - before;
        }
        before += c[j];
      }
    }
    __syncthreads();
    prefix = sh_prefix;
    rank = sh_rank;
  }
  const unsigned KEY_NINF = SMP_KEY_NINF;
  const unsigned thr = prefix;            // key of the k-th largest; every finite logit with key >= thr is kept (ties included)

  // 3. gather the candidates, (key, ~id) in one u64 so that a descending sort is (logit desc, id asc)
  int mine = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) mine += (kv[i][e] >= thr && kv[i][e] > KEY_NINF) ? 1 : 0;
  const int incl = smp_block_scan<int>(mine, isum);
  int n = 0;
#pragma unroll
  for (int i = 0; i < SNW; ++i) n += isum[i];
  if (n == 0 || n > MH_SAMPLE_CAP) {      // tied top-k set past the cap (or nothing finite): the host draws this row
    if (tid == 0) {
      out[row] = all.idx;
      kept[row] = -1;
      if (u_out) u_out[row] = sh_u;
    }
    return;
  }
  int o = incl - mine;
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (kv[i][e] >= thr && kv[i][e] > KEY_NINF) {
        const unsigned id = (unsigned)((i * SNT + tid) * 4 + e);
        cand[o++] = ((unsigned long long)kv[i][e] << 32) | (0xffffffffu - id);
      }
  int P = 1;
  while (P < n) P <<= 1;
  for (int i = n + tid; i < P; i += SNT) cand[i] = 0ull;      // below every candidate
  __syncthreads();

  // 4. bitonic sort of the P <= 1024 entries, descending
  for (int size = 2; size <= P; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      if (tid < (P >> 1)) {
        const int lo = 2 * tid - (tid & (stride - 1)), hi = lo + stride;
        const bool desc = (lo & size) == 0;
        const unsigned long long a = cand[lo], b = cand[hi];
        if ((a < b) == desc) { cand[lo] = b; cand[hi] = a; }
      }
      __syncthreads();
    }

  // 5. softmax over the top-k set, top-p cut (keep i iff its exclusive prefix mass < top_p), inverse-CDF draw
  const float vmax = smp_unkey((unsigned)(cand[0] >> 32));
  if (vmax == __builtin_inff()) {         // a finite logit the temperature pushed to +inf: as a +inf logit, the first of the order
    if (tid == 0) {
      out[row] = (long)(0xffffffffu - (unsigned)(cand[0] & 0xffffffffull));
      kept[row] = 1;
      if (u_out) u_out[row] = sh_u;
    }
    return;
  }
  const float p = tid < n ? expf(smp_unkey((unsigned)(cand[tid] >> 32)) - vmax) : 0.f;
  const float c = smp_block_scan<float>(p, fsum);
  if (tid < n) cum[tid] = c;
  __syncthreads();
  const float total = cum[n - 1];
  const float excl = tid == 0 ? 0.f : (tid < n ? cum[tid - 1] : 0.f);
  int mk = __syncthreads_count(tid < n && (top_p >= 1.f || excl < top_p * total));
  mk = mk > 0 ? mk : 1;                   // the largest token is always kept (min_tokens_to_keep = 1)
  const float target = sh_u * cum[mk - 1];
  int sel = __syncthreads_count(tid < mk && cum[tid] <= target);
  sel = sel < mk ? sel : mk - 1;
  if (tid == 0) {
    out[row] = (long)(0xffffffffu - (unsigned)(cand[sel] & 0xffffffffull));
    kept[row] = mk;
    if (u_out) u_out[row] = sh_u;
  }
}
