// One output sample of the align_corners=True bilinear resize, shared by bilinear_ac_kernel (expert.hip) and the reference
// bank's finish kernel (expert_bank.hip) so that both evaluate the same expression on the same values.
#pragma once
#include "common.h"

// the divisor of an output axis of n_out samples: the source position is o (n_in - 1) / (n_out - 1) as one correctly rounded
// division of exact integers (o * fl(step) carries two roundings of a value up to n_in - 1, which a steep cell turns into the
// largest part of the output's error)
__device__ __forceinline__ float bilinear_ac_div(int n_out) { return n_out > 1 ? (float)(n_out - 1) : 1.f; }

// ib: one [h, w_in] plane (global or LDS); (oy, ox): the output sample; dy, dx: bilinear_ac_div of the output's H and W
__device__ __forceinline__ float bilinear_ac_at(const float* ib, int h, int w_in, int oy, int ox, float dy, float dx) {
  const float fy = (float)(oy * (h - 1)) / dy, fx = (float)(ox * (w_in - 1)) / dx;
  int y0 = (int)fy, x0 = (int)fx;
  y0 = y0 < h - 1 ? y0 : (h > 1 ? h - 2 : 0);
  x0 = x0 < w_in - 1 ? x0 : (w_in > 1 ? w_in - 2 : 0);
  const int y1 = y0 + (h > 1), x1 = x0 + (w_in > 1);
  const float wy = fy - y0, wx = fx - x0;
  const float v = (1.f - wy) * ((1.f - wx) * ib[y0 * w_in + x0] + wx * ib[y0 * w_in + x1]) +
                  wy * ((1.f - wx) * ib[y1 * w_in + x0] + wx * ib[y1 * w_in + x1]);
  return v;
}
