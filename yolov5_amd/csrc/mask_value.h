// The low-resolution value of one instance mask at pixel (gx, gy) of the prototype grid, as process_mask computes it before any
// upsampling (utils/segment/general.py:42-46 + crop_mask :22): 0 outside the box scaled to the grid, else sigmoid(coef . protos[:, gy, gx]).
// ONE definition for every kernel that needs these bits (mask.hip's y5_process_mask / y5_process_mask_batch, seg_val.h's y5_val_match_masks):
// the order of the additions and the contraction of the products into FMAs are part of the result, so every includer is compiled with
// mask.hip's flags (FMA contraction allowed) and the bit `v > 0.5f` is the same in all of them.
#pragma once
#include <hip/hip_runtime.h>

template <typename TP>
__device__ __forceinline__ float y5_mask_lowres(const TP* P, long long plane, int mw, int c, const float* coef, int gx, int gy, float x1,
                                                float y1, float x2, float y2) {
  const float r = (float)gx, cc = (float)gy;
  float v = 0.f;
  if (r >= x1 && r < x2 && cc >= y1 && cc < y2) {  // crop_mask, general.py:22
    float s = 0.f;
    const TP* q = P + (long long)gy * mw + gx;
    int k = 0;
    for (; k + 8 <= c; k += 8) {   // eight prototype planes in flight (the plain loop waits for every load before the next: a latency chain of c round trips)
      TP t[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) t[e] = q[(k + e) * plane];
#pragma unroll
      for (int e = 0; e < 8; ++e) s += coef[k + e] * (float)t[e];   // (same order of additions as the plain loop)
    }
    for (; k < c; ++k) s += coef[k] * (float)q[k * plane];
    v = 1.0f / (1.0f + expf(-s));
  }
  return v;
}

// The same value WITHOUT the crop, for process_mask_native (utils/segment/general.py:67): there the sigmoid plane is resized first and
// crop_mask runs at full resolution (:74-75), so every pixel of the window carries sigmoid(coef . protos[:, gy, gx]).  The order of the
// additions, the 8-wide unroll and 1 / (1 + expf(-s)) are y5_mask_lowres's.
template <typename TP>
__device__ __forceinline__ float y5_mask_value(const TP* P, long long plane, int mw, int c, const float* coef, int gx, int gy) {
  float s = 0.f;
  const TP* q = P + (long long)gy * mw + gx;
  int k = 0;
  for (; k + 8 <= c; k += 8) {
    TP t[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) t[e] = q[(k + e) * plane];
#pragma unroll
    for (int e = 0; e < 8; ++e) s += coef[k + e] * (float)t[e];
  }
  for (; k < c; ++k) s += coef[k] * (float)q[k * plane];
  return 1.0f / (1.0f + expf(-s));
}
