// Classification input transform on the device (included from preprocess.hip, built with -ffp-contract=off) -- for a ragged batch of uint8 HWC BGR
// frames in one launch, utils/augmentations.py:297-341 `classify_transforms(size)` as utils/dataloaders.py:949-985 applies it (the `torch_transforms`
// branch, on the BGR frame) and classify/predict.py:120-126 (`im.half() if model.fp16 else im.float()`):
//     CenterCrop(size): m = min(h0, w0), top = (h0 - m) // 2, left = (w0 - m) // 2, cv2.resize(im[top:top + m, left:left + m], (S, S), INTER_LINEAR)
//     ToTensor:         HWC -> CHW, BGR -> RGB, .float() (or .half()), / 255
//     Normalize:        (x - IMAGENET_MEAN) / IMAGENET_STD                                            utils/augmentations.py:15-16
// The resize is resize_u8.h's restatement of OpenCV's 8-bit INTER_LINEAR (identity, exact 2x area mean, 11-bit general path), taps clamped at the
// CROP's edge as cv2.resize of the cropped view clamps them.  Behind it a pixel is one of 256 values per channel, so ToTensor + Normalize is a table:
// the caller supplies lut[c][u] (3 x 256 fp32, c in RGB order) built with the reference's own two fp32 expressions -- the fp32 output is the
// reference's by construction, the fp16 output its round-to-nearest-even.  One lane produces 8 consecutive pixels of a row and stores 16 bytes per
// vector along each channel plane (two for fp32, one for fp16).
#pragma once
#include <hip/hip_runtime.h>

#include "y5_common.h"
#include "resize_u8.h"

namespace {
constexpr int kClsPx = 8;  // output pixels per lane
struct ClsTfParams {
  const y5_classify_job* jobs; const float* lut; void* dst;
  int B, S, f16;
};
}  // namespace

__global__ __launch_bounds__(256)
void y5_classify_transform_kernel(const ClsTfParams p) {
  const int b = blockIdx.y, S = p.S;
  const int nxg = (S + kClsPx - 1) / kClsPx;  // lanes per output row
  const int id = blockIdx.x * 256 + threadIdx.x;
  const int y = id / nxg;
  if (y >= S) return;
  const int x0 = (id - y * nxg) * kClsPx;
  const y5_classify_job j = p.jobs[b];
  if (!j.src || j.h0 < 1 || j.w0 < 1 || j.stride < 3 * j.w0) return;   // (a broken job leaves its image unwritten rather than reading out of bounds)
  const int m = j.h0 < j.w0 ? j.h0 : j.w0, top = (j.h0 - m) / 2, left = (j.w0 - m) / 2;
  const unsigned char* src = static_cast<const unsigned char*>(j.src) + (size_t)top * j.stride + (size_t)left * 3;
  const ResizeGeom g = resize_geom(m, m, S, S);
  const int nvalid = S - x0 < kClsPx ? S - x0 : kClsPx;
  float v[3][kClsPx];
#pragma unroll
  for (int i = 0; i < kClsPx; ++i) {
    int o[3] = {0, 0, 0};
    if (i < nvalid) resized_pixel(src, m, m, j.stride, g, y, x0 + i, o);
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c][i] = p.lut[c * 256 + o[2 - c]];   // BGR -> RGB
  }
  const size_t plane = (size_t)S * S;
  const size_t at = (size_t)b * 3 * plane + (size_t)y * S + x0;
  const bool vec = nvalid == kClsPx && (S & 7) == 0;
  if (p.f16) {
    _Float16* d = static_cast<_Float16*>(p.dst) + at;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (vec) {
        half8_t h;
#pragma unroll
        for (int i = 0; i < kClsPx; ++i) h[i] = (_Float16)v[c][i];
        *reinterpret_cast<half8_t*>(d + c * plane) = h;
      } else {
        for (int i = 0; i < nvalid; ++i) d[c * plane + i] = (_Float16)v[c][i];
      }
    }
  } else {
    float* d = static_cast<float*>(p.dst) + at;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (vec) {
        float4_t a, q;
#pragma unroll
        for (int i = 0; i < 4; ++i) { a[i] = v[c][i]; q[i] = v[c][4 + i]; }
        *reinterpret_cast<float4_t*>(d + c * plane) = a;
        *reinterpret_cast<float4_t*>(d + c * plane + 4) = q;
      } else {
        for (int i = 0; i < nvalid; ++i) d[c * plane + i] = v[c][i];
      }
    }
  }
}

extern "C" int y5_classify_transform_batch(const y5_classify_job* jobs_dev, int B, int S, const float* lut, void* dst, int dst_dtype, void* stream_) {
  if (!jobs_dev || !lut || !dst) return y5_fail(Y5_ERR_BAD_ARG, "classify_transform_batch: null pointer");
  if (B < 1 || B > 65535 || S < 1) return y5_fail(Y5_ERR_BAD_ARG, "classify_transform_batch: need 1 <= B <= 65535, S >= 1");
  if (dst_dtype != Y5_F16 && dst_dtype != Y5_F32) return y5_fail(Y5_ERR_BAD_ARG, "classify_transform_batch: dst dtype must be f16 or f32");
  if (((uintptr_t)dst & 15) || ((uintptr_t)lut & 3) || ((uintptr_t)jobs_dev & 7)) return y5_fail(Y5_ERR_BAD_ARG, "classify_transform_batch: dst must be 16-byte aligned");
  const long long lanes = (long long)S * ((S + kClsPx - 1) / kClsPx);
  if (lanes > 0x7fffffffLL) return y5_fail(Y5_ERR_UNSUPPORTED, "classify_transform_batch: output too large");
  ClsTfParams p{};
  p.jobs = jobs_dev; p.lut = lut; p.dst = dst; p.B = B; p.S = S; p.f16 = dst_dtype == Y5_F16;
  hipLaunchKernelGGL(y5_classify_transform_kernel, dim3((unsigned)((lanes + 255) / 256), B), dim3(256), 0, static_cast<hipStream_t>(stream_), p);
  return y5_check_launch("y5_classify_transform_batch");
}
