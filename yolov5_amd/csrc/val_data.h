// Validation input pipeline of a detection dataset (utils/dataloaders.py:768-790 `load_image` + :715-716 `letterbox(auto=False,
// scaleup=False)` + :763 HWC -> CHW, BGR -> RGB) for a ragged batch in ONE launch: y5_letterbox_area_batch.  Included by preprocess.hip
// (built with -ffp-contract=off: every product and sum below is rounded on its own).
//
// Per job (include/yolov5_hip.h: y5_area_job) the host (yolov5_amd/dataloaders.py:area_jobs) picks the path:
//   COPY     nh == h0 && nw == w0
//   LINEAR   nh > h0 || nw > w0: the 8-bit INTER_LINEAR of resize_u8.h, unchanged
//   AREA2    both scales exactly 2: (a + b + c + d + 2) >> 2 (area2 of resize_u8.h)
//   AREA_INT both scales integer: s = integer sum of the iy x ix block, sat_u8(rint((float)s * (1.0f / (ix * iy)))), product in fp32
//   AREA_TAB otherwise: OpenCV's general INTER_AREA (modules/imgproc/src/resize.cpp: computeResizeAreaTab, ResizeArea_Invoker).  The tap
//            tables are built on the host in double and uploaded with the job table; entry d of an axis is {first source index, tap count,
//            word offset of the fp32 weights}: the taps of one output index are consecutive source indices.  One output value: for every
//            source row of the y entry, in order, row = 0.f, row += (float)S * alpha over the x taps in order; acc = beta * row for the
//            first row, acc += beta * row after it; sat_u8(rint(acc)).
// cv2 is a third-party dependency of the reference that is absent here: like INTER_LINEAR and warpAffine this layer restates the PUBLISHED
// algorithm and its parity with the real library is unpinned by necessity.
//
// Launch shape: byte gather, memory-bound, no cross-thread reduction -- every output value is an independent weighted sum in a fixed
// order, so the result is bitwise repeatable.  One WAVE owns 64 consecutive output pixels of one row of one image: adjacent lanes take
// adjacent output pixels, so their source spans are adjacent and a wave's loads fall into a few consecutive cache lines of each source
// row; the three planes of a pixel come from one pass over its source pixels.  A wave whose 64 pixels are all padding (rows above / below
// the image, columns left / right of it) writes them with 16-byte stores from the first lanes instead.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/yolov5_hip.h"
#include "resize_u8.h"

namespace {
constexpr int VA_WAVE = 64;   // output pixels per wave
constexpr int VA_WAVES = 4;   // waves per workgroup

struct AreaParams {
  const y5_area_job* jobs;
  const int* tabs;          // tap tables of all AREA_TAB jobs: int32 words, weights as fp32 bits
  long long tab_words;
  void* dst;
  int B, H, W, pad, dst_dtype, div255, chunks;   // chunks = ceil(W / 64)
};

__device__ inline int sat_u8_rint(float v) {  // saturate_cast<uchar>(float): round half to even, then clamp
  const int i = (int)rintf(v);
  return i < 0 ? 0 : (i > 255 ? 255 : i);
}

template <typename T> __device__ inline T va_value(int v, int div255);
template <> __device__ inline unsigned char va_value<unsigned char>(int v, int) { return (unsigned char)v; }
template <> __device__ inline _Float16 va_value<_Float16>(int v, int div255) {
  const float f = (float)v;                                  // `.half() / 255`: fp32 division of the (exact) half value, rounded once
  return (_Float16)(div255 ? f / 255.0f : f);
}
template <> __device__ inline float va_value<float>(int v, int div255) {
  const float f = (float)v;
  return div255 ? f / 255.0f : f;
}

// one pixel (yy, xx) of the resized image of job j -> BGR in out[3]
__device__ inline void va_pixel(const AreaParams& p, const y5_area_job& j, const ResizeGeom& g, int yy, int xx, int out[3]) {
  const unsigned char* src = static_cast<const unsigned char*>(j.src);
  out[0] = out[1] = out[2] = p.pad;
  // a job or a table that points outside its image or outside the table is not followed: the host builds both, this keeps a bad one from reading
  if (j.mode == Y5_AREA_INT) {
    if (j.ix < 1 || j.iy < 1 || (long long)j.nw * j.ix > j.w0 || (long long)j.nh * j.iy > j.h0) return;
    int s0 = 0, s1 = 0, s2 = 0;
    for (int r = 0; r < j.iy; ++r) {
      const unsigned char* q = src + (size_t)(yy * j.iy + r) * j.stride + (size_t)xx * j.ix * 3;
      for (int c = 0; c < j.ix; ++c) { s0 += q[3 * c]; s1 += q[3 * c + 1]; s2 += q[3 * c + 2]; }
    }
    const float sc = 1.0f / (float)(j.ix * j.iy);
    out[0] = sat_u8_rint((float)s0 * sc); out[1] = sat_u8_rint((float)s1 * sc); out[2] = sat_u8_rint((float)s2 * sc);
  } else if (j.mode == Y5_AREA_TAB) {
    if (j.xtab < 0 || j.ytab < 0 || (long long)j.xtab + 3 * (long long)j.nw > p.tab_words || (long long)j.ytab + 3 * (long long)j.nh > p.tab_words) return;
    const int* ex = p.tabs + j.xtab + 3 * xx;
    const int* ey = p.tabs + j.ytab + 3 * yy;
    const int xs = ex[0], xn = ex[1], ys = ey[0], yn = ey[1];
    if (xs < 0 || xn < 1 || xs + xn > j.w0 || ys < 0 || yn < 1 || ys + yn > j.h0 || ex[2] < 0 || ey[2] < 0 ||
        (long long)ex[2] + xn > p.tab_words || (long long)ey[2] + yn > p.tab_words) return;
    const float* alpha = reinterpret_cast<const float*>(p.tabs + ex[2]);
    const float* beta = reinterpret_cast<const float*>(p.tabs + ey[2]);
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    if (xn <= 4) {
      // up to four x taps (any scale below 3): weights and byte offsets in registers, the row loop is 12 loads and 12 products.  A missing tap
      // re-reads the last one with weight 0: row + S * 0.f == row exactly (row >= 0), so the sum is the one of the general loop bit for bit
      float w[4];
      int o[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) { o[c] = 3 * (c < xn ? c : xn - 1); w[c] = c < xn ? alpha[c] : 0.f; }
      for (int r = 0; r < yn; ++r) {
        const unsigned char* q = src + (size_t)(ys + r) * j.stride + (size_t)xs * 3;
        float r0 = 0.f, r1 = 0.f, r2 = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) { r0 += (float)q[o[c]] * w[c]; r1 += (float)q[o[c] + 1] * w[c]; r2 += (float)q[o[c] + 2] * w[c]; }
        const float b = beta[r];
        if (r == 0) { a0 = b * r0; a1 = b * r1; a2 = b * r2; }
        else { a0 += b * r0; a1 += b * r1; a2 += b * r2; }
      }
    } else {
      for (int r = 0; r < yn; ++r) {
        const unsigned char* q = src + (size_t)(ys + r) * j.stride + (size_t)xs * 3;
        float r0 = 0.f, r1 = 0.f, r2 = 0.f;
        for (int c = 0; c < xn; ++c) {
          const float a = alpha[c];
          r0 += (float)q[3 * c] * a; r1 += (float)q[3 * c + 1] * a; r2 += (float)q[3 * c + 2] * a;
        }
        const float b = beta[r];
        if (r == 0) { a0 = b * r0; a1 = b * r1; a2 = b * r2; }
        else { a0 += b * r0; a1 += b * r1; a2 += b * r2; }
      }
    }
    out[0] = sat_u8_rint(a0); out[1] = sat_u8_rint(a1); out[2] = sat_u8_rint(a2);
  } else {
    resized_pixel(src, j.h0, j.w0, j.stride, g, yy, xx, out);   // COPY, LINEAR, AREA2: resize_u8.h decides from the geometry (clamped taps)
  }
}

template <typename T>
__device__ inline void va_wave(const AreaParams& p, int b, int y, int x0, int lane) {
  const y5_area_job j = p.jobs[b];
  const size_t plane = (size_t)p.H * p.W;
  T* d = static_cast<T*>(p.dst) + (size_t)b * 3 * plane + (size_t)y * p.W;
  const int yy = y - j.top;
  const int xe = x0 + VA_WAVE < p.W ? x0 + VA_WAVE : p.W;   // this wave's pixels: [x0, xe)
  const bool all_pad = yy < 0 || yy >= j.nh || xe <= j.left || x0 >= j.left + j.nw;
  constexpr int PER = 16 / (int)sizeof(T);                  // elements of one 16-byte store
  if (all_pad && xe - x0 == VA_WAVE && (reinterpret_cast<size_t>(d + x0) & 15) == 0 && ((plane * sizeof(T)) & 15) == 0) {
    constexpr int NV = VA_WAVE / PER;                       // stores per plane: 4 (u8), 8 (f16), 16 (f32) -> at most 48 lanes
    if (lane < 3 * NV) {
      const T v = va_value<T>(p.pad, p.div255);
      alignas(16) T vec[PER];
#pragma unroll
      for (int i = 0; i < PER; ++i) vec[i] = v;
      T* o = d + (size_t)(lane / NV) * plane + x0 + (lane % NV) * PER;
      *reinterpret_cast<uint4_t*>(o) = *reinterpret_cast<const uint4_t*>(vec);
    }
    return;
  }
  const int x = x0 + lane;
  if (x >= p.W) return;
  const int xx = x - j.left;
  int v[3] = {p.pad, p.pad, p.pad};
  if (yy >= 0 && yy < j.nh && xx >= 0 && xx < j.nw) {
    const ResizeGeom g = resize_geom(j.h0, j.w0, j.nh, j.nw);
    va_pixel(p, j, g, yy, xx, v);
  }
  d[x] = va_value<T>(v[2], p.div255);                        // BGR -> RGB
  d[plane + x] = va_value<T>(v[1], p.div255);
  d[2 * plane + x] = va_value<T>(v[0], p.div255);
}
}  // namespace

__global__ __launch_bounds__(256)
void y5_letterbox_area_kernel(const AreaParams p) {
  const int lane = threadIdx.x & (VA_WAVE - 1);
  const long long unit = (long long)blockIdx.x * VA_WAVES + (threadIdx.x >> 6);   // (row, 64-pixel chunk) of image blockIdx.y
  const int y = (int)(unit / p.chunks);
  if (y >= p.H) return;
  const int x0 = (int)(unit - (long long)y * p.chunks) * VA_WAVE;
  if (p.dst_dtype == Y5_U8) va_wave<unsigned char>(p, blockIdx.y, y, x0, lane);
  else if (p.dst_dtype == Y5_F16) va_wave<_Float16>(p, blockIdx.y, y, x0, lane);
  else va_wave<float>(p, blockIdx.y, y, x0, lane);
}

extern "C" int y5_letterbox_area_batch(const y5_area_job* jobs_dev, const int* tabs_dev, long long tab_words, int B, int H, int W, int pad_value,
                                       void* dst, int dst_dtype, int div255, void* stream_) {
  if (!jobs_dev || !dst) return y5_fail(Y5_ERR_BAD_ARG, "letterbox_area_batch: null pointer");
  if (tab_words < 0 || (tab_words > 0 && !tabs_dev)) return y5_fail(Y5_ERR_BAD_ARG, "letterbox_area_batch: tap table missing");
  if (B < 1 || B > 65535 || H < 1 || W < 1 || pad_value < 0 || pad_value > 255)
    return y5_fail(Y5_ERR_BAD_ARG, "letterbox_area_batch: need 1 <= B <= 65535, H, W >= 1, 0 <= pad_value <= 255");
  if (dst_dtype != Y5_U8 && dst_dtype != Y5_F16 && dst_dtype != Y5_F32)
    return y5_fail(Y5_ERR_BAD_ARG, "letterbox_area_batch: dst dtype must be u8, f16 or f32");
  AreaParams p{};
  p.jobs = jobs_dev; p.tabs = tabs_dev; p.tab_words = tab_words; p.dst = dst; p.B = B; p.H = H; p.W = W; p.pad = pad_value;
  p.dst_dtype = dst_dtype; p.div255 = div255; p.chunks = (W + VA_WAVE - 1) / VA_WAVE;
  const long long units = (long long)H * p.chunks;
  if (units > 0x7fffffffLL) return y5_fail(Y5_ERR_UNSUPPORTED, "letterbox_area_batch: output too large");
  hipLaunchKernelGGL(y5_letterbox_area_kernel, dim3((unsigned)((units + VA_WAVES - 1) / VA_WAVES), B), dim3(VA_WAVE * VA_WAVES), 0,
                     static_cast<hipStream_t>(stream_), p);
  return y5_check_launch("y5_letterbox_area_batch");
}
