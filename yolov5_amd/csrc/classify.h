// Classification head and post-processing (included from head.hip, built with -ffp-contract=off).
//
// y5_classify_head: what models/common.py:1120-1140 `Classify.forward` does behind its Conv -- `linear(drop(pool(x).flatten(1)))` in eval mode
// (Dropout is the identity) -- on the Conv's NHWC output (B, HW, C):
//     pooled[b, c] = (fp32 sum over the HW pixels) / HW                        nn.AdaptiveAvgPool2d(1)
//     logits[b, j] = bias[j] + sum_c pooled[b, c] * w[j, c]   (fp32)           nn.Linear(1280, nc)
// `pooled` stays in fp32 on fp16 plans, where the reference rounds the pool's output to fp16 before the Linear: this head is the more
// accurate of the two (tests hold it to the forward error bound of fp32 summation, not to the reference's fp16 noise).
// Two forms, both built; measured on an MI355X at the yolov5s-cls shape (B 128, HW 49, C 1280, nc 1000, fp16; DESIGN.md 4.6b has the byte / FLOP budget):
// form 2 takes 18.2 us and is what `form = 0` runs, form 1 takes 50.7 us (F.adaptive_avg_pool2d + F.linear: 23.0 us).
//   form 1, one launch : one workgroup per image pools its 1280 channels into LDS, then its waves walk the nc filter rows (plain FMAs, a
//                        wave per row group, xor-butterfly reduction); every workgroup reads the whole filter from L2.
//   form 2, two launches: a pool kernel writes pooled (B, C) fp32 to the workspace; fp16: a 32 (classes) x 32 (images) MFMA tile per
//                        workgroup, K split over its four waves and added in wave order -- the fp32 `pooled` enters the fp16 MFMA as
//                        hi + lo halves (hi = fp16(p), lo = fp16(p - hi): 22 bits of p), two MFMAs per K step (v_mfma_f32_32x32x16_f16, the shape
//                        the host emulator models); fp32: form 1's row walk on a (class group, image) grid.
// Determinism: every (b, j) is summed in an order fixed by (HW, C) alone -- four pixel phases added 0..3, K quarters added 0..3, butterflies --
// never by B, by the image's position in the batch or by the grid; no atomics.  A batch equals its single-row calls bit for bit.
//
// y5_classify_post: classify/predict.py:133,152 and classify/val.py:119,122 for a batch of logits in one launch: softmax(dim=1), the first
// min(5, nc) columns of argsort(1, descending=True), and nn.CrossEntropyLoss(label_smoothing, reduction='none').  One wave per row; the row is
// read once into LDS as fp32.  Ties in the ranking go to the LOWER index (torch's unstable sort leaves them undefined).
#pragma once
#include <hip/hip_runtime.h>

#include "y5_common.h"

namespace {
constexpr int kClsParts = 4;         // pixel phases of the pool: pixel p belongs to phase p % 4; phases are added 0, 1, 2, 3
constexpr int kClsMaxC = 8192;       // pooled (C fp32) + the phase partials must fit the default 64 KiB of dynamic LDS
constexpr int kClsRowsPerWave = 4;   // filter rows a wave walks at once (independent accumulators: loads in flight)

struct ClsHeadParams {
  const void* x; const void* w; const float* bias; void* logits; float* pooled;
  int B, HW, C, ld, nc, ldo;
};

template <typename T> __device__ __forceinline__ void cls_load8(const T* p, float (&v)[8]);
template <> __device__ __forceinline__ void cls_load8<_Float16>(const _Float16* p, float (&v)[8]) {
  const half8_t h = *reinterpret_cast<const half8_t*>(p);
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = (float)h[e];
}
template <> __device__ __forceinline__ void cls_load8<float>(const float* p, float (&v)[8]) {
  const float4_t a = *reinterpret_cast<const float4_t*>(p), b = *reinterpret_cast<const float4_t*>(p + 4);
#pragma unroll
  for (int e = 0; e < 4; ++e) { v[e] = a[e]; v[4 + e] = b[e]; }
}

// Mean over the pixels of image `xb` for the channel octets [oct0, oct0 + blockDim.x / 4): thread (lane = tid % nl, phase = tid / nl) sums
// the pixels phase, phase + 4, ... of octet oct0 + lane in pixel order; the four phases are then added in phase order and divided by HW.
// out[c - 8 * oct0] for the channels of these octets (LDS or global).  part: LDS, 4 * nl * 8 floats.  Reached by every thread of the block.
template <typename T>
__device__ __forceinline__ void cls_pool_octets(const T* xb, int HW, int C, int ld, int oct0, float* part, float* out) {
  const int nl = blockDim.x / kClsParts, lane = threadIdx.x % nl, phase = threadIdx.x / nl;
  const int c0 = (oct0 + lane) * 8;
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (c0 < C)
    for (int p = phase; p < HW; p += kClsParts) {
      float v[8];
      cls_load8<T>(xb + (size_t)p * ld + c0, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) s[e] += v[e];
    }
#pragma unroll
  for (int e = 0; e < 8; ++e) part[(phase * nl + lane) * 8 + e] = s[e];
  __syncthreads();
  const float n = (float)HW;
  for (int o = threadIdx.x; o < nl * 8; o += blockDim.x)
    if (oct0 * 8 + o < C) out[o] = (((part[o] + part[nl * 8 + o]) + part[2 * nl * 8 + o]) + part[3 * nl * 8 + o]) / n;
  __syncthreads();
}

// logits[j] = bias[j] + sum_c pooled[c] * w[j, c] for the rows j0 <= j < j1: wave wv of nwv takes groups of four rows; a lane owns the channel
// octets lane, lane + 64, ... in ascending order, then the 64 lane sums meet in an xor butterfly.  pooled: LDS.
template <typename T>
__device__ __forceinline__ void cls_rows(const float* pooled, const T* w, const float* bias, T* out, int C, int j0, int j1) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nwv = blockDim.x >> 6;
  for (int jb = j0 + wv * kClsRowsPerWave; jb < j1; jb += nwv * kClsRowsPerWave) {
    float acc[kClsRowsPerWave];
#pragma unroll
    for (int r = 0; r < kClsRowsPerWave; ++r) acc[r] = 0.f;
    for (int c = lane * 8; c < C; c += 512) {
      float p[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) p[e] = pooled[c + e];
#pragma unroll
      for (int r = 0; r < kClsRowsPerWave; ++r) {
        const int j = jb + r < j1 ? jb + r : j1 - 1;   // (a row past the end repeats the last one; its sum is dropped)
        float v[8];
        cls_load8<T>(w + (size_t)j * C + c, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[r] = fmaf(p[e], v[e], acc[r]);
      }
    }
#pragma unroll
    for (int r = 0; r < kClsRowsPerWave; ++r) {
      float a = acc[r];
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) a += __shfl(a, lane ^ m);
      if (lane == 0 && jb + r < j1) out[jb + r] = (T)(bias[jb + r] + a);
    }
  }
}
}  // namespace

// form 1: grid (B), 1024 threads; LDS: pooled [C] + partials [4][256][8]
template <typename T>
__global__ __launch_bounds__(1024)
void y5_classify_head_fused_kernel(const ClsHeadParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* pooled = reinterpret_cast<float*>(smem);
  float* part = pooled + p.C;
  const int b = blockIdx.x, nl = blockDim.x / kClsParts;
  const T* xb = static_cast<const T*>(p.x) + (size_t)b * p.HW * p.ld;
  for (int oct0 = 0; oct0 * 8 < p.C; oct0 += nl) cls_pool_octets<T>(xb, p.HW, p.C, p.ld, oct0, part, pooled + oct0 * 8);
  cls_rows<T>(pooled, static_cast<const T*>(p.w), p.bias, static_cast<T*>(p.logits) + (size_t)b * p.ldo, p.C, 0, p.nc);
}

// form 2, first launch: grid (ceil(C / 8 / 64), B), 256 threads; LDS: partials [4][64][8]
template <typename T>
__global__ __launch_bounds__(256)
void y5_classify_pool_kernel(const ClsHeadParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int b = blockIdx.y, oct0 = blockIdx.x * (blockDim.x / kClsParts);
  const T* xb = static_cast<const T*>(p.x) + (size_t)b * p.HW * p.ld;
  cls_pool_octets<T>(xb, p.HW, p.C, p.ld, oct0, reinterpret_cast<float*>(smem), p.pooled + (size_t)b * p.C + oct0 * 8);
}

// form 2, second launch, fp32: grid (ceil(nc / 64), B), 256 threads; LDS: pooled [C]
__global__ __launch_bounds__(256)
void y5_classify_rows_f32_kernel(const ClsHeadParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* pooled = reinterpret_cast<float*>(smem);
  const int b = blockIdx.y, j0 = blockIdx.x * 64;
  for (int c = threadIdx.x; c < p.C; c += blockDim.x) pooled[c] = p.pooled[(size_t)b * p.C + c];
  __syncthreads();
  cls_rows<float>(pooled, static_cast<const float*>(p.w), p.bias, static_cast<float*>(p.logits) + (size_t)b * p.ldo, p.C, j0, j0 + 64 < p.nc ? j0 + 64 : p.nc);
}

// form 2, second launch, fp16: grid (ceil(nc / 32), ceil(B / 32)), 256 threads; LDS: partial tiles [4][64][16].
// D = W(32 classes x 16) * pooled^T(16 x 32 images): lane l supplies W[j0 + l % 32][k0 + 8 (l / 32) ..] and pooled[b0 + l % 32][the same k];
// it receives, for image b0 + l % 32, the classes j0 + (r % 4) + 8 (r / 4) + 4 (l / 32), r = 0..15.
__global__ __launch_bounds__(256)
void y5_classify_gemm_f16_kernel(const ClsHeadParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* tiles = reinterpret_cast<float*>(smem);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int j0 = blockIdx.x * 32, b0 = blockIdx.y * 32;
  const int jr = j0 + (lane & 31) < p.nc ? j0 + (lane & 31) : p.nc - 1;   // (rows / images past the end repeat the last one; never stored)
  const int br = b0 + (lane & 31) < p.B ? b0 + (lane & 31) : p.B - 1;
  const _Float16* wrow = static_cast<const _Float16*>(p.w) + (size_t)jr * p.C;
  const float* prow = p.pooled + (size_t)br * p.C;
  const int nsteps = (p.C + 15) / 16, per = (nsteps + 3) / 4;
  const int s0 = wv * per, s1 = s0 + per < nsteps ? s0 + per : nsteps;
  float16_t acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (int s = s0; s < s1; ++s) {
    const int k = s * 16 + 8 * (lane >> 5);
    half8_t a, hi, lo;
    if (k < p.C) {
      a = *reinterpret_cast<const half8_t*>(wrow + k);
      float v[8];
      cls_load8<float>(prow + k, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        hi[e] = (_Float16)v[e];
        lo[e] = (_Float16)(v[e] - (float)hi[e]);
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) { a[e] = (_Float16)0.f; hi[e] = (_Float16)0.f; lo[e] = (_Float16)0.f; }
    }
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, hi, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, lo, acc, 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) tiles[(wv * 64 + lane) * 16 + r] = acc[r];
  __syncthreads();
  if (wv == 0 && b0 + (lane & 31) < p.B) {
    _Float16* out = static_cast<_Float16*>(p.logits) + (size_t)(b0 + (lane & 31)) * p.ldo;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int j = j0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      const float s = ((tiles[lane * 16 + r] + tiles[(64 + lane) * 16 + r]) + tiles[(128 + lane) * 16 + r]) + tiles[(192 + lane) * 16 + r];
      if (j < p.nc) out[j] = (_Float16)(p.bias[j] + s);
    }
  }
}

extern "C" size_t y5_classify_head_workspace_bytes(int B, int C) {
  return B < 1 || C < 1 ? 0 : (size_t)B * (size_t)C * sizeof(float);
}

// the form `form = 0` stands for: the faster one on the MI355X at the yolov5s-cls shape (scripts/classify_bench.py)
#define Y5_CLASSIFY_HEAD_DEFAULT_FORM 2

extern "C" int y5_classify_head(const void* x, int dtype, int B, int HW, int C, int ld, const void* w, const float* bias, int nc, void* logits, int ldo,
                                int form, void* workspace, size_t workspace_bytes, void* stream_) {
  if (!x || !w || !bias || !logits) return y5_fail(Y5_ERR_BAD_ARG, "classify_head: null pointer");
  if (dtype != Y5_F16 && dtype != Y5_F32) return y5_fail(Y5_ERR_BAD_ARG, "classify_head: dtype must be f16 or f32");
  if (B < 1 || HW < 1 || C < 1 || nc < 1 || ld < C || ldo < nc) return y5_fail(Y5_ERR_BAD_ARG, "classify_head: need B, HW, C, nc >= 1, ld >= C, ldo >= nc");
  if (form < 0 || form > 2) return y5_fail(Y5_ERR_BAD_ARG, "classify_head: form must be 0 (default), 1 (one launch) or 2 (pool + GEMM)");
  const int es = dtype == Y5_F16 ? 2 : 4;
  if (((uintptr_t)x | (uintptr_t)w) & 15 || ((uintptr_t)bias & 3) || ((uintptr_t)logits & (es - 1)))
    return y5_fail(Y5_ERR_BAD_ARG, "classify_head: x and w must be 16-byte aligned");
  if ((C & 7) || ((size_t)ld * es & 15)) return y5_fail(Y5_ERR_UNSUPPORTED, "classify_head: needs C % 8 == 0 and pixel rows of a multiple of 16 bytes");
  if (C > kClsMaxC || B > 65535 || (long long)B * HW * ld * es >= (1LL << 40)) return y5_fail(Y5_ERR_UNSUPPORTED, "classify_head: C <= 8192, B <= 65535");
  if (!form) form = Y5_CLASSIFY_HEAD_DEFAULT_FORM;
  hipStream_t st = static_cast<hipStream_t>(stream_);
  ClsHeadParams p{};
  p.x = x; p.w = w; p.bias = bias; p.logits = logits; p.B = B; p.HW = HW; p.C = C; p.ld = ld; p.nc = nc; p.ldo = ldo;
  if (form == 1) {
    const size_t lds = (size_t)C * 4 + (size_t)kClsParts * 256 * 8 * 4;
    if (dtype == Y5_F16) hipLaunchKernelGGL(y5_classify_head_fused_kernel<_Float16>, dim3(B), dim3(1024), lds, st, p);
    else hipLaunchKernelGGL(y5_classify_head_fused_kernel<float>, dim3(B), dim3(1024), lds, st, p);
    return y5_check_launch("y5_classify_head(one launch)");
  }
  if (!workspace || ((uintptr_t)workspace & 15) || workspace_bytes < y5_classify_head_workspace_bytes(B, C))
    return y5_fail(Y5_ERR_WORKSPACE, "classify_head: workspace missing, misaligned or smaller than y5_classify_head_workspace_bytes");
  p.pooled = static_cast<float*>(workspace);
  const dim3 gp((unsigned)((C / 8 + 63) / 64), (unsigned)B);
  const size_t lds_p = (size_t)kClsParts * 64 * 8 * 4;
  if (dtype == Y5_F16) hipLaunchKernelGGL(y5_classify_pool_kernel<_Float16>, gp, dim3(256), lds_p, st, p);
  else hipLaunchKernelGGL(y5_classify_pool_kernel<float>, gp, dim3(256), lds_p, st, p);
  int rc = y5_check_launch("y5_classify_head(pool)");
  if (rc) return rc;
  if (dtype == Y5_F16) {
    if ((nc + 31) / 32 > 0x7fffffff / 32) return y5_fail(Y5_ERR_UNSUPPORTED, "classify_head: nc too large");
    hipLaunchKernelGGL(y5_classify_gemm_f16_kernel, dim3((unsigned)((nc + 31) / 32), (unsigned)((B + 31) / 32)), dim3(256), (size_t)4 * 64 * 16 * 4, st, p);
  } else {
    hipLaunchKernelGGL(y5_classify_rows_f32_kernel, dim3((unsigned)((nc + 63) / 64), (unsigned)B), dim3(256), (size_t)C * 4, st, p);
  }
  return y5_check_launch("y5_classify_head(gemm)");
}

// ---- softmax / top-5 / cross-entropy ----------------------------------------------------------------------------------------------------------
namespace {
struct ClsPostParams {
  const void* logits; const int* labels; int* top5; float* probs; float* row_loss;
  int B, nc, ld; float eps;
};
constexpr int kClsPostMaxNc = 36864;   // nc fp32 values of LDS (144 KiB)

__device__ __forceinline__ float cls_wave_sum(float a, int lane) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) a += __shfl(a, lane ^ m);
  return a;
}
}  // namespace

// grid (B), 64 threads: one wave per row; lane l owns the columns l, l + 64, ... (ascending), lane sums meet in an xor butterfly
template <typename T>
__global__ __launch_bounds__(64)
void y5_classify_post_kernel(const ClsPostParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* z = reinterpret_cast<float*>(smem);
  const int b = blockIdx.x, lane = threadIdx.x, nc = p.nc;
  const T* row = static_cast<const T*>(p.logits) + (size_t)b * p.ld;
  float mx = -INFINITY, sz = 0.f;
  for (int i = lane; i < nc; i += 64) {
    const float v = (float)row[i];
    z[i] = v;
    mx = fmaxf(mx, v);
    sz += v;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) mx = fmaxf(mx, __shfl(mx, lane ^ m));
  sz = cls_wave_sum(sz, lane);
  __syncthreads();
  float se = 0.f;
  for (int i = lane; i < nc; i += 64) se += expf(z[i] - mx);
  se = cls_wave_sum(se, lane);
  if (p.probs)
    for (int i = lane; i < nc; i += 64) p.probs[(size_t)b * nc + i] = expf(z[i] - mx) / se;
  if (p.row_loss && lane == 0) {
    const float lse = mx + logf(se);
    const int y = p.labels[b];
    const float zy = y >= 0 && y < nc ? z[y] : NAN;   // (a label outside [0, nc) has no loss: NaN, visible in the mean)
    p.row_loss[b] = (1.f - p.eps) * (lse - zy) + p.eps * (lse - sz / (float)nc);
  }
  // ranking: five rounds of "largest value that comes AFTER the previous pick" in the order (value descending, index ascending)
  float pv = INFINITY;
  int pi = -1;
  for (int r = 0; r < 5; ++r) {
    float bv = 0.f;
    int bi = -1;
    for (int i = lane; i < nc; i += 64) {
      const float v = z[i];
      const bool after = v < pv || (v == pv && i > pi);
      if (after && (bi < 0 || v > bv)) { bv = v; bi = i; }   // (ascending i: an equal value never displaces an earlier index)
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const float ov = __shfl(bv, lane ^ m);
      const int oi = __shfl(bi, lane ^ m);
      if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
    }
    if (lane == 0) p.top5[b * 5 + r] = bi;
    if (bi < 0) { pv = -INFINITY; pi = 0x7fffffff; } else { pv = bv; pi = bi; }
  }
}

extern "C" int y5_classify_post(const void* logits, int dtype, int B, int nc, int ld, const int* labels, float label_smoothing, int* top5, float* probs,
                                float* row_loss, void* stream_) {
  if (!logits || !top5) return y5_fail(Y5_ERR_BAD_ARG, "classify_post: null pointer");
  if (dtype != Y5_F16 && dtype != Y5_F32) return y5_fail(Y5_ERR_BAD_ARG, "classify_post: logits must be f16 or f32");
  if (B < 1 || nc < 1 || ld < nc) return y5_fail(Y5_ERR_BAD_ARG, "classify_post: need B >= 1, nc >= 1, ld >= nc");
  if (!(label_smoothing >= 0.f && label_smoothing <= 1.f)) return y5_fail(Y5_ERR_BAD_ARG, "classify_post: label_smoothing must lie in [0, 1]");
  const int es = dtype == Y5_F16 ? 2 : 4;
  if (((uintptr_t)logits & (es - 1)) || ((uintptr_t)top5 & 3) || ((uintptr_t)probs & 3) || ((uintptr_t)row_loss & 3) || ((uintptr_t)labels & 3))
    return y5_fail(Y5_ERR_BAD_ARG, "classify_post: misaligned pointer");
  if (nc > kClsPostMaxNc || B > 0x7fffffff / 5) return y5_fail(Y5_ERR_UNSUPPORTED, "classify_post: nc <= 36864 (the row lives in LDS)");
  ClsPostParams p{};
  p.logits = logits; p.labels = labels; p.top5 = top5; p.probs = probs; p.row_loss = labels ? row_loss : nullptr; p.B = B; p.nc = nc; p.ld = ld;
  p.eps = label_smoothing;
  static bool attr_done = false;
  if (!attr_done) {
    hipFuncSetAttribute(reinterpret_cast<const void*>(y5_classify_post_kernel<_Float16>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipFuncSetAttribute(reinterpret_cast<const void*>(y5_classify_post_kernel<float>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr_done = true;
  }
  const size_t lds = (size_t)nc * 4;
  hipStream_t st = static_cast<hipStream_t>(stream_);
  if (dtype == Y5_F16) hipLaunchKernelGGL(y5_classify_post_kernel<_Float16>, dim3(B), dim3(64), lds, st, p);
  else hipLaunchKernelGGL(y5_classify_post_kernel<float>, dim3(B), dim3(64), lds, st, p);
  return y5_check_launch("y5_classify_post");
}
