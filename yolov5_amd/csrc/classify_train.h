// Training side of the classification head (included from head.hip behind classify.h, built with -ffp-contract=off): the train-mode
// forward of `linear(drop(pool(x).flatten(1)))` (models/common.py:1120-1140), its backward, and the gradient of
// nn.CrossEntropyLoss(label_smoothing) (utils/torch_utils.py:52-58, classify/train.py:214-219).
//
// y5_classify_head_train: form 2 of y5_classify_head (classify.h) with the pooled rows (B, C) fp32 in a buffer of the CALLER's -- the saved
//   activation of the backward -- and Dropout applied to them in place between the pool and the GEMM / row kernel:
//     launch 1  y5_classify_pool_kernel            pooled[b, c] = mean over the pixels (fp32)
//     launch 2  y5_classify_dropout_kernel         pooled[b, c] = keep(b, c) ? pooled[b, c] / (1 - p) : 0      (only when p > 0)
//     launch 3  y5_classify_gemm_f16_kernel / y5_classify_rows_f32_kernel
//   With p == 0 nothing else is launched and the logits are those of y5_classify_head(form = 2) bit for bit.
//
// Dropout mask: nn.Dropout(p) semantics (keep with probability 1 - p, kept values / (1 - p), p == 1 gives zeros) on a counter-based stream,
// so the backward regenerates the mask from (seed, element index) instead of storing it.  Philox4x32-10 (Salmon, Moraes, Dror, Shaw:
// "Parallel random numbers: as easy as 1, 2, 3", SC'11) with
//     key     = (k0, k1) = (seed & 0xffffffff, seed >> 32)
//     counter = (c0, c1, c2, c3) = (i & 0xffffffff, i >> 32, 0, 0),   i = b * C + c   (64-bit element index)
//     round   : hi0:lo0 = 0xD2511F53 * c0, hi1:lo1 = 0xCD9E8D57 * c2;  (c0, c1, c2, c3) <- (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0)
//     ten rounds; before each round but the first the key is bumped by (0x9E3779B9, 0xBB67AE85)
//     r       = c0 after the tenth round;  u = (r >> 8) * 2^-24 (exact in fp32);  keep <=> u >= p (compared in fp32)
// This is NOT torch's Dropout stream (whose CPU and CUDA streams differ from each other as well): runs repeat under the same seed, they do
// not reproduce the reference's masks.
//
// y5_classify_head_bwd: three launches, no atomics, every sum in an order fixed by (B, nc, C, HW):
//     launch 1  dW[j, c] = sum_b dlogits[b, j] * pooled_d[b, c]  (b ascending),  dbias[j] = sum_b dlogits[b, j]  (b ascending, fp32)
//               fp16: one 32 (classes) x 32 (channels) MFMA tile per wave, K = images in steps of 16; the fp32 pooled_d enters as hi + lo fp16
//               halves like the forward's (two v_mfma_f32_32x32x16_f16 per step), each channel's column scaled by a power of two first so
//               that lo does not underflow; fp32: plain FMAs, a thread per (16 classes, channel)
//     launch 2  g[b, c] = keep(b, c) ? (sum_j dlogits[b, j] * w[j, c]) / (1 - p) / HW : 0   into the workspace (fp32)
//               fp16: a 32 (images) x 32 (channels) MFMA tile per workgroup, K = classes split over its four waves and added in wave order
//               (both operands are fp16: one MFMA per step); fp32: plain FMAs over j ascending, a thread per (image, channel)
//     launch 3  dx[b, pixel, c] = (T) g[b, c] at every pixel of image b  (Dropout and the pool are elementwise / a mean: one value per image)
//   g[b, :] depends on row b of dlogits alone: dx of an image equals the single-row call bit for bit.
//
// y5_classify_ce_bwd: one wave per row, the row in LDS as fp32 (as y5_classify_post_kernel): recomputes max and sum exp, then
//     dlogits[b, j] = grad_rows[b] * (exp(z_j - max) / sum - (1 - eps) [j == y_b] - eps / nc)
//   in the logits' dtype.  A label outside [0, nc) gives a NaN row (the forward's loss of that row is NaN as well).
#pragma once
#include <hip/hip_runtime.h>

#include "classify.h"

namespace {
__device__ __forceinline__ unsigned cls_philox(unsigned long long seed, unsigned long long i) {
  unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
  unsigned c0 = (unsigned)i, c1 = (unsigned)(i >> 32), c2 = 0u, c3 = 0u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    if (r) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
    const unsigned long long m0 = 0xD2511F53ull * c0, m1 = 0xCD9E8D57ull * c2;
    const unsigned n0 = (unsigned)(m1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(m0 >> 32) ^ c3 ^ k1;
    c1 = (unsigned)m1; c3 = (unsigned)m0; c0 = n0; c2 = n2;
  }
  return c0;
}

// nn.Dropout's keep decision of element i (p == 0 keeps everything without a draw; p == 1 keeps nothing: u < 1 always)
__device__ __forceinline__ bool cls_keep(unsigned long long seed, unsigned long long i, float p) {
  return p <= 0.f || (float)(cls_philox(seed, i) >> 8) * 5.9604644775390625e-08f >= p;
}

struct ClsHeadBwdParams {
  const void* dlogits; const float* pooled; const void* w; float* dbias; float* dw; float* g; void* dx;
  int B, HW, C, ld, nc, ldd; float p; unsigned long long seed;
};

struct ClsCeBwdParams {
  const void* logits; const int* labels; const float* grad_rows; void* dlogits;
  int B, nc, ld, ldd; float eps;
};
}  // namespace

// grid (ceil(n / 256)), 256 threads: pooled[i] for i < n = B * C
__global__ __launch_bounds__(256)
void y5_classify_dropout_kernel(float* pooled, long long n, float p, unsigned long long seed) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  pooled[i] = cls_keep(seed, (unsigned long long)i, p) ? pooled[i] / (1.f - p) : 0.f;
}

// launch 1, fp16: grid (ceil(C / 128), ceil(nc / 32)), 256 threads: wave wv owns the tile classes j0.., channels c0 + 32 wv..
// D = dlogits^T(32 classes x 16 images) * pooled_d(16 images x 32 channels): lane l supplies dlogits[k0 + 8 (l / 32) ..][j0 + l % 32] and
// pooled_d[the same images][c0 + l % 32]; it receives, for channel c0 + l % 32, the classes j0 + (r % 4) + 8 (r / 4) + 4 (l / 32), r = 0..15.
__global__ __launch_bounds__(256)
void y5_classify_dw_f16_kernel(const ClsHeadBwdParams p) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int j0 = blockIdx.y * 32, c0 = blockIdx.x * 128 + wv * 32;
  const _Float16* dl = static_cast<const _Float16*>(p.dlogits);
  if (blockIdx.x == 0 && threadIdx.x < 32 && j0 + (int)threadIdx.x < p.nc) {
    float s = 0.f;
    for (int b = 0; b < p.B; ++b) s += (float)dl[(size_t)b * p.ldd + j0 + threadIdx.x];
    p.dbias[j0 + threadIdx.x] = s;
  }
  if (c0 >= p.C) return;
  const int jr = j0 + (lane & 31) < p.nc ? j0 + (lane & 31) : p.nc - 1;   // (classes / channels past the end repeat the last one; never stored)
  const int cr = c0 + (lane & 31) < p.C ? c0 + (lane & 31) : p.C - 1;
  // The hi + lo split holds 22 bits of a value only while lo stays a normal fp16 number.  A weight gradient has just B terms per output, so a
  // small pooled value is not hidden behind larger terms as in the forward's sum over the channels: the column is scaled by a power of two that
  // brings its largest magnitude to [2^13, 2^14) (exact; undone on the result), which keeps every value within 2^-17 of that maximum at 22 bits.
  float mx = 0.f;
  for (int b = 0; b < p.B; ++b) mx = fmaxf(mx, fabsf(p.pooled[(size_t)b * p.C + cr]));
  int ex = 0;
  if (mx > 0.f && mx <= 3.0e38f) frexpf(mx, &ex); else ex = 14;
  if (ex < -100) ex = -100;
  const float sc = ldexpf(1.f, 14 - ex), inv_sc = ldexpf(1.f, ex - 14);
  float16_t acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (int k0 = 0; k0 < p.B; k0 += 16) {
    half8_t a, hi, lo;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int b = k0 + 8 * (lane >> 5) + e;
      if (b < p.B) {
        a[e] = dl[(size_t)b * p.ldd + jr];
        const float v = p.pooled[(size_t)b * p.C + cr] * sc;
        hi[e] = (_Float16)v;
        lo[e] = (_Float16)(v - (float)hi[e]);
      } else {
        a[e] = (_Float16)0.f; hi[e] = (_Float16)0.f; lo[e] = (_Float16)0.f;
      }
    }
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, hi, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, lo, acc, 0, 0, 0);
  }
  if (c0 + (lane & 31) < p.C) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int j = j0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      if (j < p.nc) p.dw[(size_t)j * p.C + c0 + (lane & 31)] = acc[r] * inv_sc;
    }
  }
}

// launch 1, fp32: grid (ceil(C / 128), ceil(nc / 32)), 256 threads: thread (t % 128, t / 128) walks the images for channel c0 + t % 128 and the
// sixteen classes j0 + 16 (t / 128) ..
__global__ __launch_bounds__(256)
void y5_classify_dw_f32_kernel(const ClsHeadBwdParams p) {
  const int j0 = blockIdx.y * 32, c = blockIdx.x * 128 + (threadIdx.x & 127), jb = j0 + 16 * (threadIdx.x >> 7);
  const float* dl = static_cast<const float*>(p.dlogits);
  if (blockIdx.x == 0 && threadIdx.x < 32 && j0 + (int)threadIdx.x < p.nc) {
    float s = 0.f;
    for (int b = 0; b < p.B; ++b) s += dl[(size_t)b * p.ldd + j0 + threadIdx.x];
    p.dbias[j0 + threadIdx.x] = s;
  }
  if (c >= p.C || jb >= p.nc) return;
  float acc[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (int b = 0; b < p.B; ++b) {
    const float v = p.pooled[(size_t)b * p.C + c];
    const float* row = dl + (size_t)b * p.ldd;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = fmaf(row[jb + r < p.nc ? jb + r : p.nc - 1], v, acc[r]);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r)
    if (jb + r < p.nc) p.dw[(size_t)(jb + r) * p.C + c] = acc[r];
}

// launch 2, fp16: grid (ceil(C / 32), ceil(B / 32)), 256 threads; LDS: partial tiles [4][64][16].
// D = w^T(32 channels x 16 classes) * dlogits^T(16 classes x 32 images): lane l supplies w[k0 + 8 (l / 32) ..][c0 + l % 32] and
// dlogits[b0 + l % 32][the same classes]; it receives, for image b0 + l % 32, the channels c0 + (r % 4) + 8 (r / 4) + 4 (l / 32), r = 0..15.
__global__ __launch_bounds__(256)
void y5_classify_dpool_f16_kernel(const ClsHeadBwdParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* tiles = reinterpret_cast<float*>(smem);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int c0 = blockIdx.x * 32, b0 = blockIdx.y * 32;
  const int cr = c0 + (lane & 31) < p.C ? c0 + (lane & 31) : p.C - 1;   // (channels / images past the end repeat the last one; never stored)
  const int br = b0 + (lane & 31) < p.B ? b0 + (lane & 31) : p.B - 1;
  const _Float16* wcol = static_cast<const _Float16*>(p.w) + cr;
  const _Float16* drow = static_cast<const _Float16*>(p.dlogits) + (size_t)br * p.ldd;
  const int nsteps = (p.nc + 15) / 16, per = (nsteps + 3) / 4;
  const int s0 = wv * per, s1 = s0 + per < nsteps ? s0 + per : nsteps;
  float16_t acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (int s = s0; s < s1; ++s) {
    half8_t a, d;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int j = s * 16 + 8 * (lane >> 5) + e;
      if (j < p.nc) { a[e] = wcol[(size_t)j * p.C]; d[e] = drow[j]; }
      else { a[e] = (_Float16)0.f; d[e] = (_Float16)0.f; }
    }
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, d, acc, 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) tiles[(wv * 64 + lane) * 16 + r] = acc[r];
  __syncthreads();
  if (wv == 0 && b0 + (lane & 31) < p.B) {
    const int b = b0 + (lane & 31);
    const float n = (float)p.HW;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int c = c0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      const float s = ((tiles[lane * 16 + r] + tiles[(64 + lane) * 16 + r]) + tiles[(128 + lane) * 16 + r]) + tiles[(192 + lane) * 16 + r];
      if (c < p.C) {
        const size_t i = (size_t)b * p.C + c;
        p.g[i] = cls_keep(p.seed, i, p.p) ? s / (1.f - p.p) / n : 0.f;
      }
    }
  }
}

// launch 2, fp32: grid (ceil(C / 256), B), 256 threads: a thread per (image, channel), classes ascending
__global__ __launch_bounds__(256)
void y5_classify_dpool_f32_kernel(const ClsHeadBwdParams p) {
  const int b = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
  if (c >= p.C) return;
  const float* drow = static_cast<const float*>(p.dlogits) + (size_t)b * p.ldd;
  const float* wcol = static_cast<const float*>(p.w) + c;
  float s = 0.f;
  for (int j = 0; j < p.nc; ++j) s = fmaf(drow[j], wcol[(size_t)j * p.C], s);
  const size_t i = (size_t)b * p.C + c;
  p.g[i] = cls_keep(p.seed, i, p.p) ? s / (1.f - p.p) / (float)p.HW : 0.f;
}

// launch 3: grid (ceil(C / 8 / 256), min(HW, 64), B), 256 threads: a thread per channel octet of image b, pixels blockIdx.y, + gridDim.y, ...
template <typename T>
__global__ __launch_bounds__(256)
void y5_classify_dx_kernel(const ClsHeadBwdParams p) {
  const int oct = blockIdx.x * 256 + threadIdx.x, b = blockIdx.z;
  if (oct * 8 >= p.C) return;
  float v[8];
  cls_load8<float>(p.g + (size_t)b * p.C + oct * 8, v);
  T* out = static_cast<T*>(p.dx) + (size_t)b * p.HW * p.ld + oct * 8;
  if constexpr (sizeof(T) == 2) {
    half8_t h;
#pragma unroll
    for (int e = 0; e < 8; ++e) h[e] = (_Float16)v[e];
    for (int px = blockIdx.y; px < p.HW; px += gridDim.y) *reinterpret_cast<half8_t*>(out + (size_t)px * p.ld) = h;
  } else {
    float4_t a, c;
#pragma unroll
    for (int e = 0; e < 4; ++e) { a[e] = v[e]; c[e] = v[4 + e]; }
    for (int px = blockIdx.y; px < p.HW; px += gridDim.y) {
      *reinterpret_cast<float4_t*>(out + (size_t)px * p.ld) = a;
      *reinterpret_cast<float4_t*>(out + (size_t)px * p.ld + 4) = c;
    }
  }
}

extern "C" int y5_classify_head_train(const void* x, int dtype, int B, int HW, int C, int ld, const void* w, const float* bias, int nc, void* logits,
                                      int ldo, float* pooled, size_t pooled_bytes, float p_drop, unsigned long long seed, void* stream_) {
  if (!x || !w || !bias || !logits) return y5_fail(Y5_ERR_BAD_ARG, "classify_head_train: null pointer");
  if (dtype != Y5_F16 && dtype != Y5_F32) return y5_fail(Y5_ERR_BAD_ARG, "classify_head_train: dtype must be f16 or f32");
  if (B < 1 || HW < 1 || C < 1 || nc < 1 || ld < C || ldo < nc) return y5_fail(Y5_ERR_BAD_ARG, "classify_head_train: need B, HW, C, nc >= 1, ld >= C, ldo >= nc");
  if (!(p_drop >= 0.f && p_drop <= 1.f)) return y5_fail(Y5_ERR_BAD_ARG, "classify_head_train: the Dropout probability must lie in [0, 1]");
  const int es = dtype == Y5_F16 ? 2 : 4;
  if (((uintptr_t)x | (uintptr_t)w) & 15 || ((uintptr_t)bias & 3) || ((uintptr_t)logits & (es - 1)))
    return y5_fail(Y5_ERR_BAD_ARG, "classify_head_train: x and w must be 16-byte aligned");
  if ((C & 7) || ((size_t)ld * es & 15)) return y5_fail(Y5_ERR_UNSUPPORTED, "classify_head_train: needs C % 8 == 0 and pixel rows of a multiple of 16 bytes");
  if (C > kClsMaxC || B > 65535 || (long long)B * HW * ld * es >= (1LL << 40)) return y5_fail(Y5_ERR_UNSUPPORTED, "classify_head_train: C <= 8192, B <= 65535");
  if (!pooled || ((uintptr_t)pooled & 15) || pooled_bytes < y5_classify_head_workspace_bytes(B, C))
    return y5_fail(Y5_ERR_WORKSPACE, "classify_head_train: pooled buffer missing, misaligned or smaller than y5_classify_head_workspace_bytes");
  hipStream_t st = static_cast<hipStream_t>(stream_);
  ClsHeadParams p{};
  p.x = x; p.w = w; p.bias = bias; p.logits = logits; p.B = B; p.HW = HW; p.C = C; p.ld = ld; p.nc = nc; p.ldo = ldo; p.pooled = pooled;
  const dim3 gp((unsigned)((C / 8 + 63) / 64), (unsigned)B);
  const size_t lds_p = (size_t)kClsParts * 64 * 8 * 4;
  if (dtype == Y5_F16) hipLaunchKernelGGL(y5_classify_pool_kernel<_Float16>, gp, dim3(256), lds_p, st, p);
  else hipLaunchKernelGGL(y5_classify_pool_kernel<float>, gp, dim3(256), lds_p, st, p);
  int rc = y5_check_launch("y5_classify_head_train(pool)");
  if (rc) return rc;
  if (p_drop > 0.f) {
    const long long n = (long long)B * C;
    hipLaunchKernelGGL(y5_classify_dropout_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, pooled, n, p_drop, seed);
    rc = y5_check_launch("y5_classify_head_train(dropout)");
    if (rc) return rc;
  }
  if (dtype == Y5_F16) {
    if ((nc + 31) / 32 > 0x7fffffff / 32) return y5_fail(Y5_ERR_UNSUPPORTED, "classify_head_train: nc too large");
    hipLaunchKernelGGL(y5_classify_gemm_f16_kernel, dim3((unsigned)((nc + 31) / 32), (unsigned)((B + 31) / 32)), dim3(256), (size_t)4 * 64 * 16 * 4, st, p);
  } else {
    hipLaunchKernelGGL(y5_classify_rows_f32_kernel, dim3((unsigned)((nc + 63) / 64), (unsigned)B), dim3(256), (size_t)C * 4, st, p);
  }
  return y5_check_launch("y5_classify_head_train(gemm)");
}

extern "C" int y5_classify_head_bwd(const void* dlogits, int dtype, int B, int nc, int ldd, const float* pooled_d, const void* w, int HW, int C,
                                    float p_drop, unsigned long long seed, float* dbias, float* dw, void* dx, int ld, void* workspace,
                                    size_t workspace_bytes, void* stream_) {
  if (!dlogits || !pooled_d || !w || !dbias || !dw || !dx) return y5_fail(Y5_ERR_BAD_ARG, "classify_head_bwd: null pointer");
  if (dtype != Y5_F16 && dtype != Y5_F32) return y5_fail(Y5_ERR_BAD_ARG, "classify_head_bwd: dtype must be f16 or f32");
  if (B < 1 || HW < 1 || C < 1 || nc < 1 || ld < C || ldd < nc) return y5_fail(Y5_ERR_BAD_ARG, "classify_head_bwd: need B, HW, C, nc >= 1, ld >= C, ldd >= nc");
  if (!(p_drop >= 0.f && p_drop <= 1.f)) return y5_fail(Y5_ERR_BAD_ARG, "classify_head_bwd: the Dropout probability must lie in [0, 1]");
  const int es = dtype == Y5_F16 ? 2 : 4;
  if (((uintptr_t)dx | (uintptr_t)w | (uintptr_t)pooled_d) & 15 || (((uintptr_t)dbias | (uintptr_t)dw) & 3) || ((uintptr_t)dlogits & (es - 1)))
    return y5_fail(Y5_ERR_BAD_ARG, "classify_head_bwd: dx, w and pooled_d must be 16-byte aligned");
  if ((C & 7) || ((size_t)ld * es & 15)) return y5_fail(Y5_ERR_UNSUPPORTED, "classify_head_bwd: needs C % 8 == 0 and pixel rows of a multiple of 16 bytes");
  if (C > kClsMaxC || B > 65535 || (long long)B * HW * ld * es >= (1LL << 40) || (nc + 31) / 32 > 65535)
    return y5_fail(Y5_ERR_UNSUPPORTED, "classify_head_bwd: C <= 8192, B <= 65535, nc <= 2097120");
  if (!workspace || ((uintptr_t)workspace & 15) || workspace_bytes < y5_classify_head_workspace_bytes(B, C))
    return y5_fail(Y5_ERR_WORKSPACE, "classify_head_bwd: workspace missing, misaligned or smaller than y5_classify_head_workspace_bytes");
  hipStream_t st = static_cast<hipStream_t>(stream_);
  ClsHeadBwdParams p{};
  p.dlogits = dlogits; p.pooled = pooled_d; p.w = w; p.dbias = dbias; p.dw = dw; p.g = static_cast<float*>(workspace); p.dx = dx;
  p.B = B; p.HW = HW; p.C = C; p.ld = ld; p.nc = nc; p.ldd = ldd; p.p = p_drop; p.seed = seed;
  const dim3 gw((unsigned)((C + 127) / 128), (unsigned)((nc + 31) / 32));
  if (dtype == Y5_F16) hipLaunchKernelGGL(y5_classify_dw_f16_kernel, gw, dim3(256), 0, st, p);
  else hipLaunchKernelGGL(y5_classify_dw_f32_kernel, gw, dim3(256), 0, st, p);
  int rc = y5_check_launch("y5_classify_head_bwd(dW)");
  if (rc) return rc;
  if (dtype == Y5_F16)
    hipLaunchKernelGGL(y5_classify_dpool_f16_kernel, dim3((unsigned)((C + 31) / 32), (unsigned)((B + 31) / 32)), dim3(256), (size_t)4 * 64 * 16 * 4, st, p);
  else hipLaunchKernelGGL(y5_classify_dpool_f32_kernel, dim3((unsigned)((C + 255) / 256), (unsigned)B), dim3(256), 0, st, p);
  rc = y5_check_launch("y5_classify_head_bwd(dpooled)");
  if (rc) return rc;
  const dim3 gx((unsigned)((C / 8 + 255) / 256), (unsigned)(HW < 64 ? HW : 64), (unsigned)B);
  if (dtype == Y5_F16) hipLaunchKernelGGL(y5_classify_dx_kernel<_Float16>, gx, dim3(256), 0, st, p);
  else hipLaunchKernelGGL(y5_classify_dx_kernel<float>, gx, dim3(256), 0, st, p);
  return y5_check_launch("y5_classify_head_bwd(dx)");
}

// grid (B), 64 threads: one wave per row; lane l owns the columns l, l + 64, ... (ascending), lane sums meet in an xor butterfly
template <typename T>
__global__ __launch_bounds__(64)
void y5_classify_ce_bwd_kernel(const ClsCeBwdParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* z = reinterpret_cast<float*>(smem);
  const int b = blockIdx.x, lane = threadIdx.x, nc = p.nc;
  const T* row = static_cast<const T*>(p.logits) + (size_t)b * p.ld;
  float mx = -INFINITY;
  for (int i = lane; i < nc; i += 64) {
    const float v = (float)row[i];
    z[i] = v;
    mx = fmaxf(mx, v);
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) mx = fmaxf(mx, __shfl(mx, lane ^ m));
  __syncthreads();
  float se = 0.f;
  for (int i = lane; i < nc; i += 64) se += expf(z[i] - mx);
  se = cls_wave_sum(se, lane);
  const int y = p.labels[b];
  const float g = y >= 0 && y < nc ? p.grad_rows[b] : NAN;
  const float off = p.eps / (float)nc, on = 1.f - p.eps;
  T* out = static_cast<T*>(p.dlogits) + (size_t)b * p.ldd;
  for (int i = lane; i < nc; i += 64) out[i] = (T)(g * ((expf(z[i] - mx) / se - (i == y ? on : 0.f)) - off));
}

extern "C" int y5_classify_ce_bwd(const void* logits, int dtype, int B, int nc, int ld, const int* labels, float label_smoothing, const float* grad_rows,
                                  void* dlogits, int ldd, void* stream_) {
  if (!logits || !labels || !grad_rows || !dlogits) return y5_fail(Y5_ERR_BAD_ARG, "classify_ce_bwd: null pointer");
  if (dtype != Y5_F16 && dtype != Y5_F32) return y5_fail(Y5_ERR_BAD_ARG, "classify_ce_bwd: logits must be f16 or f32");
  if (B < 1 || nc < 1 || ld < nc || ldd < nc) return y5_fail(Y5_ERR_BAD_ARG, "classify_ce_bwd: need B >= 1, nc >= 1, ld >= nc, ldd >= nc");
  if (!(label_smoothing >= 0.f && label_smoothing <= 1.f)) return y5_fail(Y5_ERR_BAD_ARG, "classify_ce_bwd: label_smoothing must lie in [0, 1]");
  const int es = dtype == Y5_F16 ? 2 : 4;
  if ((((uintptr_t)logits | (uintptr_t)dlogits) & (es - 1)) || (((uintptr_t)labels | (uintptr_t)grad_rows) & 3))
    return y5_fail(Y5_ERR_BAD_ARG, "classify_ce_bwd: misaligned pointer");
  if (nc > kClsPostMaxNc) return y5_fail(Y5_ERR_UNSUPPORTED, "classify_ce_bwd: nc <= 36864 (the row lives in LDS)");
  ClsCeBwdParams p{};
  p.logits = logits; p.labels = labels; p.grad_rows = grad_rows; p.dlogits = dlogits; p.B = B; p.nc = nc; p.ld = ld; p.ldd = ldd; p.eps = label_smoothing;
  static bool attr_done = false;
  if (!attr_done) {
    hipFuncSetAttribute(reinterpret_cast<const void*>(y5_classify_ce_bwd_kernel<_Float16>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipFuncSetAttribute(reinterpret_cast<const void*>(y5_classify_ce_bwd_kernel<float>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr_done = true;
  }
  hipStream_t st = static_cast<hipStream_t>(stream_);
  if (dtype == Y5_F16) hipLaunchKernelGGL(y5_classify_ce_bwd_kernel<_Float16>, dim3(B), dim3(64), (size_t)nc * 4, st, p);
  else hipLaunchKernelGGL(y5_classify_ce_bwd_kernel<float>, dim3(B), dim3(64), (size_t)nc * 4, st, p);
  return y5_check_launch("y5_classify_ce_bwd");
}
