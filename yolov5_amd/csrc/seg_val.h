// Mask validation matching on the device: the mask branch of process_batch (utils/metrics.py:239-249, masks=True) for every image of a batch
// in ONE C-ABI call, as segment/val.py:287-308 runs it per image:
//     gt_masks = masks[[si]] (overlap) | masks[targets[:, 0] == si]                                       segment/val.py:287-288
//     pred_masks = process_mask(proto, pred[:, 6:], pred[:, :4], shape=im.shape[2:])  (upsample=False)    :289
//     overlap: gt_masks = where(gt_masks.repeat(nl, 1, 1) == arange(nl) + 1, 1., 0.)                     utils/metrics.py:241-245
//     gt_masks = interpolate(gt_masks[None], pred_masks.shape[1:], bilinear, align_corners=False).gt_(0.5)   :246-248 (shapes differ)
//     iou = mask_iou(gt_masks, pred_masks)  -> the threshold / uniqueness scan of process_batch            :250-265
// Included by mask.hip, so it is compiled with mask.hip's flags: the predicted bits come from y5_mask_lowres (mask_value.h), the same
// function and the same FMA contraction as y5_process_mask_batch(upsample=0).  The matching itself has no product to contract: IoU is
// (float)inter / ((float)(a + b - inter) + 1e-7f) over exact integer pixel counts -- the fp32 matmul and sums of mask_iou over 0/1 values are
// exact integers below 2^24, so this IS the reference's value -- and the scan only compares.
//
// Three launches, no host synchronisation, no float atomics:
//   1. one workgroup per label row: its rank among the labels of its image (overlap index rank + 1) and its area at the prediction resolution;
//   2. one workgroup per (detection, image): detections with no label of their class in the image stop at once (row all 0).  Otherwise the
//      prediction's bits are built over its crop box (computed mode) or the whole grid (loaded mode) as 64-bit words in LDS, one ballot per
//      word; then, for every class-matched label in target order, the ground-truth bits are decoded at the prediction's set bits only and
//      the intersection is a popcount of a ballot.  Best label l*(d) and iou*(d) with metrics.hip's tie rule (the later label wins);
//   3. one workgroup per image: metrics.hip's threshold scan, correct[d, i] = iou*(d) >= iouv[i] and no d' < d with l*(d') == l*(d) passing.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/yolov5_hip.h"
#include "mask_value.h"
#include "y5_common.h"
#include "y5_host.h"

namespace segval {
constexpr int NT = 256;              // threads per workgroup
constexpr int NW = NT / 64;          // waves per workgroup
constexpr int MAX_WORDS = 4096;      // 64-bit words of one prediction bitmap in LDS (32 KB): mh * ceil(mw / 64) <= MAX_WORDS

struct Params {
  const float* det;           // (bs, max_det, ld_det) rows x1,y1,x2,y2,conf,cls,coef[nm] in letterboxed pixels
  const int* det_count;       // (bs) or nullptr
  const float* lab;           // (M, ld_lab)
  const void* gt;             // (bs | M, gh, gw)
  const void* protos;         // (bs, nm, mh, mw) or nullptr
  const unsigned char* pm;    // (bs, max_det, mh, mw) or nullptr
  const float* iouv;
  unsigned char* correct;     // (bs, max_det, niou)
  int* w_rank;                // (M) rank of the label among its image's labels, -1: no image of this batch
  int* w_area;                // (M) ground-truth area at (mh, mw)
  int* w_best;                // (bs, max_det) l*(d) as a label row, -1 none
  float* w_iou;               // (bs, max_det) iou*(d)
  int bs, max_det, ld_det, M, ld_lab, img_col, cls_col;
  int gt_dtype, overlap, gh, gw, resize;
  int proto_dtype, nm, mh, mw;
  int niou;
  float sx, sy;               // mw / iw, mh / ih (general.py:42-46)
  float rh, rw;               // gh / mh, gw / mw: source pixels per destination pixel of the ground-truth resize
};

// sum over the workgroup (every thread calls it; s_part holds NW ints)
__device__ inline int block_sum(int v, int* s_part) {
  const int lane = threadIdx.x & 63;
  for (int k = 32; k >= 1; k >>= 1) v += __shfl(v, lane ^ k);
  __syncthreads();
  if (lane == 0) s_part[threadIdx.x >> 6] = v;
  __syncthreads();
  int t = 0;
#pragma unroll
  for (int w = 0; w < NW; ++w) t += s_part[w];
  return t;
}

// image of a label row: -1 unless it is an integer in [0, bs)
__device__ inline int label_image(const Params& p, int t) {
  if (p.img_col < 0) return 0;
  const float f = p.lab[(long long)t * p.ld_lab + p.img_col];
  return (f >= 0.f && f < (float)p.bs && f == floorf(f)) ? (int)f : -1;
}

// 0/1 indicator of ground-truth element `off` of `base`: overlap maps select the value `want` (torch.where(gt == index), utils/metrics.py:245),
// per-instance masks are foreground where non-zero
__device__ inline int gt_ind(const Params& p, const void* base, long long off, int want) {
  if (p.gt_dtype == Y5_U8) {
    const int v = static_cast<const unsigned char*>(base)[off];
    return p.overlap ? v == want : v != 0;
  }
  if (p.gt_dtype == Y5_I32) {
    const int v = static_cast<const int*>(base)[off];
    return p.overlap ? v == want : v != 0;
  }
  const float v = static_cast<const float*>(base)[off];
  return p.overlap ? v == (float)want : v != 0.f;
}

// ground-truth bit at prediction pixel (x, y): the indicator itself, or F.interpolate(bilinear, align_corners=False) of the indicator and > 0.5
// (utils/metrics.py:246-248) in upsample_bilinear2d's arithmetic -- source index max(scale * (dst + 0.5) - 0.5, 0), its floor capped at the
// last row / column, the weights of mask.hip's upsampling path
__device__ inline int gt_bit(const Params& p, const void* base, int want, int x, int y) {
  if (!p.resize) return gt_ind(p, base, (long long)y * p.gw + x, want);
  const float h1r = fmaxf(p.rh * ((float)y + 0.5f) - 0.5f, 0.f);
  const int h = (int)h1r < p.gh - 1 ? (int)h1r : p.gh - 1;
  const int hp = h < p.gh - 1 ? 1 : 0;
  const float hl1 = fminf(fmaxf(h1r - (float)h, 0.f), 1.f), hl0 = 1.0f - hl1;
  const float w1r = fmaxf(p.rw * ((float)x + 0.5f) - 0.5f, 0.f);
  const int w = (int)w1r < p.gw - 1 ? (int)w1r : p.gw - 1;
  const int wp = w < p.gw - 1 ? 1 : 0;
  const float wl1 = fminf(fmaxf(w1r - (float)w, 0.f), 1.f), wl0 = 1.0f - wl1;
  const long long r0 = (long long)h * p.gw, r1 = (long long)(h + hp) * p.gw;
  const float v00 = (float)gt_ind(p, base, r0 + w, want), v01 = (float)gt_ind(p, base, r0 + w + wp, want);
  const float v10 = (float)gt_ind(p, base, r1 + w, want), v11 = (float)gt_ind(p, base, r1 + w + wp, want);
  const float val = hl0 * (wl0 * v00 + wl1 * v01) + hl1 * (wl0 * v10 + wl1 * v11);
  return val > 0.5f;
}

// ground-truth plane and selected value of label row t (rank >= 0)
__device__ inline const void* gt_plane(const Params& p, int t, int img, int rank, int& want) {
  const size_t esz = p.gt_dtype == Y5_U8 ? 1 : 4;
  const long long plane = (long long)p.gh * p.gw;
  want = rank + 1;
  return static_cast<const char*>(p.gt) + (size_t)(p.overlap ? img : t) * plane * esz;
}
}  // namespace segval

// 1. per label row: rank within its image and area at the prediction resolution
__global__ __launch_bounds__(256)
void y5_val_mask_labels_kernel(const segval::Params p) {
  using namespace segval;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int* s_part = reinterpret_cast<int*>(smem);   // [NW]
  const int t = blockIdx.x, tid = threadIdx.x;
  const int img = label_image(p, t);
  int c = 0;
  if (img >= 0 && p.img_col >= 0) {
    const float f = p.lab[(long long)t * p.ld_lab + p.img_col];
    for (int u = tid; u < t; u += NT) c += p.lab[(long long)u * p.ld_lab + p.img_col] == f ? 1 : 0;
  }
  const int rank = p.img_col >= 0 ? block_sum(c, s_part) : t;
  int a = 0;
  if (img >= 0) {
    int want;
    const void* base = gt_plane(p, t, img, rank, want);
    for (int i = tid; i < p.mh * p.mw; i += NT) {
      const int y = i / p.mw, x = i - y * p.mw;
      a += gt_bit(p, base, want, x, y);
    }
  }
  a = block_sum(a, s_part);
  if (tid == 0) {
    p.w_rank[t] = img >= 0 ? rank : -1;
    p.w_area[t] = a;
  }
}

// 2. per (detection, image): best class-matched label by mask IoU
template <typename TP>
__global__ __launch_bounds__(256)
void y5_val_mask_best_kernel(const segval::Params p) {
  using namespace segval;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int* s_part = reinterpret_cast<int*>(smem);                                   // [NW] (16 bytes)
  int* s_flag = s_part + 4;                                                     // [NT] class-matched labels of the current tile
  float* s_coef = reinterpret_cast<float*>(s_flag + NT);                        // [256] coefficients (computed mode)
  unsigned long long* s_bits = reinterpret_cast<unsigned long long*>(s_coef + 256);  // [units] prediction bits
  const int d = blockIdx.x, si = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int n = p.det_count ? p.det_count[si] : p.max_det;
  n = n < 0 ? 0 : (n > p.max_det ? p.max_det : n);
  if (d >= n) return;  // workgroup-uniform; the scan writes these rows as 0
  const float* row = p.det + ((long long)si * p.max_det + d) * p.ld_det;
  const float cls = row[5];
  const float fsi = (float)si;
  // class filter first: correct_class = labels[:, 0:1] == detections[:, 5] (utils/metrics.py:255)
  int any = 0;
  for (int t = tid; t < p.M; t += NT) {
    const float* l = p.lab + (long long)t * p.ld_lab;
    any |= (p.img_col < 0 ? si == 0 : l[p.img_col] == fsi) && l[p.cls_col] == cls && p.w_rank[t] >= 0;
  }
  if (block_sum(any, s_part) == 0) {
    if (tid == 0) { p.w_best[(long long)si * p.max_det + d] = -1; p.w_iou[(long long)si * p.max_det + d] = -1.f; }
    return;
  }
  // the prediction's bits over a region that holds all of them: its crop box (computed) or the whole grid (loaded)
  int rx0 = 0, ry0 = 0, rx1 = p.mw, ry1 = p.mh;
  float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f;
  if (p.protos) {
    x1 = row[0] * p.sx; y1 = row[1] * p.sy; x2 = row[2] * p.sx; y2 = row[3] * p.sy;  // general.py:42-46
    if (x1 < x2 && y1 < y2) {  // (NaN-safe: a crop with no pixel keeps the empty region)
      rx0 = (int)fminf(fmaxf(floorf(x1), 0.f), (float)p.mw); rx1 = (int)fminf(fmaxf(ceilf(x2) + 1.f, 0.f), (float)p.mw);
      ry0 = (int)fminf(fmaxf(floorf(y1), 0.f), (float)p.mh); ry1 = (int)fminf(fmaxf(ceilf(y2) + 1.f, 0.f), (float)p.mh);
    } else {
      rx1 = rx0; ry1 = ry0;
    }
    for (int i = tid; i < p.nm; i += NT) s_coef[i] = row[6 + i];
    __syncthreads();
  }
  const int wpr = rx1 > rx0 ? (rx1 - rx0 + 63) >> 6 : 0;
  const int units = ry1 > ry0 ? (ry1 - ry0) * wpr : 0;
  const long long plane = (long long)p.mh * p.mw;
  int pa = 0;
  for (int u = wave; u < units; u += NW) {
    const int ry = u / wpr, x = rx0 + (u - ry * wpr) * 64 + lane, y = ry0 + ry;
    int bit = 0;
    if (x < rx1) {
      if (p.protos) {
        const TP* P = static_cast<const TP*>(p.protos) + (long long)si * p.nm * plane;
        bit = y5_mask_lowres(P, plane, p.mw, p.nm, s_coef, x, y, x1, y1, x2, y2) > 0.5f;   // general.py:51 gt_(0.5)
      } else {
        bit = p.pm[((long long)si * p.max_det + d) * plane + (long long)y * p.mw + x] != 0;
      }
    }
    const unsigned long long word = __ballot(bit);
    if (lane == 0) { s_bits[u] = word; pa += __popcll(word); }
  }
  pa = block_sum(pa, s_part);   // (its barriers also publish s_bits)
  // every class-matched label in target order: intersection at the prediction's set bits
  float best = -1.f;
  int bt = -1;
  for (int t0 = 0; t0 < p.M; t0 += NT) {
    __syncthreads();
    {
      const int t = t0 + tid;
      int f = 0;
      if (t < p.M) {
        const float* l = p.lab + (long long)t * p.ld_lab;
        f = (p.img_col < 0 ? si == 0 : l[p.img_col] == fsi) && l[p.cls_col] == cls && p.w_rank[t] >= 0;
      }
      s_flag[tid] = f;
    }
    __syncthreads();
    const int tn = p.M - t0 < NT ? p.M - t0 : NT;
    for (int j = 0; j < tn; ++j) {
      if (!s_flag[j]) continue;   // workgroup-uniform
      const int t = t0 + j;
      int want;
      const void* base = gt_plane(p, t, si, p.w_rank[t], want);
      int c = 0;
      for (int u = wave; u < units; u += NW) {
        const unsigned long long word = s_bits[u];
        if (!word) continue;   // wave-uniform
        const int ry = u / wpr, x = rx0 + (u - ry * wpr) * 64 + lane, y = ry0 + ry;
        const int g = ((word >> lane) & 1ull) ? gt_bit(p, base, want, x, y) : 0;
        const unsigned long long m = __ballot(g);
        if (lane == 0) c += __popcll(m);
      }
      const int inter = block_sum(c, s_part);
      const int a = p.w_area[t];
      const float iou = (float)inter / ((float)(a + pa - inter) + 1e-7f);   // mask_iou: inter / (area1 + area2 - inter + eps)
      if (iou >= best) { best = iou; bt = t; }   // tie: the later label wins (csrc/metrics.hip)
    }
  }
  if (tid == 0) { p.w_best[(long long)si * p.max_det + d] = bt; p.w_iou[(long long)si * p.max_det + d] = best; }
}

// 3. per image: the threshold scan of process_batch (utils/metrics.py:256-265), csrc/metrics.hip's rule
__global__ __launch_bounds__(256)
void y5_val_mask_scan_kernel(const segval::Params p) {
  using namespace segval;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int* s_best = reinterpret_cast<int*>(smem);                         // [max_det] l*(d), -1 none
  unsigned* s_mask = reinterpret_cast<unsigned*>(s_best + p.max_det);  // [max_det] bit i: iou*(d) >= iouv[i]
  const int si = blockIdx.x, tid = threadIdx.x;
  int n = p.det_count ? p.det_count[si] : p.max_det;
  n = n < 0 ? 0 : (n > p.max_det ? p.max_det : n);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int d = tid + k * NT;
    if (d < n) {
      const int bl = p.w_best[(long long)si * p.max_det + d];
      const float bi = p.w_iou[(long long)si * p.max_det + d];
      unsigned m = 0;
      if (bl >= 0)
        for (int i = 0; i < p.niou; ++i) m |= (bi >= p.iouv[i] ? 1u : 0u) << i;
      s_best[d] = bl;
      s_mask[d] = m;
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int d = tid + k * NT;
    if (d >= p.max_det) continue;
    unsigned ok = 0;
    if (d < n) {
      ok = s_mask[d];
      const int l = s_best[d];
      for (int e = 0; e < d && ok; ++e)
        if (s_best[e] == l) ok &= ~s_mask[e];
    }
    unsigned char* o = p.correct + ((long long)si * p.max_det + d) * p.niou;
    for (int i = 0; i < p.niou; ++i) o[i] = (ok >> i) & 1u;  // rows past the count are written as 0
  }
}

extern "C" long long y5_val_match_masks_ws_bytes(int bs, int max_det, int nlabels) {
  if (bs < 1 || max_det < 1 || nlabels < 0) return y5_fail(Y5_ERR_BAD_ARG, "val_match_masks_ws_bytes: need bs >= 1, max_det >= 1, nlabels >= 0");
  return ((long long)bs * max_det * 2 + (long long)nlabels * 2) * 4;
}

extern "C" int y5_val_match_masks(const float* det, int ld_det, int max_det, const int* det_count, int bs, const float* labels, int ld_lab,
                                  int nlabels, int img_col, int cls_col, const void* gt_masks, int gt_dtype, int overlap, int gh, int gw,
                                  const void* protos, int proto_dtype, int nm, const unsigned char* pred_masks, int mh, int mw, int ih, int iw,
                                  const float* iouv, int niou, unsigned char* correct, void* workspace, size_t workspace_bytes, void* stream_) {
  using namespace segval;
  if (!det || !iouv || !correct || (nlabels > 0 && (!labels || !gt_masks)))
    return y5_fail(Y5_ERR_BAD_ARG, "val_match_masks: null pointer");
  if (bs < 1 || bs > 65535 || max_det < 1 || max_det > 4 * NT || ld_det < 6 || niou < 1 || niou > 32 || nlabels < 0)
    return y5_fail(Y5_ERR_BAD_ARG, "val_match_masks: need 1 <= bs <= 65535, 1 <= max_det <= 1024, ld_det >= 6, 1 <= niou <= 32, nlabels >= 0");
  if (nlabels > 0 && (cls_col < 0 || cls_col >= ld_lab || img_col >= ld_lab))
    return y5_fail(Y5_ERR_BAD_ARG, "val_match_masks: label columns outside the row");
  if (gt_dtype != Y5_U8 && gt_dtype != Y5_I32 && gt_dtype != Y5_F32) return y5_fail(Y5_ERR_BAD_ARG, "val_match_masks: gt_masks must be u8, i32 or f32");
  if ((protos != nullptr) == (pred_masks != nullptr)) return y5_fail(Y5_ERR_BAD_ARG, "val_match_masks: give exactly one of protos / pred_masks");
  if (gh < 1 || gw < 1 || mh < 1 || mw < 1 || (long long)gh * gw > (1LL << 31)) return y5_fail(Y5_ERR_BAD_ARG, "val_match_masks: bad mask shape");
  if ((long long)mh * ((mw + 63) / 64) > MAX_WORDS)
    return y5_fail(Y5_ERR_UNSUPPORTED, "val_match_masks: prediction grid too large (mh * ceil(mw / 64) must be <= 4096)");
  if (protos) {
    if (proto_dtype != Y5_F16 && proto_dtype != Y5_F32) return y5_fail(Y5_ERR_BAD_ARG, "val_match_masks: protos must be f16 or f32");
    if (nm < 1 || nm > 256 || ld_det < 6 + nm || ih < 1 || iw < 1) return y5_fail(Y5_ERR_BAD_ARG, "val_match_masks: need 1 <= nm <= 256, ld_det >= 6 + nm, ih, iw >= 1");
  }
  const long long need = y5_val_match_masks_ws_bytes(bs, max_det, nlabels);
  if (!workspace || (size_t)need > workspace_bytes || ((uintptr_t)workspace & 3)) return y5_fail(Y5_ERR_WORKSPACE, "val_match_masks: workspace too small or misaligned");
  Params p{};
  p.det = det; p.det_count = det_count; p.lab = labels; p.gt = gt_masks; p.protos = protos; p.pm = pred_masks; p.iouv = iouv; p.correct = correct;
  p.w_best = static_cast<int*>(workspace);
  p.w_iou = reinterpret_cast<float*>(p.w_best + (size_t)bs * max_det);
  p.w_rank = reinterpret_cast<int*>(p.w_iou + (size_t)bs * max_det);
  p.w_area = p.w_rank + nlabels;
  p.bs = bs; p.max_det = max_det; p.ld_det = ld_det; p.M = nlabels; p.ld_lab = ld_lab; p.img_col = img_col; p.cls_col = cls_col;
  p.gt_dtype = gt_dtype; p.overlap = overlap ? 1 : 0; p.gh = gh; p.gw = gw; p.resize = (gh != mh || gw != mw) ? 1 : 0;
  p.proto_dtype = proto_dtype; p.nm = nm; p.mh = mh; p.mw = mw; p.niou = niou;
  if (protos) { p.sx = (float)((double)mw / (double)iw); p.sy = (float)((double)mh / (double)ih); }
  p.rh = (float)gh / (float)mh; p.rw = (float)gw / (float)mw;
  hipStream_t st = static_cast<hipStream_t>(stream_);
  if (nlabels > 0) {
    hipLaunchKernelGGL(y5_val_mask_labels_kernel, dim3(nlabels), dim3(NT), 16, st, p);
    const int rc = y5_check_launch("y5_val_match_masks (labels)");
    if (rc) return rc;
  }
  const size_t lds = (4 + NT + 256) * 4 + (size_t)mh * ((mw + 63) / 64) * 8;
  const dim3 grid(max_det, bs);
  if (protos && proto_dtype == Y5_F16) hipLaunchKernelGGL((y5_val_mask_best_kernel<half_t>), grid, dim3(NT), lds, st, p);
  else hipLaunchKernelGGL((y5_val_mask_best_kernel<float>), grid, dim3(NT), lds, st, p);
  int rc = y5_check_launch("y5_val_match_masks (best)");
  if (rc) return rc;
  hipLaunchKernelGGL(y5_val_mask_scan_kernel, dim3(bs), dim3(NT), (size_t)max_det * 8, st, p);
  return y5_check_launch("y5_val_match_masks (scan)");
}
