// Segmentation ComputeLoss (utils/segment/loss.py:47-120, 122-199): the mask term and the extra build_targets outputs, on top of the
// detection kernels of loss_kernels.h run with the row stride no = 5 + nc + nm.  No host synchronisation, no float atomics.
//
//   S1 y5_seg_tidx_kernel     loss.py:130-136: tidx of every target.  overlap: the positional concatenation over images i = 0..bs-1 of
//      1..count_i (== the per-image rank only when targets are sorted by image); otherwise the target index itself.
//   S2 y5_seg_group_kernel    one workgroup per image b: the rows of every level whose image is b, as a list in (level, row) order at a
//      fixed offset (exclusive prefix of the per-image counts, integer LDS histogram).  Per list entry: crop box, area and gt index from
//      xywhn = (t * gain) / gain (loss.py:196), mxyxy = xywh2xyxy(xywhn * [mw, mh, mw, mh]) (:92), marea (:91), the row count of its
//      (level, image) group (the mean of :103 / :120) and the row's nm mask coefficients widened to fp32.
//   S3 y5_seg_rows_kernel     one workgroup per entry: loss.py:116-120 for one row over its crop only (the BCE is multiplied by 0
//      outside it), L_r = sum_crop BCE(c_r . P_b, gt_r), and the unit-scale coefficient gradient sum_crop dBCE * P_b written into the
//      row gradient G[5 + nc + k], which the detection backward (K5) sums over duplicate cells in ascending row order.
//   S4 y5_seg_finish_kernel   fixed-order fp64 sum of L_r / (mh mw) / area_r / n_(level, image), x hyp_box / bs (loss.py:111), and
//      out5 = [(lbox + lobj + lcls + lseg) * bs, lbox, lseg, lobj, lcls] (loss.py:113-114).
//   S5 y5_seg_dproto_kernel   one workgroup per (64 x 4 pixel tile, image): dproto = scale * sum over the image's entries (list order) of
//      c_r * dBCE_r, every element written (zero where no crop covers the pixel).  Entries whose crop misses the tile are skipped.
//
// Arithmetic: fp32 on fp32 (fp16 inputs widened) with k-ordered products; BCE without pos_weight (F.binary_cross_entropy_with_logits).
#pragma once
#include "loss_kernels.h"

#define Y5_SEG_MAX_NM 32
#define Y5_SEG_MAX_BS 4096
#define Y5_SEG_GROUP_LDS(bs) (4112 + 4 * (bs))
#define Y5_SEG_ROWS_LDS (4 * (Y5_SEG_MAX_NM + 1) * 4)

struct Y5SegParams {
  const void* proto;     // (bs, nm, mh, mw), dtype of p
  void* dproto;          // (bs, nm, mh, mw) gradient (backward only)
  const void* masks;     // overlap: (bs, mh, mw); else (nt, mh, mw); float32 or uint8
  int nm, mh, mw, overlap, nmask;  // nmask = masks.shape[0]
  float* ti;             // [nt] tidx per target
  int* img_cnt;          // [bs] targets per image (overlap tidx)
  int* img_off;          // [bs] first list entry of image b
  int* img_n;            // [bs] list entries of image b
  // list entries [E = nl * cap], grouped by image, (level, row) order inside an image
  int* e_lvl; int* e_row; int* e_b; int* e_gt; int* e_n;
  float* e_box;          // [E][4] x1 y1 x2 y2 at mask resolution
  float* e_area;         // [E] xywhn w * h
  float* e_coef;         // [E][nm] fp32
  float* e_loss;         // [E] sum over the crop of the BCE
  float* out4;           // detection result [loss, lbox, lobj, lcls]
  float* out5;           // [loss, lbox, lseg, lobj, lcls]
};

// integer pixel range [lo, hi) that contains every c with lo_f <= c < hi_f (the exact float test is applied per pixel)
__device__ __forceinline__ void y5_seg_range(float lo_f, float hi_f, int n, int& lo, int& hi) {
  if (!(lo_f < hi_f)) { lo = 0; hi = 0; return; }  // also NaN
  const float a = fminf(fmaxf(floorf(lo_f), 0.0f), (float)n), b = fminf(fmaxf(floorf(hi_f) + 1.0f, 0.0f), (float)n);
  lo = (int)a; hi = (int)b;
}

template <typename MT>
__device__ __forceinline__ float y5_seg_gt(const Y5SegParams& s, int b, int gt, long long pix) {
  const long long hw = (long long)s.mh * s.mw;
  const MT* m = static_cast<const MT*>(s.masks);
  if (s.overlap) return (float)m[(long long)b * hw + pix] == (float)gt ? 1.0f : 0.0f;  // loss.py:97
  return (float)m[(long long)gt * hw + pix];                                           // loss.py:99
}

// ---- S1 -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024)
void y5_seg_tidx_kernel(const Y5LossParams p, const Y5SegParams s) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int& s_total = *reinterpret_cast<int*>(smem);
  const int tid = threadIdx.x;
  for (int b = tid; b < p.bs; b += 1024) {
    int c = 0;
    for (int t = 0; t < p.nt; ++t) c += p.targets[(long long)t * 6] == (float)b ? 1 : 0;  // loss.py:133
    s.img_cnt[b] = c;
  }
  __syncthreads();
  if (tid == 0) {  // exclusive prefix of the per-image TARGET counts (S2 overwrites img_off with list offsets afterwards)
    int o = 0;
    for (int b = 0; b < p.bs; ++b) { s.img_off[b] = o; o += s.img_cnt[b]; }
    s_total = o;
  }
  __syncthreads();
  for (int t = tid; t < p.nt; t += 1024) {
    float v = (float)t;
    if (s.overlap) {
      v = 0.0f;  // position past the concatenation (targets of images outside the batch): the reference raises; no row uses it
      if (t < s_total) {
        int lo = 0, hi = p.bs - 1;  // last image whose offset <= t and which has targets
        while (lo < hi) {
          const int mid = (lo + hi + 1) >> 1;
          if (s.img_off[mid] <= t) lo = mid; else hi = mid - 1;
        }
        v = (float)(t - s.img_off[lo] + 1);
      }
    }
    s.ti[t] = v;
  }
}

// ---- S2 -------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(1024)
void y5_seg_group_kernel(const Y5LossParams p, const Y5SegParams s) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int* s_scan = reinterpret_cast<int*>(smem);          // [1024]
  int& s_off = *reinterpret_cast<int*>(smem + 4096);
  int* s_hist = reinterpret_cast<int*>(smem + 4112);  // [bs]
  const int b = blockIdx.x, tid = threadIdx.x;
  for (int i = tid; i < p.bs; i += 1024) s_hist[i] = 0;
  __syncthreads();
  for (int i = 0; i < p.nl; ++i) {
    const int n = p.n_rows[i];
    for (int r = tid; r < n; r += 1024) atomicAdd(&s_hist[p.lv[i].rb[r]], 1);  // integer: order-free
  }
  __syncthreads();
  if (tid == 0) {
    int o = 0;
    for (int q = 0; q < b; ++q) o += s_hist[q];
    s_off = o;
    s.img_off[b] = o;
    s.img_n[b] = s_hist[b];
  }
  __syncthreads();
  const int base = s_off;
  int pos = base;
  const float fmw = (float)s.mw, fmh = (float)s.mh;
  for (int i = 0; i < p.nl; ++i) {
    const Y5LossLevel& L = p.lv[i];
    const int n = p.n_rows[i];
    const int lstart = pos;
    for (int c0 = 0; c0 < n; c0 += 1024) {
      const int r = c0 + tid;
      const int f = (r < n && L.rb[r] == b) ? 1 : 0;
      s_scan[tid] = f;
      __syncthreads();
      for (int d = 1; d < 1024; d <<= 1) {
        const int v = tid >= d ? s_scan[tid - d] : 0;
        __syncthreads();
        s_scan[tid] += v;
        __syncthreads();
      }
      if (f) {
        const int e = pos + s_scan[tid] - 1;
        const int t = L.rt[r];
        const float* tg = p.targets + (long long)t * 6;
        const float fnx = (float)L.nx, fny = (float)L.ny;
        const float xn = (tg[2] * fnx) / fnx, yn = (tg[3] * fny) / fny;  // loss.py:196 xywhn = (t * gain) / gain
        const float wn = (tg[4] * fnx) / fnx, hn = (tg[5] * fny) / fny;
        const float X = xn * fmw, Y = yn * fmh, W = wn * fmw, H = hn * fmh;  // loss.py:92
        const float hw_ = W / 2, hh_ = H / 2;
        s.e_box[e * 4 + 0] = X - hw_; s.e_box[e * 4 + 1] = Y - hh_;
        s.e_box[e * 4 + 2] = X + hw_; s.e_box[e * 4 + 3] = Y + hh_;
        s.e_area[e] = wn * hn;                                               // loss.py:91
        s.e_lvl[e] = i; s.e_row[e] = r; s.e_b[e] = b;
        s.e_gt[e] = s.overlap ? (int)s.ti[t] : t;
        const long long cell = (((long long)b * p.na + L.ra[r]) * L.ny + L.rgj[r]) * L.nx + L.rgi[r];
        const T* row = static_cast<const T*>(L.p) + cell * p.no + 5 + p.nc;
        for (int k = 0; k < s.nm; ++k) s.e_coef[(long long)e * s.nm + k] = (float)row[k];
      }
      const int tot = s_scan[1023];
      __syncthreads();
      pos += tot;
    }
    for (int e = lstart + tid; e < pos; e += 1024) s.e_n[e] = pos - lstart;
  }
}

// ---- S3 -------------------------------------------------------------------------------------------------
template <typename T, typename MT>
__global__ __launch_bounds__(256)
void y5_seg_rows_kernel(const Y5LossParams p, const Y5SegParams s) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float (*s_red)[Y5_SEG_MAX_NM + 1] = reinterpret_cast<float (*)[Y5_SEG_MAX_NM + 1]>(smem);  // [4][nm + 1]
  int ntot = 0;
  for (int i = 0; i < p.nl; ++i) ntot += p.n_rows[i];
  const int e = blockIdx.x;
  if (e >= ntot) return;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int nm = s.nm, b = s.e_b[e], gt = s.e_gt[e];
  const float x1 = s.e_box[e * 4], y1 = s.e_box[e * 4 + 1], x2 = s.e_box[e * 4 + 2], y2 = s.e_box[e * 4 + 3];
  int cx0, cx1, cy0, cy1;
  y5_seg_range(x1, x2, s.mw, cx0, cx1);
  y5_seg_range(y1, y2, s.mh, cy0, cy1);
  const int cw = cx1 - cx0, npix = cw * (cy1 - cy0);
  float c[Y5_SEG_MAX_NM], acc[Y5_SEG_MAX_NM];
#pragma unroll
  for (int k = 0; k < Y5_SEG_MAX_NM; ++k) { c[k] = k < nm ? s.e_coef[(long long)e * nm + k] : 0.f; acc[k] = 0.f; }
  const long long hw = (long long)s.mh * s.mw;
  const T* P = static_cast<const T*>(s.proto) + (long long)b * nm * hw;
  float lsum = 0.f;
  for (int q = tid; q < npix; q += 256) {
    const int y = cy0 + q / cw, x = cx0 + q % cw;
    const float fx = (float)x, fy = (float)y;
    if (!(fx >= x1 && fx < x2 && fy >= y1 && fy < y2)) continue;  // crop_mask (utils/segment/general.py:22)
    const long long pix = (long long)y * s.mw + x;
    float pk[Y5_SEG_MAX_NM];
    float S = 0.f;
#pragma unroll
    for (int k = 0; k < Y5_SEG_MAX_NM; ++k) {
      pk[k] = k < nm ? (float)P[k * hw + pix] : 0.f;
      S += c[k] * pk[k];
    }
    float dx;
    lsum += y5_bce(S, y5_seg_gt<MT>(s, b, gt, pix), 1.0f, dx);
#pragma unroll
    for (int k = 0; k < Y5_SEG_MAX_NM; ++k) acc[k] += dx * pk[k];
  }
  // fixed-order block reduction: wave butterflies, then the 4 waves in order
  lsum = y5_wave_sum(lsum);
#pragma unroll
  for (int k = 0; k < Y5_SEG_MAX_NM; ++k) acc[k] = y5_wave_sum(acc[k]);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < Y5_SEG_MAX_NM; ++k) s_red[wv][k] = acc[k];
    s_red[wv][Y5_SEG_MAX_NM] = lsum;
  }
  __syncthreads();
  if (tid <= nm) {
    const int k = tid < nm ? tid : Y5_SEG_MAX_NM;
    const float v = ((s_red[0][k] + s_red[1][k]) + s_red[2][k]) + s_red[3][k];
    if (tid == nm) {
      s.e_loss[e] = v;
    } else {
      // d((lseg * hyp_box / bs) * bs) / dS = hyp_box / (n * mh * mw * area) * dBCE
      const float w = p.hyp_box / ((float)s.e_n[e] * (float)hw * s.e_area[e]);
      p.lv[s.e_lvl[e]].G[(long long)s.e_row[e] * p.no + 5 + p.nc + k] = v * w;
    }
  }
}

// ---- S4 -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256)
void y5_seg_finish_kernel(const Y5LossParams p, const Y5SegParams s) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* s_red = reinterpret_cast<double*>(smem);  // [256]
  int ntot = 0;
  for (int i = 0; i < p.nl; ++i) ntot += p.n_rows[i];
  const double hw = (double)s.mh * s.mw;
  double v = 0.0;
  for (int e = threadIdx.x; e < ntot; e += 256) v += (double)s.e_loss[e] / hw / (double)s.e_area[e] / (double)s.e_n[e];
  s_red[threadIdx.x] = v;
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) {
    if ((int)threadIdx.x < d) s_red[threadIdx.x] += s_red[threadIdx.x + d];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float lseg = (float)s_red[0] * (p.hyp_box / (float)p.bs);  // loss.py:111
    const float lbox = s.out4[1], lobj = s.out4[2], lcls = s.out4[3];
    s.out5[0] = (lbox + lobj + lcls + lseg) * (float)p.bs;          // loss.py:113-114
    s.out5[1] = lbox; s.out5[2] = lseg; s.out5[3] = lobj; s.out5[4] = lcls;
  }
}

// ---- S5 -------------------------------------------------------------------------------------------------
#define Y5_SEG_TW 64
#define Y5_SEG_TH 4

template <typename T, typename MT>
__global__ __launch_bounds__(256)
void y5_seg_dproto_kernel(const Y5LossParams p, const Y5SegParams s) {
  const int ntx = (s.mw + Y5_SEG_TW - 1) / Y5_SEG_TW;
  const int tx0 = (blockIdx.x % ntx) * Y5_SEG_TW, ty0 = (blockIdx.x / ntx) * Y5_SEG_TH;
  const int b = blockIdx.y, tid = threadIdx.x;
  const int x = tx0 + (tid & 63), y = ty0 + (tid >> 6);
  const bool in = x < s.mw && y < s.mh;
  const int nm = s.nm;
  const long long hw = (long long)s.mh * s.mw;
  const long long pix = in ? (long long)y * s.mw + x : 0;
  const float scale = p.gscale ? *p.gscale : 1.0f;
  const T* P = static_cast<const T*>(s.proto) + (long long)b * nm * hw;
  T* D = static_cast<T*>(s.dproto) + (long long)b * nm * hw;
  float pk[Y5_SEG_MAX_NM], d[Y5_SEG_MAX_NM];
#pragma unroll
  for (int k = 0; k < Y5_SEG_MAX_NM; ++k) { pk[k] = (in && k < nm) ? (float)P[k * hw + pix] : 0.f; d[k] = 0.f; }
  const float fx = (float)x, fy = (float)y;
  const int e0 = s.img_off[b], e1 = e0 + s.img_n[b];
  for (int e = e0; e < e1; ++e) {
    const float x1 = s.e_box[e * 4], y1 = s.e_box[e * 4 + 1], x2 = s.e_box[e * 4 + 2], y2 = s.e_box[e * 4 + 3];
    int cx0, cx1, cy0, cy1;
    y5_seg_range(x1, x2, s.mw, cx0, cx1);
    y5_seg_range(y1, y2, s.mh, cy0, cy1);
    if (cx1 <= tx0 || cx0 >= tx0 + Y5_SEG_TW || cy1 <= ty0 || cy0 >= ty0 + Y5_SEG_TH) continue;  // uniform: crop misses the tile
    if (!(in && fx >= x1 && fx < x2 && fy >= y1 && fy < y2)) continue;
    float c[Y5_SEG_MAX_NM];
    float S = 0.f;
#pragma unroll
    for (int k = 0; k < Y5_SEG_MAX_NM; ++k) {
      c[k] = k < nm ? s.e_coef[(long long)e * nm + k] : 0.f;
      S += c[k] * pk[k];
    }
    float dx;
    y5_bce(S, y5_seg_gt<MT>(s, b, s.e_gt[e], pix), 1.0f, dx);
    const float g = dx * (p.hyp_box / ((float)s.e_n[e] * (float)hw * s.e_area[e]));
#pragma unroll
    for (int k = 0; k < Y5_SEG_MAX_NM; ++k) d[k] += c[k] * g;
  }
  if (in) {
    for (int k = 0; k < nm; ++k) D[k * hw + pix] = (T)(d[k] * scale);
  }
}
