// process_mask_native (utils/segment/general.py:54-76, the `retina_masks` branch of segment/predict.py:167-170) for every image of a batch
// in ONE launch: masks in the pixels of the ORIGINAL image, each image with its own (h0, w0).
//     masks = sigmoid(coef (n, c) @ protos (c, mh*mw))                                   general.py:67
//     masks = masks[:, top:bottom, left:right]      the letterbox padding cut away         :68-72 (the window comes from the host)
//     masks = interpolate(masks, (h0, w0), bilinear, align_corners=False)                  :74   (scale above OR below 1)
//     masks = crop_mask(masks, boxes)               boxes in original pixels               :75
//     masks.gt_(0.5)                                                                       :76
// Included by mask.hip, so it is compiled with mask.hip's flags and shares mask_value.h with the other mask kernels.
//
// One workgroup per (image, instance, tile); a tile is 64 output rows x 256 BYTES of a row, y5_process_mask_batch's shape (the comment above
// that kernel has the tile shapes that camped on a quarter of the memory channels).  w0 is arbitrary (810, 202 ...), so neither a row nor an
// instance plane starts on a 16-byte boundary in general.  The 16 lanes of a row therefore do not own fixed columns: they own the 16-byte
// groups of the OUTPUT BUFFER that the tile's columns fall into -- for row Y the tile's first column moves left by
// a = (plane offset + Y * w0) mod AL elements, AL = 128 bytes' worth.  Every group that lies inside the row is one aligned 16-byte store
// whatever w0 is; only the groups that straddle a row end are written element by element, and only the elements that belong to the row.
// 128 bytes, not 16: a row segment is then two whole 128-byte lines, never a line shared with the neighbouring tile's workgroup.  Measured
// (scripts/mask_native_bench.py, bs 32, 100 instances, 1080 x 810 and 720 x 1280 alternating; 810 * 4 B rows are no multiple of 128 B):
// float32 3.31 TB/s of output with 16-byte alignment, 5.12 with 128, 5.05 with 256; uint8 2.29 / 2.40 / 2.08.
// Tiles wholly outside the instance's box (most of them) are plain zero stores: no LDS, no barrier, no prototype read.  The others compute
// the sigmoid values their taps can touch once into LDS and blend from there; when the image is SMALLER than its window (scale > 1) that
// source region can exceed the LDS of the launch, and the tile then evaluates its four taps directly -- the same y5_mask_value, the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/yolov5_hip.h"
#include "mask_value.h"
#include "y5_common.h"
#include "y5_host.h"

namespace masknative {
constexpr int TH = 64;             // output rows per tile
constexpr int ALIGN_BYTES = 128;   // a tile's row segments start on multiples of this in the output buffer (measured below)
constexpr int MAX_IMG = 48;        // images per launch: 48 descriptors of 64 bytes + the header stay under the 4 KB kernel-argument limit
constexpr int LDS_CAP = 17664;     // floats of low-resolution values per workgroup (69 KB; y5_process_mask_batch's uint8 launch uses 70 KB)

struct Img {
  const float* coef;      // row i at coef + i*ld_m, c values
  const float* boxes;     // row i at boxes + i*ld_b: x1,y1,x2,y2 in original-image pixels
  long long out_off;      // element offset of the image's (n, h0, w0) block in the output, a multiple of 16 bytes
  int ld_m, ld_b, n, h0, w0;
  int top, left, ch, cw;  // the window of the prototype plane that is resized (general.py:70-72)
  int pad_;
};
static_assert(sizeof(Img) == 64, "descriptor size");

struct Params {
  const void* protos;     // (B, c, mh, mw)
  void* out;
  int c, mh, mw, lds_elems;
  Img img[MAX_IMG];
};
static_assert(sizeof(Params) <= 4096, "kernel arguments above 4 KB");

// upsample_bilinear2d's source coordinate, align_corners=False (area_pixel_compute_source_index)
__device__ __forceinline__ float src_of(float scale, int dst) { return fmaxf(scale * ((float)dst + 0.5f) - 0.5f, 0.f); }
}  // namespace masknative

template <typename TP, typename TO>
__global__ __launch_bounds__(256)
void y5_process_mask_native_kernel(const masknative::Params p) {
  using namespace masknative;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int VEC = 16 / (int)sizeof(TO);
  constexpr int TW = 16 * VEC;                                  // output columns per tile: 256 bytes of a row
  constexpr int AL = ALIGN_BYTES / (int)sizeof(TO);             // elements per alignment unit (a multiple of VEC, at most TW)
  float* s_coef = reinterpret_cast<float*>(smem);               // [256]
  float* s_m = s_coef + 256;                                    // [wh][ww] sigmoid values of the tile's source region
  typedef uint32_t u4 __attribute__((ext_vector_type(4)));
  const int tid = threadIdx.x;
  const int b = blockIdx.y;
  const Img im = p.img[b];
  const int h0 = im.h0, w0 = im.w0;
  const int tiles_x = (w0 + AL - 1 + TW - 1) / TW;              // (AL - 1: the shifted rows reach that much further)
  const int per_inst = tiles_x * ((h0 + TH - 1) / TH);
  const int inst = blockIdx.x / per_inst, ti = blockIdx.x - inst * per_inst;
  if (inst >= im.n) return;
  const int ty = ti / tiles_x, tx = ti - ty * tiles_x;
  const int Y0 = ty * TH, Yl = (Y0 + TH < h0 ? Y0 + TH : h0) - 1;
  // the columns any row of this tile can own: [tx*TW - a, tx*TW + TW - a) for a in [0, AL)
  const int Xa = tx * TW - (AL - 1) > 0 ? tx * TW - (AL - 1) : 0, Xb = (tx * TW + TW < w0 ? tx * TW + TW : w0) - 1;
  const float* bx = im.boxes + (long long)inst * im.ld_b;
  const float x1 = bx[0], y1 = bx[1], x2 = bx[2], y2 = bx[3];
  // can any pixel of the tile lie inside the box (x1 <= X < x2, y1 <= Y < y2; general.py:22)?  The SAME float comparisons as the per-pixel
  // test below on the tile's corner pixels (monotone in X / Y): a tile that fails has no pixel that passes, so it is exactly all zero.
  const bool hit = (float)Xb >= x1 && (float)Xa < x2 && (float)Yl >= y1 && (float)Y0 < y2;
  const long long plane_off = (long long)inst * h0 * w0;
  TO* out = static_cast<TO*>(p.out) + im.out_off + plane_off;
  const int vy = tid >> 4, vx = (tid & 15) * VEC;               // this lane's 16-byte group inside a 16-row slab of the tile
  if (!hit) {
    const u4 z = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < TH / 16; ++k) {
      const int Y = Y0 + k * 16 + vy;
      if (Y > Yl) continue;
      const long long row = (long long)Y * w0;
      const int Xg = tx * TW + vx - (int)((plane_off + row) & (AL - 1));
      if (Xg >= 0 && Xg + VEC <= w0) {
        *reinterpret_cast<u4*>(out + row + Xg) = z;
      } else {
        for (int e = 0; e < VEC; ++e)
          if (Xg + e >= 0 && Xg + e < w0) out[row + Xg + e] = (TO)0;
      }
    }
    return;
  }
  for (int i = tid; i < p.c; i += 256) s_coef[i] = im.coef[(long long)inst * im.ld_m + i];
  const float rh = (float)im.ch / (float)h0, rw = (float)im.cw / (float)w0;
  // source region (relative to the window) of the bilinear taps of rows [Y0, Yl] / columns [Xa, Xb]
  const int wy0 = (int)src_of(rh, Y0), wx0 = (int)src_of(rw, Xa);
  int wy1 = (int)src_of(rh, Yl) + 1, wx1 = (int)src_of(rw, Xb) + 1;
  wy1 = wy1 > im.ch - 1 ? im.ch - 1 : wy1;
  wx1 = wx1 > im.cw - 1 ? im.cw - 1 : wx1;
  const int wh = wy1 - wy0 + 1, ww = wx1 - wx0 + 1;
  const bool use_lds = (long long)wh * ww <= (long long)p.lds_elems;   // workgroup-uniform
  const long long plane = (long long)p.mh * p.mw;
  const TP* P = static_cast<const TP*>(p.protos) + (long long)b * p.c * plane;
  __syncthreads();
  if (use_lds) {
    for (int i = tid; i < ww * wh; i += 256) {
      const int ly = i / ww, lx = i - ly * ww;
      s_m[i] = y5_mask_value(P, plane, p.mw, p.c, s_coef, im.left + wx0 + lx, im.top + wy0 + ly);
    }
    __syncthreads();
  }
#pragma unroll 1
  for (int k = 0; k < TH / 16; ++k) {
    const int Y = Y0 + k * 16 + vy;
    if (Y > Yl) continue;
    const long long row = (long long)Y * w0;
    const int Xg = tx * TW + vx - (int)((plane_off + row) & (AL - 1));
    if (Xg + VEC <= 0 || Xg >= w0) continue;
    const bool yin = (float)Y >= y1 && (float)Y < y2;
    // upsample_bilinear2d, align_corners=False (F.interpolate, general.py:74); indices relative to the window, clamped at ITS edge
    const float h1r = src_of(rh, Y);
    int hh = (int)h1r;
    hh = hh > im.ch - 1 ? im.ch - 1 : hh;
    const int h1p = hh < im.ch - 1 ? 1 : 0;
    const float hl1 = h1r - (float)hh, hl0 = 1.0f - hl1;
    TO r[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const int X = Xg + e;
      int bit = 0;
      if (yin && X >= 0 && X < w0 && (float)X >= x1 && (float)X < x2) {   // crop_mask at full resolution (general.py:75)
        const float w1r = src_of(rw, X);
        int wi = (int)w1r;
        wi = wi > im.cw - 1 ? im.cw - 1 : wi;
        const int w1p = wi < im.cw - 1 ? 1 : 0;
        const float wl1 = w1r - (float)wi, wl0 = 1.0f - wl1;
        float v00, v01, v10, v11;
        if (use_lds) {
          const int a0 = (hh - wy0) * ww + (wi - wx0), a1 = (hh + h1p - wy0) * ww + (wi - wx0);
          v00 = s_m[a0]; v01 = s_m[a0 + w1p];
          v10 = s_m[a1]; v11 = s_m[a1 + w1p];
        } else {
          const int gx = im.left + wi, gy = im.top + hh;
          v00 = y5_mask_value(P, plane, p.mw, p.c, s_coef, gx, gy);
          v01 = y5_mask_value(P, plane, p.mw, p.c, s_coef, gx + w1p, gy);
          v10 = y5_mask_value(P, plane, p.mw, p.c, s_coef, gx, gy + h1p);
          v11 = y5_mask_value(P, plane, p.mw, p.c, s_coef, gx + w1p, gy + h1p);
        }
        const float val = hl0 * (wl0 * v00 + wl1 * v01) + hl1 * (wl0 * v10 + wl1 * v11);
        bit = val > 0.5f ? 1 : 0;   // general.py:76 gt_(0.5)
      }
      r[e] = (TO)bit;
    }
    if (Xg >= 0 && Xg + VEC <= w0) {
      u4 v4;
      __builtin_memcpy(&v4, r, 16);
      *reinterpret_cast<u4*>(out + row + Xg) = v4;
    } else {
#pragma unroll
      for (int e = 0; e < VEC; ++e)
        if (Xg + e >= 0 && Xg + e < w0) out[row + Xg + e] = r[e];
    }
  }
}

extern "C" int y5_process_mask_native_batch(const void* protos, int proto_dtype, int B, int c, int mh, int mw, const y5_mask_native_img* imgs,
                                            void* out, long long out_elems, int out_dtype, void* stream_) {
  using namespace masknative;
  hipStream_t st = static_cast<hipStream_t>(stream_);
  if (!protos || !imgs || B < 1 || c < 1 || c > 256 || mh < 1 || mw < 1 || out_elems < 0)
    return y5_fail(Y5_ERR_BAD_ARG, "process_mask_native_batch: bad args");
  if ((long long)mh * mw > 0x7fffffffLL / 256) return y5_fail(Y5_ERR_BAD_ARG, "process_mask_native_batch: prototype plane too large");
  if (proto_dtype != Y5_F16 && proto_dtype != Y5_F32) return y5_fail(Y5_ERR_BAD_ARG, "process_mask_native_batch: protos must be f16 or f32");
  if (out_dtype != Y5_F32 && out_dtype != Y5_U8) return y5_fail(Y5_ERR_BAD_ARG, "process_mask_native_batch: out dtype must be Y5_F32 or Y5_U8");
  const int vec = out_dtype == Y5_F32 ? 4 : 16;
  const int tw = 16 * vec, al = ALIGN_BYTES / (out_dtype == Y5_F32 ? 4 : 1);
  // every descriptor is checked before anything is launched
  long long total = 0;
  for (int i = 0; i < B; ++i) {
    const y5_mask_native_img& s = imgs[i];
    if (s.n < 0) return y5_fail(Y5_ERR_BAD_ARG, "process_mask_native_batch: negative instance count");
    if (s.n == 0) continue;
    if (!s.masks_in || !s.boxes || s.ld_m < c || s.ld_b < 4) return y5_fail(Y5_ERR_BAD_ARG, "process_mask_native_batch: bad image descriptor");
    if (s.h0 < 1 || s.w0 < 1 || s.h0 > (1 << 24) || s.w0 > (1 << 24)) return y5_fail(Y5_ERR_BAD_ARG, "process_mask_native_batch: bad image size");
    if (s.ch < 1 || s.cw < 1) return y5_fail(Y5_ERR_BAD_ARG, "process_mask_native_batch: empty window");
    if (s.top < 0 || s.left < 0 || s.top > mh - s.ch || s.left > mw - s.cw)
      return y5_fail(Y5_ERR_BAD_ARG, "process_mask_native_batch: window outside the prototype plane");
    const long long tiles = (long long)((s.w0 + al - 1 + tw - 1) / tw) * ((s.h0 + TH - 1) / TH);
    if (tiles > 0x7fffffffLL / s.n) return y5_fail(Y5_ERR_UNSUPPORTED, "process_mask_native_batch: grid out of range");
    const long long block = (long long)s.n * s.h0 * s.w0;   // (at most 2^31 tiles of 2^14 elements: no overflow)
    if (s.out_off < 0 || s.out_off % vec || s.out_off > out_elems || block > out_elems - s.out_off)
      return y5_fail(Y5_ERR_BAD_ARG, "process_mask_native_batch: image block misaligned or outside the output");
    total += s.n;
  }
  if (total == 0) return Y5_OK;
  if (!out || ((uintptr_t)out & 15)) return y5_fail(Y5_ERR_BAD_ARG, "process_mask_native_batch: output null or not 16-byte aligned");
  const size_t psz = proto_dtype == Y5_F16 ? 2 : 4;
  for (int b0 = 0; b0 < B; b0 += MAX_IMG) {
    Params p{};
    const int nb = B - b0 < MAX_IMG ? B - b0 : MAX_IMG;
    long long gx = 0, lds_elems = 1;
    for (int i = 0; i < nb; ++i) {
      const y5_mask_native_img& s = imgs[b0 + i];
      Img& d = p.img[i];
      if (s.n == 0) {   // (its workgroups leave at once; sizes that keep their index arithmetic defined)
        d.h0 = d.w0 = d.ch = d.cw = 1;
        continue;
      }
      d.coef = s.masks_in; d.boxes = s.boxes; d.out_off = s.out_off; d.ld_m = s.ld_m; d.ld_b = s.ld_b; d.n = s.n; d.h0 = s.h0; d.w0 = s.w0;
      d.top = s.top; d.left = s.left; d.ch = s.ch; d.cw = s.cw;
      const long long g = (long long)((s.w0 + al - 1 + tw - 1) / tw) * ((s.h0 + TH - 1) / TH) * s.n;
      gx = g > gx ? g : gx;
      // upper bound of a tile's source region: (columns or rows of the tile) * scale + the second tap + rounding, at most the window
      const double bw = (double)(tw + al - 1) * s.cw / s.w0 + 3.0, bh = (double)TH * s.ch / s.h0 + 3.0;
      const long long e = (long long)(bw < s.cw ? bw : s.cw) * (long long)(bh < s.ch ? bh : s.ch);
      lds_elems = e > lds_elems ? e : lds_elems;
    }
    if (gx == 0) continue;
    p.protos = static_cast<const char*>(protos) + (size_t)b0 * c * mh * mw * psz;
    p.out = out;
    p.c = c; p.mh = mh; p.mw = mw;
    p.lds_elems = (int)(lds_elems < LDS_CAP ? lds_elems : LDS_CAP);   // larger regions take the direct path inside the kernel
    const size_t lds = ((size_t)p.lds_elems + 256) * 4;
    const dim3 grid((unsigned)gx, (unsigned)nb), block(256);
    if (proto_dtype == Y5_F16) {
      if (out_dtype == Y5_F32) hipLaunchKernelGGL((y5_process_mask_native_kernel<half_t, float>), grid, block, lds, st, p);
      else hipLaunchKernelGGL((y5_process_mask_native_kernel<half_t, unsigned char>), grid, block, lds, st, p);
    } else {
      if (out_dtype == Y5_F32) hipLaunchKernelGGL((y5_process_mask_native_kernel<float, float>), grid, block, lds, st, p);
      else hipLaunchKernelGGL((y5_process_mask_native_kernel<float, unsigned char>), grid, block, lds, st, p);
    }
    const int rc = y5_check_launch("y5_process_mask_native_batch");
    if (rc) return rc;
  }
  return Y5_OK;
}
