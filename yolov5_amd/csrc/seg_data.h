// Polygon labels -> training / validation masks on the device: what utils/segment/dataloaders.py:180-199 does per image on a CPU worker
//     polygons2masks_overlap(img.shape[:2], segments, downsample_ratio)   (overlap)    -> one index plane per image + the area order
//     polygons2masks(img.shape[:2], segments, color=1, downsample_ratio)  (no overlap) -> one 0/1 plane per instance
// each of them, per instance, polygon2mask = np.asarray(polygon, int32) -> cv2.fillPoly(zeros(H, W), [pts], 1) -> cv2.resize to
// (H // ratio, W // ratio), plus the mask half of the flips (:212-223), for a whole batch in one C-ABI call.
// ultralytics.data.utils and opencv-python are third-party dependencies of the reference (absent here): restated from the published
// sources -- modules/imgproc/src/drawing.cpp (fillPoly: CollectPolyEdges, FillEdgeCollection, Line / LineIterator, clipLine) and
// ultralytics/data/utils.py -- and pinned against the NumPy restatement tests/seg_data_ref.py; cv2.resize is resize_u8.h.
// Included by augment.hip: compiled with -ffp-contract=off (clipLine's double products must round like the CPU's).
//
// cv2.fillPoly of ONE contour is the union of (a) the 8-connected Bresenham line of every edge and (b) the scanline fill.  (b) keeps the
// edges that cross a row sorted by x and fills between the 1st and 2nd, 3rd and 4th, ...; a closed contour crosses every row an even
// number of times and an edge's x at row y is x0 + (y - y0) * dx in exact 64-bit fixed point, so with r_e = x_e >> 16 a pixel x of row y
// is filled iff  #{e : r_e < x} is odd  OR  some r_e == x  (the second term is the closed right end of a span).  That is order-free:
//   1. every (edge, row) crossing toggles ONE bit, at column r_e + 1, of a bit plane in LDS (atomic xor);
//   2. a prefix-xor along each row turns the toggles into the parity of #{r_e < x};
//   3. every crossing ORs its own bit r_e, every edge ORs its Bresenham pixels;
//   4. the plane is shrunk with cv2.resize's arithmetic (resized_value) to h x w bits in the caller's workspace, the area is reduced
//      without atomics.
// One workgroup per instance, one wave-64 quad; the edge work is integer, the plane never leaves LDS.  Then one thread per instance
// ranks it among the instances of its image (key = 0 - area in uint64: LARGEST area first, but zero area wraps to key 0 and sorts first,
// as np.argsort(-areas) of a uint64 array does; ties: lower label index first), and a third launch writes the planes with the flips.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/yolov5_hip.h"
#include "resize_u8.h"
#include "y5_common.h"
#include "y5_host.h"

namespace segdata {
constexpr int NT = 256;
constexpr int XY_SHIFT = 16;
constexpr long long XY_ONE = 1LL << XY_SHIFT;
constexpr size_t MAX_LDS = 160 * 1024;

struct Params {
  const double* xy;
  const int* poly_off;
  const int* inst_img;
  const unsigned char* flip;
  void* masks;
  int* order;
  long long* area;
  unsigned* bits;   // workspace: (n_inst, h, w32) shrunk bit planes
  int* rank;        // workspace: (n_inst)
  int n_inst, B, H, W, h, w, W32, w32, overlap, mask_dtype;
};

// LDS bit updates.  (The host emulator of the test suite runs the lanes of a workgroup one at a time and has no atomic xor / or.)
__device__ inline void lds_xor(unsigned* p, unsigned v) {
#ifdef Y5_EMU
  *p ^= v;
#else
  atomicXor(p, v);
#endif
}
__device__ inline void lds_or(unsigned* p, unsigned v) {
#ifdef Y5_EMU
  *p |= v;
#else
  atomicOr(p, v);
#endif
}

// np.asarray(float64, dtype=np.int32): truncation toward zero (a coordinate in (-1, 0) becomes 0); out of range / NaN -> INT_MIN (cvttsd2si)
__device__ inline int trunc_i32(double v) {
  if (!(v > -2147483649.0 && v < 2147483648.0)) return -2147483647 - 1;
  return (int)v;
}

// cv::clipLine(Size2l(W, H), pt1, pt2)
__device__ inline bool clip_line(int W, int H, long long& x1, long long& y1, long long& x2, long long& y2) {
  const long long right = W - 1, bottom = H - 1;
  int c1 = (x1 < 0) + (x1 > right) * 2 + (y1 < 0) * 4 + (y1 > bottom) * 8;
  int c2 = (x2 < 0) + (x2 > right) * 2 + (y2 < 0) * 4 + (y2 > bottom) * 8;
  if ((c1 & c2) == 0 && (c1 | c2) != 0) {
    long long a;
    if (c1 & 12) {
      a = c1 < 8 ? 0 : bottom;
      x1 += (long long)((double)(a - y1) * (double)(x2 - x1) / (double)(y2 - y1));
      y1 = a;
      c1 = (x1 < 0) + (x1 > right) * 2;
    }
    if (c2 & 12) {
      a = c2 < 8 ? 0 : bottom;
      x2 += (long long)((double)(a - y2) * (double)(x2 - x1) / (double)(y2 - y1));
      y2 = a;
      c2 = (x2 < 0) + (x2 > right) * 2;
    }
    if ((c1 & c2) == 0 && (c1 | c2) != 0) {
      if (c1) {
        a = c1 == 1 ? 0 : right;
        y1 += (long long)((double)(a - x1) * (double)(y2 - y1) / (double)(x2 - x1));
        x1 = a;
        c1 = 0;
      }
      if (c2) {
        a = c2 == 1 ? 0 : right;
        y2 += (long long)((double)(a - x2) * (double)(y2 - y1) / (double)(x2 - x1));
        x2 = a;
        c2 = 0;
      }
    }
  }
  return (c1 | c2) == 0;
}

__device__ inline bool inside(int W, int H, long long x, long long y) { return x >= 0 && x < W && y >= 0 && y < H; }

struct Edge { long long x, dx; int y0, y1; };
// the PolyEdge CollectPolyEdges makes of the contour edge (X0, Y0) -> (X1, Y1) (shift 0, offset 0, non-antialiased); false: horizontal
__device__ inline bool make_edge(int W, int H, int X0, int Y0, int X1, int Y1, Edge& e) {
  if (Y0 == Y1) return false;
  long long c0x = (long long)X0 * XY_ONE, c1x = (long long)X1 * XY_ONE, c0y = Y0, c1y = Y1;
  if (!inside(W, H, X0, Y0) || !inside(W, H, X1, Y1)) {
    long long t0x = X0, t0y = Y0, t1x = X1, t1y = Y1;
    clip_line(W, H, t0x, t0y, t1x, t1y);
    if (t0y != t1y) { c0y = t0y; c1y = t1y; c0x = t0x * XY_ONE; c1x = t1x * XY_ONE; }
  } else {
    c0x += XY_ONE >> 1;
    c1x += XY_ONE >> 1;
  }
  e.dx = (c1x - c0x) / (c1y - c0y);
  if (Y0 < Y1) { e.y0 = Y0; e.y1 = Y1; e.x = c0x + ((long long)Y0 - c0y) * e.dx; }
  else { e.y0 = Y1; e.y1 = Y0; e.x = c1x + ((long long)Y1 - c1y) * e.dx; }
  return true;
}

// Line(img, p1, p2, color, 8): LineIterator(8-connected, left to right) after clipLine; ORs the pixels that fall on the rows [y_lo, y_hi) into
// `rows`, the bit rows of that window (`pitch` words each, the first one is row y_lo).  The whole plane is the window [0, H).
__device__ inline void draw_line(unsigned* rows, int pitch, int W, int H, int y_lo, int y_hi, int X0, int Y0, int X1, int Y1) {
  long long ax = X0, ay = Y0, bx = X1, by = Y1;
  if (!inside(W, H, ax, ay) || !inside(W, H, bx, by)) {
    if (!clip_line(W, H, ax, ay, bx, by)) return;
  }
  if ((ay < y_lo && by < y_lo) || (ay >= y_hi && by >= y_hi)) return;   // the line does not reach the window
  int dx = (int)(bx - ax), dy = (int)(by - ay), x = (int)ax, y = (int)ay, sy = 1;
  if (dx < 0) { dx = -dx; dy = -dy; x = (int)bx; y = (int)by; }
  if (dy < 0) { dy = -dy; sy = -1; }
  const bool vert = dy > dx;
  if (vert) { const int t = dx; dx = dy; dy = t; }
  int err = dx - (dy + dy);
  const int plus = dx + dx, minus = -(dy + dy);
  for (int k = 0; k <= dx; ++k) {
    // (x and the plane's rows are always in range after the clip; the guard is the bound)
    if (x >= 0 && x < W && y >= y_lo && y < y_hi) lds_or(&rows[(y - y_lo) * pitch + (x >> 5)], 1u << (x & 31));
    const bool neg = err < 0;
    err += minus + (neg ? plus : 0);
    if (vert) { y += sy; x += neg ? 1 : 0; }
    else { x += 1; y += neg ? sy : 0; }
  }
}

// The crossings of edge e with the rows [y_lo, y_hi) of the same window: step 1 toggles the bit at column r + 1, step 3 ORs the bit at r.
__device__ inline void toggle_crossings(unsigned* rows, int pitch, int W, const Edge& e, int y_lo, int y_hi) {
  const int ya = e.y0 > y_lo ? e.y0 : y_lo, yb = e.y1 < y_hi ? e.y1 : y_hi;
  for (int y = ya; y < yb; ++y) {
    const long long c = ((e.x + (long long)((long long)y - e.y0) * e.dx) >> XY_SHIFT) + 1;
    if (c < W) {
      const int cc = c < 0 ? 0 : (int)c;
      lds_xor(&rows[(y - y_lo) * pitch + (cc >> 5)], 1u << (cc & 31));
    }
  }
}
__device__ inline void or_crossings(unsigned* rows, int pitch, int W, const Edge& e, int y_lo, int y_hi) {
  const int ya = e.y0 > y_lo ? e.y0 : y_lo, yb = e.y1 < y_hi ? e.y1 : y_hi;
  for (int y = ya; y < yb; ++y) {
    const long long r = (e.x + (long long)((long long)y - e.y0) * e.dx) >> XY_SHIFT;
    if (r >= 0 && r < W) lds_or(&rows[(y - y_lo) * pitch + (int)(r >> 5)], 1u << (int)(r & 31));
  }
}

// step 2 on one row of W32 words: the toggles become the parity of the toggles to their left (inclusive)
__device__ inline void prefix_xor_row(unsigned* row, int W32) {
  unsigned carry = 0u;
  for (int k = 0; k < W32; ++k) {
    unsigned v = row[k];
    v ^= v << 1; v ^= v << 2; v ^= v << 4; v ^= v << 8; v ^= v << 16;
    if (carry) v = ~v;
    carry = v >> 31;
    row[k] = v;
  }
}

__device__ inline int lower_bound(const int* a, int n, int v) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}
}  // namespace segdata

__global__ __launch_bounds__(segdata::NT)
void y5_polygon_raster_kernel(const segdata::Params p) {
  using namespace segdata;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned* plane = reinterpret_cast<unsigned*>(smem);
  int* s_part = reinterpret_cast<int*>(smem + (size_t)p.H * p.W32 * 4);
  const int inst = blockIdx.x, tid = threadIdx.x;
  const int H = p.H, W = p.W, W32 = p.W32;
  const int o0 = p.poly_off[inst], np = p.poly_off[inst + 1] - o0;
  const double* xy = p.xy + (size_t)o0 * 2;
  for (int i = tid; i < H * W32; i += NT) plane[i] = 0u;
  __syncthreads();
  // 1. crossings -> toggles at r + 1
  for (int i = tid; i < np; i += NT) {
    const int j = i == 0 ? np - 1 : i - 1;
    Edge e;
    if (!make_edge(W, H, trunc_i32(xy[2 * j]), trunc_i32(xy[2 * j + 1]), trunc_i32(xy[2 * i]), trunc_i32(xy[2 * i + 1]), e)) continue;
    toggle_crossings(plane, W32, W, e, 0, H);
  }
  __syncthreads();
  // 2. prefix xor along every row
  for (int y = tid; y < H; y += NT) prefix_xor_row(plane + y * W32, W32);
  __syncthreads();
  // 3. the crossings' own pixels and the edges' lines
  for (int i = tid; i < np; i += NT) {
    const int j = i == 0 ? np - 1 : i - 1;
    const int X0 = trunc_i32(xy[2 * j]), Y0 = trunc_i32(xy[2 * j + 1]), X1 = trunc_i32(xy[2 * i]), Y1 = trunc_i32(xy[2 * i + 1]);
    draw_line(plane, W32, W, H, 0, H, X0, Y0, X1, Y1);
    Edge e;
    if (!make_edge(W, H, X0, Y0, X1, Y1, e)) continue;
    or_crossings(plane, W32, W, e, 0, H);
  }
  __syncthreads();
  // 4. cv2.resize(mask, (w, h)) -> bits, area
  const ResizeGeom g = resize_geom(H, W, p.h, p.w);
  auto src = [&](int y, int x) -> int { return (int)((plane[y * W32 + (x >> 5)] >> (x & 31)) & 1u); };
  unsigned* out = p.bits + (size_t)inst * p.h * p.w32;
  int cnt = 0;
  for (int wd = tid; wd < p.h * p.w32; wd += NT) {
    const int oy = wd / p.w32, wx = wd - oy * p.w32;
    unsigned v = 0u;
    for (int b = 0; b < 32; ++b) {
      const int ox = wx * 32 + b;
      if (ox < p.w && resized_value(H, W, g, oy, ox, src) != 0) v |= 1u << b;
    }
    out[wd] = v;
    cnt += __popcll((unsigned long long)v);
  }
  const int lane = tid & 63;
  for (int k = 32; k >= 1; k >>= 1) cnt += __shfl(cnt, lane ^ k);
  if (lane == 0) s_part[tid >> 6] = cnt;
  __syncthreads();
  if (tid == 0) {
    int t = 0;
    for (int wv = 0; wv < NT / 64; ++wv) t += s_part[wv];
    p.area[inst] = t;
  }
}

// rank of every instance among the instances of its image and the permutation `order` (local label indices, as polygons2masks_overlap returns)
__global__ __launch_bounds__(segdata::NT)
void y5_polygon_rank_kernel(const segdata::Params p) {
  using namespace segdata;
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i >= p.n_inst) return;
  const int b = p.inst_img[i];
  const int lo = lower_bound(p.inst_img, p.n_inst, b), hi = lower_bound(p.inst_img, p.n_inst, b + 1);
  const unsigned long long ki = 0ull - (unsigned long long)p.area[i];
  int r = 0;
  for (int j = lo; j < hi; ++j) {
    const unsigned long long kj = 0ull - (unsigned long long)p.area[j];
    r += (kj < ki || (kj == ki && j < i)) ? 1 : 0;
  }
  p.rank[i] = r;
  p.order[lo + r] = i - lo;
}

// grid (pixels / NT, planes): overlap -> plane = image, value = 1 + the highest rank among the covering instances; else plane = instance, 0 / 1
__global__ __launch_bounds__(segdata::NT)
void y5_polygon_compose_kernel(const segdata::Params p) {
  using namespace segdata;
  const int px = blockIdx.x * NT + threadIdx.x, pl = blockIdx.y;
  if (px >= p.h * p.w) return;
  const int oy = px / p.w, ox = px - oy * p.w;
  const int b = p.overlap ? pl : p.inst_img[pl];
  const bool ok = b >= 0 && b < p.B;
  const int fy = ok && p.flip && p.flip[2 * b] ? p.h - 1 - oy : oy, fx = ok && p.flip && p.flip[2 * b + 1] ? p.w - 1 - ox : ox;
  const size_t word = (size_t)fy * p.w32 + (fx >> 5);
  const unsigned bit = 1u << (fx & 31);
  int v = 0;
  if (p.overlap) {
    const int lo = lower_bound(p.inst_img, p.n_inst, b), hi = lower_bound(p.inst_img, p.n_inst, b + 1);
    for (int i = lo; i < hi; ++i) {
      if (p.bits[(size_t)i * p.h * p.w32 + word] & bit) { const int r = p.rank[i] + 1; v = r > v ? r : v; }
    }
  } else {
    v = (p.bits[(size_t)pl * p.h * p.w32 + word] & bit) ? 1 : 0;
  }
  const size_t o = (size_t)pl * p.h * p.w + px;
  if (p.mask_dtype == Y5_U8) static_cast<unsigned char*>(p.masks)[o] = (unsigned char)v;
  else static_cast<float*>(p.masks)[o] = (float)v;
}

extern "C" size_t y5_polygon_masks_ws_bytes(int n_inst, int H, int W, int ratio) {
  if (n_inst < 0 || H < 1 || W < 1 || ratio < 1) return 0;
  const size_t h = (size_t)(H / ratio), w32 = (size_t)(W / ratio + 31) / 32;
  return ((size_t)n_inst * (h * w32 + 1) * 4 + 255) & ~(size_t)255;
}

extern "C" int y5_polygon_masks(const double* xy, const int* poly_off, const int* inst_img, int n_inst, int B, int H, int W, int ratio, int overlap,
                                const unsigned char* flip, void* masks, int mask_dtype, int* order, long long* area, void* ws, size_t ws_bytes,
                                void* stream_) {
  using namespace segdata;
  if (n_inst < 0 || B < 1 || B > 65535 || n_inst > 65535 * 16 || H < 1 || W < 1 || H > 16384 || W > 16384 || ratio < 1 || H / ratio < 1 || W / ratio < 1)
    return y5_fail(Y5_ERR_BAD_ARG, "polygon_masks: bad n_inst / B / H / W / ratio");
  if (mask_dtype != Y5_U8 && mask_dtype != Y5_F32) return y5_fail(Y5_ERR_BAD_ARG, "polygon_masks: mask dtype must be u8 or f32");
  if (!masks && (overlap || n_inst)) return y5_fail(Y5_ERR_BAD_ARG, "polygon_masks: null masks");
  if (n_inst && (!xy || !poly_off || !inst_img || !order || !area || !ws)) return y5_fail(Y5_ERR_BAD_ARG, "polygon_masks: null pointer");
  if (n_inst && ws_bytes < y5_polygon_masks_ws_bytes(n_inst, H, W, ratio)) return y5_fail(Y5_ERR_WORKSPACE, "polygon_masks: workspace too small");
  Params p{};
  p.xy = xy; p.poly_off = poly_off; p.inst_img = inst_img; p.flip = flip; p.masks = masks; p.order = order; p.area = area;
  p.n_inst = n_inst; p.B = B; p.H = H; p.W = W; p.h = H / ratio; p.w = W / ratio; p.W32 = (W + 31) / 32; p.w32 = (p.w + 31) / 32;
  p.overlap = overlap ? 1 : 0; p.mask_dtype = mask_dtype;
  p.bits = static_cast<unsigned*>(ws);
  p.rank = reinterpret_cast<int*>(p.bits + (size_t)n_inst * p.h * p.w32);
  if (n_inst > 65535 && !overlap) return y5_fail(Y5_ERR_UNSUPPORTED, "polygon_masks: more than 65535 instances without overlap");
  const size_t lds = (size_t)H * p.W32 * 4 + 64;
  if (lds > MAX_LDS) return y5_fail(Y5_ERR_UNSUPPORTED, "polygon_masks: H x W bit plane exceeds the LDS (160 KiB)");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (n_inst) {
    if (lds > 64 * 1024) hipFuncSetAttribute((const void*)y5_polygon_raster_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)MAX_LDS);
    hipLaunchKernelGGL(y5_polygon_raster_kernel, dim3((unsigned)n_inst), dim3(NT), lds, stream, p);
    hipLaunchKernelGGL(y5_polygon_rank_kernel, dim3((unsigned)((n_inst + NT - 1) / NT)), dim3(NT), 0, stream, p);
  }
  const int planes = overlap ? B : n_inst;
  if (planes) hipLaunchKernelGGL(y5_polygon_compose_kernel, dim3((unsigned)((p.h * p.w + NT - 1) / NT), (unsigned)planes), dim3(NT), 0, stream, p);
  return y5_check_launch("y5_polygon_masks");
}
