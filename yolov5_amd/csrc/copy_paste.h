// Copy-paste augmentation of the mosaic loaders (utils/augmentations.py:200-222 `copy_paste`, called from both `load_mosaic`s after the
// clip and before random_perspective: utils/dataloaders.py:842, utils/segment/dataloaders.py:280).  The reference draws the ACCEPTED original
// polygons of a mosaic into a zero image (cv2.drawContours(..., FILLED)), flips image and raster left-right and copies the flipped image
// where the flipped raster is set: canvas pixel (y, x) becomes the un-pasted canvas pixel (y, w - 1 - x) wherever the raster covers
// (y, w - 1 - x).  The renderer (augment.hip) never materialises the canvas, so the paste is a redirect inside `canvas_pixel`, driven by ONE
// BIT PLANE per pasting mosaic that `y5_paste_planes` makes here; the host (yolov5_amd/dataloaders.py `_copy_paste`) draws the sample, runs
// the bbox_ioa acceptance and hands over the accepted polygons, truncated with the reference's own astype(np.int32).
// drawContours(FILLED) of one contour is CollectPolyEdges + FillEdgeCollection with line type 8 and shift 0 -- the fill of cv2.fillPoly that
// seg_data.h restates (published source, parity unpinned by necessity); its edge, line and crossing helpers are used here on a row window.
//
// seg_data.h keeps a whole plane in LDS; the 2s x 2s canvas of s = 640 is 1280 x 40 words = 204 800 B and does not fit in 160 KiB.  So the
// plane is cut into ROW BANDS of BAND rows: grid (bands, planes), one workgroup per band.  The fill rule is row-local (a row's bits depend on
// the crossings of that row and on the line pixels that fall on it), so a band needs no neighbour.  Per polygon of the plane, in the band:
//   1. every (edge, row) crossing toggles the bit at column r + 1 of a scratch band (LDS xor);
//   2. a prefix-xor along each row of the scratch band;
//   3. the crossings' own bits and the band's part of every edge's Bresenham line are ORed in;
//   4. the scratch band is ORed into the accumulated band and cleared.
// A polygon is a few hundred rows tall at most while the canvas has 2s / BAND bands, so a pre-pass over the plane's edges first marks, in an
// LDS bit map, the polygons that have an edge reaching the band (the y range of an edge's end points bounds its crossings and its clipped
// line); the loop skips the others -- uniformly over the workgroup, without a barrier.  Polygons past the first MAX_MARKED of a plane are
// never skipped.
// The parity fill is per polygon and the polygons are united afterwards: xor-ing two overlapping polygons into one plane would cancel
// their intersection.  At the end the accumulated band goes to memory with plain stores that cover every word of the band (a plane without
// polygons is written as zeros: no memset), bits at x >= S2 of the last word cleared.  No global atomics: every output word has ONE writer
// and the LDS updates are commutative (xor / or), so the result does not depend on scheduling.
// LDS: two bands of BAND x pitch words, pitch = W32 | 1.  In step 2 lane r walks row r, so the lanes of a wave access words r * pitch + k:
// with the natural pitch of 40 words (s = 640) that is 8 distinct banks of the 32 a ds_write_b32 / ds_read_b32 half-wave spreads over (40 mod 32
// = 8): an 8-way conflict; an odd pitch puts the 32 rows on 32 different banks.  s = 640: 2 x 32 x 41 x 4 + 128 = 10 624 B per workgroup.
#pragma once
#include "seg_data.h"

namespace copypaste {
constexpr int BAND = 32;        // rows per workgroup (of segdata::NT lanes) = lanes of step 2
constexpr int MAX_S2 = 8160;    // two bands of 32 x 255 words + the bit map = 65 408 B: the largest side within the 64 KiB a launch gets without asking
constexpr int MAX_MARKED = 1024;   // polygons of a plane the band's bit map covers

struct Params {
  const int* pts;          // (poly_off[n_poly], 2) int32 canvas points
  const int* poly_off;     // (n_poly + 1)
  const int* poly_plane;   // (n_poly) ascending
  unsigned* planes;        // (n_planes, S2, W32)
  int n_poly, n_planes, S2, W32, pitch;
};
}  // namespace copypaste

__global__ __launch_bounds__(segdata::NT)
void y5_paste_planes_kernel(const copypaste::Params p) {
  using namespace copypaste;
  using namespace segdata;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned* acc = reinterpret_cast<unsigned*>(smem);
  unsigned* scr = acc + BAND * p.pitch;
  unsigned* marked = scr + BAND * p.pitch;   // MAX_MARKED bits
  const int tid = threadIdx.x, pl = blockIdx.y;
  const int S2 = p.S2, W32 = p.W32, pitch = p.pitch;
  const int y_lo = blockIdx.x * BAND, y_hi = y_lo + BAND < S2 ? y_lo + BAND : S2, rows = y_hi - y_lo;
  const int q0 = lower_bound(p.poly_plane, p.n_poly, pl), q1 = lower_bound(p.poly_plane, p.n_poly, pl + 1);   // uniform over the workgroup
  for (int i = tid; i < 2 * BAND * pitch + MAX_MARKED / 32; i += NT) acc[i] = 0u;
  __syncthreads();
  if (q1 > q0) {
    const int i0 = p.poly_off[q0], i1 = p.poly_off[q1];
    for (int i = i0 + tid; i < i1; i += NT) {   // edge (previous point of its polygon -> point i)
      const int k = lower_bound(p.poly_off + q0, q1 - q0 + 1, i + 1) - 1;   // poly_off[q0 + k] <= i < poly_off[q0 + k + 1]
      if (k >= MAX_MARKED) continue;
      const int o0 = p.poly_off[q0 + k], j = i == o0 ? p.poly_off[q0 + k + 1] - 1 : i - 1;
      const int ya = p.pts[2 * j + 1], yb = p.pts[2 * i + 1];
      if ((ya > yb ? ya : yb) >= y_lo && (ya < yb ? ya : yb) < y_hi) lds_or(&marked[k >> 5], 1u << (k & 31));
    }
  }
  __syncthreads();
  for (int q = q0; q < q1; ++q) {
    const int k = q - q0;
    if (k < MAX_MARKED && !((marked[k >> 5] >> (k & 31)) & 1u)) continue;   // no edge of the polygon reaches the band
    const int o0 = p.poly_off[q], np = p.poly_off[q + 1] - o0;
    const int* xy = p.pts + (size_t)o0 * 2;
    for (int i = tid; i < np; i += NT) {
      const int j = i == 0 ? np - 1 : i - 1;
      Edge e;
      if (make_edge(S2, S2, xy[2 * j], xy[2 * j + 1], xy[2 * i], xy[2 * i + 1], e)) toggle_crossings(scr, pitch, S2, e, y_lo, y_hi);
    }
    __syncthreads();
    for (int r = tid; r < rows; r += NT) prefix_xor_row(scr + r * pitch, W32);
    __syncthreads();
    for (int i = tid; i < np; i += NT) {
      const int j = i == 0 ? np - 1 : i - 1;
      draw_line(scr, pitch, S2, S2, y_lo, y_hi, xy[2 * j], xy[2 * j + 1], xy[2 * i], xy[2 * i + 1]);
      Edge e;
      if (make_edge(S2, S2, xy[2 * j], xy[2 * j + 1], xy[2 * i], xy[2 * i + 1], e)) or_crossings(scr, pitch, S2, e, y_lo, y_hi);
    }
    __syncthreads();
    for (int i = tid; i < rows * pitch; i += NT) {
      acc[i] |= scr[i];
      scr[i] = 0u;
    }
    __syncthreads();
  }
  const unsigned tail = (S2 & 31) ? (1u << (S2 & 31)) - 1u : 0xffffffffu;
  unsigned* out = p.planes + ((size_t)pl * S2 + y_lo) * W32;
  for (int i = tid; i < rows * W32; i += NT) {
    const int r = i / W32, k = i - r * W32;
    const unsigned v = acc[r * pitch + k];
    out[i] = k == W32 - 1 ? v & tail : v;
  }
}

extern "C" int y5_paste_planes(const int* pts, const int* poly_off, const int* poly_plane, int n_poly, int n_planes, int S2, unsigned* planes,
                               void* stream_) {
  using namespace copypaste;
  using segdata::NT;
  if (n_poly < 0 || n_planes < 1 || n_planes > 65535 || S2 < 2 || S2 > MAX_S2) return y5_fail(Y5_ERR_BAD_ARG, "paste_planes: bad n_poly / n_planes / S2");
  if (!planes || (n_poly && (!pts || !poly_off || !poly_plane))) return y5_fail(Y5_ERR_BAD_ARG, "paste_planes: null pointer");
  Params p{};
  p.pts = pts; p.poly_off = poly_off; p.poly_plane = poly_plane; p.planes = planes;
  p.n_poly = n_poly; p.n_planes = n_planes; p.S2 = S2; p.W32 = (S2 + 31) / 32; p.pitch = p.W32 | 1;
  const size_t lds = (size_t)2 * BAND * p.pitch * 4 + MAX_MARKED / 8;
  hipLaunchKernelGGL(y5_paste_planes_kernel, dim3((unsigned)((S2 + BAND - 1) / BAND), (unsigned)n_planes), dim3(NT), lds, static_cast<hipStream_t>(stream_), p);
  return y5_check_launch("y5_paste_planes");
}
