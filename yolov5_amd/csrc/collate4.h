// The image half of `LoadImagesAndLabels.collate_fn4` (utils/dataloaders.py:865-891, train.py --quad) for a whole batch in ONE launch.
// The reference turns every group of four (C, H, W) uint8 images 4i .. 4i + 3 into one (C, 2H, 2W) image, by a coin per group:
//   flag 1: F.interpolate(im[4i][None].float(), scale_factor=2.0, mode="bilinear", align_corners=False)[0].type(im[4i].type())  (:878-880)
//   flag 0: torch.cat((torch.cat((im[4i], im[4i + 1]), 1), torch.cat((im[4i + 2], im[4i + 3]), 1)), 2)                          (:883)
//           -- 4i over 4i + 1 in the LEFT column, 4i + 2 over 4i + 3 in the RIGHT column.
// The coins are the host's (yolov5_amd/dataloaders.py `collate_fn4`, Python's `random`), handed over as n = B / 4 bytes on the device.
//
// Upsample by exactly 2, align_corners = False: the source coordinate of output x is x / 2 - 1 / 4 clamped at 0, so an even output 2k blends
// source k - 1 and k with weights 1/4, 3/4 and an odd output 2k + 1 blends k and k + 1 with 3/4, 1/4; a neighbour past the border is the border
// pixel itself.  The weights and their pairwise products are multiples of 1/16 and the values are bytes: every product and every partial sum
// is exact in fp32 (at most 8 + 4 significant bits), so the result does not depend on the evaluation order or on FMA contraction and the
// kernel, torch's CPU kernel and the NumPy restatement (tests/quad_ref.py) agree bit for bit.  `.type(uint8)` of a non-negative float is a
// truncation: (unsigned char)v.
//
// One lane writes 16 consecutive output bytes of one output row.  W % 16 == 0 (every loader canvas: a multiple of the model stride): a chunk
// never straddles the two columns of the tiling, so flag 0 is one 16-byte load and one 16-byte store; flag 1 reads the 8 source bytes under
// its chunk plus the neighbour on either side from its two source rows once (8-byte loads: W % 16 == 0 keeps them aligned), blends the two rows
// into 10 fp32 values and those into the 16 outputs.  Any other W takes the byte-wise form of the same arithmetic.  Memory-bound: 1 byte read
// and 1 written per output byte (tiling), 1/4 read per output byte (upsample; the second source row of a lane is its row neighbour's first and
// comes from L2).
#pragma once

namespace collate4 {
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

struct Params {
  const unsigned char* src;     // (B, C, H, W)
  const unsigned char* flags;   // (n): 1 = upsample image 4i, 0 = tile images 4i .. 4i + 3
  unsigned char* dst;           // (n, C, 2H, 2W)
  int n, C, H, W, chunks;       // chunks = ceil(2W / 16) lanes per output row
  long long lanes;              // n * C * 2H * chunks
};

// source rows (y0, y1) and the weight of y1 (in quarters) of output row oy; the same rule serves the columns
__device__ inline void taps(int o, int size, int& i0, int& i1, float& l1) {
  const int r = o >> 1;
  if (o & 1) { i0 = r; i1 = r + 1 < size ? r + 1 : size - 1; l1 = 0.25f; }
  else       { i0 = r > 0 ? r - 1 : 0; i1 = r; l1 = 0.75f; }
}
}  // namespace collate4

template <bool VEC>
__global__ __launch_bounds__(256)
void y5_collate4_kernel(const collate4::Params p) {
  using namespace collate4;
  const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
  if (id >= p.lanes) return;
  const int H = p.H, W = p.W, OW = 2 * W;
  const int ck = (int)(id % p.chunks);
  const long long row = id / p.chunks;               // (i * C + c) * 2H + oy
  const int oy = (int)(row % (2 * H));
  const long long pc = row / (2 * H);                // i * C + c
  const int c = (int)(pc % p.C), i = (int)(pc / p.C);
  const int ox0 = ck * 16;
  unsigned char* out = p.dst + row * OW + ox0;
  const size_t plane = (size_t)H * W;
  if (!p.flags[i]) {
    const int sy = oy < H ? oy : oy - H, dn = oy < H ? 0 : 1;
    if (VEC) {
      const int rt = ox0 < W ? 0 : 2;
      const unsigned char* s = p.src + ((size_t)(4 * i + dn + rt) * p.C + c) * plane + (size_t)sy * W + (ox0 - (rt ? W : 0));
      *reinterpret_cast<u32x4*>(out) = *reinterpret_cast<const u32x4*>(s);
    } else {
      for (int k = 0; k < 16 && ox0 + k < OW; ++k) {
        const int ox = ox0 + k, rt = ox < W ? 0 : 2;
        out[k] = p.src[((size_t)(4 * i + dn + rt) * p.C + c) * plane + (size_t)sy * W + (ox - (rt ? W : 0))];
      }
    }
    return;
  }
  int y0, y1;
  float ly;
  taps(oy, H, y0, y1, ly);
  const unsigned char* r0 = p.src + ((size_t)(4 * i) * p.C + c) * plane + (size_t)y0 * W;
  const unsigned char* r1 = p.src + ((size_t)(4 * i) * p.C + c) * plane + (size_t)y1 * W;
  if (VEC) {
    const int sx = ck * 8;                           // source bytes sx .. sx + 7 lie under the chunk; sx - 1 and sx + 8 beside it (clamped)
    const int xl = sx > 0 ? sx - 1 : 0, xr = sx + 8 < W ? sx + 8 : W - 1;
    const u32x2 a = *reinterpret_cast<const u32x2*>(r0 + sx), b = *reinterpret_cast<const u32x2*>(r1 + sx);
    float v[10];
    v[0] = (1.f - ly) * (float)r0[xl] + ly * (float)r1[xl];
    v[9] = (1.f - ly) * (float)r0[xr] + ly * (float)r1[xr];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const unsigned ta = (k < 4 ? a.x : a.y) >> (8 * (k & 3)) & 0xffu, tb = (k < 4 ? b.x : b.y) >> (8 * (k & 3)) & 0xffu;
      v[k + 1] = (1.f - ly) * (float)ta + ly * (float)tb;
    }
    unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const unsigned e = (unsigned)(unsigned char)(0.25f * v[k] + 0.75f * v[k + 1]);        // output 2k: sources k - 1, k
      const unsigned o = (unsigned)(unsigned char)(0.75f * v[k + 1] + 0.25f * v[k + 2]);    // output 2k + 1: sources k, k + 1
      w[k >> 1] |= (e | o << 8) << (16 * (k & 1));
    }
    u32x4 q;
    q.x = w[0]; q.y = w[1]; q.z = w[2]; q.w = w[3];
    *reinterpret_cast<u32x4*>(out) = q;
  } else {
    for (int k = 0; k < 16 && ox0 + k < OW; ++k) {
      int x0, x1;
      float lx;
      taps(ox0 + k, W, x0, x1, lx);
      const float t = (1.f - lx) * (float)r0[x0] + lx * (float)r0[x1], u = (1.f - lx) * (float)r1[x0] + lx * (float)r1[x1];
      out[k] = (unsigned char)((1.f - ly) * t + ly * u);
    }
  }
}

extern "C" int y5_collate4(const unsigned char* src, int B, int Cn, int H, int W, const unsigned char* flags_dev, unsigned char* dst, void* stream_) {
  using namespace collate4;
  if (!src || !flags_dev || !dst) return y5_fail(Y5_ERR_BAD_ARG, "collate4: null pointer");
  if (B < 4 || Cn < 1 || H < 1 || W < 1 || H > (1 << 20) || W > (1 << 20)) return y5_fail(Y5_ERR_BAD_ARG, "collate4: need B >= 4, C, H, W >= 1");
  Params p{};
  p.src = src; p.flags = flags_dev; p.dst = dst; p.n = B / 4; p.C = Cn; p.H = H; p.W = W;
  p.chunks = (2 * W + 15) / 16;
  p.lanes = (long long)p.n * Cn * 2 * H * p.chunks;
  const long long blocks = (p.lanes + 255) / 256;
  if (blocks > 0x7fffffffLL) return y5_fail(Y5_ERR_UNSUPPORTED, "collate4: output too large");
  // the 16-byte form needs W % 16 == 0 and 16-byte aligned tensors (the 8-byte source loads then are aligned as well)
  const bool vec = W % 16 == 0 && (reinterpret_cast<size_t>(src) | reinterpret_cast<size_t>(dst)) % 16 == 0;
  hipStream_t st = static_cast<hipStream_t>(stream_);
  if (vec) hipLaunchKernelGGL(y5_collate4_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, st, p);
  else hipLaunchKernelGGL(y5_collate4_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, p);
  return y5_check_launch("y5_collate4");
}
