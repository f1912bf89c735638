"""TEST INFRASTRUCTURE ONLY: NumPy restatements for train.py's `--quad` and `--multi-scale` (tests/test_emu_multiscale_quad.py and its GPU twin).

  * `collate4_images`: the image half of `LoadImagesAndLabels.collate_fn4` (utils/dataloaders.py:865-891) -- per group of four, by a flag, the
    2x bilinear upsample (align_corners=False) of the first image in fp32 on the byte values, truncated to uint8, or the 2 x 2 tiling with
    images 4i / 4i + 1 in the left column and 4i + 2 / 4i + 3 in the right one.  With a scale of exactly 2 the interpolation weights are 0,
    1/4, 3/4 and 1: every product and sum is exact in fp32, so this file, torch's CPU F.interpolate and csrc/collate4.h agree bit for bit
    (tests/golden/quad.npz holds the reference's own output).
  * `collate4_labels`: the label half, in float32, the reference's operand order.
  * `multi_scale_sizes`: the draws of train.py:394-397 from a `random.Random`.
"""
import math

import numpy as np


def _axis(out_size, in_size):
    """Source taps of F.interpolate(scale_factor=2, mode="bilinear", align_corners=False) along one axis: (i0, i1, weight of i1) in fp32."""
    o = np.arange(out_size, dtype=np.float32)
    src = np.maximum(np.float32(0.5) * (o + np.float32(0.5)) - np.float32(0.5), np.float32(0.0))
    i0 = np.floor(src).astype(np.int64)
    i1 = np.minimum(i0 + 1, in_size - 1)
    return i0, i1, (src - i0.astype(np.float32)).astype(np.float32)


def upsample2x(im):
    """(C, H, W) uint8 -> (C, 2H, 2W) uint8: `F.interpolate(im[None].float(), scale_factor=2.0, ...)[0].type(uint8)` (:878-880)."""
    C, H, W = im.shape
    y0, y1, ly = _axis(2 * H, H)
    x0, x1, lx = _axis(2 * W, W)
    f = im.astype(np.float32)
    ly, lx = ly[None, :, None], lx[None, None, :]
    one = np.float32(1.0)
    top = (one - lx) * f[:, y0][:, :, x0] + lx * f[:, y0][:, :, x1]
    bot = (one - lx) * f[:, y1][:, :, x0] + lx * f[:, y1][:, :, x1]
    v = (one - ly) * top + ly * bot
    assert v.dtype == np.float32 and v.min() >= 0 and v.max() <= 255
    return v.astype(np.uint8)   # truncation, like .type(torch.uint8) of a non-negative float


def collate4_images(imgs, flags):
    """imgs (B, C, H, W) uint8, flags: B // 4 booleans (True = upsample) -> (B // 4, C, 2H, 2W) uint8."""
    out = []
    for i, up in enumerate(flags):
        a, b, c, d = imgs[4 * i:4 * i + 4]
        out.append(upsample2x(a) if up else np.concatenate((np.concatenate((a, b), 1), np.concatenate((c, d), 1)), 2))   # :883
    return np.stack(out, 0)


def collate4_labels(targets, flags):
    """targets (nt, 6) float32 [image index in batch, cls, xc, yc, w, h] -> the (nt', 6) float32 targets of the quad batch (:872-889)."""
    t = np.asarray(targets, np.float32)
    ho = np.array([[0.0, 0, 0, 1, 0, 0]], np.float32)
    wo = np.array([[0.0, 0, 1, 0, 0, 0]], np.float32)
    s = np.array([[1, 1, 0.5, 0.5, 0.5, 0.5]], np.float32)
    out = []
    for i, up in enumerate(flags):
        a, b, c, d = (t[t[:, 0] == 4 * i + k].copy() for k in range(4))
        lb = a if up else np.concatenate((a, b + ho, c + wo, d + ho + wo), 0) * s
        lb[:, 0] = i
        out.append(lb.astype(np.float32))
    return np.concatenate(out, 0) if out else np.zeros((0, 6), np.float32)


def multi_scale_sizes(rng, imgsz, gs, n, hw):
    """n draws of train.py:394-397 for batches of size hw = (h, w): [(sz, sf, ns or None when sf == 1)]."""
    out = []
    for _ in range(n):
        sz = rng.randrange(int(imgsz * 0.5), int(imgsz * 1.5) + gs) // gs * gs
        sf = sz / max(hw)
        out.append((sz, sf, None if sf == 1 else tuple(math.ceil(x * sf / gs) * gs for x in hw)))
    return out


def byte_patterns(B, C, H, W, seed=0):
    """uint8 images that put 0 and 255 next to each other (checkerboards, stripes, single hot pixels) among random bytes: every blend of the two
    ends with the quarter weights (63.75, 191.25, 143.4375 ...) has a fraction, so truncation, rounding and saturation all differ."""
    rng = np.random.default_rng(seed)
    im = rng.integers(0, 256, (B, C, H, W), dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    for b in range(B):
        k = b % 4
        if k == 0:
            im[b, 0] = ((yy + xx) % 2 * 255).astype(np.uint8)
        elif k == 1:
            im[b, 1] = (xx % 2 * 255).astype(np.uint8)
        elif k == 2:
            im[b, 2] = (yy % 2 * 255).astype(np.uint8)
        im[b, b % C, 0, 0], im[b, b % C, H - 1, W - 1] = 255, 0
        if W > 1:
            im[b, (b + 1) % C, 0, W - 1], im[b, (b + 1) % C, H - 1, 0] = 0, 255
    return im
