"""Output rate of process_mask_native_batch (csrc/mask_native.h) at segment/predict.py's shapes with retina_masks: batch 32, prototypes
(32, 160, 160) fp16, 100 instances per image, original images alternating 1080 x 810 and 720 x 1280, float32 and uint8 masks.  Timed with
device events after a warm-up.  Printed beside it, from the same process on the same GPU:
  * process_mask_batch(upsample=True) at 640 x 640 for the same prototypes and instance counts (the kernel the tile shape was taken from);
  * the torch composition of process_mask_native (matmul, sigmoid, slice, F.interpolate, crop, gt_), one image after the other.
The rate is OUTPUT bytes per second: the kernel is bound by the HBM writes of the masks (kernel table).

    python scripts/mask_native_bench.py [--bs 32] [--n 100] [--iters 10]"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from yolov5_amd.segment import native_window, process_mask_batch, process_mask_native_batch  # noqa: E402


def boxes_for(n, h, w, gen):
    xy1 = torch.rand((n, 2), generator=gen) * 0.5 * torch.tensor([w, h])
    wh = (0.05 + 0.45 * torch.rand((n, 2), generator=gen)) * torch.tensor([w, h])
    return torch.cat((xy1, xy1 + wh), 1).round()


def torch_native(protos, masks_in, bboxes, shape):
    """The composition of utils/segment/general.py:54-76 in torch ops on the device."""
    c, mh, mw = protos.shape
    masks = (masks_in @ protos.float().view(c, -1)).sigmoid().view(-1, mh, mw)
    top, left, bottom, right = native_window(mh, mw, shape)
    masks = F.interpolate(masks[None, :, top:bottom, left:right], shape, mode="bilinear", align_corners=False)[0]
    x1, y1, x2, y2 = torch.chunk(bboxes[:, :, None], 4, 1)
    r = torch.arange(shape[1], device=masks.device, dtype=x1.dtype)[None, None, :]
    cc = torch.arange(shape[0], device=masks.device, dtype=x1.dtype)[None, :, None]
    return (masks * ((r >= x1) * (r < x2) * (cc >= y1) * (cc < y2))).gt_(0.5)


def timed(fn, iters, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / iters * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=32)
    ap.add_argument("--n", type=int, default=100)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mask_native_bench needs a GPU")
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    protos = (torch.rand((a.bs, 32, 160, 160), generator=gen) * 2 - 1).half().to(dev)
    shapes = [(1080, 810) if i % 2 == 0 else (720, 1280) for i in range(a.bs)]
    coef = [torch.rand((a.n, 32), generator=gen) * 2 - 1 for _ in range(a.bs)]
    zeros2 = torch.zeros((a.n, 2))
    dets = [torch.cat((boxes_for(a.n, h, w, gen), zeros2, cf), 1).to(dev) for (h, w), cf in zip(shapes, coef)]
    dets640 = [torch.cat((boxes_for(a.n, 640, 640, gen), zeros2, cf), 1).to(dev) for cf in coef]
    px = sum(a.n * h * w for h, w in shapes)
    px640 = a.bs * a.n * 640 * 640
    res = {"bs": a.bs, "instances_per_image": a.n, "shapes": sorted(set(shapes)), "iters": a.iters}
    for name, dt, esz in (("float32", torch.float32, 4), ("uint8", torch.uint8, 1)):
        t = timed(lambda: process_mask_native_batch(protos, dets, shapes, out_dtype=dt), a.iters)
        t6 = timed(lambda: process_mask_batch(protos, dets640, (640, 640), upsample=True, out_dtype=dt), a.iters)
        res[name] = {"native_ms": round(t * 1e3, 3), "native_out_GB": round(px * esz / 1e9, 3), "native_TBps": round(px * esz / t / 1e12, 3),
                     "batch640_ms": round(t6 * 1e3, 3), "batch640_out_GB": round(px640 * esz / 1e9, 3), "batch640_TBps": round(px640 * esz / t6 / 1e12, 3)}
        print(f"[mask_native_bench] {name}: native {t * 1e3:.2f} ms for {px * esz / 1e9:.2f} GB = {px * esz / t / 1e12:.2f} TB/s of output | "
              f"process_mask_batch 640x640 {t6 * 1e3:.2f} ms for {px640 * esz / 1e9:.2f} GB = {px640 * esz / t6 / 1e12:.2f} TB/s", flush=True)

    def torch_loop():
        for i, (d, s) in enumerate(zip(dets, shapes)):
            torch_native(protos[i], d[:, 6:], d[:, :4], s)

    tt = timed(torch_loop, max(1, a.iters // 3), warmup=1)
    res["torch_float32"] = {"ms": round(tt * 1e3, 3), "TBps": round(px * 4 / tt / 1e12, 3)}
    print(f"[mask_native_bench] torch composition (float32, per image): {tt * 1e3:.2f} ms = {px * 4 / tt / 1e12:.2f} TB/s of output", flush=True)
    # same bits as the torch composition, up to pixels within rounding of 0.5
    got = process_mask_native_batch(protos[:2], dets[:2], shapes[:2])
    diff = sum(int((g != torch_native(protos[i], dets[i][:, 6:], dets[i][:, :4], shapes[i])).sum()) for i, g in enumerate(got))
    res["pixels_differing_from_torch"] = [diff, sum(g.numel() for g in got)]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
