"""Segmentation input-pipeline timing on one GPU: a full-size training batch (64 x 640^2 from 16 frames of 1280 x 720, 8 polygons each,
overlap masks at ratio 4), all four figures in ONE process after warm-up.

    python scripts/seg_data_bench.py [--out profiles/seg_data/bench.json]

  masks_us        (a) device time of the y5_polygon_masks launches (csrc/seg_data.h), events, median of 20
  mosaic_us       (b) device time of the y5_mosaic_batch launch on the same batch, events, median of 20: the yardstick of (a)
  loader_ms       (c) host wall time per SegMosaicLoader batch, ending in a synchronise, mean over one epoch after a warm-up epoch;
                      geometry_ms / upload_masks_ms: its host stages (polygon geometry; uploads + mask launches + the order read)
  step_ms         (d) yolov5s-seg training step (forward, loss, backward, fused optimizer) at the same batch size, mean of 5 after 2
The loader is called synchronously between steps, so its host time is hidden only if (c) < (d): `hidden` says whether it holds."""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import augment_oracle as ao, yolo_oracle as yo  # noqa: E402
from tests import seg_data_ref as sd  # noqa: E402
from yolov5_amd import dataloaders as D, train_loop  # noqa: E402


def events(fn, n=20):
    ms = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)) * 1e3, float(min(ms)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    s, n, B = 640, 16, 64
    ims, classes, segments = sd.full_size_dataset(n, per=8, seed=7)
    labels = [D.labels_from_segments(c, sg) for c, sg in zip(classes, segments)]
    ims_t = [torch.from_numpy(im).to(dev) for im in ims]
    hyp = dict(ao.HYP_AUG)
    random.seed(13); np.random.seed(13)
    draws = [D.draw_sample_seg(i % n, n, s, hyp) for i in range(B)]
    t0 = time.perf_counter()
    jobs, labs, polys, inst = D.seg_mosaic_geometry(ims_t, labels, segments, draws, s, hyp)
    geometry_ms = (time.perf_counter() - t0) * 1e3
    flips = [(bool(d["flipud"]), bool(d["fliplr"])) for d in draws]
    res = dict(bs=B, imgsz=s, instances=len(polys), device=torch.cuda.get_device_name(0), geometry_ms=geometry_ms)

    # (a): the launches alone -- inputs resident, as polygon_masks hands them over
    nI = len(polys)
    off = np.zeros(nI + 1, np.int32)
    np.cumsum([len(p) for p in polys], out=off[1:])
    xy = torch.from_numpy(np.concatenate(polys, 0)).to(dev)
    meta = torch.from_numpy(np.concatenate((off, np.asarray(inst, np.int32)))).to(dev)
    fl = torch.from_numpy(np.asarray(flips, np.uint8)).to(dev)
    masks = torch.empty((B, s // 4, s // 4), dtype=torch.uint8, device=dev)
    order = torch.empty(nI, dtype=torch.int32, device=dev)
    area = torch.empty(nI, dtype=torch.int64, device=dev)
    lib = D._lib.lib()
    nb = int(lib.y5_polygon_masks_ws_bytes(nI, s, s, 4))
    ws = D._lib.workspace(nb, dev)
    C = D.C

    def launch_masks():
        D._lib.check(lib.y5_polygon_masks(C.c_void_p(xy.data_ptr()), C.c_void_p(meta.data_ptr()), C.c_void_p(meta.data_ptr() + 4 * (nI + 1)), nI, B,
                                          s, s, 4, 1, C.c_void_p(fl.data_ptr()), C.c_void_p(masks.data_ptr()), D._lib.Y5_U8,
                                          C.c_void_p(order.data_ptr()), C.c_void_p(area.data_ptr()), C.c_void_p(ws.data_ptr()), nb, D._lib.stream(dev)), lib)

    table = torch.frombuffer(bytearray(jobs), dtype=torch.uint8).to(dev)
    out = torch.empty((B, 3, s, s), dtype=torch.float16, device=dev)

    def launch_mosaic():
        D._lib.check(lib.y5_mosaic_batch(C.c_void_p(table.data_ptr()), B, s, 114, C.c_void_p(out.data_ptr()), D._lib.Y5_F16, 1, D._lib.stream(dev)), lib)

    for _ in range(3):
        launch_masks(); launch_mosaic()
    res["masks_us"], res["masks_us_min"] = events(launch_masks)
    res["mosaic_us"], res["mosaic_us_min"] = events(launch_mosaic)

    t0 = time.perf_counter()
    for _ in range(3):
        D.polygon_masks(polys, inst, B, s, s, 4, True, flips, dev)
    torch.cuda.synchronize()
    res["upload_masks_ms"] = (time.perf_counter() - t0) / 3 * 1e3

    # (c)
    loader = D.SegMosaicLoader(ims_t * 8, labels * 8, segments * 8, img_size=s, batch_size=B, hyp=hyp, dtype=torch.float16, overlap=True, mask_ratio=4)
    for _ in loader:
        pass
    torch.cuda.synchronize()
    t0, k = time.perf_counter(), 0
    for batch in loader:
        torch.cuda.synchronize()
        k += 1
    res["loader_ms"] = (time.perf_counter() - t0) / k * 1e3

    # (d)
    from yolov5_amd.yolo import SegmentationModel

    cfg = yo.model_cfg("yolov5s-seg")
    m = SegmentationModel("yolov5s-seg.yaml")
    m.load_state_dict(yo.det_state_dict(cfg, 0, fused=False))
    m.hyp = dict(yo.HYP_SCRATCH_LOW)
    m = m.to(dev).train()
    imgs, targets, _ = D.seg_mosaic_batch(ims_t, labels, segments, draws, s, hyp, dtype=torch.uint8, overlap=True, mask_ratio=4)[0:3]
    step_batches = [(imgs, targets, None, None, masks.clone())] * 7
    t_steps = []

    class Timed(list):
        def __iter__(self):
            for b in list.__iter__(self):
                torch.cuda.synchronize()
                t_steps.append(time.perf_counter())
                yield b

    train_loop.train(m, Timed(step_batches), hyp=dict(train_loop.HYP_SCRATCH_LOW), epochs=1, batch_size=B, nbs=B, ema=True)
    torch.cuda.synchronize()
    t_steps.append(time.perf_counter())
    d = np.diff(t_steps)[2:]
    res["step_ms"] = float(d.mean()) * 1e3
    res["hidden"] = bool(res["loader_ms"] < res["step_ms"])
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
