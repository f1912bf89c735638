"""Mask-validation timing on one GPU: yolov5s-seg, bs 32, 640^2, NMS at conf_thres 0.001 (full 300-row images), both overlap modes.

    python scripts/seg_val_bench.py [--out profiles/seg_val/bench.json]

Reports, per overlap mode:
  match_ms          y5_val_match_masks (metrics.match_masks_batch, computed bits) per batch, CUDA events, median of 20
  run_ms_per_img    segment_val.run over 4 batches (no loss), wall clock per image, after one warm-up run
  ref_ms_per_img    segment/val.py:274-308's per-image mask path restated with torch ops on the GPU -- process_mask (matmul, sigmoid,
                    crop), the overlap repeat / where, bilinear resize, mask_iou matmul, process_batch with .cpu().numpy() per threshold --
                    on the same NMS output, wall clock per image
The labels are made from the model's own predicted masks (12 per image, at 640^2: the bilinear path), so the matcher finds matches."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import seg_val_ref as sv  # noqa: E402
from tests.test_gpu_seg_train import _data  # noqa: E402
from tests.test_gpu_seg_val import _conditioned, _pred_bits, _targets_from  # noqa: E402
from yolov5_amd import metrics, segment_val  # noqa: E402
from yolov5_amd.general import non_max_suppression  # noqa: E402


def torch_process_mask(protos, masks_in, bboxes, shape):
    """utils/segment/general.py:25-51 (upsample=False) in torch ops."""
    c, mh, mw = protos.shape
    ih, iw = shape
    masks = (masks_in @ protos.float().view(c, -1)).sigmoid().view(-1, mh, mw)
    b = bboxes.clone()
    b[:, 0] *= mw / iw
    b[:, 2] *= mw / iw
    b[:, 3] *= mh / ih
    b[:, 1] *= mh / ih
    x1, y1, x2, y2 = torch.chunk(b[:, :, None], 4, 1)
    r = torch.arange(mw, device=masks.device, dtype=x1.dtype)[None, None, :]
    cc = torch.arange(mh, device=masks.device, dtype=x1.dtype)[None, :, None]
    masks = masks * ((r >= x1) * (r < x2) * (cc >= y1) * (cc < y2))
    return masks.gt_(0.5)


def ref_loop(out, cnt, protos, t, gt, overlap, shape, iouv):
    n_img = out.shape[0]
    for si in range(n_img):
        pred = out[si, : int(cnt[si])]
        labels = t[t[:, 0] == si, 1:]
        nl = labels.shape[0]
        g = gt[[si]] if overlap else gt[t[:, 0] == si]
        g = g.float()
        pm = torch_process_mask(protos[si], pred[:, 6:], pred[:, :4], shape)
        if nl:
            if overlap:
                index = torch.arange(nl, device=g.device).view(nl, 1, 1) + 1
                g = torch.where(g.repeat(nl, 1, 1) == index, 1.0, 0.0)
            if g.shape[1:] != pm.shape[1:]:
                g = F.interpolate(g[None], pm.shape[1:], mode="bilinear", align_corners=False)[0].gt_(0.5)
            iou = sv.mask_iou(g.view(nl, -1), pm.view(pm.shape[0], -1))
            correct_class = labels[:, 0:1] == pred[:, 5]
            correct = np.zeros((pred.shape[0], 10), bool)
            for i in range(10):   # utils/metrics.py:256-265, one host copy per threshold
                x = torch.where((iou >= iouv[i]) & correct_class)
                if x[0].shape[0]:
                    matches = torch.cat((torch.stack(x, 1), iou[x[0], x[1]][:, None]), 1).cpu().numpy()
                    if x[0].shape[0] > 1:
                        matches = matches[matches[:, 2].argsort()[::-1]]
                        matches = matches[np.unique(matches[:, 1], return_index=True)[1]]
                        matches = matches[np.unique(matches[:, 0], return_index=True)[1]]
                    correct[matches[:, 1].astype(int), i] = True
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B, S = 32, 640
    m = _conditioned("yolov5s-seg", dev)
    m.eval()
    x, _, _ = _data(B, S, 1, 5)
    with torch.no_grad():
        z, protos, _ = m(x.to(dev))
    out, cnt = non_max_suppression(z, 0.001, 0.6, multi_label=True, max_det=300, nm=32, padded=True)
    pm = _pred_bits(protos, out, cnt, (S, S))
    iouv = torch.linspace(0.5, 0.95, 10, device=dev)
    res = dict(model="yolov5s-seg", bs=B, imgsz=S, conf_thres=0.001, rows=int(cnt.sum()), device=torch.cuda.get_device_name(0))
    for overlap in (True, False):
        t, gt = _targets_from(out, cnt, pm, 12, overlap, 4, 3)
        t, gt = t.to(dev), gt.to(dev)
        key = "overlap" if overlap else "per_instance"
        for _ in range(3):
            metrics.match_masks_batch(out, cnt, protos, t, gt, iouv, overlap, (S, S))
        ms = []
        for _ in range(20):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            c = metrics.match_masks_batch(out, cnt, protos, t, gt, iouv, overlap, (S, S))
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        ref_loop(out, cnt, protos, t, gt, overlap, (S, S), iouv)  # warm-up
        t0 = time.perf_counter()
        ref_loop(out, cnt, protos, t, gt, overlap, (S, S), iouv)
        ref = (time.perf_counter() - t0) / B * 1e3
        tn = t.clone()
        tn[:, 2:] /= S
        batches = [((x * 255).round().to(torch.uint8), tn, None, None, gt)] * 4
        segment_val.run(m, batches, half=True, overlap=overlap)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r, _, _ = segment_val.run(m, batches, half=True, overlap=overlap)
        torch.cuda.synchronize()
        run = (time.perf_counter() - t0) / (4 * B) * 1e3
        res[key] = dict(labels=int(t.shape[0]), matches_at_05=int(c[..., 0].sum()), match_ms=float(np.median(ms)), match_ms_min=float(min(ms)),
                        run_ms_per_img=run, ref_ms_per_img=ref, mask_map50=float(r[6]))
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
