"""The reference's segmentation validation loop (segment/val.py:run, :202-331 set-up, batch loop and metrics, :389-390 return value) for a
model already on the device, composed like val_loop.run.  Not the CLI: no dataset yaml, plots, txt / json / RLE export, confusion matrix.

    (mp_b, mr_b, map50_b, map_b, mp_m, mr_m, map50_m, map_m, box, seg, obj, cls), maps, (pre-process, inference, NMS ms per image)

MI355X mapping, per batch: forward plan -> `non_max_suppression(..., nm=32, padded=True)` (no host sync) -> `SegValStats.update` = ONE
`y5_val_match` (boxes: both scale_boxes calls, xywh2xyxy, process_batch) and ONE `y5_val_match_masks` (masks: process_mask(upsample=False)
fused into process_batch(masks=True), the ground truth's overlap decode and bilinear resize included) for the whole batch.  The per-image
loop of segment/val.py:274-311 and its host syncs per image and IoU threshold do not exist; the statistics stay on the device until
`compute()`, and ap_per_class_box_and_mask runs on the host once per run as in the reference.
"""
from __future__ import annotations

import time

import numpy as np
import torch

from .general import non_max_suppression
from .metrics import match_batch, match_masks_batch
from .segment_metrics import Metrics, ap_per_class_box_and_mask


def _sync(device):
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize(device)


class SegValStats:
    """The `stats` list of segment/val.py:240,308 -- (correct_masks, correct_bboxes, conf, pcls, tcls) per batch -- on the device until
    `compute()`."""

    def __init__(self, iouv, overlap=False):
        self.iouv, self.overlap = iouv, overlap
        self.cm, self.cb, self.conf, self.pcls, self.tcls = [], [], [], [], []
        self.seen = 0

    def update(self, out, counts, protos, targets, masks, shape, shapes=None):
        """out/counts: padded NMS result of one batch (nm coefficient columns); protos (bs, nm, mh, mw); targets (M, 6) in letterboxed
        pixels; masks as the dataloader gives them; shape: the letterboxed input (h, w); shapes as in metrics.match_batch."""
        bs, max_det, _ = out.shape
        cb = match_batch(out, counts, targets, shapes, self.iouv)
        cm = match_masks_batch(out, counts, protos, targets, masks, self.iouv, self.overlap, shape)
        valid = torch.arange(max_det, device=out.device)[None, :] < counts.to(out.device)[:, None]
        self.cm.append(cm[valid].bool())
        self.cb.append(cb[valid].bool())
        self.conf.append(out[..., 4][valid])
        self.pcls.append(out[..., 5][valid])
        self.tcls.append(targets[:, 1].to(out.device))
        self.seen += bs

    def compute(self, nc=None):
        """segment/val.py:319-323 -> (Metrics, nt)."""
        metrics = Metrics()
        if not self.cm:
            return metrics, np.zeros(nc or 0, int)
        st = [torch.cat(x).cpu().numpy() for x in (self.cm, self.cb, self.conf, self.pcls, self.tcls)]
        if len(st) and st[0].any():
            metrics.update(ap_per_class_box_and_mask(*st))
        return metrics, np.bincount(st[4].astype(int), minlength=nc or 0)


def run(model, dataloader, conf_thres=0.001, iou_thres=0.6, max_det=300, half=True, single_cls=False, compute_loss=None, nc=None,
        overlap=False, training=True, profile=False, retina_masks=False, save_json=False, plots=False, augment=False, save_hybrid=False):
    """segment/val.py:run for a model that is already on the device.

    dataloader yields (im uint8|float BCHW, targets (M, 6) [img, cls, x, y, w, h] normalised, paths, shapes, masks): masks (bs, gh, gw)
    index maps with overlap=True (value k + 1 = the k-th label of the image in target order), else (M, gh, gw) 0/1 in target order; shapes as
    val_loop.run takes them, or None.  `half`: the model is converted IN PLACE for the run and back to float afterwards (segment/val.py:
    187,388), as val_loop.run does.  compute_loss((train_out, protos), targets, masks)[1] accumulates (box, seg, obj, cls)."""
    for flag, what in ((retina_masks, "retina_masks (process_mask_native)"), (save_json, "save_json / COCO RLE export"), (plots, "plots"),
                       (augment, "augment"), (save_hybrid, "save_hybrid")):
        if flag:
            raise NotImplementedError(f"segment_val.run: {what} is not implemented")
    device = next(model.parameters()).device
    was_training = model.training
    model.half() if half else model.float()
    model.eval()
    det = model.model[-1]
    nm = int(getattr(det, "nm", 32))
    if nc is None:
        nc = 1 if single_cls else int(getattr(det, "nc", 80))
    iouv = torch.linspace(0.5, 0.95, 10, device=device)
    stats = SegValStats(iouv, overlap)
    loss = torch.zeros(4, device=device)
    dt = [0.0, 0.0, 0.0]
    nb_batches = 0
    for im, targets, paths, shapes, masks in dataloader:
        t0 = time.perf_counter()
        im = im.to(device, non_blocking=True)
        targets = targets.to(device).clone()
        masks = masks.to(device)
        if im.dtype != torch.uint8:  # uint8 goes in as it is: the input kernel divides by 255
            im = im.half() if half else im.float()
        nb, _, height, width = im.shape
        if profile:
            _sync(device)
        t1 = time.perf_counter()
        preds, protos, train_out = model(im)
        if compute_loss is not None:
            loss += compute_loss((train_out, protos), targets, masks)[1]
        if profile:
            _sync(device)
        t2 = time.perf_counter()
        targets[:, 2:] *= torch.tensor((width, height, width, height), device=device, dtype=targets.dtype)
        out, cnt = non_max_suppression(preds, conf_thres, iou_thres, multi_label=True, agnostic=single_cls, max_det=max_det, nm=nm, padded=True)
        if single_cls:
            out[..., 5] = 0
        stats.update(out, cnt, protos, targets, masks, (height, width), shapes)
        if profile:
            _sync(device)
        t3 = time.perf_counter()
        dt[0] += t1 - t0
        dt[1] += t2 - t1
        dt[2] += t3 - t2
        nb_batches += 1
    metrics, _ = stats.compute(nc)
    seen = max(stats.seen, 1)
    t = tuple(x / seen * 1e3 for x in dt)
    model.float()
    if was_training:
        model.train()
    losses = (loss.cpu() / max(nb_batches, 1)).tolist()
    return (*metrics.mean_results(), *losses), metrics.get_maps(nc), t
