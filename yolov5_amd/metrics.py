"""Validation metrics with the reference's names.

Device side (one HIP launch per batch, `csrc/metrics.hip` -> `y5_val_match`):
    process_batch(detections, labels, iouv, ...)       utils/metrics.py:224-265, box branch and (masks=True, `y5_val_match_masks`) mask branch
    match_batch(out, counts, targets, shapes, iouv)    val.py:282-307 for all images of a batch: de-letterbox of the
                                                        predictions and labels fused with the matching
    ValStats                                            the `stats` list of val.py:218,308 kept on the device
    match_masks_batch(out, counts, protos, targets,     segment/val.py:287-308 mask matching for all images of a batch, the predicted
                      masks, iouv, overlap, shape)      masks computed from the prototypes inside the matcher (never written)
    ConfusionMatrix                                     utils/metrics.py:129-183 as an int32 device accumulator: `update` = one
                                                        `y5_val_confusion` launch per batch, `.matrix` = one D2H copy on read
Host side -- numpy, as in the reference (SURVEY keeps `ap_per_class` on the CPU: it runs once per epoch on a few
thousand rows): `ap_per_class`, `compute_ap`, `smooth`, `fitness`.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _need_gpu(t, what):
    if not _lib.accepts(t):
        raise RuntimeError(f"yolov5_amd.metrics.{what} needs GPU tensors (no CPU path)")


def process_batch(detections, labels, iouv, pred_masks=None, gt_masks=None, overlap=False, masks=False):
    """utils/metrics.py:224-265: detections (N,6+) [x1,y1,x2,y2,conf,cls], labels (M,5) [cls,x1,y1,x2,y2], iouv (niou)
    -> bool (N, niou) on the device.  Tie rule and the equivalence with the reference's sort are in csrc/metrics.hip.
    masks=True: the mask branch (:239-249) -- pred_masks (N, mh, mw) 0/1, gt_masks (M, gh, gw) 0/1 or, with overlap, one (1, gh, gw) / (gh, gw)
    index map (value k + 1 = label k); the ground truth is resized to (mh, mw) when the shapes differ (`y5_val_match_masks`, loaded bits)."""
    _need_gpu(detections, "process_batch")
    n = detections.shape[0]
    niou = iouv.numel()
    if n == 0:
        return torch.zeros((0, niou), dtype=torch.bool, device=detections.device)
    if n > 1024:
        raise ValueError("process_batch: at most 1024 detections per image")
    if masks:
        pm = pred_masks.to(detections.device)
        pm = (pm if pm.dtype == torch.uint8 else (pm != 0).to(torch.uint8)).contiguous()
        gt = gt_masks if not overlap or gt_masks.dim() == 3 else gt_masks[None]
        correct = _match_masks(detections.float().contiguous()[None], None, labels.float().contiguous(), -1, 0, gt, overlap, iouv,
                               pred_masks=pm[None])
        return correct[0].bool()
    det = detections.float().contiguous()
    lab = labels.float().contiguous()
    iv = iouv.to(device=det.device, dtype=torch.float32).contiguous()
    correct = torch.empty((1, n, niou), dtype=torch.uint8, device=det.device)
    lib = _lib.lib()
    rc = lib.y5_val_match(_p(det), det.shape[1], n, None, 1, _p(lab) if lab.numel() else None, 5, lab.shape[0], -1, 0, 1, 0, None, _p(iv), niou,
                          _p(correct), None, _lib.stream(det.device))
    _lib.check(rc, lib)
    return correct[0].bool()


def match_batch(out, counts, targets, shapes, iouv, predn=False):
    """val.py:282-307 for the whole batch in one launch.

    out (bs, max_det, 6+nm) / counts (bs) int32: the padded NMS result (`general.non_max_suppression(..., padded=True)`);
    targets (M,6) [img, cls, cx, cy, w, h] in letterboxed pixels (after val.py:274); shapes: the dataloader's per-image
    ((h0, w0), ((gain, gain), (pad_x, pad_y))) or None to compare the boxes as given.
    Returns correct (bs, max_det, niou) uint8 [rows past counts are 0] and, with predn=True, the native-space boxes
    (bs, max_det, 4) of val.py:297-298."""
    _need_gpu(out, "match_batch")
    bs, max_det, ld = out.shape
    dev = out.device
    if out.dtype != torch.float32 or not out.is_contiguous():
        out = out.float().contiguous()
    tg = targets.to(device=dev, dtype=torch.float32).contiguous()
    iv = iouv.to(device=dev, dtype=torch.float32).contiguous()
    niou = iv.numel()
    sc = None
    if shapes is not None:
        sc = torch.tensor([[rp[0][0], rp[1][0], rp[1][1], s0[0], s0[1]] for s0, rp in shapes], dtype=torch.float32).to(dev, non_blocking=True)
    correct = torch.empty((bs, max_det, niou), dtype=torch.uint8, device=dev)
    pn = torch.empty((bs, max_det, 4), dtype=torch.float32, device=dev) if predn else None
    cn = counts.to(device=dev, dtype=torch.int32) if counts is not None else None
    lib = _lib.lib()
    rc = lib.y5_val_match(_p(out), ld, max_det, _p(cn), bs, _p(tg) if tg.numel() else None, 6, tg.shape[0], 0, 1, 2, 1, _p(sc), _p(iv), niou,
                          _p(correct), _p(pn), _lib.stream(dev))
    _lib.check(rc, lib)
    return (correct, pn) if predn else correct


def _gt_masks(masks, dev):
    m = masks.to(dev)
    if m.dtype == torch.bool:
        m = m.to(torch.uint8)
    elif m.dtype not in (torch.uint8, torch.int32, torch.float32):
        m = m.float()
    return m.contiguous(), {torch.uint8: _lib.Y5_U8, torch.int32: _lib.Y5_I32, torch.float32: _lib.Y5_F32}[m.dtype]


def _match_masks(det, counts, labels, img_col, cls_col, gt_masks, overlap, iouv, protos=None, shape=None, pred_masks=None):
    """One y5_val_match_masks call: det (bs, max_det, ld) fp32 contiguous; either protos (bs, nm, mh, mw) and the letterboxed input `shape`
    (computed bits) or pred_masks (bs, max_det, mh, mw) uint8 (loaded bits).  Returns correct (bs, max_det, niou) uint8."""
    bs, max_det, ld = det.shape
    dev = det.device
    lib = _lib.lib()
    iv = iouv.to(device=dev, dtype=torch.float32).contiguous()
    niou = iv.numel()
    gt, gdt = _gt_masks(gt_masks, dev)
    gh, gw = gt.shape[-2:]
    nl = labels.shape[0]
    if nl and gt.shape[0] != (bs if overlap else nl):
        raise ValueError(f"match_masks: {gt.shape[0]} ground-truth masks, expected {bs if overlap else nl} ({'overlap' if overlap else 'per instance'})")
    ws = lib.y5_val_match_masks_ws_bytes(bs, max_det, nl)
    if ws < 0:
        _lib.check(int(ws), lib)
    work = torch.empty(((ws + 3) // 4,), dtype=torch.int32, device=dev)
    correct = torch.empty((bs, max_det, niou), dtype=torch.uint8, device=dev)
    cn = counts.to(device=dev, dtype=torch.int32) if counts is not None else None
    if protos is not None:
        pr = protos if protos.dtype in (torch.float16, torch.float32) else protos.float()
        pr = pr.contiguous()
        nm, mh, mw = pr.shape[1:]
        src = (_p(pr), _lib.Y5_F16 if pr.dtype == torch.float16 else _lib.Y5_F32, nm, None, mh, mw, int(shape[0]), int(shape[1]))
    else:
        mh, mw = pred_masks.shape[-2:]
        src = (None, 0, 0, _p(pred_masks), mh, mw, 1, 1)
    rc = lib.y5_val_match_masks(_p(det), ld, max_det, _p(cn), bs, _p(labels) if nl else None, labels.shape[1] if labels.dim() == 2 else 1, nl,
                                img_col, cls_col, _p(gt) if nl else None, gdt, 1 if overlap else 0, gh, gw, *src, _p(iv), niou, _p(correct),
                                _p(work), work.numel() * 4, _lib.stream(dev))
    _lib.check(rc, lib)
    return correct


def match_masks_batch(out, counts, protos, targets, masks, iouv, overlap, shape):
    """The mask branch of segment/val.py:282-308 for the whole batch in one C-ABI call (`y5_val_match_masks`, computed bits):
    process_mask(proto, pred[:, 6:], pred[:, :4], shape) (upsample=False) fused with process_batch(..., masks=True) -- no predicted mask is written.

    out (bs, max_det, 6+nm) / counts (bs): the padded NMS result (boxes in letterboxed pixels, before scale_boxes); protos (bs, nm, mh, mw)
    f16|f32; targets (M, 6) [img, cls, ...] (only the image and the class are read); masks: (bs, gh, gw) index maps with overlap, else
    (M, gh, gw) 0/1 in target order, uint8 / int32 / float32; shape: the letterboxed input (h, w).  Returns correct (bs, max_det, niou) uint8,
    rows past counts 0."""
    _need_gpu(out, "match_masks_batch")
    dev = out.device
    if out.dtype != torch.float32 or not out.is_contiguous():
        out = out.float().contiguous()
    tg = targets.to(device=dev, dtype=torch.float32).contiguous()
    return _match_masks(out, counts, tg, 0, 1, masks, overlap, iouv, protos=protos, shape=shape)


class ValStats:
    """The `stats` accumulator of val.py:218,308-309,325: (correct, conf, pcls, tcls) per batch, kept on the device until
    `compute()`; one D2H copy per validation run instead of one per image."""

    def __init__(self, iouv):
        self.iouv = iouv
        self.correct, self.conf, self.pcls, self.tcls = [], [], [], []
        self.seen = 0

    def update(self, out, counts, targets, shapes=None):
        """out/counts: padded NMS result of one batch; targets (M,6) in letterboxed pixels; shapes as in match_batch."""
        bs, max_det, _ = out.shape
        correct = match_batch(out, counts, targets, shapes, self.iouv)
        valid = torch.arange(max_det, device=out.device)[None, :] < counts.to(out.device)[:, None]
        self.correct.append(correct[valid].bool())
        self.conf.append(out[..., 4][valid])
        self.pcls.append(out[..., 5][valid])
        self.tcls.append(targets[:, 1].to(out.device))
        self.seen += bs

    def compute(self, nc=None):
        """val.py:325-330 -> dict(mp, mr, map50, map, ap, ap_class, nt)."""
        if not self.correct:
            return dict(mp=0.0, mr=0.0, map50=0.0, map=0.0, ap=np.zeros((0, self.iouv.numel())), ap_class=np.zeros(0, int), nt=np.zeros(0, int))
        tp = torch.cat(self.correct).cpu().numpy()
        conf = torch.cat(self.conf).cpu().numpy()
        pcls = torch.cat(self.pcls).cpu().numpy()
        tcls = torch.cat(self.tcls).cpu().numpy()
        res = dict(mp=0.0, mr=0.0, map50=0.0, map=0.0, ap=np.zeros((0, tp.shape[1])), ap_class=np.zeros(0, int))
        if tp.shape[0] and tp.any():
            _, _, p, r, _, ap, ap_class = ap_per_class(tp, conf, pcls, tcls)
            res.update(mp=float(p.mean()), mr=float(r.mean()), map50=float(ap[:, 0].mean()), map=float(ap.mean()), ap=ap, ap_class=ap_class)
        res["nt"] = np.bincount(tcls.astype(int), minlength=nc or 0)
        return res


class ConfusionMatrix:
    """utils/metrics.py:129-183 on the device.  The counts live in one (nc + 1, nc + 1) int32 tensor that `y5_val_confusion` adds to with
    integer atomics -- no `.cpu().numpy()` round trip and no Python loop per image (val.py:293,309), no host synchronisation until `.matrix` is
    read.  Rows are predicted classes, columns true classes, index nc is the background.  Semantics (strict `conf > self.conf` and
    `iou > iou_thres`, the two-stage matching, the `if n:` gate of the false positives) are stated at include/yolov5_hip.h; two pairs of equal
    IoU, whose order the reference leaves to argsort, go to the lower index.  `single_cls` is the caller's business, as in val_loop."""

    def __init__(self, nc, conf=0.25, iou_thres=0.45):
        self.nc, self.conf, self.iou_thres = int(nc), conf, iou_thres
        self._counts = None

    def _acc(self, dev):
        if self._counts is None:
            self._counts = torch.zeros((self.nc + 1, self.nc + 1), dtype=torch.int32, device=dev)
        return self._counts

    @property
    def matrix(self):
        """(nc + 1, nc + 1) float64 numpy array, as the reference keeps it: one device-to-host copy."""
        if self._counts is None:
            return np.zeros((self.nc + 1, self.nc + 1))
        return self._counts.cpu().numpy().astype(np.float64)

    def _launch(self, det, counts, bs, lab, img_col, cls_col, box_col, xywh, sc, dev):
        lib = _lib.lib()
        max_det = det.shape[1] if det is not None else 0
        rc = lib.y5_val_confusion(_p(det), det.shape[2] if det is not None else 0, max_det, _p(counts), bs, _p(lab) if lab.numel() else None,
                                  lab.shape[1], lab.shape[0], img_col, cls_col, box_col, xywh, _p(sc), float(self.conf), float(self.iou_thres),
                                  self.nc, _p(self._acc(dev)), _lib.stream(dev))
        _lib.check(rc, lib)

    def process_batch(self, detections, labels):
        """The reference's signature for ONE image: detections (N, 6) [x1, y1, x2, y2, conf, cls] or None, labels (M, 5) [cls, x1, y1, x2, y2]
        (with detections=None: the (M) class vector, val.py:293), both in one pixel space."""
        _need_gpu(labels, "ConfusionMatrix.process_batch")
        dev = labels.device
        if detections is None:
            lab = torch.zeros((labels.numel(), 5), dtype=torch.float32, device=dev)
            lab[:, 0] = labels.reshape(-1).float()
            return self._launch(None, None, 1, lab, -1, 0, 1, 0, None, dev)
        if detections.shape[0] > 1024:
            raise ValueError("ConfusionMatrix.process_batch: at most 1024 detections per image")
        lab = labels.float().contiguous()
        if detections.shape[0] == 0:
            return self._launch(None, None, 1, lab, -1, 0, 1, 0, None, dev)
        self._launch(detections.float().contiguous()[None], None, 1, lab, -1, 0, 1, 0, None, dev)

    def update(self, out, counts, targets, shapes=None):
        """val.py:289-309 for a whole batch in one launch; arguments as `match_batch`: the padded NMS result, targets (M, 6) [img, cls, cx, cy, w, h] in
        letterboxed pixels, the loader's `shapes` or None.  An image without detections sends its labels to the background row; an image
        without labels adds nothing."""
        _need_gpu(out, "ConfusionMatrix.update")
        bs, max_det, _ = out.shape
        dev = out.device
        if out.dtype != torch.float32 or not out.is_contiguous():
            out = out.float().contiguous()
        tg = targets.to(device=dev, dtype=torch.float32).contiguous()
        sc = None
        if shapes is not None:
            sc = torch.tensor([[rp[0][0], rp[1][0], rp[1][1], s0[0], s0[1]] for s0, rp in shapes], dtype=torch.float32).to(dev, non_blocking=True)
        cn = counts.to(device=dev, dtype=torch.int32) if counts is not None else None
        self._launch(out, cn, bs, tg, 0, 1, 2, 1, sc, dev)

    def plot(self, normalize=True, save_dir="", names=()):
        raise NotImplementedError("ConfusionMatrix.plot: the seaborn heat map is outside the hot path")

    def print(self):
        """utils/metrics.py:218-221."""
        m = self.matrix
        for i in range(self.nc + 1):
            print(" ".join(map(str, m[i])))


# ----------------------------------------------------------------------------------------------------------------------
# host side (numpy; CPU in the reference as well)
# ----------------------------------------------------------------------------------------------------------------------
def fitness(x):
    """utils/metrics.py:19-22: 0.1 * mAP@0.5 + 0.9 * mAP@0.5:0.95 of rows [P, R, mAP@0.5, mAP@0.5:0.95, ...]."""
    return (np.asarray(x)[:, :4] * np.array([0.0, 0.0, 0.1, 0.9])).sum(1)


def smooth(y, f=0.05):
    """ultralytics.utils.metrics.smooth (used at utils/metrics.py:91): moving average over an odd window of about
    2*f*len(y) samples, the ends extended with the first / last value."""
    taps = round(len(y) * f * 2) // 2 + 1
    half = taps // 2
    padded = np.concatenate((np.full(half, y[0], dtype=float), y, np.full(half, y[-1], dtype=float)))
    return np.convolve(padded, np.full(taps, 1.0 / taps), mode="valid")


def compute_ap(recall, precision):
    """utils/metrics.py:98-126 ('interp'): area under the monotone precision envelope sampled at 101 recall points."""
    mrec = np.concatenate(([0.0], recall, [1.0]))
    mpre = np.concatenate(([1.0], precision, [0.0]))
    mpre = np.maximum.accumulate(mpre[::-1])[::-1]
    x = np.linspace(0, 1, 101)
    y = np.interp(x, mrec, mpre)
    ap = ((y[1:] + y[:-1]) * (x[1:] - x[:-1]) / 2.0).sum()
    return ap, mpre, mrec


def ap_per_class(tp, conf, pred_cls, target_cls, plot=False, save_dir=".", names=(), eps=1e-16, prefix=""):
    """utils/metrics.py:25-95.  tp (n, niou) bool, conf (n), pred_cls (n), target_cls (m) ->
    tp, fp, p, r, f1 (per class at the best mean-F1 confidence), ap (nc, niou), unique classes.  Plots are not produced."""
    if plot:
        raise NotImplementedError("ap_per_class(plot=True): PR / F1 curve plots are outside the hot path")
    order = np.argsort(-conf)
    tp, conf, pred_cls = tp[order], conf[order], pred_cls[order]
    classes, n_labels = np.unique(target_cls, return_counts=True)
    nc, niou = classes.shape[0], tp.shape[1]
    grid = np.linspace(0, 1, 1000)
    ap = np.zeros((nc, niou))
    p_curve = np.zeros((nc, 1000))
    r_curve = np.zeros((nc, 1000))
    for ci, c in enumerate(classes):
        sel = pred_cls == c
        if not sel.any() or n_labels[ci] == 0:
            continue
        hits = tp[sel]
        tpc = hits.cumsum(0)
        fpc = (1 - hits).cumsum(0)
        recall = tpc / (n_labels[ci] + eps)
        precision = tpc / (tpc + fpc)
        neg_conf = -conf[sel]
        r_curve[ci] = np.interp(-grid, neg_conf, recall[:, 0], left=0)
        p_curve[ci] = np.interp(-grid, neg_conf, precision[:, 0], left=1)
        for j in range(niou):
            ap[ci, j] = compute_ap(recall[:, j], precision[:, j])[0]
    f1_curve = 2 * p_curve * r_curve / (p_curve + r_curve + eps)
    best = smooth(f1_curve.mean(0), 0.1).argmax()
    p, r, f1 = p_curve[:, best], r_curve[:, best], f1_curve[:, best]
    tp_n = (r * n_labels).round()
    fp_n = (tp_n / (p + eps) - tp_n).round()
    return tp_n, fp_n, p, r, f1, ap, classes.astype(int)
