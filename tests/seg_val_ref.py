"""Cases of the mask-validation tests (tests/golden/seg_val.npz, scripts/make_golden_seg_val.py) and the one third-party formula the
reference's mask branch calls.

`mask_iou` restates ultralytics.utils.metrics.mask_iou (the published formula: intersection = mask1 @ mask2.T clamped at 0, union = the
sum of the two areas minus the intersection, IoU = intersection / (union + eps)).  The pip package is not installed where the golden file
is written, so this restatement is parity unpinned by necessity, like oracle/thirdparty.py's box_iou.  Over 0/1 masks every term is an exact
integer in fp32, so only the final division rounds.

Every case is one image of segment/val.py's loop: detections (N, 6) [x1, y1, x2, y2, conf, cls] in letterboxed pixels, labels (M, 5)
[cls, x1, y1, x2, y2], predicted masks (N, mh, mw) 0/1 float32 (what process_mask returns), the ground truth (overlap: (1, gh, gw)
index map, value k + 1 = label k; else (M, gh, gw) 0/1).
"""
import numpy as np
import torch

IOUV = torch.linspace(0.5, 0.95, 10)
NC = 4


def mask_iou(mask1, mask2, eps=1e-7):
    inter = torch.matmul(mask1, mask2.T).clamp_(0)
    union = (mask1.sum(1)[:, None] + mask2.sum(1)[None]) - inter
    return inter / (union + eps)


def _rect(h, w, rng):
    y0, x0 = rng.integers(0, h - 2), rng.integers(0, w - 2)
    y1, x1 = rng.integers(y0 + 2, min(h, y0 + h // 2) + 1), rng.integers(x0 + 2, min(w, x0 + w // 2) + 1)
    return y0, x0, y1, x1


def _blob(h, w, rng):
    """A rectangle with a few pixels flipped at random: IoUs with its neighbours are not simple ratios."""
    m = np.zeros((h, w), np.float32)
    y0, x0, y1, x1 = _rect(h, w, rng)
    m[y0:y1, x0:x1] = 1
    flip = rng.random((h, w)) < 0.01
    m[flip] = 1 - m[flip]
    return m


def _jitter(m, rng, p=0.05):
    """A prediction near a ground-truth mask: shifted by up to a pixel, some pixels flipped."""
    out = np.roll(m, (int(rng.integers(-1, 2)), int(rng.integers(-1, 2))), (0, 1)).copy()
    flip = rng.random(m.shape) < p * rng.random()
    out[flip] = 1 - out[flip]
    return out


def _box(m):
    ys, xs = np.nonzero(m)
    if not len(ys):
        return [0.0, 0.0, 1.0, 1.0]
    return [float(xs.min()), float(ys.min()), float(xs.max() + 1), float(ys.max() + 1)]


def _make(seed, n, m, mh, up, overlap, ncls=NC, nomatch=False, single=False, tie=False, high_idx=False):
    rng = np.random.default_rng(seed)
    gt_lo = np.stack([_blob(mh, mh, rng) for _ in range(m)]) if m else np.zeros((0, mh, mh), np.float32)
    if tie and m >= 2:
        gt_lo[1] = gt_lo[0]
    lcls = rng.integers(0, ncls, m).astype(np.float32)
    if tie and m >= 2:
        lcls[1] = lcls[0]
    if single:
        lcls[:] = 0
    pm, dets = [], []
    for i in range(n):
        if m and rng.random() < 0.7:
            k = int(rng.integers(0, m))
            pmask = _jitter(gt_lo[k], rng)
            c = lcls[k] if rng.random() < 0.85 else float(rng.integers(0, ncls))
        else:
            pmask, c = _blob(mh, mh, rng), float(rng.integers(0, ncls))
        if nomatch:
            c = float(ncls + 1 + (i % 2))
        if single:
            c = 0.0
        pm.append(pmask)
        dets.append(_box(pmask) + [float(rng.random()), c])
    if tie and n:
        pm[0] = gt_lo[0].copy()
        dets[0][5] = float(lcls[0])
    pm = np.stack(pm).astype(np.float32) if n else np.zeros((0, mh, mh), np.float32)
    det = np.array(dets, np.float32).reshape(n, 6)
    det[:, :4] *= 4  # letterboxed pixels (mask_downsample_ratio 4)
    lab = np.concatenate([lcls[:, None], np.array([_box(g) for g in gt_lo], np.float32).reshape(m, 4) * 4], 1).astype(np.float32)
    gh = mh * 4 if up else mh
    # ground truth at gh: nearest-neighbour upsampling of the low-resolution masks plus a few flipped pixels, so the bilinear path sees edges
    gt = np.repeat(np.repeat(gt_lo, gh // mh, 1), gh // mh, 2) if m else np.zeros((0, gh, gh), np.float32)
    if up and m:
        flip = rng.random(gt.shape) < 0.004
        gt[flip] = 1 - gt[flip]
    if overlap:
        idx = np.zeros((1, gh, gh), np.float32)
        for k in range(m):  # later labels on top, as the reference's polygons2masks_overlap sorts by area; any order is a valid map
            idx[0][gt[k] > 0] = k + 1
        if high_idx:
            idx[0, : gh // 4, : gh // 4] = m + 3  # values above nl: ignored by torch.where(gt == index)
        gt = idx
    return dict(det=det, lab=lab, pm=pm, gt=gt.astype(np.float32), overlap=overlap)


CASES = {
    "overlap_same": dict(seed=1, n=12, m=6, mh=32, up=False, overlap=True),
    "inst_same": dict(seed=2, n=12, m=6, mh=32, up=False, overlap=False),
    "overlap_4x": dict(seed=3, n=10, m=5, mh=32, up=True, overlap=True),
    "inst_4x": dict(seed=4, n=10, m=5, mh=32, up=True, overlap=False),
    "no_pred": dict(seed=5, n=0, m=4, mh=32, up=False, overlap=True),
    "no_label": dict(seed=6, n=7, m=0, mh=32, up=False, overlap=False),
    "no_class_match": dict(seed=7, n=6, m=4, mh=32, up=False, overlap=False, nomatch=True),
    "single_cls": dict(seed=8, n=12, m=6, mh=32, up=False, overlap=True, single=True),
    "tie": dict(seed=9, n=4, m=3, mh=32, up=False, overlap=False, tie=True),
    "high_idx": dict(seed=10, n=10, m=5, mh=32, up=False, overlap=True, high_idx=True),
    "big": dict(seed=11, n=300, m=100, mh=64, up=False, overlap=False, ncls=3),
}


def case(name):
    return _make(**CASES[name])
