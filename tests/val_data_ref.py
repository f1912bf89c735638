"""TEST HELPER for the detection validation data path (tests/test_emu_val_data.py, tests/test_gpu_val_data.py, scripts/make_golden_val_data.py):
data from seeds and NumPy restatements.

  * `resize_area`: OpenCV's INTER_AREA for 8-bit images as include/yolov5_hip.h states it (cv2 is absent: restated from the published
    algorithm, modules/imgproc/src/resize.cpp -- parity with the real library unpinned by necessity), written as the literal (di, si, alpha)
    tap list of `computeResizeAreaTab` and the row loop of `ResizeArea_Invoker`, NOT as the product's {first, count} tables.
  * `area_mean_exact`: the fp64 area mean the restatement is checked against, with `tap_counts`.
  * `letterbox_area_ref`: load_image + pad + CHW / RGB (+ / 255) of a ragged batch.
  * `val_dataset`: the 9 seeded images (h, w) of SIZES and their labels.
  * `CM_CASES` / `cm_case`: detections and labels of the confusion-matrix cases; every image's over-threshold IoUs are pairwise distinct
    (asserted), so no case rests on the tie rule."""
import math

import numpy as np

from oracle import thirdparty as tp

IMG_SIZE, STRIDE, PAD, BATCH = 64, 32, 0.5, 4
# (h, w): wide, tall, square, long side exactly 64, long side 40 (up-scale), exact 2x, 3x on the long side, two general ones
SIZES = [(60, 100), (110, 70), (90, 90), (48, 64), (40, 30), (128, 96), (64, 192), (150, 97), (211, 160)]


# ---- INTER_AREA ---------------------------------------------------------------------------------------------------------------------------
def area_tab(ssize, dsize):
    """computeResizeAreaTab for one axis -> list of (di, si, alpha float32)."""
    scale = float(ssize) / dsize
    tab = []
    for d in range(dsize):
        f1 = d * scale
        f2 = f1 + scale
        cell = min(scale, ssize - f1)
        s1 = math.ceil(f1)
        s2 = min(math.floor(f2), ssize - 1)
        s1 = min(s1, s2)
        if s1 - f1 > 1e-3:
            tab.append((d, s1 - 1, np.float32((s1 - f1) / cell)))
        for s in range(s1, s2):
            tab.append((d, s, np.float32(1.0 / cell)))
        if f2 - s2 > 1e-3:
            tab.append((d, s2, np.float32(min(min(f2 - s2, 1.0), cell) / cell)))
    return tab


def tap_counts(ssize, dsize):
    n = np.zeros(dsize, int)
    for d, _s, _a in area_tab(ssize, dsize):
        n[d] += 1
    return n


def _iscale(ssize, dsize):
    scale = float(ssize) / dsize
    k = int(round(scale))
    return k if abs(scale - k) < np.finfo(np.float64).eps else 0


def _sat_u8(v):
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def resize_area(src, dsize):
    """cv2.resize(src, (dw, dh), interpolation=cv2.INTER_AREA) for a uint8 (h, w, c) image that shrinks (or keeps) both sides."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 3
    sh, sw = src.shape[:2]
    dw, dh = int(dsize[0]), int(dsize[1])
    assert dw <= sw and dh <= sh
    ix, iy = _iscale(sw, dw), _iscale(sh, dh)
    if ix and iy:                                                # ResizeAreaFast_Invoker
        a = src[:dh * iy, :dw * ix].astype(np.int32).reshape(dh, iy, dw, ix, -1)
        s = a.sum((1, 3))
        if ix == 2 and iy == 2:
            return ((s + 2) >> 2).astype(np.uint8)
        return _sat_u8(s.astype(np.float32) * (np.float32(1.0) / np.float32(ix * iy)))
    xtab, ytab = area_tab(sw, dw), area_tab(sh, dh)              # ResizeArea_Invoker
    S = src.astype(np.float32)
    out = np.zeros((dh, dw, src.shape[2]), np.float32)
    prev = -1
    for dy, sy, beta in ytab:
        row = np.zeros((dw, src.shape[2]), np.float32)
        for dx, sx, alpha in xtab:
            row[dx] = row[dx] + S[sy, sx] * alpha                # float32 product, float32 sum, x taps in order
        out[dy] = beta * row if dy != prev else out[dy] + beta * row
        prev = dy
    return _sat_u8(out)


def area_mean_exact(src, dsize):
    """The mean of the source over every output cell [d * scale, (d + 1) * scale) in float64 (overlap lengths as weights, not rounded)."""
    src = np.asarray(src, dtype=np.float64)
    sh, sw = src.shape[:2]
    dw, dh = int(dsize[0]), int(dsize[1])

    def weights(ssize, n):
        scale = ssize / n
        W = np.zeros((n, ssize))
        for d in range(n):
            lo, hi = d * scale, min((d + 1) * scale, ssize)
            for s in range(int(math.floor(lo)), min(int(math.ceil(hi)), ssize)):
                W[d, s] = max(0.0, min(hi, s + 1) - max(lo, s))
            W[d] /= W[d].sum()
        return W

    return np.einsum("ys,swc,xw->yxc", weights(sh, dh), src, weights(sw, dw))


# ---- load_image + pad ---------------------------------------------------------------------------------------------------------------------
def cv2_resize(src, dsize, dst=None, fx=0, fy=0, interpolation=1):
    """The cv2.resize the golden script binds: INTER_LINEAR (1) is oracle/thirdparty.py's restatement, INTER_AREA (3) this file's."""
    if interpolation == 3:
        return resize_area(src, dsize)
    return tp.cv2_resize(src, dsize, interpolation=interpolation)


def resized(im, nh, nw):
    h0, w0 = im.shape[:2]
    if (nh, nw) == (h0, w0):
        return im
    return cv2_resize(im, (nw, nh), interpolation=1 if (nh > h0 or nw > w0) else 3)


def letterbox_area_ref(ims, sizes, places, H, W, dtype=np.uint8, normalize=False, pad=114):
    out = np.full((len(ims), H, W, 3), pad, np.uint8)
    for b, (im, (nh, nw), (top, left)) in enumerate(zip(ims, sizes, places)):
        out[b, top:top + nh, left:left + nw] = resized(im, nh, nw)
    out = np.ascontiguousarray(out.transpose(0, 3, 1, 2)[:, ::-1])
    if dtype == np.uint8:
        return out
    if dtype == np.float16:                                       # `.half() / 255`: fp32 division of the half value, rounded once
        f = out.astype(np.float16).astype(np.float32)
        return (f / np.float32(255.0) if normalize else f).astype(np.float16)
    f = out.astype(np.float32)
    return f / np.float32(255.0) if normalize else f


def pattern(kind, h, w, seed=0):
    if kind == "random":
        return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "white":
        return np.full((h, w, 3), 255, np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    return np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], 3, 2)   # 0 / 255 checkerboard


# ---- the 9-image dataset ------------------------------------------------------------------------------------------------------------------
def val_dataset(seed=11):
    """-> (images: list of uint8 (h, w, 3) BGR arrays, labels: list of (k, 5) float32 [cls, xc, yc, w, h] normalised).  Image 3 has no labels;
    some boxes reach the border (the clip of xyxy2xywhn)."""
    rng = np.random.default_rng(seed)
    ims, labels = [], []
    for i, (h, w) in enumerate(SIZES):
        ims.append(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
        k = 0 if i == 3 else int(rng.integers(1, 5))
        lb = np.zeros((k, 5), np.float32)
        lb[:, 0] = rng.integers(0, 80, k)
        wh = rng.uniform(0.1, 0.6, (k, 2))
        c = rng.uniform(0.0, 1.0, (k, 2)) * (1 - wh) + wh / 2
        lb[:, 1:3], lb[:, 3:5] = c, wh
        if k:
            lb[0, 1:5] = [0.5, 0.5, 1.0, 1.0] if i % 2 else [0.25, 0.5, 0.5, 1.0]      # touches the border
        labels.append(lb)
    return ims, labels


# ---- confusion matrix ---------------------------------------------------------------------------------------------------------------------
CONF, IOU_THRES = 0.25, 0.45


def _iou(lab_boxes, det_boxes):
    a, b = np.asarray(lab_boxes, np.float32)[:, None], np.asarray(det_boxes, np.float32)[None]
    inter = (np.minimum(a[..., 2:], b[..., 2:]) - np.maximum(a[..., :2], b[..., :2])).clip(0).prod(-1)
    return inter / ((a[..., 2:] - a[..., :2]).prod(-1) + (b[..., 2:] - b[..., :2]).prod(-1) - inter + np.float32(1e-7))


def _det(rows):
    return np.asarray(rows, np.float32).reshape(-1, 6)


def _lab(rows):
    return np.asarray(rows, np.float32).reshape(-1, 5)


def _seeded(seed, nc=5, nd=40, nl=12, size=200.0):
    rng = np.random.default_rng(seed)
    nl, nd = int(rng.integers(nl // 2, nl + 1)), int(rng.integers(nd // 2, nd + 1))
    xy = rng.uniform(0, size - 60, (nl, 2))
    wh = rng.uniform(20, 60, (nl, 2))
    lab = np.concatenate((rng.integers(0, nc, (nl, 1)), xy, xy + wh), 1).astype(np.float32)
    src = rng.integers(0, nl, nd)
    box = lab[src, 1:] + rng.normal(0, 5.0, (nd, 4)).astype(np.float32)
    box[:, 2:] = np.maximum(box[:, 2:], box[:, :2] + 2)
    far = rng.random(nd) < 0.2
    box[far] += 300
    cls = np.where(rng.random(nd) < 0.7, lab[src, 0], rng.integers(0, nc, nd))
    det = np.concatenate((box, rng.uniform(0.05, 1.0, (nd, 1)), cls[:, None]), 1).astype(np.float32)
    return nc, det, lab


L0 = [0, 0, 10, 10]
CM_CASES = {
    # name: (nc, detections (N, 6) or None, labels (M, 5) -- with detections None the (M) class vector)
    "none_with_labels": lambda: (3, None, np.asarray([0, 2, 2], np.float32)),
    "no_labels": lambda: (3, _det([[0, 0, 10, 10, 0.9, 1]]), _lab([])),
    "all_below_conf": lambda: (3, _det([[0, 0, 10, 10, 0.2, 1], [0, 0, 10, 9, 0.1, 0]]), _lab([[1, *L0], [2, 20, 20, 30, 30]])),
    "no_pair_over_thres": lambda: (3, _det([[0, 0, 10, 4, 0.9, 1], [50, 50, 60, 60, 0.8, 0]]), _lab([[1, *L0]])),
    "one_pair": lambda: (3, _det([[0, 0, 10, 9, 0.9, 1], [50, 50, 60, 60, 0.8, 0]]), _lab([[1, *L0], [2, 80, 80, 90, 90]])),
    "two_dets_one_label": lambda: (3, _det([[0, 0, 10, 8, 0.9, 1], [0, 0, 10, 9, 0.6, 1]]), _lab([[1, *L0]])),
    "one_det_two_labels": lambda: (3, _det([[0, 0, 10, 9, 0.9, 2]]), _lab([[2, *L0], [0, 0, 0, 10, 7]])),
    "wrong_class": lambda: (3, _det([[0, 0, 10, 9, 0.9, 0]]), _lab([[2, *L0]])),
    "conf_exactly_025": lambda: (3, _det([[0, 0, 10, 9, 0.25, 1], [20, 20, 30, 29, 0.26, 1]]), _lab([[1, *L0], [1, 20, 20, 30, 30]])),
    "nc1": lambda: (1, _det([[0, 0, 10, 9, 0.9, 0], [40, 40, 50, 50, 0.9, 0]]), _lab([[0, *L0], [0, 70, 70, 80, 80]])),
    "nc80_last_class": lambda: (80, _det([[0, 0, 10, 9, 0.9, 79], [40, 40, 50, 50, 0.9, 79]]), _lab([[79, *L0], [79, 70, 70, 80, 80]])),
    # d1 prefers l0 at 0.9 and also overlaps l1 at 0.667; d0 overlaps only l0 at 0.8 -> d1 -> l0, d0 a false positive, l1 a false negative
    "two_stage_not_greedy": lambda: (3, _det([[0, 2, 10, 10, 0.9, 0], [0, 0, 10, 9, 0.8, 1]]), _lab([[1, *L0], [2, 0, 0, 10, 6]])),
    "seeded0": lambda: _seeded(100),
    "seeded1": lambda: _seeded(101),
    "seeded2": lambda: _seeded(102, nc=80),
}


def cm_case(name):
    nc, det, lab = CM_CASES[name]()
    if det is not None and len(det) and len(lab):
        iou = _iou(lab[:, 1:], det[det[:, 4] > CONF, :4])
        over = iou[iou > IOU_THRES]
        assert len(np.unique(over)) == len(over), f"{name}: two over-threshold pairs of equal IoU"
    return nc, det, lab


def batch_case(seed=7, bs=5, max_det=48, nc=5, size=200.0):
    """A padded NMS result + targets in letterboxed pixels + loader shapes for the batch form: image 1 has count 0 and labels, image 3 has
    detections and no labels.  -> (out (bs, max_det, 6), counts (bs) int32, targets (M, 6) [img, cls, cx, cy, w, h], shapes, nc)."""
    out = np.zeros((bs, max_det, 6), np.float32)
    counts = np.zeros(bs, np.int32)
    tg, shapes = [], []
    for si in range(bs):
        _, det, lab = _seeded(seed * 10 + si, nc=nc, nd=max_det - 8, size=size)
        if si == 1:
            det = det[:0]
        if si == 3:
            lab = lab[:0]
        counts[si] = len(det)
        out[si, :len(det)] = det
        xywh = np.concatenate(((lab[:, 1:3] + lab[:, 3:5]) / 2, lab[:, 3:5] - lab[:, 1:3]), 1)
        tg.append(np.concatenate((np.full((len(lab), 1), si, np.float32), lab[:, :1], xywh), 1).astype(np.float32))
        gain = 0.5 + 0.1 * si
        shapes.append(((int(size / gain) - 7, int(size / gain)), ((gain, gain), (3.0 + si, 5.5))))
    return out, counts, np.concatenate(tg, 0), shapes, nc
