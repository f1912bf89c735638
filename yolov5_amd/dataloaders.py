"""Input pipelines with the pixel work on the device: the dataset's uint8 BGR images live in HBM, the host draws the random numbers and does
the geometry + label transform of a whole batch (a few hundred floats) in the reference's own expressions, and ONE launch renders the batch
directly in the a0 tensor contract of the model (uint8, or fp16 / 255).  At the training rates of this engine (3 k img/s per GPU) the
reference's 8 cv2 worker processes cannot keep a GPU fed.

The loaders and what they restate:
    MosaicLoader / mosaic_batch            utils/dataloaders.py:696-863 `LoadImagesAndLabels.__getitem__` (augment = True, rect = False: the mosaic
                                           branch and, where the hyp['mosaic'] gate sends a sample there, the letterbox branch :710-733) + `collate_fn`;
                                           utils/augmentations.py:69-83 `augment_hsv`, :118-209 `random_perspective`, :246-258 `box_candidates`
    SegMosaicLoader / seg_mosaic_batch     utils/segment/dataloaders.py:130-301 `LoadImagesAndLabelsAndMasks`, utils/segment/augmentations.py:14-91;
                                           the polygons go through the reference's float64 expressions on the host and ONE `y5_polygon_masks` call
                                           (csrc/seg_data.h) rasterises, shrinks, orders and flips the masks of the batch
    SegValLoader / seg_letterbox_batch     the augment = False, rect = False branch of the same `__getitem__`
    ValLoader / letterbox_area_batch       `LoadImagesAndLabels(augment=False, rect=..., pad=...)`: :589-612 rect ordering and batch shapes, :710-736 the
                                           letterbox branch, :784-788 `load_image` with INTER_AREA for a down-scale, + `collate_fn`; ONE
                                           `y5_letterbox_area_batch` launch per batch (csrc/val_data.h)
    ClassificationLoader                   utils/dataloaders.py:949-1013, the torch_transforms branch (augmentations.classify_transform_batch)

The host rules they share, each written once:
    draws        `_perspective_draws`, `_mosaic_draws`, `_draw_sample`: the reference's ORDER per sample, so that a `random.seed()` /
                 `np.random.seed()`-ed run consumes the generators exactly as `__getitem__` does (the generators can also be passed in: parity
                 tests).  `draw_sample` and `draw_sample_seg` differ in the shuffle of the tile indices and in how the mixup partner is picked.
    geometry     `_resized_hw` (load_image; every loader), `_tile_rects`, `_affine`, `_invert_affine`, `_fill_job` (one y5_mosaic_batch job:
                 both training loaders and `seg_letterbox_batch`), `_check_image` (the image contract, also `area_jobs`)
    labels       `_xywhn2xyxy` (`_canvas_boxes`, `ValLoader`), `_canvas_boxes` (`_labels`, `_seg_labels`, `seg_letterbox_batch`), `_xyn2xy`
                 (`_canvas_stage`, `seg_letterbox_batch`), `_canvas_stage` + `_warp_polygons` (`_labels` with polygons, `_seg_labels`),
                 `_box_candidates` (`_labels`, `_warp_polygons`), `_finish_labels` (every detection and
                 segmentation loader)
    batches      `_assemble` (the job and label loop of `mosaic_batch` and `seg_mosaic_geometry`: mixup partners, HSV tables, batch index),
                 `_render` (the y5_mosaic_batch / y5_mosaic_batch_paste launch: both training loaders, `seg_letterbox_batch`), `_masks_and_targets` (both segmentation
                 batch functions), `_targets`
    epochs       `MosaicLoader._epoch_order` (seeded shuffle, rank stride, padding); `SegMosaicLoader` overrides only `_batch`
Copy-paste (hyp['copy_paste'], utils/augmentations.py:200-222; both loaders, mosaics only, mixup partners included): `_mosaic_draws` draws its one
random.sample at the reference's position (needs `counts`, the polygons of every image), `_copy_paste` restates the label half (bbox_ioa
against the growing label array) in `_canvas_stage`, `paste_planes` (ONE y5_paste_planes launch, csrc/copy_paste.h) fills the accepted
original polygons into a bit plane per pasting job and `_render` then launches y5_mosaic_batch_paste, which redirects the covered canvas
pixels to their mirror position.  `MosaicLoader(segments=...)` also takes random_perspective's `use_segments` branch (`_warp_polygons`).
Not covered: reading images and label files from disk and the caches, image_weights, rect batches for TRAINING, collate_fn4,
albumentations, perspective != 0."""
from __future__ import annotations

import ctypes as C
import functools
import math
import random

import numpy as np
import torch

from . import _lib

HYP_AUG = {"hsv_h": 0.015, "hsv_s": 0.7, "hsv_v": 0.4, "degrees": 0.0, "translate": 0.1, "scale": 0.5, "shear": 0.0, "perspective": 0.0,
           "flipud": 0.0, "fliplr": 0.5, "mosaic": 1.0, "mixup": 0.0, "copy_paste": 0.0}  # data/hyps/hyp.scratch-low.yaml:25-37


def _perspective_draws(d, hyp, rng):
    """random_perspective's eight (augmentations.py:135-156; segment/augmentations.py:42-61): perspective x2, angle, scale, shear x2, translate x2."""
    d["persp"] = (rng.uniform(-hyp["perspective"], hyp["perspective"]), rng.uniform(-hyp["perspective"], hyp["perspective"]))
    d["angle"] = rng.uniform(-hyp["degrees"], hyp["degrees"])
    d["scale"] = rng.uniform(1 - hyp["scale"], 1 + hyp["scale"])
    d["shear"] = (rng.uniform(-hyp["shear"], hyp["shear"]), rng.uniform(-hyp["shear"], hyp["shear"]))
    d["translate"] = (rng.uniform(0.5 - hyp["translate"], 0.5 + hyp["translate"]), rng.uniform(0.5 - hyp["translate"], 0.5 + hyp["translate"]))
    return d


def _mosaic_draws(index, n_images, s, hyp, rng, shuffle, counts=None):
    """Draws of one mosaic (load_mosaic -> copy_paste -> random_perspective): centre yc, xc; three extra indices, shuffled with `index` when
    `shuffle`; copy_paste's ONE draw, random.sample(range(n), k=round(p * n)) under its `if p and n` gate (augmentations.py:206-209), n = the
    polygons of the four tiles (`counts`: the number of polygons of every dataset image); the eight."""
    d = {"mosaic": True}
    d["yc"], d["xc"] = (int(rng.uniform(-x, 2 * s + x)) for x in (-s // 2, -s // 2))
    d["indices"] = [index, *rng.choices(range(n_images), k=3)]
    if shuffle:
        rng.shuffle(d["indices"])
    p = hyp.get("copy_paste", 0.0)
    if p and counts is not None:
        n = sum(int(counts[i]) for i in d["indices"])
        if n:
            d["paste"] = rng.sample(range(n), k=round(p * n))
    return _perspective_draws(d, hyp, rng)


def _draw_sample(index, n_images, s, hyp, rng, np_rng, shuffle, partner, counts=None):
    """The draw order both `__getitem__`s share: mosaic gate; the mosaic's draws; mixup gate, `partner()` index, the partner mosaic's own draws
    (its own copy_paste sample included), np.random.beta in mixup(); three HSV gains from numpy (augmentations.py:72); flipud, fliplr gates.
    copy_paste runs in load_mosaic only: the letterbox branch draws nothing for it."""
    if rng.random() < hyp["mosaic"]:
        d = _mosaic_draws(index, n_images, s, hyp, rng, shuffle, counts)
        if rng.random() < hyp["mixup"]:
            d["partner"] = _mosaic_draws(partner(), n_images, s, hyp, rng, shuffle, counts)
            d["mix_r"] = float(np_rng.beta(32.0, 32.0))
    else:   # letterbox branch (dataloaders.py:710-733): the next draws are random_perspective's; no mixup gate on this side
        d = _perspective_draws({"mosaic": False, "indices": [index]}, hyp, rng)
    d["hsv"] = np_rng.uniform(-1, 1, 3) * [hyp["hsv_h"], hyp["hsv_s"], hyp["hsv_v"]] + 1
    d["flipud"] = rng.random() < hyp["flipud"]
    d["fliplr"] = rng.random() < hyp["fliplr"]
    return d


def draw_sample(index, n_images, s, hyp, rng=random, np_rng=np.random, counts=None):
    """Random numbers of one sample in the reference's order: mosaic gate (dataloaders.py:701); centre yc, xc (:802); three extra
    indices + shuffle (:803-804); copy_paste's sample (:842, augmentations.py:209) when hyp['copy_paste'] and `counts` -- the number of
    polygons of every dataset image -- are given; perspective x2, angle, scale, shear x2, translate x2 (augmentations.py:135-156); mixup gate
    (dataloaders.py:707), partner = random.choice(indices) (:708); three HSV gains from numpy (augmentations.py:72); flipud, fliplr gates
    (dataloaders.py:747,753).  Without counts the dataset has no polygons: copy_paste's `if p and n` gate then draws nothing."""
    if hyp["perspective"]:
        raise NotImplementedError("MosaicLoader: perspective != 0 (cv2.warpPerspective) is not implemented")
    return _draw_sample(index, n_images, s, hyp, rng, np_rng, True, lambda: rng.choice(range(n_images)), counts)


def draw_sample_seg(index, n_images, s, hyp, rng=random, np_rng=np.random, counts=None):
    """Random numbers of one sample in the order of the SEGMENTATION `__getitem__` (utils/segment/dataloaders.py), which is not `draw_sample`'s:
    mosaic gate (:135); centre yc, xc (:239); three extra indices, NOT shuffled (:242); copy_paste's sample (:280, augmentations.py:209; nothing
    at p = 0), which needs `counts`, the number of polygons of every dataset image; random_perspective's eight
    (segment/augmentations.py:42-61); mixup gate (:141), partner = randint(0, n - 1) (:142), the partner mosaic's own draws, np.random.beta
    (segment/augmentations.py:19); three HSV gains from numpy; flipud, fliplr gates (:212,219)."""
    if hyp.get("copy_paste", 0.0) and counts is None:
        raise NotImplementedError("draw_sample_seg: copy_paste != 0 needs counts, the number of polygons of every image")
    if hyp["perspective"]:
        raise NotImplementedError("SegMosaicLoader: perspective != 0 (cv2.warpPerspective) is not implemented")
    return _draw_sample(index, n_images, s, hyp, rng, np_rng, False, lambda: rng.randint(0, n_images - 1), counts)


def _resized_hw(h0, w0, s):
    """dataloaders.py:783-787."""
    r = s / max(h0, w0)
    return (h0, w0) if r == 1 else (math.ceil(h0 * r), math.ceil(w0 * r))


def _tile_rects(hw, yc, xc, s):
    """Canvas rectangle [x1a, x2a) x [y1a, y2a) and source offset (x1b, y1b) of the 4 tiles around (xc, yc) (dataloaders.py:810-822)."""
    rects = []
    for t, (h, w) in enumerate(hw):
        left, top = t in (0, 2), t in (0, 1)
        x1a, x2a = (max(xc - w, 0), xc) if left else (xc, min(xc + w, 2 * s))
        y1a, y2a = (max(yc - h, 0), yc) if top else (yc, min(2 * s, yc + h))
        x1b = w - (x2a - x1a) if left else 0
        y1b = h - (y2a - y1a) if top else 0
        rects.append((x1a, y1a, x2a, y2a, x1b, y1b))
    return rects


def _affine(d, s, mosaic=True):
    """M = T S R P C of random_perspective (augmentations.py:124-160) -> (M 3x3, out w, h): the 2s x 2s mosaic canvas with border (-s/2, -s/2), or
    the s x s letterboxed image of the non-mosaic branch with border (0, 0)."""
    src = 2 * s if mosaic else s
    height = width = src + (2 * (-s // 2) if mosaic else 0)
    Cm = np.eye(3)
    Cm[0, 2] = Cm[1, 2] = -src / 2
    a = d["angle"] * math.pi / 180.0
    ca, sa = math.cos(a) * d["scale"], math.sin(a) * d["scale"]
    R = np.array([[ca, sa, 0.0], [-sa, ca, 0.0], [0.0, 0.0, 1.0]])      # cv2.getRotationMatrix2D(angle, (0, 0), scale)
    Sh = np.eye(3)
    Sh[0, 1] = math.tan(d["shear"][0] * math.pi / 180)
    Sh[1, 0] = math.tan(d["shear"][1] * math.pi / 180)
    T = np.eye(3)
    T[0, 2], T[1, 2] = d["translate"][0] * width, d["translate"][1] * height
    return T @ Sh @ R @ np.eye(3) @ Cm, width, height


def _invert_affine(M):
    """The inverse map cv::warpAffine builds from the forward matrix (same operation order, double precision)."""
    m = np.array(M[:2], dtype=np.float64).copy()
    D = m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]
    D = 1.0 / D if D != 0 else 0.0
    a11, a22 = m[1, 1] * D, m[0, 0] * D
    m[0, 0] = a11
    m[0, 1] *= -D
    m[1, 0] *= -D
    m[1, 1] = a22
    b1 = -m[0, 0] * m[0, 2] - m[0, 1] * m[1, 2]
    b2 = -m[1, 0] * m[0, 2] - m[1, 1] * m[1, 2]
    m[0, 2], m[1, 2] = b1, b2
    return m


def _xywhn2xyxy(x, w, h, padw, padh):
    """ultralytics.utils.ops.xywhn2xyxy (call sites utils/dataloaders.py:721,838), the reference's expressions: the TYPES of w, h, padw, padh decide
    whether numpy evaluates them in float32 or float64, so the caller passes scalars made the way the reference makes them."""
    y = x.copy()
    y[..., 0] = w * (x[..., 0] - x[..., 2] / 2) + padw
    y[..., 1] = h * (x[..., 1] - x[..., 3] / 2) + padh
    y[..., 2] = w * (x[..., 0] + x[..., 2] / 2) + padw
    y[..., 3] = h * (x[..., 1] + x[..., 3] / 2) + padh
    return y


def _canvas_boxes(labels, d, hw, pads, s):
    """Tile labels -> canvas pixels (xywhn2xyxy, :838 / :720), mosaic only: clipped to the canvas (:845-846).
    -> ((n, 5) float32 [cls, x1, y1, x2, y2], the number of rows of every tile)."""
    parts = []
    for i, (h, w), (padw, padh) in zip(d["indices"], hw, pads):
        lb = np.array(labels[i], dtype=np.float32).reshape(-1, 5).copy()
        if lb.size:
            lb[:, 1:] = _xywhn2xyxy(lb[:, 1:], w, h, padw, padh)
        parts.append(lb)
    t = np.concatenate(parts, 0)
    if d.get("mosaic", True):
        np.clip(t[:, 1:], 0, 2 * s, out=t[:, 1:])
    return t, [len(lb) for lb in parts]


def _box_candidates(t, new, scale, area_thr):
    """box_candidates(box1=t[:, 1:5].T * scale, box2=new.T, area_thr) (augmentations.py:246-258; wh_thr = 2, ar_thr = 100, eps = 1e-16) and what
    both random_perspectives do with it: -> (the rows of t it keeps, with their boxes replaced by `new`; the keep mask)."""
    b1 = t[:, 1:5].T * scale
    w1, h1 = b1[2] - b1[0], b1[3] - b1[1]
    w2, h2 = new[:, 2] - new[:, 0], new[:, 3] - new[:, 1]
    ar = np.maximum(w2 / (h2 + 1e-16), h2 / (w2 + 1e-16))
    keep = (w2 > 2) & (h2 > 2) & (w2 * h2 / (w1 * h1 + 1e-16) > area_thr) & (ar < 100)
    t = t[keep]
    t[:, 1:5] = new[keep]
    return t, keep


def _bbox_ioa(box1, box2, eps=1e-7):
    """ultralytics.utils.metrics.bbox_ioa(box1 (n, 4), box2 (m, 4), iou=False): intersection over the area of box2 -> (n, m).  Restated from the
    published source (the package is a third-party dependency of the reference): parity unpinned by necessity."""
    b1_x1, b1_y1, b1_x2, b1_y2 = box1.T
    b2_x1, b2_y1, b2_x2, b2_y2 = box2.T
    inter_area = (np.minimum(b1_x2[:, None], b2_x2) - np.maximum(b1_x1[:, None], b2_x1)).clip(0) * \
                 (np.minimum(b1_y2[:, None], b2_y2) - np.maximum(b1_y1[:, None], b2_y1)).clip(0)
    area = (b2_x2 - b2_x1) * (b2_y2 - b2_y1)
    return inter_area / (area + eps)


def _copy_paste(labels, segments, sample, w):
    """The label half of copy_paste (augmentations.py:209-216) on the canvas of width w, in the reference's expressions and dtypes: for every
    j of `sample` (the draw), the mirrored box against the labels AS GROWN SO FAR; where every ioa < 0.30, the mirrored label and polygon are
    appended.  -> (labels, segments: what random_perspective sees; the accepted js, whose ORIGINAL polygons the image half fills)."""
    if sample and max(sample) >= len(segments):
        raise ValueError(f"copy_paste: the sample was drawn for more than the {len(segments)} polygons of this mosaic")
    segments, accepted = list(segments), []
    for j in sample:
        label, segment = labels[j], segments[j]
        box = w - label[3], label[2], w - label[1], label[4]
        ioa = _bbox_ioa(np.array(box)[None], labels[:, 1:5])
        if (ioa < 0.30).all():
            labels = np.concatenate((labels, [[label[0], *box]]), 0)
            segments.append(np.concatenate((w - segment[:, 0:1], segment[:, 1:2]), 1))
            accepted.append(j)
    return labels, segments, accepted


def _canvas_stage(labels, segments, d, hw, pads, s):
    """What load_mosaic hands to random_perspective (dataloaders.py:828-842; segment/dataloaders.py:266-280), or the letterbox branch of the
    segmentation `__getitem__`: `_canvas_boxes`, the polygons likewise (xyn2xy in float32; mosaic only: clipped to the canvas), then
    `_copy_paste` where the sample drew one.  -> (labels (n, 5), n polygons (k, 2) float32, the int32 polygons the image half pastes)."""
    t, counts = _canvas_boxes(labels, d, hw, pads, s)
    mosaic = d.get("mosaic", True)
    segs = []
    for i, (h, w), (padw, padh), k in zip(d["indices"], hw, pads, counts):
        if len(segments[i]) != k:
            raise ValueError(f"image {i}: {k} labels but {len(segments[i])} polygons")
        if k:
            # all polygons of the tile at once
            y = _xyn2xy(np.concatenate([np.asarray(g, dtype=np.float32).reshape(-1, 2) for g in segments[i]], 0), w, h, padw, padh)
            if mosaic:
                np.clip(y, 0, 2 * s, out=y)
            segs.extend(np.split(y, np.cumsum([len(g) for g in segments[i]])[:-1]))
    paste = []
    if mosaic and d.get("paste"):
        t, segs, accepted = _copy_paste(t, segs, d["paste"], 2 * s)
        paste = [segs[j].astype(np.int32) for j in accepted]               # augmentations.py:216
    return t, segs, paste


def _warp_polygons(t, segs, d, M, width, height):
    """random_perspective's `use_segments` branch (augmentations.py:166-176, :193-195; all of segment/augmentations.py:71-89):
    resample_segments(n = 1000), xy @ M.T, new box = segment2box(xy, width, height) (NOT the warped corners), box_candidates(area_thr = 0.01).
    -> ((k, 5) [cls, x1, y1, x2, y2], (k, 1000, 2) float64 polygons) in output pixels."""
    n = len(t)
    if not n:
        return t, np.zeros((0, 1000, 2))
    xy = np.ones((n, 1000, 3))
    xy[:, :, :2] = resample_segments(segs)
    xy = (xy @ M.T)[:, :, :2]                                          # n products of the reference's own shape (1000, 3) @ (3, 3)
    x, y = xy[:, :, 0], xy[:, :, 1]
    ins = (x >= 0) & (y >= 0) & (x <= width) & (y <= height)            # segment2box (general.py:592-600)
    any_in = ins.any(1)
    new = np.stack((np.where(ins, x, np.inf).min(1), np.where(ins, y, np.inf).min(1), np.where(ins, x, -np.inf).max(1),
                    np.where(ins, y, -np.inf).max(1)), 1)
    new[~any_in] = 0.0
    t, keep = _box_candidates(t, new, d["scale"], 0.01)
    return t, xy[keep]


def _labels(labels, segments, d, hw, pads, M, width, height, s):
    """Label half of the sample up to random_perspective -> ((k, 5) [cls, x1, y1, x2, y2] in output pixels, the polygons to paste).
    Without polygons, and on the letterbox branch (dataloaders.py:719-732 passes none): `_canvas_boxes`, corners through M + hull + clip +
    box_candidates(area_thr = 0.10) (augmentations.py:177-195).  A mosaic of a dataset with polygons: `_canvas_stage` (copy_paste) and
    the `use_segments` branch, `_warp_polygons`."""
    paste = []
    if segments is not None and d.get("mosaic", True):
        t, segs, paste = _canvas_stage(labels, segments, d, hw, pads, s)
        if any(x.any() for x in segs):                                   # use_segments (augmentations.py:164)
            return _warp_polygons(t, segs, d, M, width, height)[0], paste
    else:
        t, _ = _canvas_boxes(labels, d, hw, pads, s)
    n = len(t)
    if n:
        pts = np.ones((n * 4, 3))
        pts[:, :2] = t[:, [1, 2, 3, 4, 1, 4, 3, 2]].reshape(n * 4, 2)
        pts = (pts @ M.T)[:, :2].reshape(n, 8)
        xs, ys = pts[:, [0, 2, 4, 6]], pts[:, [1, 3, 5, 7]]
        new = np.concatenate((xs.min(1), ys.min(1), xs.max(1), ys.max(1))).reshape(4, n).T
        new[:, [0, 2]] = new[:, [0, 2]].clip(0, width)
        new[:, [1, 3]] = new[:, [1, 3]].clip(0, height)
        t, _ = _box_candidates(t, new, d["scale"], 0.10)
    return t, paste


def _finish_labels(t, d, width, height):
    """dataloaders.py:735-757 on the (possibly mixup-concatenated) pixel boxes: normalised xywh with clipping (:737), flips."""
    if len(t):
        b = t[:, 1:5]
        b[:, [0, 2]] = b[:, [0, 2]].clip(0, width - 1e-3)
        b[:, [1, 3]] = b[:, [1, 3]].clip(0, height - 1e-3)
        out = b.copy()
        out[:, 0] = ((b[:, 0] + b[:, 2]) / 2) / width
        out[:, 1] = ((b[:, 1] + b[:, 3]) / 2) / height
        out[:, 2] = (b[:, 2] - b[:, 0]) / width
        out[:, 3] = (b[:, 3] - b[:, 1]) / height
        t[:, 1:5] = out
        if d["flipud"]:
            t[:, 2] = 1 - t[:, 2]
        if d["fliplr"]:
            t[:, 1] = 1 - t[:, 1]
    res = np.zeros((len(t), 6), dtype=np.float32)
    if len(t):
        res[:, 1:] = t
    return res


def _check_image(im, who):
    """The image contract of the batched kernels: uint8 (h, w, 3) with contiguous rows -> (h0, w0)."""
    if not (_lib.accepts(im) and im.dtype == torch.uint8 and im.ndim == 3 and im.shape[2] == 3 and im.stride(2) == 1 and im.stride(1) == 3):
        raise ValueError(f"{who}: images must be uint8 (h, w, 3) device tensors with contiguous rows")
    return int(im.shape[0]), int(im.shape[1])


def _fill_job(j, images, d, s):
    """Geometry half of one job of the y5_mosaic_batch table (tiles, rectangles, inverse affine map) -> (hw, pads, M, width, height): the resized
    (h, w) of every tile and the (padw, padh) that move its labels to the canvas -- the integer tile offsets of a mosaic, the FLOAT half-borders
    dw, dh on the letterbox branch."""
    hw = []
    for t, i in enumerate(d["indices"]):
        im = images[i]
        h0, w0 = _check_image(im, "mosaic_batch")
        rh, rw = _resized_hw(h0, w0, s)
        hw.append((rh, rw))
        j.src[t], j.h0[t], j.w0[t], j.stride[t], j.rh[t], j.rw[t] = im.data_ptr(), h0, w0, int(im.stride(0)), rh, rw
    mosaic = d.get("mosaic", True)
    if mosaic:
        rects = _tile_rects(hw, d["yc"], d["xc"], s)
        pads = [(x1a - x1b, y1a - y1b) for x1a, y1a, _x2a, _y2a, x1b, y1b in rects]
    else:
        # letterbox(auto=False, scaleup=True) of an image whose longest side already is s (augmentations.py:85-115): r = 1, no second resize;
        # the image sits at (left, top) = (round(dw - 0.1), round(dh - 0.1)) of an s x s canvas of 114s, the labels move by the FLOAT dw, dh
        (rh, rw), = hw
        dw, dh = (s - rw) / 2, (s - rh) / 2
        left, top = int(round(dw - 0.1)), int(round(dh - 0.1))
        rects, pads = [(left, top, left + rw, top + rh, 0, 0)], [(dw, dh)]
        j.canvas = s
    for t, (x1a, y1a, x2a, y2a, x1b, y1b) in enumerate(rects):
        j.x1a[t], j.y1a[t], j.x2a[t], j.y2a[t], j.x1b[t], j.y1b[t] = x1a, y1a, x2a, y2a, x1b, y1b
    M, width, height = _affine(d, s, mosaic)
    A = _invert_affine(M)
    for k in range(6):
        j.A[k] = float(A.reshape(-1)[k])
    return hw, pads, M, width, height


def _finish_job(j, d, use_hsv):
    """HSV look-up tables (augmentations.py:76-79) and flips of one rendered job."""
    x = np.arange(0, 256, dtype=np.float64)
    r = np.asarray(d["hsv"], dtype=np.float64)
    luts = (((x * r[0]) % 180).astype(np.uint8), np.clip(x * r[1], 0, 255).astype(np.uint8), np.clip(x * r[2], 0, 255).astype(np.uint8))
    for c in range(3):
        C.memmove(j.lut[c], luts[c].ctypes.data, 256)
    j.hsv, j.flipud, j.fliplr = int(use_hsv), int(bool(d["flipud"])), int(bool(d["fliplr"]))


def paste_planes(polys, poly_plane, n_planes, S2, device):
    """ONE y5_paste_planes launch (csrc/copy_paste.h): polys: int32 (k, 2) canvas polygons; poly_plane: their planes, ascending.
    -> (n_planes, S2, ceil(S2 / 32)) int32 words; bit x & 31 of word x >> 5 of row y = the un-flipped union of the plane's filled polygons."""
    plane = np.asarray(poly_plane, dtype=np.int32).reshape(-1)
    if len(plane) != len(polys) or (len(plane) and (plane.min() < 0 or plane.max() >= n_planes or (np.diff(plane) < 0).any())):
        raise ValueError("paste_planes: poly_plane must be ascending plane indices in [0, n_planes), one per polygon")
    off = np.zeros(len(polys) + 1, dtype=np.int32)
    np.cumsum([len(pg) for pg in polys], out=off[1:])
    pts = [np.asarray(pg, dtype=np.int32).reshape(-1) for pg in polys]
    meta = torch.from_numpy(np.concatenate((*pts, off, plane)).astype(np.int32)).to(device)
    planes = torch.empty((n_planes, S2, (S2 + 31) // 32), dtype=torch.int32, device=device)
    lib = _lib.lib()
    p_off = meta.data_ptr() + 8 * int(off[-1])
    _lib.check(lib.y5_paste_planes(C.c_void_p(meta.data_ptr()), C.c_void_p(p_off), C.c_void_p(p_off + 4 * len(off)), len(polys), n_planes, S2,
                                   C.c_void_p(planes.data_ptr()), _lib.stream(device)), lib)
    return planes


def _render(jobs, B, s, dev, dtype, normalize, pasted=None):
    """The y5_mosaic_batch launch over a filled job table -> (B, 3, s, s).  pasted: {job index: its int32 polygons to paste} in job-loop
    order; when a job pastes, ONE `paste_planes` launch makes a plane per pasting job and the launch is y5_mosaic_batch_paste."""
    table = _lib.device_table(jobs, dev)
    out = torch.empty((B, 3, s, s), dtype=dtype, device=dev)
    lib = _lib.lib()
    args = (B, s, 114, C.c_void_p(out.data_ptr()), _lib.dtype_code(dtype), int(normalize and dtype != torch.uint8), _lib.stream(dev))
    if pasted:
        job_plane = np.full(len(jobs), -1, dtype=np.int32)
        for k, job in enumerate(pasted):
            job_plane[job] = k
        planes = paste_planes([pg for polys in pasted.values() for pg in polys], [k for k, polys in enumerate(pasted.values()) for _ in polys],
                              len(pasted), 2 * s, dev)
        job_plane = torch.from_numpy(job_plane).to(dev)
        _lib.check(lib.y5_mosaic_batch_paste(C.c_void_p(table.data_ptr()), len(jobs), C.c_void_p(job_plane.data_ptr()),
                                             C.c_void_p(planes.data_ptr()), *args), lib)
    else:
        _lib.check(lib.y5_mosaic_batch(C.c_void_p(table.data_ptr()), *args), lib)
    return out


def _assemble(images, draws, s, hyp, sample_labels):
    """Host half of a training batch: the filled y5_mosaic_batch job table, the (k, 6) targets of every image and, when the dataset has them, the
    warped polygons with their images.  sample_labels(d, hw, pads, M, width, height) -> (pixel boxes (k, 5), paste) or (pixel boxes, polygons
    (k, ...), paste) of one mosaic or letterboxed image, paste = the int32 canvas polygons copy_paste accepted (`_canvas_stage`).
    -> (jobs, labs, polys, inst, pasted: {job index: paste} of the jobs that paste, the input of `_render`)."""
    B = len(draws)
    use_hsv = bool(hyp["hsv_h"] or hyp["hsv_s"] or hyp["hsv_v"])

    def fill(j, d):
        hw, pads, M, width, height = _fill_job(jobs[j], images, d, s)
        *parts, paste = sample_labels(d, hw, pads, M, width, height)
        if paste:
            pasted[j] = paste
        return parts, width, height

    jobs = (_lib.MosaicJob * (B + sum(d.get("partner") is not None for d in draws)))()
    labs, polys, inst, npart, pasted = [], [], [], 0, {}
    for b, d in enumerate(draws):
        j = jobs[b]
        parts, width, height = fill(b, d)
        if d.get("partner") is not None:
            # mixup (dataloaders.py:707-708; segment/augmentations.py:14-23): the partner mosaic is a job of its own behind the B rendered ones,
            # its labels (and segments) are concatenated; it ran its own copy_paste
            parts2, _, _ = fill(B + npart, d["partner"])
            j.mix_job, j.mix_r = B + npart + 1, float(d["mix_r"])
            npart += 1
            parts = [np.concatenate(p, 0) for p in zip(parts, parts2)]
        _finish_job(j, d, use_hsv)
        lb = _finish_labels(parts[0], d, width, height)
        lb[:, 0] = b                                             # collate_fn (dataloaders.py:860-862; segment/dataloaders.py:299-300)
        labs.append(lb)
        for sg in parts[1:]:
            polys.extend(sg)
            inst.extend([b] * len(sg))
    return jobs, labs, polys, inst, pasted


def _targets(labs):
    return torch.from_numpy(np.concatenate(labs, 0) if labs else np.zeros((0, 6), np.float32))


def mosaic_batch(images, labels, draws, s, hyp=None, dtype=torch.uint8, normalize=False, segments=None):
    """Render one training batch.  images: list of uint8 (h, w, 3) BGR tensors resident on the device (any sizes); labels: list of
    (k, 5) arrays [cls, xc, yc, w, h] normalised; draws: list (one per output image) of `draw_sample` dicts.  segments: None, or per image
    the list of (k, 2) normalised polygons of its label rows (a COCO-style label cache; ValueError when they are not one per row): the
    mosaics then take random_perspective's `use_segments` branch, and the draws' copy_paste samples (`draw_sample(counts=...)`) are pasted.
    Returns (imgs (B, 3, s, s) `dtype` RGB CHW, targets (nt, 6) float32 [image index in batch, cls, xc, yc, w, h])."""
    hyp = HYP_AUG if hyp is None else hyp
    jobs, labs, _, _, pasted = _assemble(images, draws, s, hyp, lambda d, *geo: _labels(labels, segments, d, *geo, s))
    return _render(jobs, len(draws), s, images[0].device, dtype, normalize, pasted), _targets(labs)


def collate_fn4(imgs, targets, paths, shapes, rng=random):
    """`LoadImagesAndLabels.collate_fn4` (utils/dataloaders.py:865-891; train.py --quad) on a batch that `collate_fn` already made: imgs
    (B, C, H, W) uint8 on the device, targets (nt, 6) float32 with the image index in column 0.  Every group of four images becomes one
    (C, 2H, 2W) image -- by a coin per group (`rng.random() < 0.5`, drawn in order AFTER every sample draw of the batch, as the reference's
    collate runs after its __getitem__s) the 2x bilinear upsample of the first with its labels, or the 2 x 2 tiling of the four with the
    labels shifted and halved by the reference's own expression in float32.  One `y5_collate4` launch (csrc/collate4.h) makes the images.
    -> (imgs (B // 4, C, 2H, 2W) uint8, targets, paths[:B // 4], shapes[:B // 4]); the B % 4 trailing samples are dropped (:869)."""
    if imgs.dtype != torch.uint8:
        raise TypeError("collate_fn4: a uint8 image batch is expected (the reference's loader collates uint8 images)")
    if imgs.dim() != 4 or not _lib.accepts(imgs):
        raise TypeError("collate_fn4: a (B, C, H, W) GPU batch is expected")
    B, Cn, H, W = (int(v) for v in imgs.shape)
    n = B // 4
    if n < 1:
        raise ValueError(f"collate_fn4: a quad batch needs at least 4 samples, got {B}")
    flags = [rng.random() < 0.5 for _ in range(n)]                                                   # :877
    imgs = imgs.contiguous()
    dev = imgs.device
    out = torch.empty((n, Cn, 2 * H, 2 * W), dtype=torch.uint8, device=dev)
    fl = torch.tensor(flags, dtype=torch.uint8).to(dev)
    lib = _lib.lib()
    _lib.check(lib.y5_collate4(C.c_void_p(imgs.data_ptr()), B, Cn, H, W, C.c_void_p(fl.data_ptr()), C.c_void_p(out.data_ptr()), _lib.stream(dev)), lib)
    t = targets.detach().cpu().float()
    label = [t[t[:, 0] == b] for b in range(4 * n)]          # (boolean selection keeps the row order and copies)
    ho = torch.tensor([[0.0, 0, 0, 1, 0, 0]])
    wo = torch.tensor([[0.0, 0, 1, 0, 0, 0]])
    s = torch.tensor([[1, 1, 0.5, 0.5, 0.5, 0.5]])
    label4 = []
    for i, up in enumerate(flags):
        a, b, c, d = label[4 * i:4 * i + 4]
        lb = a if up else torch.cat((a, b + ho, c + wo, d + ho + wo), 0) * s                            # :881, :884
        lb[:, 0] = i                                                                                   # :888-889
        label4.append(lb)
    return out, torch.cat(label4, 0), paths[:n] if paths is not None else None, shapes[:n] if shapes is not None else None


class MosaicLoader:
    """Re-iterable training loader over an in-HBM dataset: every epoch visits the images in a fresh random order (DataLoader
    shuffle=True / SmartDistributedSampler: rank r takes indices r::world of the epoch's permutation), each batch is one
    `mosaic_batch` launch.  Yields (imgs, targets, paths, shapes) like the reference's collate_fn.
    quad=True (train.py --quad, utils/dataloaders.py:159,184): every batch goes through `collate_fn4` -- batch_size / 4 images of twice the
    side -- and the trailing incomplete batch of an epoch is dropped (`drop_last=quad`); the images must be uint8."""

    def __init__(self, images, labels, img_size=640, batch_size=16, hyp=None, dtype=torch.uint8, rank=-1, world_size=1, seed=0, paths=None,
                 segments=None, quad=False):
        if segments is not None and [len(sg) for sg in segments] != [len(lb) for lb in labels]:
            raise ValueError("MosaicLoader: segments must hold one polygon per label row of every image")
        if quad and dtype != torch.uint8:
            raise TypeError("MosaicLoader: quad batches are collated from uint8 images (collate_fn4)")
        if quad and batch_size < 4:
            raise ValueError("MosaicLoader: quad needs batch_size >= 4")
        self.quad = bool(quad)
        self.images, self.labels, self.s, self.bs = images, labels, img_size, batch_size
        self.segments = segments                                          # see `mosaic_batch`
        self.counts = None if segments is None else [len(sg) for sg in segments]
        self.hyp = dict(HYP_AUG if hyp is None else hyp)
        self.dtype, self.rank, self.world, self.seed, self.epoch = dtype, rank, world_size, seed, 0
        self.paths = paths or [f"image{i}" for i in range(len(images))]
        n = len(images)
        # SmartDistributedSampler pads every rank to num_samples = ceil(n / world) (utils/dataloaders.py:94-101): same batch count on all ranks
        self.n_local = (n + world_size - 1) // world_size if rank != -1 else n

    def set_epoch(self, epoch):
        self.epoch = epoch

    @property
    def sampler(self):
        return self

    @property
    def shapes(self):
        """(n_images, 2) float64 (w, h) of the source images, like the reference dataset's `.shapes` (utils/dataloaders.py:558): with `.labels`
        this is all autoanchor.check_anchors / kmean_anchors read, so the loader can be passed to them as the dataset."""
        return np.array([[int(im.shape[1]), int(im.shape[0])] for im in self.images], dtype=np.float64)

    def __len__(self):
        return self.n_local // self.bs if self.quad else (self.n_local + self.bs - 1) // self.bs

    def _epoch_order(self):
        """This rank's image ids of the current epoch: the seeded shuffle, every `world`-th from `rank`, padded to the common length."""
        g = random.Random(self.seed + self.epoch)
        order = list(range(len(self.images)))
        g.shuffle(order)
        if self.rank != -1:
            from .train_loop import pad_to_common

            order = pad_to_common(order[self.rank::self.world], len(self.images), self.world)
        return order

    def _batch(self, ids):
        draws = [draw_sample(i, len(self.images), self.s, self.hyp, counts=self.counts) for i in ids]
        imgs, targets = mosaic_batch(self.images, self.labels, draws, self.s, self.hyp, self.dtype, normalize=True, segments=self.segments)
        return imgs, targets, [self.paths[i] for i in ids], None

    def __iter__(self):
        order = self._epoch_order()
        for b0 in range(0, len(self) * self.bs if self.quad else len(order), self.bs):
            batch = self._batch(order[b0:b0 + self.bs])
            yield collate_fn4(*batch) if self.quad else batch
        self.epoch += 1


# ---- segmentation datasets: utils/segment/dataloaders.py:130-301, utils/segment/augmentations.py:14-91 ---------------------------------
def labels_from_segments(cls, segments):
    """(k, 5) float32 [cls, xc, yc, w, h] from k polygons: the `segments2boxes` rule the reference applies when it reads a polygon label
    file (utils/dataloaders.py:923; general.py `segments2boxes`: min / max of the polygon, then xyxy2xywh), so a dataset needs only polygons."""
    boxes = []
    for sgm in segments:
        x, y = np.asarray(sgm).T
        boxes.append([x.min(), y.min(), x.max(), y.max()])
    b = np.array(boxes, dtype=np.float64).reshape(-1, 4)
    out = np.empty((len(b), 5), dtype=np.float32)
    out[:, 0] = np.asarray(cls, dtype=np.float32).reshape(-1)
    out[:, 1], out[:, 2] = (b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2
    out[:, 3], out[:, 4] = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    return out


_GRIDS = {}


def _grid(k, n):
    """np.linspace(0, k - 1, n) as np.interp sees it over xp = arange(k): interval index j, x - xp[j], and the exact hits of a knot."""
    g = _GRIDS.get((k, n))
    if g is None:
        x = np.linspace(0, k - 1, n)
        j = np.minimum(np.floor(x).astype(np.intp), max(k - 2, 0))
        g = _GRIDS[(k, n)] = (j, np.minimum(j + 1, k - 1), x - j, x == j, x == j + 1)
    return g


def resample_segments(segs, n=1000):
    """general.py:603-610 on a list of (k, 2) arrays -> (len, n, 2) float64.  np.interp over the integer knots xp = arange(k + 1) is
    fp[j] + (fp[j + 1] - fp[j]) * (x - j) (its slope divides by xp[j + 1] - xp[j] = 1) with fp[j] returned where x hits a knot; polygons of
    equal length share x, so they are resampled together (tests/test_emu_seg_data.py pins this against np.interp and the literal loop)."""
    out = np.empty((len(segs), n, 2), dtype=np.float64)
    by_len = {}
    for i, sg in enumerate(segs):
        by_len.setdefault(len(sg), []).append(i)
    for k, ids in by_len.items():
        fp = np.stack([segs[i] for i in ids]).astype(np.float64)
        fp = np.concatenate((fp, fp[:, 0:1]), 1)
        j, j1, dx, hit0, hit1 = _grid(k + 1, n)
        a, b = fp.take(j, axis=1), fp.take(j1, axis=1)
        v = (b - a) * dx[None, :, None] + a
        out[ids] = np.where(hit0[None, :, None], a, np.where(hit1[None, :, None], b, v))
    return out


def _xyn2xy(x, w, h, padw, padh):
    """general.py:584-589 `xyn2xy` on (..., 2) float32 polygon points: normalised -> pixels."""
    y = np.copy(x)
    y[..., 0] = w * x[..., 0] + padw
    y[..., 1] = h * x[..., 1] + padh
    return y


def _seg_labels(labels, segments, d, hw, pads, M, width, height, s):
    """Label half of one sample as the segmentation loader computes it: `_canvas_stage`, then utils/segment/augmentations.py:26-91
    `random_perspective`, `_warp_polygons`.  -> ((k, 5) float32 [cls, x1, y1, x2, y2], (k, 1000, 2) float64 polygons in output pixels,
    the polygons to paste)."""
    t, segs, paste = _canvas_stage(labels, segments, d, hw, pads, s)
    return (*_warp_polygons(t, segs, d, M, width, height), paste)


def polygon_masks(polys, inst_img, B, H, W, ratio, overlap, flips, device):
    """ONE y5_polygon_masks call (csrc/seg_data.h) for the polygons of a batch.  polys: list of (k, 2) float pixel polygons in target order;
    inst_img: their images, non-decreasing; flips: (B, 2) {up-down, left-right} or None.
    -> (masks, order): overlap: (B, h, w) index planes (uint8 up to 255 instances per image, float32 beyond) and `order` (n,) on the HOST,
    the per-image permutation (local indices) the target rows must follow -- the ONE device-to-host read; else (n, h, w) uint8, None."""
    n = len(polys)
    h, w = H // ratio, W // ratio
    inst = np.asarray(inst_img, dtype=np.int32).reshape(-1)
    if n and (inst.min() < 0 or inst.max() >= B or (np.diff(inst) < 0).any()):
        raise ValueError("polygon_masks: inst_img must be non-decreasing image indices in [0, B)")
    counts = np.bincount(inst, minlength=B) if n else np.zeros(B, np.int64)
    f32 = bool(overlap) and n and int(counts.max()) > 255
    dtype = torch.float32 if f32 else torch.uint8
    masks = torch.empty((B if overlap else n, h, w), dtype=dtype, device=device)
    lib = _lib.lib()
    if n:
        off = np.zeros(n + 1, dtype=np.int32)
        np.cumsum([len(p) for p in polys], out=off[1:])
        xy = np.concatenate([np.asarray(p, dtype=np.float64).reshape(-1, 2) for p in polys], 0)
        xy_d = torch.from_numpy(np.ascontiguousarray(xy)).to(device)
        meta = torch.from_numpy(np.concatenate((off, inst))).to(device)
        order = torch.empty(n, dtype=torch.int32, device=device)
        area = torch.empty(n, dtype=torch.int64, device=device)
        nb = int(lib.y5_polygon_masks_ws_bytes(n, H, W, ratio))
        ws = _lib.workspace(nb, device)
        ptrs = (xy_d.data_ptr(), meta.data_ptr(), meta.data_ptr() + 4 * (n + 1), order.data_ptr(), area.data_ptr(), ws.data_ptr())
    else:
        order, nb, ptrs = None, 0, (None,) * 6
    fl = None if flips is None else torch.from_numpy(np.ascontiguousarray(np.asarray(flips, dtype=np.uint8).reshape(B, 2))).to(device)
    if overlap or n:
        _lib.check(lib.y5_polygon_masks(C.c_void_p(ptrs[0]), C.c_void_p(ptrs[1]), C.c_void_p(ptrs[2]), n, B, H, W, ratio, int(bool(overlap)),
                                        C.c_void_p(fl.data_ptr() if fl is not None else None), C.c_void_p(masks.data_ptr()),
                                        _lib.Y5_F32 if f32 else _lib.Y5_U8, C.c_void_p(ptrs[3]), C.c_void_p(ptrs[4]), C.c_void_p(ptrs[5]), nb,
                                        _lib.stream(device)), lib)
    if not overlap:
        return masks, None
    return masks, (order.cpu().numpy() if n else np.zeros(0, np.int32))


def _reorder(labs, order):
    """labels = labels[sorted_idx] (segment/dataloaders.py:189) for every image of the batch from the kernel's per-image permutations."""
    out, o = [], 0
    for lb in labs:
        k = len(lb)
        out.append(lb[order[o:o + k]] if k else lb)
        o += k
    return out


def seg_mosaic_geometry(images, labels, segments, draws, s, hyp):
    """Host half of `seg_mosaic_batch`: the filled y5_mosaic_batch job table, the (k, 6) targets of every image in LABEL order, and the warped
    polygons (float64 output pixels) with their images -- the input of `polygon_masks`."""
    return _seg_assemble(images, labels, segments, draws, s, hyp)[:4]


def _seg_assemble(images, labels, segments, draws, s, hyp):
    return _assemble(images, draws, s, hyp, lambda d, *geo: _seg_labels(labels, segments, d, *geo, s))


def _masks_and_targets(labs, polys, inst, B, s, mask_ratio, overlap, flips, dev):
    """The mask half of a segmentation batch: ONE `polygon_masks` call, then, with overlap, the target rows of every image in its area order."""
    masks, order = polygon_masks(polys, inst, B, s, s, mask_ratio, overlap, flips, dev)
    if overlap:
        labs = _reorder(labs, order)
    return _targets(labs), masks


def seg_mosaic_batch(images, labels, segments, draws, s, hyp=None, dtype=torch.uint8, normalize=False, overlap=True, mask_ratio=4):
    """One training batch of a segmentation dataset.  images / labels as `mosaic_batch`; segments[i]: the list of (k, 2) float arrays of
    image i, normalised xy, one per label row; draws: `draw_sample_seg` dicts.  The image half is `mosaic_batch`'s launch over the same job
    table.  Returns (imgs (B, 3, s, s), targets (nt, 6) float32 -- with overlap, the rows of every image in the mask kernel's area order --,
    masks: overlap (B, s // mask_ratio, s // mask_ratio) index planes, else (nt, ...) 0 / 1 in target order)."""
    hyp = HYP_AUG if hyp is None else hyp
    dev = images[0].device
    B = len(draws)
    jobs, labs, polys, inst, pasted = _seg_assemble(images, labels, segments, draws, s, hyp)
    out = _render(jobs, B, s, dev, dtype, normalize, pasted)
    flips = [(bool(d["flipud"]), bool(d["fliplr"])) for d in draws]
    targets, masks = _masks_and_targets(labs, polys, inst, B, s, mask_ratio, overlap, flips, dev)
    return out, targets, masks


class SegMosaicLoader(MosaicLoader):
    """`MosaicLoader` for a segmentation dataset (utils/segment/dataloaders.py `LoadImagesAndLabelsAndMasks`, augment = True, rect = False):
    yields (imgs, targets, paths, None, masks) as the reference's collate_fn does -- the batch `segment_loss.ComputeLoss` and
    `train_loop.train` take.  labels may be None: they are then derived from the polygons (`labels_from_segments` needs `classes`).
    hyp['copy_paste'] > 0 (data/hyps/hyp.scratch-high.yaml: 0.1) pastes mirrored instances into the mosaics as utils/augmentations.py:200-222 does:
    the pasted polygons become label rows and go through the same warp into the one `y5_polygon_masks` call; per batch the order is host
    geometry, one y5_paste_planes launch (skipped when no job pasted), the render launch, the mask call -- no further device-to-host read."""

    def __init__(self, images, labels, segments, img_size=640, batch_size=16, hyp=None, dtype=torch.uint8, rank=-1, world_size=1, seed=0,
                 paths=None, overlap=True, mask_ratio=4, classes=None, quad=False):
        if quad:
            # the reference's LoadImagesAndLabelsAndMasks inherits collate_fn4, which cannot unpack its 5-tuples (utils/segment/dataloaders.py:82)
            raise NotImplementedError("SegMosaicLoader: quad batches are not defined for the segmentation loader")
        if labels is None:
            labels = [labels_from_segments(c, sg) for c, sg in zip(classes, segments)]
        super().__init__(images, labels, img_size, batch_size, hyp, dtype, rank, world_size, seed, paths, segments)
        self.overlap, self.mask_ratio = overlap, mask_ratio

    def _batch(self, ids):
        draws = [draw_sample_seg(i, len(self.images), self.s, self.hyp, counts=self.counts) for i in ids]
        imgs, targets, masks = seg_mosaic_batch(self.images, self.labels, self.segments, draws, self.s, self.hyp, self.dtype, normalize=True,
                                                overlap=self.overlap, mask_ratio=self.mask_ratio)
        return imgs, targets, [self.paths[i] for i in ids], None, masks


def seg_letterbox_batch(images, labels, segments, ids, s, dtype=torch.uint8, normalize=False, overlap=True, mask_ratio=1, area=False):
    """The augment = False, rect = False branch of the segmentation `__getitem__` (utils/segment/dataloaders.py:144-199) + collate_fn for the
    images `ids`: load_image, letterbox(auto=False, scaleup=False), labels and polygons to pixels with the float pad; the polygons are NOT
    resampled (own lengths); no warp, no HSV, no flips.  The image half is a `y5_mosaic_batch` launch with one-tile jobs on an s x s canvas and
    the identity map.  area=False (default, what tests/golden/seg_data_val.npz pins): an image larger than s is shrunk with INTER_LINEAR, as in
    the training branch; area=True: the image half is ONE `y5_letterbox_area_batch` launch instead, which shrinks with load_image's INTER_AREA
    (dataloaders.py:787) -- the same bits for every image that is copied or enlarged.
    Returns (imgs, targets, shapes, masks): shapes[i] = ((h0, w0), ((h / h0, w / w0), (dw, dh))) as :151."""
    dev = images[0].device
    B = len(ids)
    jobs = (_lib.MosaicJob * B)()
    ident = {"mosaic": False, "angle": 0.0, "scale": 1.0, "shear": (0.0, 0.0), "translate": (0.5, 0.5)}
    labs, polys, inst, shapes = [], [], [], []
    for b, i in enumerate(ids):
        d = dict(ident, indices=[i])
        j = jobs[b]
        hw, pads, _M, width, height = _fill_job(j, images, d, s)
        (h, w), (dw, dh) = hw[0], pads[0]
        h0, w0 = int(images[i].shape[0]), int(images[i].shape[1])
        shapes.append(((h0, w0), ((h / h0, w / w0), (dw, dh))))
        lb, _ = _canvas_boxes(labels, d, hw, pads, s)
        sgs = [_xyn2xy(np.asarray(sg, dtype=np.float32), w, h, dw, dh) for sg in segments[i]]
        if len(sgs) != len(lb):
            raise ValueError(f"image {i}: {len(lb)} labels but {len(sgs)} polygons")
        res = _finish_labels(lb, {"flipud": False, "fliplr": False}, width, height)
        res[:, 0] = b
        labs.append(res)
        polys.extend(sgs)
        inst.extend([b] * len(sgs))
    if area:
        out = letterbox_area_batch([images[i] for i in ids], [(j.rh[0], j.rw[0]) for j in jobs], [(j.y1a[0], j.x1a[0]) for j in jobs], s, s, dtype,
                                   normalize)
    else:
        out = _render(jobs, B, s, dev, dtype, normalize)
    targets, masks = _masks_and_targets(labs, polys, inst, B, s, mask_ratio, overlap, None, dev)
    return out, targets, shapes, masks


class SegValLoader:
    """Validation loader of a segmentation dataset (augment = False, rect = False): yields the (imgs, targets, paths, shapes, masks)
    five-tuple `segment_val.run` consumes, images in dataset order.  area: see `seg_letterbox_batch`."""

    def __init__(self, images, labels, segments, img_size=640, batch_size=16, dtype=torch.uint8, paths=None, overlap=True, mask_ratio=1, classes=None,
                 area=False):
        if labels is None:
            labels = [labels_from_segments(c, sg) for c, sg in zip(classes, segments)]
        self.images, self.labels, self.segments, self.s, self.bs = images, labels, segments, img_size, batch_size
        self.dtype, self.overlap, self.mask_ratio, self.area = dtype, overlap, mask_ratio, area
        self.paths = paths or [f"image{i}" for i in range(len(images))]

    def __len__(self):
        return (len(self.images) + self.bs - 1) // self.bs

    def __iter__(self):
        for b0 in range(0, len(self.images), self.bs):
            ids = list(range(b0, min(b0 + self.bs, len(self.images))))
            imgs, targets, shapes, masks = seg_letterbox_batch(self.images, self.labels, self.segments, ids, self.s, self.dtype, normalize=True,
                                                               overlap=self.overlap, mask_ratio=self.mask_ratio, area=self.area)
            yield imgs, targets, [self.paths[i] for i in ids], shapes, masks


# ---- detection validation: LoadImagesAndLabels(augment=False, rect, pad) (utils/dataloaders.py:589-612, :710-736, :768-790) -----------------
@functools.lru_cache(maxsize=256)
def _area_axis(ssize, dsize):
    """One axis of OpenCV's `computeResizeAreaTab` (modules/imgproc/src/resize.cpp) in double, as include/yolov5_hip.h states it:
    -> (entries (dsize, 2) int32 {first source index, tap count}, weights float32 in entry order).  The taps of an output index are
    consecutive source indices: the left partial cell, the full cells, the right partial cell."""
    scale = float(ssize) / dsize
    ents, wts = np.empty((dsize, 2), np.int32), []
    for d in range(dsize):
        f1 = d * scale
        f2 = f1 + scale
        cell = min(scale, ssize - f1)
        s1, s2 = math.ceil(f1), min(math.floor(f2), ssize - 1)
        s1 = min(s1, s2)
        w = []
        first = s1
        if s1 - f1 > 1e-3:
            first = s1 - 1
            w.append((s1 - f1) / cell)
        w.extend([1.0 / cell] * (s2 - s1))
        if f2 - s2 > 1e-3:
            w.append(min(min(f2 - s2, 1.0), cell) / cell)
        ents[d] = first, len(w)
        wts.extend(w)
    return ents, np.asarray(wts, dtype=np.float64).astype(np.float32)


def _int_scale(ssize, dsize):
    """The integer k when (double)ssize / dsize is within DBL_EPSILON of it (cv::resize's `is_area_fast` test), else 0."""
    scale = float(ssize) / dsize
    k = int(round(scale))
    return k if abs(scale - k) < np.finfo(np.float64).eps else 0


def area_jobs(ims, sizes, places):
    """Job table and tap tables of one `y5_letterbox_area_batch` launch.  ims: uint8 (h0, w0, 3) tensors; sizes[i] = (nh, nw) of the resized
    image (load_image); places[i] = (top, left) of it on the canvas.  The path per job: copy when the sizes agree, INTER_LINEAR when either side
    grows, else INTER_AREA -- 2x2, integer block or tap tables.  -> (ctypes array of y5_area_job, int32 words)."""
    jobs = (_lib.AreaJob * len(ims))()
    words, off, seen = [], 0, {}
    for j, im, (nh, nw), (top, left) in zip(jobs, ims, sizes, places):
        h0, w0 = _check_image(im, "letterbox_area_batch")
        j.src, j.h0, j.w0, j.stride = im.data_ptr(), h0, w0, int(im.stride(0))
        j.nh, j.nw, j.top, j.left = int(nh), int(nw), int(top), int(left)
        if (nh, nw) == (h0, w0):
            j.mode = _lib.AREA_COPY
        elif nh > h0 or nw > w0:
            j.mode = _lib.AREA_LINEAR
        else:
            ix, iy = _int_scale(w0, nw), _int_scale(h0, nh)
            if ix == 2 and iy == 2:
                j.mode = _lib.AREA_2X2
            elif ix and iy:
                j.mode, j.ix, j.iy = _lib.AREA_INT, ix, iy
            else:
                j.mode = _lib.AREA_TAB
                key = (h0, w0, int(nh), int(nw))
                if key not in seen:                              # {first, count, weight offset} per output index, then the weights, x then y
                    tabs = []
                    for ssize, dsize in ((w0, nw), (h0, nh)):
                        ents, wts = _area_axis(ssize, int(dsize))
                        e = np.empty((len(ents), 3), np.int32)
                        e[:, :2] = ents
                        e[:, 2] = off + 3 * len(ents) + np.concatenate(([0], np.cumsum(ents[:-1, 1])))
                        tabs.append(off)
                        words += [e.reshape(-1), wts.view(np.int32)]
                        off += 3 * len(ents) + len(wts)
                    seen[key] = tabs
                j.xtab, j.ytab = seen[key]
    return jobs, (np.concatenate(words) if words else np.zeros(0, np.int32))


def letterbox_area_batch(ims, sizes, places, H, W, dtype=torch.uint8, normalize=False, pad_value=114):
    """`load_image` + the padding of `letterbox` + HWC -> CHW, BGR -> RGB (+ `/ 255`) for a ragged batch in ONE launch (csrc/val_data.h).
    Arguments as `area_jobs`; -> (B, 3, H, W) `dtype`."""
    dev = ims[0].device
    B = len(ims)
    for im, (nh, nw), (top, left) in zip(ims, sizes, places):
        if nh < 1 or nw < 1 or top < 0 or left < 0 or top + nh > H or left + nw > W:
            raise ValueError(f"letterbox_area_batch: a {nh} x {nw} image at ({top}, {left}) does not fit the {H} x {W} canvas")
    jobs, tabs = area_jobs(ims, sizes, places)
    table = _lib.device_table(jobs, dev)
    tabs_d = torch.from_numpy(tabs).to(dev) if len(tabs) else None
    out = torch.empty((B, 3, H, W), dtype=dtype, device=dev)
    lib = _lib.lib()
    _lib.check(lib.y5_letterbox_area_batch(C.c_void_p(table.data_ptr()), C.c_void_p(tabs_d.data_ptr()) if tabs_d is not None else None, len(tabs),
                                           B, H, W, int(pad_value), C.c_void_p(out.data_ptr()), _lib.dtype_code(dtype),
                                           int(normalize and dtype != torch.uint8), _lib.stream(dev)), lib)
    return out


class ValLoader:
    """Validation loader of a detection dataset over frames resident on the device: `LoadImagesAndLabels(augment=False, rect=rect, pad=pad)` +
    `collate_fn` as val.py:228-237 builds it (rect=True, pad=0.5; `--task speed`: rect=False, pad=0.0).  rect sorts the images by aspect ratio
    h / w with the reference's own `argsort` call and gives every batch the smallest stride-multiple canvas that holds its images
    (:589-612); each batch is ONE `y5_letterbox_area_batch` launch on that (H, W): load_image's resize -- INTER_AREA when the image shrinks,
    INTER_LINEAR when it grows -- and the padding of letterbox(auto=False, scaleup=False), which for these shapes never resizes again
    (asserted).  Yields (imgs, targets, paths, shapes) as `val_loop.run` and `train_loop.train(val_loader=...)` consume them; re-iterable.
    `.shapes` (w, h) and `.labels` are in the sorted order, `.order[k]` is the dataset index of position k, `.batch[k]` its batch,
    `.batch_shapes[b]` the (H, W) of batch b (rect only).  A rect run makes the model build one plan per distinct (B, H, W)."""

    def __init__(self, images, labels, img_size=640, batch_size=32, stride=32, pad=0.5, rect=True, dtype=torch.uint8, paths=None, single_cls=False):
        n = len(images)
        self.images, self.img_size, self.bs, self.stride, self.pad, self.rect, self.dtype = list(images), img_size, batch_size, stride, pad, rect, dtype
        self.paths = list(paths) if paths else [f"image{i}" for i in range(n)]
        self.labels = [np.array(lb, dtype=np.float32).reshape(-1, 5).copy() for lb in labels]
        if single_cls:                                                      # :586-587
            for lb in self.labels:
                lb[:, 0] = 0
        self.shapes = np.array([[int(im.shape[1]), int(im.shape[0])] for im in images])   # wh, as the label cache holds them (:551)
        bi = np.floor(np.arange(n) / batch_size).astype(int)               # :567-569
        nb = bi[-1] + 1
        self.batch, self.order = bi, np.arange(n)
        if rect:                                                            # :589-612
            s = self.shapes
            ar = s[:, 1] / s[:, 0]
            irect = ar.argsort()
            self.order = irect
            self.images, self.paths = [self.images[i] for i in irect], [self.paths[i] for i in irect]
            self.labels = [self.labels[i] for i in irect]
            self.shapes = s[irect]
            ar = ar[irect]
            shapes = [[1, 1]] * nb
            for i in range(nb):
                ari = ar[bi == i]
                mini, maxi = ari.min(), ari.max()
                if maxi < 1:
                    shapes[i] = [maxi, 1]
                elif mini > 1:
                    shapes[i] = [1, 1 / mini]
            self.batch_shapes = np.ceil(np.array(shapes) * img_size / stride + pad).astype(int) * stride

    def __len__(self):
        return (len(self.images) + self.bs - 1) // self.bs

    def _item(self, k):
        """:712-736 for sorted position k, without the pixels -> ((nh, nw), (top, left), labels (k, 5) normalised xywh, shapes entry)."""
        im = self.images[k]
        h0, w0 = int(im.shape[0]), int(im.shape[1])
        h, w = _resized_hw(h0, w0, self.img_size)                           # load_image :784-788
        shape = self.batch_shapes[self.batch[k]] if self.rect else self.img_size
        new_shape = (shape, shape) if isinstance(shape, int) else shape     # letterbox(im, shape, auto=False, scaleup=False), augmentations.py:87-108
        r = min(new_shape[0] / h, new_shape[1] / w)
        r = min(r, 1.0)
        new_unpad = round(w * r), round(h * r)
        dw, dh = new_shape[1] - new_unpad[0], new_shape[0] - new_unpad[1]
        dw /= 2
        dh /= 2
        if (w, h) != new_unpad:
            raise AssertionError(f"ValLoader: image {self.paths[k]} ({h} x {w} after load_image) needs a second resize to fit {tuple(new_shape)}")
        top, left = round(dh - 0.1), round(dw - 0.1)
        lb = self.labels[k].copy()
        if lb.size:
            lb[:, 1:] = _xywhn2xyxy(lb[:, 1:], r * w, r * h, dw, dh)        # :721
        H, W = int(new_shape[0]), int(new_shape[1])
        lb = _finish_labels(lb, {"flipud": False, "fliplr": False}, W, H)   # :736 xyxy2xywhn(clip=True, eps=1e-3) -> (k, 6)
        return (h, w), (top, left), lb, ((h0, w0), ((h / h0, w / w0), (dw, dh))), (H, W)

    def __iter__(self):
        n = len(self.images)
        for b0 in range(0, n, self.bs):
            ks = list(range(b0, min(b0 + self.bs, n)))
            items = [self._item(k) for k in ks]
            H, W = items[0][4]
            imgs = letterbox_area_batch([self.images[k] for k in ks], [it[0] for it in items], [it[1] for it in items], H, W, self.dtype,
                                        normalize=True)
            labs = []
            for i, it in enumerate(items):
                it[2][:, 0] = i                                             # collate_fn :860-862
                labs.append(it[2])
            yield imgs, torch.from_numpy(np.concatenate(labs, 0)), [self.paths[k] for k in ks], [it[3] for it in items]


# ---- classification (utils/dataloaders.py:949-1013, the augment=False branch) -------------------------------------------------------------
class ClassificationLoader:
    """`ClassificationDataset.__getitem__`'s torch_transforms branch plus the default collate, on frames already in memory: yields
    (images (b, 3, imgsz, imgsz) fp32 | fp16, labels (b) int64) on the device, ONE transform launch per batch (augmentations.classify_transform_batch).
    frames: uint8 HWC BGR images of any sizes (device tensors, or host arrays uploaded per batch); the last batch may be short.  Reading image folders,
    the RAM / disk caches and the train-time albumentations branch are not built.  shuffle=True: a fresh torch.randperm per epoch (per __iter__)
    from the loader's own generator seeded with `seed` -- repeatable, but NOT the order of the reference's DataLoader (whose sampler draws from
    torch's global generator through its own base seed)."""

    def __init__(self, frames, labels, imgsz=224, batch_size=64, half=False, device=None, shuffle=False, seed=0):
        if len(frames) != len(labels):
            raise ValueError(f"ClassificationLoader: {len(frames)} frames, {len(labels)} labels")
        self.frames, self.imgsz, self.batch_size, self.half = list(frames), int(imgsz), int(batch_size), half
        if device is None:
            device = next((f.device for f in self.frames if torch.is_tensor(f)), None)
        if device is None:
            raise ValueError("ClassificationLoader: host frames need a device=")
        self.device = torch.device(device)
        self.labels = torch.as_tensor(np.asarray(labels), dtype=torch.int64).to(self.device)
        self.shuffle = bool(shuffle)
        self._gen = torch.Generator().manual_seed(int(seed)) if self.shuffle else None

    def __len__(self):
        return (len(self.frames) + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        from .augmentations import classify_transform_batch

        n = len(self.frames)
        order = torch.randperm(n, generator=self._gen) if self.shuffle else torch.arange(n)
        for b0 in range(0, n, self.batch_size):
            ids = order[b0:b0 + self.batch_size]
            ims = [self.frames[i] for i in ids.tolist()]
            yield classify_transform_batch(ims, self.imgsz, half=self.half, device=self.device), self.labels[ids.to(self.device)]
