"""Segmentation post-processing with the reference's names (utils/segment/general.py): `process_mask` :25-51 and
`crop_mask` :10-22 run as one HIP kernel per image (y5_process_mask); `process_mask_batch` does the per-image loop of segment/predict.py:161-172
for a whole batch in ONE launch (y5_process_mask_batch); `process_mask_native` :54-76 (predict.py's `retina_masks` branch: masks in the pixels of
the original image) and its batch form, every image with its own size, are one launch too (y5_process_mask_native_batch)."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib


def process_mask(protos, masks_in, bboxes, shape, upsample=False, out_dtype=torch.float32):
    """protos (c, mh, mw) GPU f16|f32; masks_in (n, c); bboxes (n, 4) xyxy in input pixels; shape (ih, iw).
    Returns (n, ih, iw) if upsample else (n, mh, mw), values 0/1.  `out_dtype`: torch.float32 (what the reference's
    `masks.gt_(0.5)` returns) or torch.bool / torch.uint8 (4x fewer HBM bytes).  masks_in / bboxes may be column
    views of the NMS output rows (`det[:, 6:]`, `det[:, :4]`): they are read in place through their row stride."""
    if not _lib.accepts(protos):
        raise RuntimeError("yolov5_amd.process_mask needs GPU tensors (no CPU path)")
    lib = _lib.lib()
    c, mh, mw = protos.shape
    ih, iw = int(shape[0]), int(shape[1])
    n = int(masks_in.shape[0])
    if protos.dtype not in (torch.float16, torch.float32):
        protos = protos.float()
    protos = protos.contiguous()

    def rows(t, width):
        if t.dtype != torch.float32 or t.stride(-1) != 1 or (t.shape[0] > 1 and t.stride(0) < width):
            t = t.float().contiguous()
        return t, (t.stride(0) if t.shape[0] > 1 else width)

    masks_in, ld_m = rows(masks_in, c)
    bboxes, ld_b = rows(bboxes, 4)
    oh, ow = (ih, iw) if upsample else (mh, mw)
    u8 = out_dtype in (torch.bool, torch.uint8)
    if not u8 and out_dtype != torch.float32:
        raise TypeError("process_mask: out_dtype must be float32, uint8 or bool")
    out = torch.empty((n, oh, ow), dtype=torch.uint8 if u8 else torch.float32, device=protos.device)
    rc = lib.y5_process_mask(C.c_void_p(protos.data_ptr()), _lib.Y5_F16 if protos.dtype == torch.float16 else _lib.Y5_F32,
                             c, mh, mw, C.c_void_p(masks_in.data_ptr()), ld_m, C.c_void_p(bboxes.data_ptr()), ld_b, n, ih, iw,
                             1 if upsample else 0, C.c_void_p(out.data_ptr()), _lib.Y5_U8 if u8 else _lib.Y5_F32,
                             _lib.stream(protos.device))
    _lib.check(rc, lib)
    return out.view(torch.bool) if out_dtype == torch.bool else out


def _rows(t, width):
    if t.dtype != torch.float32 or t.stride(-1) != 1 or (t.shape[0] > 1 and t.stride(0) < width):
        t = t.float().contiguous()
    return t, (t.stride(0) if t.shape[0] > 1 else width)


def process_mask_batch(protos, dets, shape, upsample=False, out_dtype=torch.float32):
    """`[process_mask(protos[i], det[:, 6:], det[:, :4], shape, upsample) for i, det in enumerate(dets)]` (segment/predict.py:161-172) as ONE launch.
    protos (B, c, mh, mw) GPU f16|f32; dets: the per-image NMS results, (n_i, 6 + c) fp32 rows [x1, y1, x2, y2, conf, cls, coefficients] -- read in place
    (they are views of the padded NMS buffer).  Returns the list of per-image masks (n_i, oh, ow) -- views of one buffer -- with values 0/1 in `out_dtype`
    (torch.float32: the reference's `masks.gt_(0.5)`; torch.bool / torch.uint8: 4x fewer HBM bytes).  Shapes the batched kernel does not take (output width not
    a multiple of 16 bytes) fall back to the per-image kernel."""
    if not _lib.accepts(protos):
        raise RuntimeError("yolov5_amd.process_mask_batch needs GPU tensors (no CPU path)")
    lib = _lib.lib()
    B, c, mh, mw = protos.shape
    if len(dets) != B:
        raise ValueError(f"process_mask_batch: {len(dets)} detection tensors for {B} prototype sets")
    ih, iw = int(shape[0]), int(shape[1])
    oh, ow = (ih, iw) if upsample else (mh, mw)
    u8 = out_dtype in (torch.bool, torch.uint8)
    if not u8 and out_dtype != torch.float32:
        raise TypeError("process_mask_batch: out_dtype must be float32, uint8 or bool")
    if protos.dtype not in (torch.float16, torch.float32):
        protos = protos.float()
    protos = protos.contiguous()
    if ow % (16 if u8 else 4):
        return [process_mask(protos[i], d[:, 6:], d[:, :4], shape, upsample, out_dtype) for i, d in enumerate(dets)]
    imgs = (_lib.MaskImg * B)()
    keep = []   # tensors the descriptors point into
    ns = []
    for i, d in enumerate(dets):
        n = int(d.shape[0])
        ns.append(n)
        if n == 0:
            imgs[i].n = 0
            continue
        if d.shape[1] != 6 + c:
            raise ValueError(f"process_mask_batch: detection rows have {d.shape[1]} columns, expected 6 + {c}")
        d, ld = _rows(d, 6 + c)
        keep.append(d)
        imgs[i].masks_in, imgs[i].boxes, imgs[i].ld_m, imgs[i].ld_b, imgs[i].n = d.data_ptr() + 24, d.data_ptr(), ld, ld, n
    total = sum(ns)
    out = torch.empty((total, oh, ow), dtype=torch.uint8 if u8 else torch.float32, device=protos.device)
    if total:
        rc = lib.y5_process_mask_batch(C.c_void_p(protos.data_ptr()), _lib.Y5_F16 if protos.dtype == torch.float16 else _lib.Y5_F32, B, c, mh, mw, imgs,
                                       ih, iw, 1 if upsample else 0, C.c_void_p(out.data_ptr()), _lib.Y5_U8 if u8 else _lib.Y5_F32, _lib.stream(protos.device))
        _lib.check(rc, lib)
    if out_dtype == torch.bool:
        out = out.view(torch.bool)
    return list(out.split(ns))


def native_window(mh, mw, shape):
    """The rows [top, bottom) and columns [left, right) of the (mh, mw) prototype plane that process_mask_native resizes to `shape`
    (utils/segment/general.py:68-71, Python double arithmetic; int(pad) and int(size - pad) truncate differently, so the window can be
    one row or column short of the unpadded area)."""
    h0, w0 = int(shape[0]), int(shape[1])
    if h0 < 1 or w0 < 1:
        raise ValueError(f"process_mask_native: bad image shape {tuple(shape)}")
    gain = min(mh / h0, mw / w0)  # gain  = old / new
    pad = (mw - w0 * gain) / 2, (mh - h0 * gain) / 2  # wh padding
    top, left = int(pad[1]), int(pad[0])  # y, x
    bottom, right = int(mh - pad[1]), int(mw - pad[0])
    if bottom <= top or right <= left:
        raise ValueError(f"process_mask_native: image shape {(h0, w0)} leaves an empty window of the {(mh, mw)} prototypes")
    return top, left, bottom, right


def _native(protos, items, shapes, out_dtype, who):
    """items[i] = (coefficients (n, c), boxes (n, 4)) of image i, both read in place through their row stride."""
    if not _lib.accepts(protos):
        raise RuntimeError(f"yolov5_amd.{who} needs GPU tensors (no CPU path)")
    lib = _lib.lib()
    B, c, mh, mw = protos.shape
    if len(items) != B or len(shapes) != B:
        raise ValueError(f"{who}: {len(items)} detection tensors and {len(shapes)} shapes for {B} prototype sets")
    u8 = out_dtype in (torch.bool, torch.uint8)
    if not u8 and out_dtype != torch.float32:
        raise TypeError(f"{who}: out_dtype must be float32, uint8 or bool")
    if protos.dtype not in (torch.float16, torch.float32):
        protos = protos.float()
    protos = protos.contiguous()
    vec = 16 if u8 else 4   # elements per 16 bytes: every image's block starts on such a boundary
    imgs = (_lib.MaskNativeImg * B)()
    keep, spans = [], []
    total = 0
    for i, ((coef, boxes), shape) in enumerate(zip(items, shapes)):
        h0, w0 = int(shape[0]), int(shape[1])
        top, left, bottom, right = native_window(mh, mw, (h0, w0))
        n = int(coef.shape[0])
        if n and (coef.shape[1] != c or boxes.shape[0] != n or boxes.shape[1] != 4):
            raise ValueError(f"{who}: image {i} has coefficients {tuple(coef.shape)} and boxes {tuple(boxes.shape)}, expected ({n}, {c}) and ({n}, 4)")
        spans.append((total, n, h0, w0))
        im = imgs[i]
        im.n, im.h0, im.w0, im.top, im.left, im.ch, im.cw, im.out_off = n, h0, w0, top, left, bottom - top, right - left, total
        if n:
            if not _lib.accepts(coef) or not _lib.accepts(boxes):
                raise RuntimeError(f"yolov5_amd.{who} needs GPU tensors (no CPU path)")
            coef, im.ld_m = _rows(coef, c)
            boxes, im.ld_b = _rows(boxes, 4)
            keep += [coef, boxes]
            im.masks_in, im.boxes = coef.data_ptr(), boxes.data_ptr()
        total += -(-n * h0 * w0 // vec) * vec
    out = torch.empty((total,), dtype=torch.uint8 if u8 else torch.float32, device=protos.device)
    if any(sp[1] for sp in spans):
        rc = lib.y5_process_mask_native_batch(C.c_void_p(protos.data_ptr()), _lib.Y5_F16 if protos.dtype == torch.float16 else _lib.Y5_F32, B, c, mh, mw,
                                              imgs, C.c_void_p(out.data_ptr()), total, _lib.Y5_U8 if u8 else _lib.Y5_F32, _lib.stream(protos.device))
        _lib.check(rc, lib)
    if out_dtype == torch.bool:
        out = out.view(torch.bool)
    return [out[off:off + n * h0 * w0].view(n, h0, w0) for off, n, h0, w0 in spans]


def process_mask_native(protos, masks_in, bboxes, shape, out_dtype=torch.float32):
    """utils/segment/general.py:54-76: protos (c, mh, mw) GPU f16|f32; masks_in (n, c); bboxes (n, 4) xyxy in the pixels of the ORIGINAL image
    (after scale_boxes and .round(), segment/predict.py:169); shape (h0, w0) of that image.  The letterbox padding is cut out of the
    prototype-resolution masks, the rest is resized to (h0, w0) -- up or down -- cropped to the boxes there and thresholded: (n, h0, w0), values
    0/1 in `out_dtype` (float32 as the reference's `gt_(0.5)`, or uint8 / bool).  masks_in / bboxes may be column views of the NMS rows."""
    if protos.dim() != 3:
        raise ValueError("process_mask_native: protos must be (c, mh, mw)")
    return _native(protos[None], [(masks_in, bboxes)], [shape], out_dtype, "process_mask_native")[0]


def process_mask_native_batch(protos, dets, shapes, out_dtype=torch.float32):
    """`[process_mask_native(protos[i], det[:, 6:], det[:, :4], shapes[i]) for i, det in enumerate(dets)]` (segment/predict.py:161-170 with
    retina_masks) as ONE launch.  protos (B, c, mh, mw) GPU f16|f32; dets: the per-image NMS results, (n_i, 6 + c) fp32 rows whose boxes are
    already in original pixels, read in place; shapes[i] = (h0, w0).  Returns the per-image masks (n_i, h0_i, w0_i): views of one allocation,
    every image's block starting on a 16-byte boundary."""
    c = protos.shape[1]
    for d in dets:
        if d.shape[0] and d.shape[1] != 6 + c:
            raise ValueError(f"process_mask_native_batch: detection rows have {d.shape[1]} columns, expected 6 + {c}")
    return _native(protos, [(d[:, 6:], d[:, :4]) for d in dets], shapes, out_dtype, "process_mask_native_batch")
