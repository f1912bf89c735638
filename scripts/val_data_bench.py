"""Detection validation data path timing on one GPU, both arms in ONE process; device events, a warm-up, windows of at least 0.5 s.

    python scripts/val_data_bench.py [--out profiles/val_data/val_data_bench.json]

  (a) loader image path: 32 frames alternating 1920 x 1080 and 1280 x 960 sent to the img_size = 640 rect canvas of such a batch (fp16 / 255
      output).  area_us: the y5_letterbox_area_batch launch (INTER_AREA, csrc/val_data.h); linear_us: y5_letterbox_batch (INTER_LINEAR) on the
      same jobs, the two alternated window by window; torch_us: F.interpolate(mode="area") per frame + pad + permute.  bytes: source bytes
      + output bytes of the launch; hbm_share: bytes / time over the 8 TB/s HBM peak.  Those frames shrink by exactly 3 and 2; the same arm
      is repeated on 1600 x 900 / 1600 x 1200 frames (2.5x: the tap-table path) as loader_images_2p5x.
  (b) confusion matrix: ConfusionMatrix.update on 128 images x 300 detections x 8-20 labels, nc = 80 (update_us: the y5_val_confusion
      launch, inputs resident) against the per-image torch / numpy restatement of the reference's loop on the same tensors (loop_ms, host wall
      time including its .cpu() copies, as val.py:293,309 pays it)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from yolov5_amd import _lib, dataloaders as D, metrics  # noqa: E402


def window(fn, min_s=0.5):
    """Median device time per call (us) over windows of >= min_s: events around runs of calls."""
    fn()
    torch.cuda.synchronize()
    n, per = 8, []
    t_end = time.perf_counter() + min_s
    while time.perf_counter() < t_end or len(per) < 5:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        per.append(e0.elapsed_time(e1) / n * 1e3)
    return float(np.median(per)), float(min(per)), float(max(per))


def arm_a(dev, hw=((1080, 1920), (960, 1280))):
    rng = np.random.default_rng(0)
    frames = [torch.from_numpy(rng.integers(0, 256, (*hw[i % 2], 3), dtype=np.uint8)).to(dev) for i in range(32)]
    labels = [np.zeros((0, 5), np.float32)] * 32
    loader = D.ValLoader(frames, labels, img_size=640, batch_size=32, dtype=torch.float16)
    items = [loader._item(k) for k in range(32)]
    H, W = items[0][4]
    ims = loader.images
    sizes, places = [it[0] for it in items], [it[1] for it in items]
    jobs, tabs = D.area_jobs(ims, sizes, places)
    table = torch.frombuffer(bytearray(jobs), dtype=torch.uint8).to(dev)
    tabs_d = torch.from_numpy(tabs).to(dev)
    out = torch.empty((32, 3, H, W), dtype=torch.float16, device=dev)
    lj = (_lib.LetterboxJob * 32)()
    for j, im, (nh, nw), (top, left) in zip(lj, ims, sizes, places):
        j.src, j.h0, j.w0, j.stride, j.nw, j.nh, j.top, j.left = im.data_ptr(), im.shape[0], im.shape[1], im.stride(0), nw, nh, top, left
    ltable = torch.frombuffer(bytearray(lj), dtype=torch.uint8).to(dev)
    out2 = torch.empty_like(out)
    lib, st = _lib.lib(), _lib.stream(dev)

    def area():
        _lib.check(lib.y5_letterbox_area_batch(C.c_void_p(table.data_ptr()), C.c_void_p(tabs_d.data_ptr()), len(tabs), 32, H, W, 114,
                                               C.c_void_p(out.data_ptr()), _lib.Y5_F16, 1, st), lib)

    def linear():
        _lib.check(lib.y5_letterbox_batch(C.c_void_p(ltable.data_ptr()), 32, H, W, 114, 1, C.c_void_p(out2.data_ptr()), _lib.Y5_F16, 1, 1, st), lib)

    def torch_path():
        o = torch.full((32, 3, H, W), 114 / 255, dtype=torch.float16, device=dev)
        for b, (im, (nh, nw), (top, left)) in enumerate(zip(ims, sizes, places)):
            x = im.permute(2, 0, 1)[None].float()
            o[b, :, top:top + nh, left:left + nw] = (F.interpolate(x, size=(nh, nw), mode="area")[0].flip(0) / 255).half()
        return o

    ra, rl = [], []
    for _ in range(3):                                           # alternated in the same process
        ra.append(window(area))
        rl.append(window(linear))
    rt = window(torch_path)
    src_bytes = sum(int(im.shape[0]) * int(im.shape[1]) * 3 for im in ims)
    out_bytes = out.numel() * 2
    a_us, l_us = float(np.median([r[0] for r in ra])), float(np.median([r[0] for r in rl]))
    return dict(canvas=[H, W], modes=sorted({int(j.mode) for j in jobs}), src_bytes=src_bytes, out_bytes=out_bytes,
                area_us=a_us, area_us_windows=[r[0] for r in ra], linear_us=l_us, linear_us_windows=[r[0] for r in rl], torch_us=rt[0],
                area_hbm_share=(src_bytes + out_bytes) / (a_us * 1e-6) / 8e12, linear_hbm_share_of_same_bytes=(src_bytes + out_bytes) / (l_us * 1e-6) / 8e12,
                area_ns_per_output_byte=a_us * 1e3 / out_bytes, linear_ns_per_output_byte=l_us * 1e3 / out_bytes)


def reference_loop(out, counts, targets, nc, conf=0.25, iou_thres=0.45):
    """The per-image loop of val.py:289-309 + utils/metrics.py:149-183 restated in torch / numpy on the same tensors (boxes compared as given)."""
    m = np.zeros((nc + 1, nc + 1))
    for si in range(out.shape[0]):
        lab = targets[targets[:, 0] == si, 1:]
        n = int(counts[si])
        if n == 0:
            for gc in lab[:, 0].int():
                m[nc, gc] += 1
            continue
        if not len(lab):
            continue
        det = out[si, :n]
        det = det[det[:, 4] > conf]
        half = lab[:, 3:5] / 2
        box = torch.cat((lab[:, 1:3] - half, lab[:, 1:3] + half), 1)
        gt, dc = lab[:, 0].int(), det[:, 5].int()
        a1, a2 = box[:, None, :2], box[:, None, 2:]
        b1, b2 = det[None, :, :2], det[None, :, 2:4]
        inter = (torch.min(a2, b2) - torch.max(a1, b1)).clamp_(0).prod(2)
        iou = inter / ((a2 - a1).prod(2) + (b2 - b1).prod(2) - inter + 1e-7)
        x = torch.where(iou > iou_thres)
        if x[0].shape[0]:
            mt = torch.cat((torch.stack(x, 1), iou[x[0], x[1]][:, None]), 1).cpu().numpy()
            if x[0].shape[0] > 1:
                mt = mt[mt[:, 2].argsort()[::-1]]
                mt = mt[np.unique(mt[:, 1], return_index=True)[1]]
                mt = mt[mt[:, 2].argsort()[::-1]]
                mt = mt[np.unique(mt[:, 0], return_index=True)[1]]
        else:
            mt = np.zeros((0, 3))
        nn = mt.shape[0] > 0
        m0, m1, _ = mt.transpose().astype(int)
        for i, gc in enumerate(gt):
            j = m0 == i
            if nn and sum(j) == 1:
                m[dc[m1[j]], gc] += 1
            else:
                m[nc, gc] += 1
        if nn:
            for i, c in enumerate(dc):
                if not any(m1 == i):
                    m[c, nc] += 1
    return m


def arm_b(dev):
    rng = np.random.default_rng(1)
    bs, max_det, nc = 128, 300, 80
    out = np.zeros((bs, max_det, 6), np.float32)
    tg = []
    for si in range(bs):
        nl = int(rng.integers(8, 21))
        xy = rng.uniform(0, 560, (nl, 2))
        wh = rng.uniform(20, 80, (nl, 2))
        cls = rng.integers(0, nc, nl)
        src = rng.integers(0, nl, max_det)
        box = np.concatenate((xy, xy + wh), 1)[src] + rng.normal(0, 6, (max_det, 4))
        box[:, 2:] = np.maximum(box[:, 2:], box[:, :2] + 2)
        out[si] = np.concatenate((box, rng.uniform(0, 1, (max_det, 1)), np.where(rng.random(max_det) < 0.8, cls[src], rng.integers(0, nc, max_det))[:, None]), 1)
        tg.append(np.concatenate((np.full((nl, 1), si), cls[:, None], xy + wh / 2, wh), 1))
    out_t = torch.from_numpy(out).to(dev)
    cnt = torch.full((bs,), max_det, dtype=torch.int32, device=dev)
    tg_t = torch.from_numpy(np.concatenate(tg, 0).astype(np.float32)).to(dev)
    cm = metrics.ConfusionMatrix(nc)
    cm.update(out_t, cnt, tg_t, None)
    t0 = time.perf_counter()
    ref = reference_loop(out_t, cnt, tg_t, nc)
    torch.cuda.synchronize()
    loop_ms = (time.perf_counter() - t0) * 1e3
    same = bool(np.array_equal(cm.matrix, ref))                 # random floats: ties have probability ~0, so the tie rule does not show
    us = window(lambda: cm.update(out_t, cnt, tg_t, None))
    return dict(bs=bs, max_det=max_det, labels=int(tg_t.shape[0]), nc=nc, update_us=us[0], update_us_min=us[1], update_us_max=us[2], loop_ms=loop_ms,
                equals_loop=same)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    # the frames of arm (a) shrink by exactly 3 and 2 (integer-block and 2x2 paths); 1600 x 900 / 1600 x 1200 shrink by 2.5 (tap tables)
    res = dict(device=torch.cuda.get_device_name(0), loader_images=arm_a(dev), loader_images_2p5x=arm_a(dev, ((900, 1600), (1200, 1600))),
               confusion=arm_b(dev))
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
