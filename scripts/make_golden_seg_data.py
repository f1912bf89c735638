"""Writes tests/golden/seg_data*.npz from the UNMODIFIED reference's segmentation loader, imported read-only through oracle.ref_shim on
torch-CPU: `LoadImagesAndLabelsAndMasks.__getitem__`, `load_mosaic`, `collate_fn` (utils/segment/dataloaders.py), with
utils/segment/augmentations.py's `random_perspective` / `mixup` underneath, on a bare dataset namespace (no files, no cache) over
tests/seg_data_ref.polygon_dataset.  Needs the reference checkout; no test runs this.

    python scripts/make_golden_seg_data.py

The shim stubs cv2 and the ultralytics package, so `cv2.fillPoly` and `ultralytics.data.utils.polygon2mask / polygons2masks /
polygons2masks_overlap` are bound to the restatements of tests/seg_data_ref.py (parity unpinned by necessity); cv2.resize, warpAffine, the
HSV conversion are oracle/thirdparty.py's, as for tests/golden/augment*.npz.  np.argsort(-areas) is unspecified for equal areas, so the
script ASSERTS that no image of any batch holds two instances of equal shrunk area: the reference alone decides every expected value.
Per configuration and seed: img{seed}, lab{seed}, mask{seed} (+ mosaic{seed} gates where the mosaic gate is drawn); the generators are
seeded with seed * 10 + index before every sample, as in oracle/make_golden.py:gen_augment."""
import math
import os
import random
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import augment_oracle as ao, ref_shim, thirdparty as tp  # noqa: E402
from tests import seg_data_ref as sd  # noqa: E402

HYP = dict(ao.HYP_AUG, degrees=5.0, shear=2.0, flipud=0.3)
# The seeds are those of each decade that pass the equal-area assertion (2, 9, 22, 25 do not) and give the most labels.
# name -> (hyp, overlap, mask_ratio, seeds, batch indices as a function of the seed)
TRAIN = {
    "seg_data": (HYP, True, 4, (1, 3, 4), lambda sd_: (sd_ % 6, (sd_ + 3) % 6)),
    "seg_data_mixed": (dict(HYP, mosaic=0.5), False, 2, (11, 13, 16), lambda sd_: (sd_ % 6, (sd_ + 2) % 6, (sd_ + 4) % 6)),
    "seg_data_mixup": (dict(HYP, mixup=0.5), True, 1, (21, 23, 24), lambda sd_: (sd_ % 6, (sd_ + 2) % 6, (sd_ + 4) % 6)),
}
S_TRAIN, S_VAL = 96, 128
VAL = {"seg_data_val": ((True, 1), (False, 4), (True, 4))}   # (overlap, mask_ratio) per batch of all 6 images


def overlap_checked(imgsz, segments, downsample_ratio=1):
    assert sd.areas_distinct(imgsz, segments, downsample_ratio), "two instances of one image have equal area: np.argsort(-areas) is unspecified"
    return sd.polygons2masks_overlap(imgsz, segments, downsample_ratio)


def dataset(cls, dl, s, hyp, augment, overlap, ratio, tiny):
    ims, classes, segments = sd.polygon_dataset(6, seed=3, tiny=tiny)
    from yolov5_amd.dataloaders import labels_from_segments

    labels = [labels_from_segments(c, sg) for c, sg in zip(classes, segments)]
    ds = types.SimpleNamespace(img_size=s, mosaic=augment, augment=augment, hyp=hyp, mosaic_border=[-s // 2, -s // 2], rect=False, n=len(ims),
                               indices=list(range(len(ims))), labels=[lb.copy() for lb in labels], segments=[[x.copy() for x in sg] for sg in segments],
                               im_files=[f"im{i}" for i in range(len(ims))], albumentations=lambda im, lb: (im, lb), overlap=overlap,
                               downsample_ratio=ratio)
    ds.load_mosaic = types.MethodType(cls.load_mosaic, ds)

    def load_image(self, i):  # dataloaders.py:770-790 with cv2.imread replaced by the in-memory image
        im = ims[i]
        h0, w0 = im.shape[:2]
        r = self.img_size / max(h0, w0)
        if r != 1:
            assert self.augment or r > 1, "INTER_AREA (validation down-scale) is not restated"
            im = dl.cv2.resize(im, (math.ceil(w0 * r), math.ceil(h0 * r)), interpolation=dl.cv2.INTER_LINEAR)
        return im, (h0, w0), im.shape[:2]

    ds.load_image = types.MethodType(load_image, ds)
    return ds


def main():
    ref_shim.load()
    cwd = os.getcwd()
    os.chdir(ref_shim.REFERENCE_ROOT)
    try:
        import utils.dataloaders as dl
        import utils.segment.dataloaders as sdl
    finally:
        os.chdir(cwd)
    sys.modules["cv2"].fillPoly = sd.fill_poly
    uu = sys.modules["ultralytics.data.utils"]
    uu.polygon2mask, uu.polygons2masks, uu.polygons2masks_overlap = sd.polygon2mask, sd.polygons2masks, overlap_checked
    sdl.polygons2masks, sdl.polygons2masks_overlap = sd.polygons2masks, overlap_checked
    sdl.xywhn2xyxy, sdl.xyxy2xywhn = tp.xywhn2xyxy, tp.xyxy2xywhn
    cls = sdl.LoadImagesAndLabelsAndMasks
    gold = os.path.join(ROOT, "tests", "golden")
    for name, (hyp, overlap, ratio, seeds, idx) in TRAIN.items():
        ds = dataset(cls, dl, S_TRAIN, hyp, True, overlap, ratio, tiny=False)
        out = {"s": np.array(S_TRAIN), "overlap": np.array(overlap), "ratio": np.array(ratio)}
        for seed in seeds:
            batch, gates = [], []
            for index in idx(seed):
                random.seed(seed * 10 + index)
                gates.append(random.random() < hyp["mosaic"])
                random.seed(seed * 10 + index)
                np.random.seed(seed * 10 + index)
                batch.append(cls.__getitem__(ds, index))
            im, lab, _, _, masks = cls.collate_fn(batch)
            out[f"img{seed}"], out[f"lab{seed}"], out[f"mask{seed}"], out[f"mosaic{seed}"] = im.numpy(), lab.numpy(), masks.numpy(), np.array(gates)
            print(name, seed, gates, tuple(im.shape), tuple(lab.shape), tuple(masks.shape), masks.dtype, int(masks.max()))
        path = os.path.join(gold, name + ".npz")
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path))
    for name, cfgs in VAL.items():
        out = {"s": np.array(S_VAL)}
        for k, (overlap, ratio) in enumerate(cfgs):
            ds = dataset(cls, dl, S_VAL, ao.HYP_AUG, False, overlap, ratio, tiny=True)
            batch = [cls.__getitem__(ds, i) for i in range(6)]
            shapes = [b[3] for b in batch]
            im, lab, _, _, masks = cls.collate_fn(batch)
            assert k == 0 or np.array_equal(out["img"], im.numpy())   # the image half does not depend on (overlap, mask_ratio): stored once
            out["img"], out[f"lab{k}"], out[f"mask{k}"] = im.numpy(), lab.numpy(), masks.numpy()
            out[f"cfg{k}"] = np.array([int(overlap), ratio])
            out[f"shapes{k}"] = np.array([[h0, w0, rh, rw, dw, dh] for (h0, w0), ((rh, rw), (dw, dh)) in shapes], np.float64)
            print(name, k, overlap, ratio, tuple(im.shape), tuple(lab.shape), tuple(masks.shape), masks.dtype)
        path = os.path.join(gold, name + ".npz")
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path))
    _ = torch


if __name__ == "__main__":
    main()
