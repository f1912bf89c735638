"""Writes tests/golden/copy_paste_seg.npz and tests/golden/copy_paste_det.npz from the UNMODIFIED reference's loaders, imported read-only
through oracle.ref_shim on torch-CPU, with hyp['copy_paste'] > 0: `LoadImagesAndLabelsAndMasks.__getitem__` (utils/segment/dataloaders.py) and
`LoadImagesAndLabels.__getitem__` (utils/dataloaders.py) with their `load_mosaic` -> `copy_paste` (utils/augmentations.py:200-222) ->
`random_perspective` and `collate_fn`, on bare dataset namespaces over tests/seg_data_ref.polygon_dataset, as scripts/make_golden_seg_data.py.
Needs the reference checkout; no test runs this.

    python scripts/make_golden_copy_paste.py

On top of that script's bindings, `utils.augmentations.bbox_ioa` (the shim sets it to None), `cv2.drawContours`, `cv2.FILLED` and `cv2.flip`
are bound to the restatements of tests/copy_paste_ref.py (parity unpinned by necessity).  The script ASSERTS that the reference alone decides
every expected value and that the fixtures exercise the feature: every configuration holds an accepted and a rejected paste, a pasted polygon
touches the canvas edge (a coordinate clipped to 0 or 2 s), and in overlap mode no image holds two instances of equal shrunk area (a pasted
instance mirrors its original, so equal areas are likelier than in seg_data*.npz; np.argsort(-areas) is unspecified for them).
Per configuration `c` and seed: {c}_img{seed}, {c}_lab{seed}, {c}_mosaic{seed} (the mosaic gates) and, for the segmentation loader,
{c}_mask{seed}; the generators are seeded with seed * 10 + index before every sample."""
import os
import random
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import make_golden_seg_data as mg  # noqa: E402
from oracle import ref_shim, thirdparty as tp  # noqa: E402
from tests import copy_paste_ref as cp, seg_data_ref as sd  # noqa: E402

S = mg.S_TRAIN
IDX3 = lambda sd_: (sd_ % 6, (sd_ + 2) % 6, (sd_ + 4) % 6)  # noqa: E731
# name -> (hyp, overlap, mask_ratio, seeds, batch indices as a function of the seed).  The seeds pass the equal-area assertion on the
# segmentation loader (4-7, 23, 26, 27, 29 do not) and hold accepted AND rejected pastes on both loaders; 11 and 13 together put a pasting
# mosaic next to letterboxed samples in either order; 24 blends partner mosaics that paste on their own.  Few seeds: the files stay small
CONFIGS = {
    "mosaic": (dict(mg.HYP, copy_paste=0.5), True, 4, (1,), lambda sd_: (sd_ % 6, (sd_ + 3) % 6)),
    "mixed": (dict(mg.HYP, mosaic=0.5, copy_paste=1.0), False, 1, (11, 13), IDX3),
    "mixup": (dict(mg.HYP, mixup=0.5, copy_paste=0.5), True, 1, (24,), IDX3),
}
STATS = {"accepted": 0, "rejected": 0, "edge": 0}


def bbox_ioa(box1, box2, iou=False, eps=1e-7):
    ioa = cp.bbox_ioa(box1, box2, iou, eps)
    STATS["accepted" if (ioa < 0.30).all() else "rejected"] += 1
    return ioa


def draw_contours(img, contours, idx, color, thickness):
    STATS["edge"] += int(any((np.asarray(c) == 0).any() or (np.asarray(c) == img.shape[1]).any() for c in contours))
    return cp.draw_contours(img, contours, idx, color, thickness)


def bind():
    """The reference's two loader classes with the third-party names bound (see the module docstring)."""
    ref_shim.load()
    cwd = os.getcwd()
    os.chdir(ref_shim.REFERENCE_ROOT)
    try:
        import utils.augmentations as aug
        import utils.dataloaders as dl
        import utils.segment.dataloaders as sdl
    finally:
        os.chdir(cwd)
    cv2 = sys.modules["cv2"]
    cv2.fillPoly, cv2.drawContours, cv2.FILLED, cv2.flip = sd.fill_poly, draw_contours, cp.FILLED, cp.flip
    aug.bbox_ioa = bbox_ioa
    uu = sys.modules["ultralytics.data.utils"]
    uu.polygon2mask, uu.polygons2masks, uu.polygons2masks_overlap = sd.polygon2mask, sd.polygons2masks, mg.overlap_checked
    sdl.polygons2masks, sdl.polygons2masks_overlap = sd.polygons2masks, mg.overlap_checked
    sdl.xywhn2xyxy, sdl.xyxy2xywhn = tp.xywhn2xyxy, tp.xyxy2xywhn
    dl.xywhn2xyxy, dl.xyxy2xywhn = tp.xywhn2xyxy, tp.xyxy2xywhn
    return dl, sdl


def run(cls, dl, seg, name, seeds=None):
    """One configuration on one loader class -> (arrays, the STATS it added)."""
    hyp, overlap, ratio, cfg_seeds, idx = CONFIGS[name]
    ds = mg.dataset(cls, dl, S, hyp, True, overlap, ratio, tiny=False)
    if not seg:   # the detection dataset namespace reads two attributes more (utils/dataloaders.py:770-779); load_image is the in-memory one
        ds.ims, ds.npy_files = [None] * ds.n, [types.SimpleNamespace(exists=lambda: False)] * ds.n
    before, out = dict(STATS), {}
    for seed in seeds or cfg_seeds:
        batch, gates = [], []
        for index in idx(seed):
            random.seed(seed * 10 + index)
            gates.append(random.random() < hyp["mosaic"])
            random.seed(seed * 10 + index)
            np.random.seed(seed * 10 + index)
            batch.append(cls.__getitem__(ds, index))
        res = cls.collate_fn(batch)
        out[f"{name}_img{seed}"], out[f"{name}_lab{seed}"], out[f"{name}_mosaic{seed}"] = res[0].numpy(), res[1].numpy(), np.array(gates)
        if seg:
            out[f"{name}_mask{seed}"] = res[4].numpy()
    return out, {k: STATS[k] - before[k] for k in STATS}


def main():
    dl, sdl = bind()
    gold = os.path.join(ROOT, "tests", "golden")
    for fname, cls, seg in (("copy_paste_seg", sdl.LoadImagesAndLabelsAndMasks, True), ("copy_paste_det", dl.LoadImagesAndLabels, False)):
        out, edge = {"s": np.array(S)}, 0
        for name, (hyp, overlap, ratio, seeds, _) in CONFIGS.items():
            arrays, st = run(cls, dl, seg, name)
            assert st["accepted"] and st["rejected"], f"{fname} {name}: {st}: the configuration needs an accepted and a rejected paste"
            edge += st["edge"]
            out.update(arrays)
            out[f"{name}_cfg"] = np.array([int(overlap), ratio])
            print(fname, name, st, {k: v.shape for k, v in arrays.items() if "lab" in k})
        assert edge, f"{fname}: no pasted polygon touches the canvas edge"
        path = os.path.join(gold, fname + ".npz")
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
