"""Writes tests/golden/val_data.npz from the UNMODIFIED reference, imported read-only through oracle.ref_shim on torch-CPU.  Needs the
reference checkout; no test runs this.

    python scripts/make_golden_val_data.py

(i) The detection validation loader, `LoadImagesAndLabels(augment=False, rect=True, pad=0.5)` of utils/dataloaders.py over
tests/val_data_ref.val_dataset (9 seeded images, img_size 64, stride 32, batch 4).  `__init__` reads files and the label cache, so it cannot be
called; what RAN, on a bare namespace that holds the dataset's attributes:
  * :565-612 of `__init__` -- "Create indices", "Update labels" and "Rectangular Training" -- taken from the reference's own source text at run
    time (inspect.getsource, the lines between the `# Create indices` and `# Cache images` comments) and executed unchanged: the sort order,
    `shapes`, `batch` and `batch_shapes` are the reference's;
  * `__getitem__` (:696-766, the augment = False letterbox branch), the real `load_image` (:768-790) with cv2.imread returning the in-memory
    image, `letterbox` (utils/augmentations.py:85-115) and `collate_fn` (:855-862).
Not run: the file / cache half of `__init__` (:470-563), the RAM / disk image caches (:614-640).
The shim stubs cv2 and the ultralytics package: cv2.resize is bound to tests/val_data_ref.cv2_resize -- INTER_LINEAR is oracle/thirdparty.py's
restatement as for every other golden, INTER_AREA (which the shim's cv2.resize refuses) the helper's restatement, parity unpinned by
necessity --, xywhn2xyxy / xyxy2xywhn to oracle/thirdparty.py's.
(ii) `ConfusionMatrix` of utils/metrics.py:129-183 (box_iou: oracle/thirdparty.py) on tests/val_data_ref.CM_CASES: cm_{name} per case on a fresh
matrix of the case's nc, and cm_all_{nc}: one matrix per nc that accumulated all cases of that nc in CM_CASES order.
The file holds data only."""
import inspect
import os
import sys
import textwrap
import types
from pathlib import Path

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim, thirdparty as tp  # noqa: E402
from tests import val_data_ref as vd  # noqa: E402


def loader_golden(dl, out):
    ims, labels = vd.val_dataset()
    n = len(ims)
    cls = dl.LoadImagesAndLabels
    names = [f"im{i}" for i in range(n)]
    by_name = dict(zip(names, ims))
    dl.cv2.imread = lambda f: by_name[f]
    dl.cv2.resize = vd.cv2_resize
    dl.xywhn2xyxy, dl.xyxy2xywhn = tp.xywhn2xyxy, tp.xyxy2xywhn
    ds = types.SimpleNamespace(img_size=vd.IMG_SIZE, augment=False, hyp=None, mosaic=False, rect=True, stride=vd.STRIDE,
                               im_files=list(names), label_files=list(names), labels=[lb.copy() for lb in labels], segments=[[] for _ in ims],
                               shapes=np.array([(im.shape[1], im.shape[0]) for im in ims]))
    src = inspect.getsource(cls.__init__).splitlines()
    a = next(i for i, ln in enumerate(src) if "# Create indices" in ln)
    b = next(i for i, ln in enumerate(src) if "# Cache images" in ln)
    env = dict(self=ds, np=np, batch_size=vd.BATCH, rank=-1, seed=0, single_cls=False, img_size=vd.IMG_SIZE, stride=vd.STRIDE, pad=vd.PAD,
               WORLD_SIZE=1, RANK=-1)
    exec(textwrap.dedent("\n".join(src[a:b])), env)                     # :565-612, the reference's own text
    ds.ims, ds.npy_files = [None] * n, [Path("/nonexistent") / f"{f}.npy" for f in ds.im_files]
    ds.load_image = types.MethodType(cls.load_image, ds)
    out["order"] = np.array([names.index(f) for f in ds.im_files])
    out["shapes"], out["batch"], out["batch_shapes"] = ds.shapes, ds.batch, ds.batch_shapes
    for k, lb in enumerate(ds.labels):
        out[f"labels{k}"] = lb
    for bno, b0 in enumerate(range(0, n, vd.BATCH)):
        batch = [cls.__getitem__(ds, i) for i in range(b0, min(b0 + vd.BATCH, n))]
        im, lab, paths, shapes = cls.collate_fn(batch)
        out[f"img{bno}"], out[f"lab{bno}"] = im.numpy(), lab.numpy()
        out[f"paths{bno}"] = np.array([names.index(p) for p in paths])
        out[f"shp{bno}"] = np.array([[h0, w0, rh, rw, dw, dh] for (h0, w0), ((rh, rw), (dw, dh)) in shapes], np.float64)
        print("batch", bno, tuple(im.shape), tuple(lab.shape), list(paths))
    print("order", out["order"], "batch_shapes", out["batch_shapes"].tolist())


def confusion_golden(metrics, out):
    acc = {}
    for name in vd.CM_CASES:
        nc, det, lab = vd.cm_case(name)
        one = metrics.ConfusionMatrix(nc, vd.CONF, vd.IOU_THRES)
        for cm in (one, acc.setdefault(nc, metrics.ConfusionMatrix(nc, vd.CONF, vd.IOU_THRES))):
            cm.process_batch(None if det is None else torch.from_numpy(det), torch.from_numpy(lab))
        out[f"cm_{name}"] = one.matrix.astype(np.int64)
        print(name, nc, None if det is None else len(det), len(lab), int(one.matrix.sum()))
    for nc, cm in acc.items():
        out[f"cm_all_{nc}"] = cm.matrix.astype(np.int64)


def main():
    ns = ref_shim.load()
    cwd = os.getcwd()
    os.chdir(ref_shim.REFERENCE_ROOT)
    try:
        import utils.dataloaders as dl
    finally:
        os.chdir(cwd)
    out = {}
    loader_golden(dl, out)
    confusion_golden(ns.metrics, out)
    path = os.path.join(ROOT, "tests", "golden", "val_data.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
