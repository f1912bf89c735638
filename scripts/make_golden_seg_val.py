"""Writes tests/golden/seg_val.npz from the UNMODIFIED reference's mask-validation functions, imported read-only through oracle.ref_shim
on torch-CPU: process_batch (utils/metrics.py:224-265, both branches) and utils/segment/metrics.py (ap_per_class_box_and_mask, Metrics,
fitness).  Needs the reference checkout; no test runs this.

    python scripts/make_golden_seg_val.py

The shim stubs the ultralytics package, so `mask_iou` is bound to tests/seg_val_ref.mask_iou (restated; parity unpinned by necessity).
Per case of tests/seg_val_ref.CASES: {name}_cm / {name}_cb = correct_masks / correct_bboxes (N, 10) as segment/val.py:300-304 computes them
for one image (all False without labels).  On the statistics of all cases stacked in CASES order (segment/val.py:308,319-323):
box_* / mask_* per-class p, r, f1, ap, ap_class, mean_results (8), maps (get_maps(NC)) and fitness (8-column)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402
from tests import seg_val_ref as sv  # noqa: E402


def main():
    ns = ref_shim.load()
    ns.metrics.mask_iou = sv.mask_iou
    cwd = os.getcwd()
    os.chdir(ref_shim.REFERENCE_ROOT)
    try:
        import utils.segment.metrics as seg_metrics
    finally:
        os.chdir(cwd)
    iouv = sv.IOUV
    out, stats = {}, []
    for name in sv.CASES:
        c = sv.case(name)
        det, lab = torch.from_numpy(c["det"]), torch.from_numpy(c["lab"])
        n, nl = det.shape[0], lab.shape[0]
        cm = torch.zeros(n, 10, dtype=torch.bool)
        cb = torch.zeros(n, 10, dtype=torch.bool)
        if n and nl:
            cb = ns.metrics.process_batch(det, lab, iouv)
            cm = ns.metrics.process_batch(det, lab, iouv, torch.from_numpy(c["pm"]), torch.from_numpy(c["gt"]), overlap=c["overlap"], masks=True)
        out[f"{name}_cm"] = cm.numpy().astype(np.uint8)
        out[f"{name}_cb"] = cb.numpy().astype(np.uint8)
        stats.append((cm, cb, det[:, 4], det[:, 5], lab[:, 0]))
        print(name, n, nl, int(cm.sum()), int(cb.sum()))
    st = [torch.cat(x, 0).numpy() for x in zip(*stats)]
    res = seg_metrics.ap_per_class_box_and_mask(*st, names={})
    for k in ("boxes", "masks"):
        for f in ("p", "r", "f1", "ap", "ap_class"):
            out[f"{k}_{f}"] = np.asarray(res[k][f])
    metrics = seg_metrics.Metrics()
    metrics.update(res)
    mr = np.array(metrics.mean_results(), np.float64)
    out["mean_results"] = mr
    out["maps"] = np.asarray(metrics.get_maps(sv.NC))
    out["fitness"] = seg_metrics.fitness(mr[None])
    print("mean_results", mr, "fitness", out["fitness"])
    path = os.path.join(ROOT, "tests", "golden", "seg_val.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
