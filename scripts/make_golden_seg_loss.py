"""Writes tests/golden/seg_loss.npz from the UNMODIFIED reference's segmentation ComputeLoss (utils/segment/loss.py), imported
read-only through oracle.ref_shim on torch-CPU.  Needs the reference checkout; no test runs this.

    python scripts/make_golden_seg_loss.py

Per case of tests/seg_loss_ref.CASES: loss, items (lbox, lseg, lobj, lcls), dp{i} (d loss / d p[i]) and dproto, evaluated in fp32
(fp16 cases: on the fp16-rounded inputs)."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim, thirdparty as tp  # noqa: E402
from tests import seg_loss_ref as sr  # noqa: E402


class _Model(torch.nn.Module):
    """What ComputeLoss reads of a model: hyp, parameters() (device) and model[-1] (Segment: nl, na, nc, nm, anchors, stride)."""

    def __init__(self, nc):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.hyp = dict(sr.HYP)
        self.model = [types.SimpleNamespace(nl=3, na=3, nc=nc, nm=sr.NM, anchors=sr.ANCHORS.clone(),
                                            stride=torch.tensor([float(s) for s in sr.STRIDES]))]


def main():
    ref_shim.load()
    cwd = os.getcwd()
    os.chdir(ref_shim.REFERENCE_ROOT)
    try:
        import utils.segment.loss as seg_loss
    finally:
        os.chdir(cwd)
    seg_loss.bbox_iou, seg_loss.smooth_bce, seg_loss.xywh2xyxy = tp.bbox_iou, tp.smooth_bce, tp.xywh2xyxy
    out = {}
    for name in sr.CASES:
        c = sr.seg_case(name)
        cl = seg_loss.ComputeLoss(_Model(c["nc"]), overlap=c["overlap"])
        p = [torch.from_numpy(a.astype(np.float32)).requires_grad_(True) for a in c["p"]]
        proto = torch.from_numpy(c["proto"].astype(np.float32)).requires_grad_(True)
        loss, items = cl((p, proto), torch.from_numpy(c["targets"]), torch.from_numpy(c["masks"]))
        loss.backward()
        out[f"{name}_loss"] = loss.detach().numpy()
        out[f"{name}_items"] = items.numpy()
        for i in range(3):
            out[f"{name}_dp{i}"] = p[i].grad.numpy()
        out[f"{name}_dproto"] = proto.grad.numpy()
        _, _, indices, _, _, _ = cl.build_targets(p, torch.from_numpy(c["targets"]))
        print(name, loss.item(), items.tolist(), [int(ix[0].numel()) for ix in indices])
    path = os.path.join(ROOT, "tests", "golden", "seg_loss.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
