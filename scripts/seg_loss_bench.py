"""Segmentation loss timing at yolov5s-seg training shapes (bs 32, 640^2: p levels 80/40/20, proto 32 x 160 x 160, fp16):
the HIP ComputeLoss forward + backward (yolov5_amd.segment_loss) against a torch-on-GPU restatement of the reference's mask-term loop
(utils/segment/loss.py:88-103: per level, per image, (n, 32) @ (32, mh mw), BCE, crop, mean) run forward + backward on the same rows.

    python scripts/seg_loss_bench.py [--iters 50] [--train-step] [--out profiles/seg_loss/bench.json]

--train-step adds the yolov5s-seg training step at the same shape (fp16 plan: forward, segmentation loss, backward; no optimizer).

Wall times are CUDA-event medians after warm-up.  Kernel-level times come from a separate rocprofv3 --kernel-trace --stats run."""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import detgen, yolo_oracle as yo  # noqa: E402
from tests import seg_loss_ref as sr  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--bs", type=int, default=32)
    ap.add_argument("--per-img", type=int, default=8)
    ap.add_argument("--train-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seg_loss", "bench.json"))
    a = ap.parse_args()
    from yolov5_amd.segment_loss import ComputeLoss

    dev = torch.device("cuda:0")
    bs, hw, nc, nm = a.bs, 640, 80, sr.NM
    p = [torch.from_numpy(detgen.uniform((bs, 3, hw // s, hw // s, 5 + nc + nm), -2.5, 2.5, name=f"b{s}", seed=5)).half().to(dev)
         for s in sr.STRIDES]
    proto = torch.from_numpy(detgen.uniform((bs, nm, hw // 4, hw // 4), -1.0, 1.0, name="bproto", seed=5)).half().to(dev)
    t = detgen.synth_targets(bs, a.per_img, nc=nc, seed=5)
    masks = torch.from_numpy(detgen.integers((bs, hw // 4, hw // 4), 0, a.per_img + 1, name="bmask", seed=5).astype(np.float32)).to(dev)
    tt = torch.from_numpy(t)
    model = types.SimpleNamespace(hyp=dict(sr.HYP), parameters=lambda: iter([proto]),
                                  model=[types.SimpleNamespace(nl=3, na=3, nc=nc, nm=nm, anchors=sr.ANCHORS.to(dev),
                                                               stride=torch.tensor([8.0, 16.0, 32.0]))])
    cl = ComputeLoss(model, overlap=True)
    pg = [pi.clone().requires_grad_(True) for pi in p]
    prg = proto.clone().requires_grad_(True)

    def hip_step():
        loss, _ = cl((pg, prg), tt, masks)
        loss.backward()

    # reference-style loop: rows from the restated build_targets, everything else on the GPU in fp16 like AMP
    _, _, indices, _ = yo.build_targets([pi.shape for pi in p], tt, sr.ANCHORS, sr.HYP["anchor_t"])
    rows = sr.build_seg_targets([pi.shape for pi in p], tt, sr.ANCHORS, True, sr.HYP["anchor_t"])
    lv = []
    mh = mw = hw // 4
    for i in range(3):
        b, an, gj, gi = (x.to(dev) for x in indices[i])
        _, tidx, xywhn = (x.to(dev) for x in rows[i])
        mxyxy = xywhn * torch.tensor([mw, mh, mw, mh], device=dev, dtype=torch.float32)
        mxyxy = torch.cat((mxyxy[:, :2] - mxyxy[:, 2:] / 2, mxyxy[:, :2] + mxyxy[:, 2:] / 2), 1)
        lv.append((b, an, gj, gi, tidx, mxyxy, xywhn[:, 2:].prod(1)))
    r = torch.arange(mw, device=dev, dtype=torch.float32)[None, None, :]
    c = torch.arange(mh, device=dev, dtype=torch.float32)[None, :, None]

    def torch_step():
        lseg = torch.zeros(1, device=dev)
        for i, (b, an, gj, gi, tidx, mxyxy, marea) in enumerate(lv):
            pmask = pg[i][b, an, gj, gi][:, 5 + nc:]
            for bi in b.unique():  # host sync per level, as the reference
                j = b == bi
                gt = torch.where(masks[bi][None] == tidx[j].view(-1, 1, 1), 1.0, 0.0)
                s = (pmask[j] @ prg[bi].view(nm, -1)).view(-1, mh, mw)
                lm = F.binary_cross_entropy_with_logits(s.float(), gt, reduction="none")
                x1, y1, x2, y2 = torch.chunk(mxyxy[j][:, :, None], 4, 1)
                lm = lm * ((r >= x1) * (r < x2) * (c >= y1) * (c < y2))
                lseg = lseg + (lm.mean(dim=(1, 2)) / marea[j]).mean()
        (lseg * sr.HYP["box"]).backward()

    def timed(fn):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return float(np.median(ts))

    n_rows = [int(ix[0].numel()) for ix in indices]
    res = {"bs": bs, "hw": hw, "targets": int(len(t)), "rows_per_level": n_rows,
           "hip_loss_fwd_bwd_ms": timed(hip_step), "torch_mask_term_loop_fwd_bwd_ms": timed(torch_step),
           "hbm_floor_bytes": 2 * proto.numel() * proto.element_size()}
    if a.train_step:
        from yolov5_amd.yolo import SegmentationModel

        m = SegmentationModel("yolov5s-seg.yaml").to(dev).train()
        m.hyp = dict(sr.HYP)
        cls = ComputeLoss(m, overlap=True)
        x = torch.from_numpy(detgen.integers((bs, 3, hw, hw), 0, 256, name="bimg", seed=5).astype(np.uint8)).to(dev)

        def train_step():
            for q in m.parameters():
                q.grad = None
            loss, _ = cls(m(x), tt, masks)
            (loss * 1024.0).backward()

        res["train_step_ms"] = timed(train_step)
        res["train_step"] = "yolov5s-seg fp16 plan, uint8 images: forward + segmentation ComputeLoss + backward (no optimizer step)"
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
