"""Measures the classification path on one MI355X: yolov5s-cls shape (ClassificationModel of yolov5s, nc = 1000), batch 128, 224 x 224, fp16.

    python scripts/classify_bench.py [--out profiles/classify/classify_bench.json]

Prints (and writes as json) three things, each timed with device events after a warm-up over a window of at least half a second:
  * images/s of forward + post (the plan replay and y5_classify_post);
  * y5_classify_head, both forms, against the torch composition F.adaptive_avg_pool2d + F.linear on the same tensors in the same process;
  * the transform launch (128 frames of 480 x 640 -> 224) against the torch composition of the same steps (crop, F.interpolate bilinear,
    channel flip, / 255, normalise -- torch has no cv2-exact resize: the composition does the same amount of work, not the same rounding).
Random weights: the timings do not depend on them.  No test gates on these figures."""
import argparse
import ctypes as C
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from yolov5_amd import _lib  # noqa: E402
from yolov5_amd.augmentations import IMAGENET_MEAN, IMAGENET_STD, classify_transform_batch  # noqa: E402
from yolov5_amd.torch_utils import classify_post  # noqa: E402
from yolov5_amd.yolo import ClassificationModel, DetectionModel  # noqa: E402


def timed(fn, min_seconds=0.5):
    """ms per call: warm-up, then batches of calls between two device events until the timed window reaches min_seconds."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    iters, total_ms, total_n = 10, 0.0, 0
    while total_ms < min_seconds * 1e3:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        total_ms += e0.elapsed_time(e1)
        total_n += iters
        iters *= 2
    return total_ms / total_n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--imgsz", type=int, default=224)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda")
    B, S, nc = a.batch, a.imgsz, 1000
    res = {"batch": B, "imgsz": S, "nc": nc, "dtype": "fp16", "device": torch.cuda.get_device_name(0)}

    model = ClassificationModel(model=DetectionModel("yolov5s.yaml"), nc=nc, cutoff=10).eval().fuse().to(dev).half()
    x = torch.rand(B, 3, S, S, device=dev).half()

    def fwd_post():
        return classify_post(model(x))

    ms = timed(fwd_post)
    res["forward_post_ms"], res["images_per_s"] = ms, B / ms * 1e3
    eng = next(iter(model._engines.values()))
    res["plan"] = [[n, c] for n, c in eng.plan_table()]

    # the head alone: the Conv's NHWC output (B, 7, 7, 1280) -> logits
    lib = _lib.lib()
    HW, Cc = (S // 32) ** 2, 1280
    feat = torch.randn(B, HW, Cc, device=dev).half()
    w = (torch.randn(nc, Cc, device=dev) / Cc ** 0.5).half()
    bias = torch.randn(nc, device=dev)
    out = torch.empty(B, nc, device=dev, dtype=torch.float16)
    nbytes = lib.y5_classify_head_workspace_bytes(B, Cc)
    ws = _lib.workspace(nbytes, dev)
    p = lambda t: C.c_void_p(t.data_ptr())

    def head(form):
        _lib.check(lib.y5_classify_head(p(feat), _lib.Y5_F16, B, HW, Cc, Cc, p(w), p(bias), nc, p(out), nc, form, p(ws), nbytes, _lib.stream(dev)), lib)

    nchw = feat.view(B, S // 32, S // 32, Cc).permute(0, 3, 1, 2)   # the layout torch's Classify sees (channels-last memory)
    bias16 = bias.half()
    res["head_one_launch_ms"] = timed(lambda: head(1))
    res["head_two_launch_ms"] = timed(lambda: head(2))
    res["head_torch_ms"] = timed(lambda: F.linear(F.adaptive_avg_pool2d(nchw, 1).flatten(1), w, bias16))
    res["head_bytes"] = B * HW * Cc * 2 + nc * Cc * 2 + B * nc * 2
    res["head_flop"] = 2 * B * Cc * nc + B * HW * Cc

    # the transform: 128 frames of 480 x 640
    frames = [torch.randint(0, 256, (480, 640, 3), dtype=torch.uint8, device=dev) for _ in range(B)]
    mean = torch.tensor(IMAGENET_MEAN, device=dev).view(1, 3, 1, 1)
    std = torch.tensor(IMAGENET_STD, device=dev).view(1, 3, 1, 1)

    def torch_transform():
        crop = torch.stack([f[:, 80:560] for f in frames]).permute(0, 3, 1, 2).float()
        r = F.interpolate(crop, size=(S, S), mode="bilinear", align_corners=False)
        return ((r.flip(1) / 255.0 - mean) / std).half()

    res["transform_ms"] = timed(lambda: classify_transform_batch(frames, S, half=True))
    res["transform_torch_ms"] = timed(torch_transform)
    res["post_ms"] = timed(lambda: classify_post(out))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
