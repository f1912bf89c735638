"""Measures classification training on one MI355X: yolov5s-cls shape (ClassificationModel of yolov5s, nc = 1000), batch 128, 224 x 224, fp16.

    python scripts/classify_train_bench.py [--optimizer SGD|Adam|AdamW|RMSProp] [--fused] [--out profiles/classify/classify_train_bench.json]

Prints (and writes as json) four things, each timed with device events after a warm-up over a window of at least half a second:
  * the whole step: train-mode forward, loss, backward and the optimizer block (unscale + clip + update) -- images/s.  --optimizer SGD (default):
    HipSGD.step_fused; another name: the torch optimizer through train_loop.host_amp_step as classify_train.train runs it by default (Adam is that
    loop's default optimizer), or with --fused the HipAdam / HipAdamW / HipRMSprop step_fused;
  * y5_classify_head_bwd alone (Dropout 0 and 0.2);
  * y5_classify_ce_bwd alone;
  * the torch autograd composition of pool + dropout + linear + cross-entropy (forward and backward) on the same tensors in the same process,
    and its backward alone, as the comparison for the head's backward + the loss gradient.
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
from yolov5_amd.torch_utils import classify_ce_bwd, smart_optimizer, smartCrossEntropyLoss  # noqa: E402
from yolov5_amd.train_loop import LossScaler, host_amp_step  # noqa: E402
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
    ap.add_argument("--optimizer", default="SGD", choices=["SGD", "Adam", "AdamW", "RMSProp"])
    ap.add_argument("--fused", action="store_true", help="smart_optimizer(fused=True): the device path for Adam / AdamW / RMSProp")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda")
    B, S, nc = a.batch, a.imgsz, 1000
    res = {"batch": B, "imgsz": S, "nc": nc, "dtype": "fp16", "device": torch.cuda.get_device_name(0), "optimizer": a.optimizer, "fused": bool(a.fused)}

    model = ClassificationModel(model=DetectionModel("yolov5s.yaml"), nc=nc, cutoff=10).to(dev).train()
    optimizer = smart_optimizer(model, a.optimizer, 0.001, momentum=0.9, decay=5e-5, fused=a.fused)
    res["optimizer_class"] = type(optimizer).__module__ + "." + type(optimizer).__name__
    scaler = LossScaler(enabled=True, init_scale=1024.0, growth_interval=10 ** 9)   # (host path only: a fixed scale, as below)
    params = list(model.parameters())
    criterion = smartCrossEntropyLoss(0.1)
    x = torch.rand(B, 3, S, S, device=dev).half()
    labels = torch.randint(0, nc, (B,), device=dev)
    scale = 1024.0

    def step():
        loss = criterion(model(x), labels)
        (loss * scale).backward()
        if hasattr(optimizer, "step_fused"):
            optimizer.step_fused(inv_scale=1.0 / scale, max_norm=10.0)
        else:
            host_amp_step(optimizer, params, scaler, 10.0)
            scaler.update()
        optimizer.zero_grad()

    ms = timed(step)
    res["step_ms"], res["images_per_s"] = ms, B / ms * 1e3

    # the head's backward alone: dlogits (B, nc) + pooled rows (B, 1280) + W -> dbias, dW, dx (B, 7 x 7, 1280)
    lib = _lib.lib()
    HW, Cc = (S // 32) ** 2, 1280
    dl = (torch.randn(B, nc, device=dev) / B).half()
    pooled = torch.randn(B, Cc, device=dev)
    w = (torch.randn(nc, Cc, device=dev) / Cc ** 0.5).half()
    dbias, dw = torch.empty(nc, device=dev), torch.empty(nc, Cc, device=dev)
    dx = torch.empty(B, HW, Cc, device=dev, dtype=torch.float16)
    nbytes = lib.y5_classify_head_workspace_bytes(B, Cc)
    ws = _lib.workspace(nbytes, dev)
    p = lambda t: C.c_void_p(t.data_ptr())

    def head_bwd(pd):
        _lib.check(lib.y5_classify_head_bwd(p(dl), _lib.Y5_F16, B, nc, nc, p(pooled), p(w), HW, Cc, pd, 12345, p(dbias), p(dw), p(dx), Cc, p(ws), nbytes,
                                            _lib.stream(dev)), lib)

    res["head_bwd_ms"] = timed(lambda: head_bwd(0.0))
    res["head_bwd_dropout_ms"] = timed(lambda: head_bwd(0.2))
    res["head_bwd_bytes"] = B * HW * Cc * 2 + nc * Cc * 2 + nc * Cc * 4 + 2 * B * Cc * 4 + B * nc * 2 * 2
    res["head_bwd_flop"] = 2 * 2 * B * Cc * nc

    logits = torch.randn(B, nc, device=dev).half()
    grad_rows = torch.full((B,), scale / B, device=dev)
    res["ce_bwd_ms"] = timed(lambda: classify_ce_bwd(logits, labels, 0.1, grad_rows))

    # torch autograd on the same shapes: the Conv's output as torch's Classify sees it (channels-last memory), fp16 like the reference under autocast
    feat = torch.randn(B, S // 32, S // 32, Cc, device=dev).half().permute(0, 3, 1, 2).requires_grad_(True)
    wt, bt = w.clone().requires_grad_(True), torch.randn(nc, device=dev).half().requires_grad_(True)

    def torch_fwd():
        z = F.linear(F.dropout(F.adaptive_avg_pool2d(feat, 1).flatten(1), 0.2, True), wt, bt)
        return F.cross_entropy(z.float(), labels, label_smoothing=0.1) * scale

    def torch_both():
        feat.grad = wt.grad = bt.grad = None
        torch_fwd().backward()

    res["torch_fwd_bwd_ms"] = timed(torch_both)
    res["torch_fwd_ms"] = timed(torch_fwd)
    res["torch_bwd_ms"] = res["torch_fwd_bwd_ms"] - res["torch_fwd_ms"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
