"""The reference's classification prediction loop, composed from the yolov5_amd seams (classify/predict.py:120-153) for a batch:
`classify_transforms -> model -> F.softmax(dim=1) -> argsort(descending)[:5]`:

  * the transform of a ragged batch of frames is one launch (augmentations.classify_transform_batch), the forward one plan replay;
  * softmax and the ranking are one launch (torch_utils.classify_post), then ONE device-to-host read brings the top-k indices and their
    probabilities of all images.

Not here: the annotator, save_txt, video / stream sources."""
from __future__ import annotations

import os

import torch

from .augmentations import classify_transform_batch
from .detect_loop import _to_device_frames, load_image
from .torch_utils import classify_post


@torch.no_grad()
def predict(model, images, imgsz=224, half=False, topk=5):
    """images: list of HWC uint8 BGR arrays / tensors (or file paths) of any sizes; model: ClassificationModel / DetectMultiBackend of one.
    Returns (results, probs): results[i] = (indices (k,) int64 CPU, probabilities (k,) fp32 CPU) of image i's k = min(topk, 5, nc) best classes,
    best first (classify/predict.py:152; equal probabilities by ascending class index); probs (B, nc) fp32 on the device (predict.py:133)."""
    if not 1 <= topk <= 5:
        raise ValueError("classify_loop.predict: topk must lie in 1..5 (the ranking kernel delivers five)")
    inner = getattr(model, "model", model) if hasattr(model, "pt") else model
    device = next(inner.parameters()).device
    imgs = [load_image(im)[..., ::-1] if isinstance(im, (str, os.PathLike)) else im for im in images]   # (files decode to RGB; cv2.imread's order is BGR)
    x = classify_transform_batch(_to_device_frames(imgs, device), imgsz, half=half)   # predict.py:120-125
    logits = model(x)                                                                  # predict.py:129
    top5, probs, _ = classify_post(logits)                                             # predict.py:133, 152
    k = min(topk, probs.shape[1])
    idx = top5[:, :k].long()
    both = torch.cat([idx.float(), probs.gather(1, idx)], 1).cpu()                     # the one device-to-host read (class indices are exact in fp32)
    return [(both[i, :k].long(), both[i, k:]) for i in range(len(imgs))], probs
