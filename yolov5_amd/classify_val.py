"""The reference's classification validation loop (classify/val.py:104-147) on the yolov5_amd seams: per batch `model(images)`, the top-5
ranking and the criterion; then top-1 / top-5 accuracy over the whole set, `loss /= n_batches`, and the per-class rows of `verbose`.
Ranking and per-row cross-entropy of a batch are ONE launch (torch_utils.classify_post); hit counts and the loss accumulate on the device and
are read once at the end.

Not here: building the dataloader from an image folder (dataloaders.ClassificationLoader takes frames in memory), the progress bar, timings."""
from __future__ import annotations

import torch

from .general import LOGGER
from .torch_utils import _HipCrossEntropyLoss, classify_post


@torch.no_grad()
def run(model, dataloader, criterion=None, half=False, verbose=False, names=None):
    """Returns (top1, top5, loss) as classify/val.py:147 does (loss = 0 without a criterion; a python float otherwise, where the reference returns
    a 0-dim tensor).  criterion: torch_utils.smartCrossEntropyLoss(...) -- its label smoothing rides in the ranking launch -- or any callable
    (logits, labels) -> 0-dim device tensor.  verbose: logs val.py:133-138's table and leaves its per-class rows [(name, images, top1, top5)] in
    `run.rows` (NaN accuracies for a class without images, as the reference's empty mean gives)."""
    inner = getattr(model, "model", model) if hasattr(model, "pt") else model
    inner.eval()                                                    # val.py:104
    inner.half() if half else inner.float()                         # val.py:76
    pred, targets, loss = [], [], None
    n = len(dataloader)                                             # number of batches
    fused = isinstance(criterion, _HipCrossEntropyLoss)
    for images, labels in dataloader:
        y = model(images.half() if half else images.float())
        top5, _, row_loss = classify_post(y, labels if fused else None, criterion.label_smoothing if fused else 0.0, want_probs=False)
        pred.append(top5)                                           # val.py:119
        targets.append(labels)
        if criterion:
            batch_loss = row_loss.mean() if fused else criterion(y, labels)
            loss = batch_loss if loss is None else loss + batch_loss    # val.py:122
    pred, targets = torch.cat(pred), torch.cat(targets)
    correct = (targets[:, None] == pred).float()                    # val.py:126
    acc = torch.stack((correct[:, 0], correct.max(1).values), dim=1)   # (top1, top5) accuracy
    nc = int(getattr(inner, "nc", 0)) or int(y.shape[1])
    names = names if names is not None else getattr(model, "names", None) or getattr(inner, "names", None) or {i: f"class{i}" for i in range(nc)}
    names = dict(enumerate(names)) if isinstance(names, (list, tuple)) else names
    head = torch.cat([acc.mean(0), (loss / n if loss is not None else torch.zeros((), device=acc.device)).float().reshape(1)])
    if verbose:
        onehot = torch.nn.functional.one_hot(targets.long(), max(nc, int(max(names)) + 1)).float()   # (N, classes)
        per = torch.cat([onehot.sum(0)[None], (onehot.T @ acc).T])   # (3, classes): images, top-1 hits, top-5 hits per class
        flat = torch.cat([head, per.reshape(-1)]).cpu()             # the one device-to-host read
        top1, top5_, lossv = flat[:3].tolist()
        cnt, s1, s5 = (v.tolist() for v in flat[3:].reshape(3, -1))
        run.rows = []
        LOGGER.info(f"{'Class':>24}{'Images':>12}{'top1_acc':>12}{'top5_acc':>12}")
        LOGGER.info(f"{'all':>24}{targets.shape[0]:>12}{top1:>12.3g}{top5_:>12.3g}")
        for i, c in names.items():
            k = int(cnt[i])
            t1, t5 = (s1[i] / k, s5[i] / k) if k else (float("nan"), float("nan"))
            run.rows.append((c, k, t1, t5))
            LOGGER.info(f"{c:>24}{k:>12}{t1:>12.3g}{t5:>12.3g}")
    else:
        top1, top5_, lossv = head.cpu().tolist()                    # the one device-to-host read
    return top1, top5_, (lossv if loss is not None else 0)
