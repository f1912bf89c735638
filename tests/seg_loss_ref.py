"""TEST INFRASTRUCTURE ONLY: the segmentation ComputeLoss (utils/segment/loss.py:47-199) restated on torch-CPU in the oracle's style,
and the named input cases of tests/golden/seg_loss.npz (written by scripts/make_golden_seg_loss.py from the unmodified reference).

The detection terms are the oracle's `compute_loss` on the first 5 + nc columns of every row; the mask term is restated here:
for every level and every image with matched rows, the mean over those rows of
    sum over the crop of BCE(coef_r . proto_b, gt_r) / (mh mw) / (w_r h_r),
summed, times hyp_box / bs (loss.py:88-111).  Autograd of this function is the gradient reference of the emulator tests."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from oracle import detgen
from oracle import yolo_oracle as yo

HYP = yo.HYP_SCRATCH_LOW
STRIDES = (8, 16, 32)
ANCHORS = torch.tensor([[10, 13, 16, 30, 33, 23], [30, 61, 62, 45, 59, 119], [116, 90, 156, 198, 373, 326]],
                       dtype=torch.float32).view(3, 3, 2) / torch.tensor(STRIDES, dtype=torch.float32).view(3, 1, 1)
NM = 32


def build_seg_targets(shapes, targets, anchors, overlap, anchor_t=4.0):
    """utils/segment/loss.py:122-199: per level (b, a, gj, gi), tidx and xywhn of every matched row, in the reference's row order."""
    na, nt = anchors.shape[1], targets.shape[0]
    bs = shapes[0][0]
    gain = torch.ones(8)
    ai = torch.arange(na).float().view(na, 1).repeat(1, nt)
    if overlap:  # positional: concatenation over images of 1..count_i (loss.py:130-136)
        ti = torch.cat([torch.arange(int((targets[:, 0] == i).sum())).float() + 1 for i in range(bs)]) if nt else torch.zeros(0)
        ti = ti.view(1, -1).repeat(na, 1)
    else:
        ti = torch.arange(nt).float().view(1, nt).repeat(na, 1)
    targets = torch.cat((targets.repeat(na, 1, 1), ai[..., None], ti[..., None]), 2)
    g = 0.5
    off = torch.tensor([[0, 0], [1, 0], [0, 1], [-1, 0], [0, -1]]).float() * g
    out = []
    for i in range(len(shapes)):
        shape = shapes[i]
        gain[2:6] = torch.tensor(shape)[[3, 2, 3, 2]]
        t = targets * gain
        if nt:
            r = t[..., 4:6] / anchors[i][:, None]
            t = t[torch.max(r, 1 / r).max(2)[0] < anchor_t]
            gxy = t[:, 2:4]
            gxi = gain[[2, 3]] - gxy
            j, k = ((gxy % 1 < g) & (gxy > 1)).T
            l, m = ((gxi % 1 < g) & (gxi > 1)).T
            t = t.repeat((5, 1, 1))[torch.stack((torch.ones_like(j), j, k, l, m))]
        else:
            t = targets[0]
        b = t[:, 0].long()
        tidx = t[:, 7].long()
        xywhn = t[:, 2:6] / gain[2:6]
        out.append((b, tidx, xywhn))
    return out


def seg_loss(p, proto, targets, masks, nc, overlap, hyp=None, anchors=ANCHORS):
    """(loss[1], items[4] = lbox, lseg, lobj, lcls) of utils/segment/loss.py:47-114; differentiable w.r.t. p and proto."""
    hyp = hyp or HYP
    bs, nm, mh, mw = proto.shape
    if tuple(masks.shape[-2:]) != (mh, mw):
        masks = F.interpolate(masks[None], (mh, mw), mode="nearest")[0]
    det_loss, det_items = yo.compute_loss([pi[..., :5 + nc] for pi in p], targets, anchors, hyp, nc)
    _, _, indices, _ = yo.build_targets([pi.shape for pi in p], targets, anchors, hyp["anchor_t"])
    rows = build_seg_targets([pi.shape for pi in p], targets, anchors, overlap, hyp["anchor_t"])
    lseg = torch.zeros(1, dtype=torch.float32)
    for i, pi in enumerate(p):
        b, a, gj, gi = indices[i]
        _, tidx, xywhn = rows[i]
        if not b.numel():
            continue
        pmask = pi[b, a, gj, gi][:, 5 + nc:].float()
        marea = xywhn[:, 2:].prod(1)
        mxyxy = xywhn * torch.tensor([mw, mh, mw, mh], dtype=torch.float32)
        mxyxy = torch.cat((mxyxy[:, :2] - mxyxy[:, 2:] / 2, mxyxy[:, :2] + mxyxy[:, 2:] / 2), 1)
        for bi in b.unique():
            j = b == bi
            if overlap:
                gt = torch.where(masks[bi][None] == tidx[j].view(-1, 1, 1).float(), 1.0, 0.0)
            else:
                gt = masks[tidx][j]
            s = (pmask[j] @ proto[bi].float().view(nm, -1)).view(-1, mh, mw)
            lm = F.binary_cross_entropy_with_logits(s, gt.float(), reduction="none")
            lseg = lseg + (yo.crop_mask(lm, mxyxy[j]).mean(dim=(1, 2)) / marea[j]).mean()
    lseg = lseg * (hyp["box"] / bs)
    lbox, lobj, lcls = det_items[0:1], det_items[1:2], det_items[2:3]
    loss = det_loss + lseg * bs
    return loss, torch.cat((lbox, lseg.detach(), lobj, lcls))


# ---- named cases of tests/golden/seg_loss.npz ------------------------------------------------------------------------------------
CASES = ("overlap", "no_overlap", "empty_level", "nc1", "hires_masks", "unsorted", "fp16")


def _targets(name, bs, seed):
    """Sorted by image; image bs-1 has no targets; two targets share cells (duplicate rows); every target is big enough to match."""
    per = 4
    t = detgen.synth_targets(bs - 1, per, nc=80, seed=seed)
    t[:, 4:6] = 0.08 + t[:, 4:6]
    dup = t[0].copy()
    dup[1] = (dup[1] + 1) % 80
    dup[2:4] += 0.004
    t = np.concatenate((t[:1], dup[None], t[1:]), 0)  # same cells as row 0, sorted order kept
    return t


def _masks(t, bs, mh, mw, overlap, seed):
    """Filled box masks of the targets (overlap: instance ids per image, later instances drawn over earlier ones)."""
    nt = len(t)
    yy, xx = np.mgrid[0:mh, 0:mw].astype(np.float32) + 0.5
    boxes = []
    for k in range(nt):
        x, y, w, h = t[k, 2] * mw, t[k, 3] * mh, t[k, 4] * mw, t[k, 5] * mh
        # a slightly smaller, shifted ellipse inside the box: gt != box crop
        boxes.append(((xx - x) / (0.45 * w)) ** 2 + ((yy - y + 0.1 * h) / (0.5 * h)) ** 2 <= 1.0)
    if overlap:
        m = np.zeros((bs, mh, mw), np.float32)
        cnt = [0] * bs
        for k in range(nt):  # instance id = position among the image's targets + 1 (what collate_fn + the loss expect)
            b = int(t[k, 0])
            cnt[b] += 1
            m[b][boxes[k]] = cnt[b]
        return m
    m = np.stack(boxes).astype(np.float32) if nt else np.zeros((0, mh, mw), np.float32)
    noise = detgen.uniform(m.shape, 0.0, 1.0, name="mnoise", seed=seed) < 0.03  # a few flipped pixels
    return np.where(noise, 1.0 - m, m).astype(np.float32)


def seg_case(name):
    """dict(p=[np], proto=np, targets=np, masks=np, nc, overlap, dtype) of a named fixture case (deterministic)."""
    bs, hw, nc, overlap, dtype, seed, mres = 3, 96, 80, True, np.float32, 21, 1
    if name == "no_overlap":
        overlap = False
    elif name == "empty_level":
        seed = 22
    elif name == "nc1":
        nc, seed = 1, 23
    elif name == "hires_masks":
        mres, seed = 2, 24
    elif name == "unsorted":
        seed = 25
    elif name == "fp16":
        dtype, seed = np.float16, 26
    elif name != "overlap":
        raise KeyError(name)
    no = 5 + nc + NM
    p = [detgen.uniform((bs, 3, hw // s, hw // s, no), -2.5, 2.5, name=f"sp{s}", seed=seed) for s in STRIDES]
    proto = detgen.uniform((bs, NM, hw // 4, hw // 4), -1.0, 1.0, name="proto", seed=seed)
    t = _targets(name, bs, seed)
    if nc == 1:
        t[:, 1] = 0
    if name == "empty_level":  # small targets only: nothing matches the stride-32 anchors
        t[:, 4:6] = 0.05 + (t[:, 4:6] - 0.1) * 0.2
    mh = mw = (hw // 4) * mres
    masks = _masks(t, bs, mh, mw, overlap, seed)
    if name == "unsorted":  # the reference's positional tidx is NOT the per-image rank here; masks were drawn for the sorted order
        t = t[detgen.integers((len(t),), 0, 1 << 30, name="perm", seed=seed).argsort(kind="stable")]
    if dtype == np.float16:
        p = [a.astype(np.float16) for a in p]
        proto = proto.astype(np.float16)
    return dict(p=p, proto=proto, targets=t.astype(np.float32), masks=masks, nc=nc, overlap=overlap, dtype=dtype)
