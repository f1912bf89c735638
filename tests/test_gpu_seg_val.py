"""GPU: mask validation -- y5_val_match_masks through metrics.process_batch(masks=True) against the reference's own results
(tests/golden/seg_val.npz), the computed-bits mode against the loaded-bits mode on yolov5s-seg bs 32 640^2 NMS output, and
segment_val.run against segment/val.py's per-image loop restated here (our process_mask, torch mask_iou, the oracle's process_batch)."""
import os

import numpy as np
import pytest
import torch

from oracle import yolo_oracle as yo
from tests import seg_val_ref as sv
from tests.test_gpu_seg_train import _data, _model

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "seg_val.npz"))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.mark.parametrize("name", list(sv.CASES))
def test_process_batch_masks_vs_reference_golden(name, dev):
    from yolov5_amd import metrics

    c = sv.case(name)
    det, lab = torch.from_numpy(c["det"]).to(dev), torch.from_numpy(c["lab"]).to(dev)
    iouv = sv.IOUV.to(dev)
    got = metrics.process_batch(det, lab, iouv, torch.from_numpy(c["pm"]).to(dev), torch.from_numpy(c["gt"]).to(dev), overlap=c["overlap"],
                                masks=True)
    assert got.dtype == torch.bool and got.shape == (det.shape[0], 10)
    assert np.array_equal(got.cpu().numpy(), G[f"{name}_cm"].astype(bool))
    # (the box branch is not compared here: these boxes come from integer mask extents, so many label boxes tie in IoU, and the reference's
    # order of equal IoUs is numpy's argsort order -- implementation-defined for such lists, csrc/metrics.hip header; tests/test_*_metrics.py
    # cover that branch)


def _conditioned(name, dev):
    """The seeded model of test_gpu_seg_train with +2 on the bias of every mask-coefficient output of Segment's detection convs: the
    seeded weights alone give masks of a few pixels; with the offset the predicted masks cover much of their crop boxes."""
    m, cfg, sd = _model(name, dev)
    det = m.model[-1]
    with torch.no_grad():
        for conv in det.m:
            b = conv.bias.view(det.na, det.no)
            b[:, 5 + det.nc:] += 2.0
    return m


def _pred_bits(protos, out, cnt, shape):
    from yolov5_amd.segment import process_mask_batch

    bs, max_det, _ = out.shape
    dets = [out[b, : int(cnt[b])] for b in range(bs)]
    ms = process_mask_batch(protos, dets, shape, upsample=False, out_dtype=torch.uint8)
    pm = torch.zeros((bs, max_det) + tuple(protos.shape[2:]), dtype=torch.uint8, device=out.device)
    for b, m in enumerate(ms):
        pm[b, : m.shape[0]] = m
    return pm


def _targets_from(out, cnt, pm, per, overlap, ratio, seed):
    """`per` labels per image from the image's predicted masks (every 7th row: several classes), upsampled by `ratio` with a few pixels
    flipped; targets [img, cls, x, y, w, h] normalised."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    bs, _, mh, mw = pm.shape
    rows, planes = [], []
    for b in range(bs):
        k = 0
        for d in range(0, int(cnt[b]), 7):
            if k == per:
                break
            m = pm[b, d].cpu()
            if m.sum() < 10:
                continue
            gm = m.repeat_interleave(ratio, 0).repeat_interleave(ratio, 1).float()
            flip = torch.rand(gm.shape, generator=g) < 0.01
            gm[flip] = 1 - gm[flip]
            x1, y1, x2, y2 = out[b, d, :4].tolist()
            rows.append([b, float(out[b, d, 5]), (x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1])
            planes.append((b, k, gm))
            k += 1
    t = torch.tensor(rows, dtype=torch.float32)
    if overlap:
        gt = torch.zeros((bs, mh * ratio, mw * ratio), dtype=torch.uint8)
        for b, k, gm in planes:
            gt[b][gm > 0] = k + 1
    else:
        gt = torch.stack([gm for _, _, gm in planes])
    return t, gt


@pytest.mark.parametrize("overlap", [True, False])
def test_computed_equals_loaded_yolov5s_seg_bs32_640(overlap, dev):
    from yolov5_amd import metrics
    from yolov5_amd.general import non_max_suppression

    m = _conditioned("yolov5s-seg", dev)
    m.eval()
    x, _, _ = _data(32, 640, 1, 5)
    with torch.no_grad():
        z, protos, _ = m(x.to(dev))
    out, cnt = non_max_suppression(z, 0.001, 0.6, multi_label=True, max_det=300, nm=32, padded=True)
    assert (cnt == 300).sum() >= 16  # conf_thres 0.001: full 300-row images
    pm = _pred_bits(protos, out, cnt, (640, 640))
    t, gt = _targets_from(out, cnt, pm, 12, overlap, 4, 3)
    t, gt = t.to(dev), gt.to(dev)
    iouv = torch.linspace(0.5, 0.95, 10, device=dev)
    computed = metrics.match_masks_batch(out, cnt, protos, t, gt, iouv, overlap, (640, 640))
    loaded = metrics._match_masks(out.contiguous(), cnt, t, 0, 1, gt, overlap, iouv, pred_masks=pm)
    assert torch.equal(computed, loaded)
    assert t.shape[0] >= 32 and int(pm.sum()) > 0
    print(f"\n[seg val match] overlap={overlap}: {int(cnt.sum())} rows, {t.shape[0]} labels, {int(computed[..., 0].sum())} matches at IoU 0.5, "
          f"{int((pm.sum((2, 3)) > 0).sum())} non-empty predicted masks")


def _match_from_iou(iou, lab_cls, det_cls, iouv):
    """utils/metrics.py:255-265 on a given IoU matrix (labels x detections), the oracle's stable-sort form (yolo_oracle.process_batch)."""
    correct = np.zeros((det_cls.shape[0], iouv.shape[0]), dtype=bool)
    correct_class = lab_cls[:, None] == det_cls[None]
    for i in range(len(iouv)):
        li, di = np.nonzero((iou >= iouv[i]) & correct_class)
        if li.shape[0]:
            matches = np.stack([li.astype(np.float64), di.astype(np.float64), iou[li, di].astype(np.float64)], 1)
            if li.shape[0] > 1:
                matches = matches[np.argsort(matches[:, 2], kind="stable")[::-1]]
                matches = matches[np.unique(matches[:, 1], return_index=True)[1]]
                matches = matches[np.unique(matches[:, 0], return_index=True)[1]]
            correct[matches[:, 1].astype(int), i] = True
    return correct


def _oracle_run(model, batches, half, overlap, compute_loss, nc):
    """segment/val.py:235-331 per image, restated: our forward / NMS (list form) / process_mask, mask_iou on the host, oracle matching."""
    from yolov5_amd import segment_metrics as sm
    from yolov5_amd.general import non_max_suppression
    from yolov5_amd.segment import process_mask

    dev = next(model.parameters()).device
    model.half() if half else model.float()
    model.eval()
    iouv = sv.IOUV.numpy()
    stats, loss = [], torch.zeros(4, device=dev)
    for im, targets, _, _, masks in batches:
        im, targets, masks = im.to(dev), targets.to(dev).clone(), masks.to(dev)
        nb, _, h, w = im.shape
        preds, protos, train_out = model(im)
        loss += compute_loss((train_out, protos), targets, masks)[1]
        targets[:, 2:] *= torch.tensor((w, h, w, h), device=dev)
        preds = non_max_suppression(preds, 0.001, 0.6, multi_label=True, max_det=300, nm=32)
        for si, pred in enumerate(preds):
            labels = targets[targets[:, 0] == si, 1:].cpu()
            nl, npr = labels.shape[0], pred.shape[0]
            cm = np.zeros((npr, 10), bool)
            cb = np.zeros((npr, 10), bool)
            if npr == 0:
                if nl:
                    stats.append((cm, cb, np.zeros(0), np.zeros(0), labels[:, 0].numpy()))
                continue
            gt = (masks[[si]] if overlap else masks[targets[:, 0] == si]).float().cpu()
            pm = process_mask(protos[si], pred[:, 6:], pred[:, :4], (h, w)).cpu()
            p = pred.cpu().numpy()
            if nl:
                tbox = labels[:, 1:5].clone()
                tbox[:, :2], tbox[:, 2:] = labels[:, 1:3] - labels[:, 3:5] / 2, labels[:, 1:3] + labels[:, 3:5] / 2
                cb = yo.process_batch(p[:, :6], torch.cat((labels[:, 0:1], tbox), 1).numpy(), iouv)
                if overlap:
                    index = torch.arange(nl).view(nl, 1, 1) + 1
                    gt = torch.where(gt.repeat(nl, 1, 1) == index, 1.0, 0.0)
                if gt.shape[1:] != pm.shape[1:]:
                    gt = torch.nn.functional.interpolate(gt[None], pm.shape[1:], mode="bilinear", align_corners=False)[0].gt_(0.5)
                iou = sv.mask_iou(gt.view(nl, -1), pm.view(npr, -1)).numpy()
                cm = _match_from_iou(iou, labels[:, 0].numpy(), p[:, 5], iouv)
            stats.append((cm, cb, p[:, 4], p[:, 5], labels[:, 0].numpy()))
    st = [np.concatenate(x, 0) for x in zip(*stats)]
    metrics = sm.Metrics()
    if st[0].any():
        metrics.update(sm.ap_per_class_box_and_mask(*st))
    model.float()
    return (*metrics.mean_results(), *(loss.cpu() / len(batches)).tolist()), metrics.get_maps(nc)


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("overlap", [True, False])
def test_segment_val_run_vs_restated_reference_loop(half, overlap, dev):
    from yolov5_amd import segment_val
    from yolov5_amd.general import non_max_suppression
    from yolov5_amd.segment_loss import ComputeLoss

    m = _conditioned("yolov5n-seg", dev)
    B, S = 4, 256
    # data conditioned on the model: labels and masks are made from its own (fp32) predictions, so the metrics are far from 0
    batches = []
    for k in range(2):
        x, _, _ = _data(B, S, 1, 40 + k)
        m.eval()
        with torch.no_grad():
            z, protos, _ = m(x.to(dev))
        out, cnt = non_max_suppression(z, 0.25, 0.45, max_det=300, nm=32, padded=True)
        pm = _pred_bits(protos, out, cnt, (S, S))
        t, gt = _targets_from(out, cnt, pm, 6, overlap, 4, 50 + k)
        t[:, 2:] /= S
        batches.append(((x * 255).round().to(torch.uint8), t, None, None, gt))
    cl = ComputeLoss(m.train(), overlap=overlap)
    nc = m.model[-1].nc
    res, maps, t = segment_val.run(m, batches, half=half, compute_loss=cl, overlap=overlap)
    ref, ref_maps = _oracle_run(m, batches, half, overlap, cl, nc)
    assert len(res) == 12 and len(t) == 3 and maps.shape == (nc,)
    assert res[:8] == ref[:8], (res[:8], ref[:8])
    np.testing.assert_allclose(res[8:], ref[8:], rtol=1e-5)
    np.testing.assert_array_equal(maps, ref_maps)
    assert res[6] > 0.02  # mask mAP@0.5 is far from 0: the conditioned labels are found (conf_thres 0.001 keeps many false positives)
    assert next(m.parameters()).dtype == torch.float32
    print(f"\n[segment_val.run] half={half} overlap={overlap}: box {tuple(round(v, 4) for v in res[:4])} mask "
          f"{tuple(round(v, 4) for v in res[4:8])} loss {tuple(round(v, 5) for v in res[8:])}")


def test_segment_val_run_unsupported_options_raise(dev):
    from yolov5_amd import segment_val

    m, _, _ = _model("yolov5n-seg", dev)
    for kw in ("retina_masks", "save_json", "plots", "augment", "save_hybrid"):
        with pytest.raises(NotImplementedError):
            segment_val.run(m, [], **{kw: True})
