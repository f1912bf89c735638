"""GPU (-m gpu): the segmentation input pipeline on the MI355X -- the twins of tests/test_emu_seg_data.py (reference-generated goldens,
bit-identical; y5_polygon_masks against the restatement on ragged polygons; the geometry check that does not rest on the restatement), a
full-size batch (64 x 640^2 from 1280 x 720 frames, 8 polygons per frame) against the restatement on a few images, and train_loop.train /
segment_val.run fed by SegMosaicLoader / SegValLoader."""
import random

import numpy as np
import pytest
import torch

from oracle import augment_oracle as ao, yolo_oracle as yo
from tests import seg_data_ref as sd
from tests import test_emu_seg_data as twin

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.mark.parametrize("name,seed", [(n, s) for n, (_, seeds, _) in twin.CONFIGS.items() for s in seeds])
def test_seg_mosaic_batch_matches_reference_golden(name, seed, dev):
    twin.check_train_config(name, seed, dev)


@pytest.mark.parametrize("k", [0, 1, 2])
def test_validation_branch_matches_reference_golden(k, dev):
    twin.check_val(k, dev)


def test_polygon_masks_matches_restatement_on_ragged_polygons(dev):
    twin.check_ragged(dev)


def test_fill_geometry_independent_of_the_restatement(dev):
    twin.check_geometry(twin.kernel_fill, dev)


def test_full_size_batch_vs_restatement_and_determinism(dev):
    from yolov5_amd.dataloaders import draw_sample_seg, labels_from_segments, seg_mosaic_batch, seg_mosaic_geometry

    s, n, B = 640, 16, 64
    ims, classes, segments = sd.full_size_dataset(n, per=8, seed=7)
    labels = [labels_from_segments(c, sg) for c, sg in zip(classes, segments)]
    ims_t = [torch.from_numpy(im).to(dev) for im in ims]
    hyp = dict(ao.HYP_AUG, degrees=5.0, shear=2.0, flipud=0.3)
    random.seed(13); np.random.seed(13)
    draws = [draw_sample_seg(i % n, n, s, hyp) for i in range(B)]
    imgs, targets, masks = seg_mosaic_batch(ims_t, labels, segments, draws, s, hyp, overlap=True, mask_ratio=4)
    assert tuple(masks.shape) == (B, 160, 160) and masks.dtype == torch.uint8
    _, labs, polys, inst = seg_mosaic_geometry(ims_t, labels, segments, draws, s, hyp)
    inst = np.array(inst)
    print(f"\n[seg data] {len(polys)} instances in the batch, {len(polys) / B:.1f} per image")
    for b in (0, 17, 63):
        ids = np.nonzero(inst == b)[0]
        ref, order, _ = sd.reference_masks([polys[i] for i in ids], [0] * len(ids), 1, s, s, 4, 1, [(draws[b]["flipud"], draws[b]["fliplr"])])
        assert np.array_equal(masks[b].cpu().numpy(), ref[0]), b
        np.testing.assert_array_equal(targets[targets[:, 0] == b].numpy(), labs[b][order])
    imgs2, targets2, masks2 = seg_mosaic_batch(ims_t, labels, segments, draws, s, hyp, overlap=True, mask_ratio=4)
    assert torch.equal(imgs, imgs2) and torch.equal(targets, targets2) and torch.equal(masks, masks2)
    m0, _, = seg_mosaic_batch(ims_t, labels, segments, draws, s, hyp, overlap=False, mask_ratio=4)[1:]
    assert m0.shape[0] == len(polys)


def test_train_loop_fed_by_seg_mosaic_loader_and_validation(dev):
    """train_loop.train on yolov5n-seg fed by SegMosaicLoader over a small synthetic polygon dataset, fixed seed: four finite loss items per
    step, mask planes of the shape the loss expects (no F.interpolate fallback), mean lseg of the last epoch below the first; then
    segment_val.run on SegValLoader returns finite box and mask metrics."""
    from yolov5_amd import segment_val, train_loop
    from yolov5_amd.dataloaders import SegMosaicLoader, SegValLoader
    from yolov5_amd.yolo import SegmentationModel

    cfg = yo.model_cfg("yolov5n-seg")
    m = SegmentationModel("yolov5n-seg.yaml")
    m.load_state_dict(yo.det_state_dict(cfg, 0, fused=False))
    m.hyp = dict(yo.HYP_SCRATCH_LOW)
    m = m.to(dev).train()
    S, B = 128, 4
    ims, classes, segments = sd.polygon_dataset(6, seed=3)
    ims, classes, segments = (ims * 6)[:32], (classes * 6)[:32], (segments * 6)[:32]   # 8 batches per epoch: the epoch mean averages the augmentation noise
    ims_t = [torch.from_numpy(im).to(dev) for im in ims]
    hyp_aug = dict(ao.HYP_AUG, mosaic=0.5)   # half of the samples keep one whole image: more mask pixels per step on this tiny set
    random.seed(5); np.random.seed(5)
    loader = SegMosaicLoader(ims_t, None, segments, img_size=S, batch_size=B, hyp=hyp_aug, seed=5, overlap=True, mask_ratio=4, classes=classes)
    first = next(iter(loader))
    assert tuple(first[4].shape) == (B, S // 4, S // 4) and first[4].dtype == torch.uint8   # proto resolution: no interpolate in the loss
    random.seed(5); np.random.seed(5)
    epochs = 8
    out = train_loop.train(m, loader, hyp=dict(train_loop.HYP_SCRATCH_LOW), epochs=epochs, batch_size=B, nbs=B, ema=True)
    losses = out["losses"]
    assert losses.shape == (epochs * len(loader), 4) and torch.isfinite(losses).all()
    lseg = out["mloss"][:, 1]
    print(f"\n[seg loader train] lseg per epoch {[round(float(v), 5) for v in lseg]}")
    assert lseg[-1] < lseg[0]
    val = SegValLoader(ims_t, None, segments, img_size=S, batch_size=B, overlap=True, mask_ratio=1, classes=classes)
    res, maps, _ = segment_val.run(m, val, half=True, overlap=True, nc=80)
    print(f"[seg loader val] {[round(float(v), 4) for v in res]}")
    assert len(res) >= 8 and np.isfinite(np.asarray(res, dtype=np.float64)).all()
