"""CPU (emulator): the segmentation input pipeline (yolov5_amd/dataloaders.py second half + csrc/seg_data.h `y5_polygon_masks`) against the
batches the REFERENCE's own LoadImagesAndLabelsAndMasks.__getitem__ / load_mosaic / collate_fn produced (tests/golden/seg_data*.npz,
scripts/make_golden_seg_data.py) with the random draws reproduced from the same seeds: images bit-identical, targets identical (values and
row order), masks bit-identical -- integer pipelines and float64 host geometry in the reference's own expressions, so NO tolerance.  Then
the kernel directly against the NumPy restatement (tests/seg_data_ref.py) on ragged polygons, and the geometry check that does not rest
on the restatement, on the restatement and the kernel alike."""
import os
import random

import numpy as np
import pytest
import torch

from oracle import augment_oracle as ao
from tests import seg_data_ref as sd
from tests.hipemu import backend as emu_backend

GOLD = os.path.join(os.path.dirname(__file__), "golden")
HYP = dict(ao.HYP_AUG, degrees=5.0, shear=2.0, flipud=0.3)
DEV = torch.device("cpu")
CONFIGS = {  # name -> (hyp, seeds, indices of the batch): scripts/make_golden_seg_data.py:TRAIN
    "seg_data": (HYP, (1, 3, 4), lambda s: (s % 6, (s + 3) % 6)),
    "seg_data_mixed": (dict(HYP, mosaic=0.5), (11, 13, 16), lambda s: (s % 6, (s + 2) % 6, (s + 4) % 6)),
    "seg_data_mixup": (dict(HYP, mixup=0.5), (21, 23, 24), lambda s: (s % 6, (s + 2) % 6, (s + 4) % 6)),
}


@pytest.fixture(autouse=True)
def _seam():
    emu_backend.install()
    yield
    emu_backend.uninstall()


def dataset(tiny=False, device=DEV):
    from yolov5_amd.dataloaders import labels_from_segments

    ims, classes, segments = sd.polygon_dataset(6, seed=3, tiny=tiny)
    labels = [labels_from_segments(c, sg) for c, sg in zip(classes, segments)]
    return [torch.from_numpy(im).to(device) for im in ims], labels, segments


def check_train_config(name, seed, device=DEV):
    from yolov5_amd.dataloaders import draw_sample_seg, seg_mosaic_batch

    hyp, _, idx = CONFIGS[name]
    g = np.load(os.path.join(GOLD, name + ".npz"))
    s, overlap, ratio = int(g["s"]), bool(g["overlap"]), int(g["ratio"])
    ims, labels, segments = dataset(device=device)
    draws = []
    for index in idx(seed):
        random.seed(seed * 10 + index)            # the generators the reference consumed (scripts/make_golden_seg_data.py)
        np.random.seed(seed * 10 + index)
        draws.append(draw_sample_seg(index, 6, s, hyp))
    assert [d["mosaic"] for d in draws] == list(g[f"mosaic{seed}"])
    imgs, targets, masks = seg_mosaic_batch(ims, labels, segments, draws, s, hyp, dtype=torch.uint8, overlap=overlap, mask_ratio=ratio)
    assert np.array_equal(imgs.cpu().numpy(), g[f"img{seed}"])
    assert targets.shape == g[f"lab{seed}"].shape
    np.testing.assert_array_equal(targets.numpy(), g[f"lab{seed}"])
    assert masks.dtype == torch.uint8 and tuple(masks.shape) == g[f"mask{seed}"].shape
    assert np.array_equal(masks.cpu().numpy(), g[f"mask{seed}"])
    return draws


def check_val(k, device=DEV):
    from yolov5_amd.dataloaders import seg_letterbox_batch

    g = np.load(os.path.join(GOLD, "seg_data_val.npz"))
    s, (overlap, ratio) = int(g["s"]), g[f"cfg{k}"]
    ims, labels, segments = dataset(tiny=True, device=device)
    imgs, targets, shapes, masks = seg_letterbox_batch(ims, labels, segments, list(range(6)), s, overlap=bool(overlap), mask_ratio=int(ratio))
    assert np.array_equal(imgs.cpu().numpy(), g["img"])
    np.testing.assert_array_equal(targets.numpy(), g[f"lab{k}"])
    assert np.array_equal(masks.cpu().numpy(), g[f"mask{k}"])
    flat = np.array([[h0, w0, rh, rw, dw, dh] for (h0, w0), ((rh, rw), (dw, dh)) in shapes], np.float64)
    np.testing.assert_array_equal(flat, g[f"shapes{k}"])


def check_ragged(device=DEV):
    """y5_polygon_masks against the restatement: single-point and two-point polygons, one entirely outside, coordinates in (-1, 0), a
    polygon that vanishes at ratio 4, images with 0, 1 and 300 instances (float32 index planes, ties by label index); with flips."""
    from yolov5_amd.dataloaders import polygon_masks

    cases, B = sd.ragged_cases()
    polys, inst = [c[0] for c in cases], [c[1] for c in cases]
    flips = [(1, 0), (0, 1), (1, 1), (0, 0)]
    for ratio in (4, 2, 1, 3):
        for overlap in (0, 1):
            for fl in (None, flips):
                masks, order = polygon_masks(polys, inst, B, 64, 64, ratio, overlap, fl, device)
                ref, ref_order, _ = sd.reference_masks(polys, inst, B, 64, 64, ratio, overlap, fl)
                assert masks.cpu().numpy().dtype == ref.dtype and np.array_equal(masks.cpu().numpy(), ref), (ratio, overlap)
                if overlap:
                    assert np.array_equal(order, ref_order)
    # the uint8 side of the 255 boundary, and an empty batch
    masks, order = polygon_masks(polys[:11], inst[:11], 3, 64, 64, 4, 1, None, device)
    assert masks.dtype == torch.uint8 and np.array_equal(masks.cpu().numpy(), sd.reference_masks(polys[:11], inst[:11], 3, 64, 64, 4, 1)[0])
    masks, order = polygon_masks([], [], 2, 64, 64, 4, 1, None, device)
    assert tuple(masks.shape) == (2, 16, 16) and not masks.any() and len(order) == 0
    masks, _ = polygon_masks([], [], 2, 64, 64, 4, 0, None, device)
    assert tuple(masks.shape) == (0, 16, 16)


def kernel_fill(pts, size, device=DEV):
    from yolov5_amd.dataloaders import polygon_masks

    return polygon_masks([np.asarray(pts, np.float64)], [0], 1, size, size, 1, 0, None, device)[0][0].cpu().numpy()


def restated_fill(pts, size, device=None):
    return sd.fill_poly(np.zeros((size, size), np.uint8), [np.asarray(pts, np.int32)])


def check_geometry(fill, device=DEV):
    """Does not rest on the restatement: an axis-aligned integer rectangle fills exactly its inclusive pixel rectangle; every lattice point
    strictly inside a convex integer polygon is set; no set pixel lies more than one pixel (Chebyshev) from the closed polygon."""
    m = fill([[3, 4], [10, 4], [10, 9], [3, 9]], 24, device)
    exp = np.zeros((24, 24), np.uint8)
    exp[4:10, 3:11] = 1
    assert np.array_equal(m, exp)
    for p in sd.convex_polygons(24, 64, seed=5):
        sd.check_fill_geometry(fill(p, 64, device), p)


@pytest.mark.parametrize("name,seed", [(n, s) for n, (_, seeds, _) in CONFIGS.items() for s in seeds])
def test_seg_mosaic_batch_matches_reference_golden(name, seed):
    draws = check_train_config(name, seed)
    if name == "seg_data_mixup":
        assert seed != 24 or any(d.get("partner") is not None for d in draws)


@pytest.mark.parametrize("k", [0, 1, 2])
def test_validation_branch_matches_reference_golden(k):
    check_val(k)


def test_polygon_masks_matches_restatement_on_ragged_polygons():
    check_ragged()


@pytest.mark.parametrize("fill", [restated_fill, kernel_fill], ids=["restatement", "kernel"])
def test_fill_geometry_independent_of_the_restatement(fill):
    check_geometry(fill)


def test_interp_formula_and_resample_match_numpy():
    """np.interp over integer xp reduces to fp[j] + (fp[j + 1] - fp[j]) * (x - j) with the exact-hit shortcut: checked against np.interp, and
    resample_segments against the reference's literal loop (general.py:603-610)."""
    from yolov5_amd.dataloaders import resample_segments

    rng = np.random.default_rng(0)
    segs = [rng.uniform(0, 190, (k, 2)).astype(np.float32) for k in (3, 4, 7, 50, 333, 7, 3)]
    ref = []
    for s in segs:
        s = np.concatenate((s, s[0:1, :]), axis=0)
        x = np.linspace(0, len(s) - 1, 1000)
        xp = np.arange(len(s))
        ref.append(np.concatenate([np.interp(x, xp, s[:, i]) for i in range(2)]).reshape(2, -1).T)
        fp = s[:, 0].astype(np.float64)
        j = np.minimum(np.floor(x).astype(int), len(s) - 2)
        formula = np.where(x == j, fp[j], np.where(x == j + 1, fp[j + 1], (fp[j + 1] - fp[j]) * (x - j) + fp[j]))
        assert np.array_equal(formula, ref[-1][:, 0])
    assert np.array_equal(resample_segments(segs), np.array(ref))


def test_draws_loaders_and_labels_from_segments():
    from yolov5_amd.dataloaders import SegMosaicLoader, SegValLoader, draw_sample_seg, labels_from_segments

    with pytest.raises(NotImplementedError):
        draw_sample_seg(0, 6, 64, dict(HYP, copy_paste=0.1))
    with pytest.raises(NotImplementedError):
        draw_sample_seg(0, 6, 64, dict(HYP, perspective=0.001))
    lb = labels_from_segments([3], [np.array([[0.2, 0.1], [0.6, 0.3], [0.4, 0.9]], np.float32)])
    np.testing.assert_allclose(lb, [[3, 0.4, 0.5, 0.4, 0.8]], rtol=1e-6)
    ims, labels, segments = dataset()
    random.seed(0); np.random.seed(0)
    s = 64
    for overlap in (True, False):
        loader = SegMosaicLoader(ims, labels, segments, img_size=s, batch_size=4, hyp=HYP, dtype=torch.float16, overlap=overlap, mask_ratio=4)
        batches = list(loader)
        assert len(loader) == 2 and [tuple(b[0].shape) for b in batches] == [(4, 3, s, s), (2, 3, s, s)]
        for imgs, targets, paths, shapes, masks in batches:
            assert shapes is None and len(paths) == imgs.shape[0] and targets.shape[1] == 6
            assert tuple(masks.shape) == ((imgs.shape[0] if overlap else len(targets)), s // 4, s // 4)
            if overlap:   # value k + 1 = the k-th target row of the image
                for b in range(imgs.shape[0]):
                    assert int(masks[b].max()) <= int((targets[:, 0] == b).sum())
    val = SegValLoader(ims, None, segments, img_size=128, batch_size=4, overlap=True, mask_ratio=1, classes=[lb[:, 0] for lb in labels])
    out = list(val)
    assert len(val) == 2 and tuple(out[0][4].shape) == (4, 128, 128) and len(out[0][3]) == 4
