"""CPU (emulator): the detection validation data path -- `y5_letterbox_area_batch` (csrc/val_data.h) against the NumPy restatement of
tests/val_data_ref.py, equal to the byte; the restatement itself against the exact fp64 area mean; `dataloaders.ValLoader` against what the
REFERENCE's own rect code, __getitem__ and collate_fn produced (tests/golden/val_data.npz, scripts/make_golden_val_data.py); and
`metrics.ConfusionMatrix` (`y5_val_confusion`, csrc/metrics.hip) against the reference's matrices of the same file, integer-exact.  The
`check_*` functions take the device: tests/test_gpu_val_data.py re-runs them on the MI355X."""
import os

import numpy as np
import pytest
import torch

from tests import seg_data_ref as sd
from tests import val_data_ref as vd
from tests.hipemu import backend as emu_backend

GOLD = os.path.join(os.path.dirname(__file__), "golden", "val_data.npz")
DEV = torch.device("cpu")
# name -> (h0, w0, nh, nw)
FACTORS = {"2x2": (20, 24, 10, 12), "3x3": (30, 36, 10, 12), "4x2": (40, 24, 10, 12), "53to32_37to23": (37, 53, 23, 32),
           "33to32": (33, 33, 32, 32), "272to32": (272, 272, 32, 32), "3x40to3x32": (3, 40, 3, 32)}
NP_DTYPE = {torch.uint8: np.uint8, torch.float16: np.float16, torch.float32: np.float32}


@pytest.fixture(autouse=True)
def _seam():
    emu_backend.install()
    yield
    emu_backend.uninstall()


def _run(ims, sizes, places, H, W, device, dtype=torch.uint8, normalize=False):
    from yolov5_amd.dataloaders import letterbox_area_batch

    return letterbox_area_batch(ims, sizes, places, H, W, dtype, normalize).cpu().numpy()


def check_factor(name, device=DEV):
    """One factor, the three contents as three jobs of one launch; odd top / left, canvas width 52 (no multiple of 16)."""
    h0, w0, nh, nw = FACTORS[name]
    ims = [vd.pattern(k, h0, w0, seed=3) for k in ("random", "white", "checker")]
    sizes, places = [(nh, nw)] * 3, [(3, 5), (1, 7), (5, 19)]
    H, W = nh + 8, 52
    got = _run([torch.from_numpy(im).to(device) for im in ims], sizes, places, H, W, device)
    ref = vd.letterbox_area_ref(ims, sizes, places, H, W)
    assert got.dtype == ref.dtype and got.shape == ref.shape
    assert np.array_equal(got, ref), f"{name}: {int((got != ref).sum())} bytes differ"
    assert (ref[1, :, places[1][0]:places[1][0] + nh, places[1][1]:places[1][1] + nw] == 255).all()   # all 255 saturates, does not wrap


def ragged_batch(device):
    """Area (tables, integer block, 2x2), linear-up and copy jobs in one launch; job 0 reads a source whose row stride is not 3 * w0."""
    rng = np.random.default_rng(5)
    wide = rng.integers(0, 256, (37, 70, 3), dtype=np.uint8)
    ims = [wide[:, :53], vd.pattern("random", 30, 36, 1), vd.pattern("checker", 20, 24), vd.pattern("random", 10, 13, 2),
           vd.pattern("random", 23, 32, 4), vd.pattern("random", 45, 61, 6)]
    sizes = [(23, 32), (10, 12), (10, 12), (23, 30), (23, 32), (31, 42)]
    places = [(1, 3), (7, 91), (0, 0), (9, 65), (15, 11), (3, 77)]
    t = [torch.from_numpy(np.ascontiguousarray(im)).to(device) for im in ims]
    t[0] = torch.from_numpy(wide).to(device)[:, :53]
    assert t[0].stride(0) == 210
    return ims, t, sizes, places


def check_ragged(device=DEV):
    ims, t, sizes, places = ragged_batch(device)
    for H, W in ((40, 128), (41, 133)):                           # 16-byte stores of the padding possible / impossible
        for dtype in (torch.uint8, torch.float16, torch.float32):
            got = _run(t, sizes, places, H, W, device, dtype, normalize=True)
            ref = vd.letterbox_area_ref(ims, sizes, places, H, W, NP_DTYPE[dtype], normalize=True)
            assert got.dtype == ref.dtype and np.array_equal(got, ref), (H, W, dtype)
            assert np.array_equal(got, _run(t, sizes, places, H, W, device, dtype, normalize=True))   # back to back: bit-identical
    raw = _run(t, sizes, places, 40, 128, device, torch.float32, normalize=False)
    assert np.array_equal(raw, vd.letterbox_area_ref(ims, sizes, places, 40, 128).astype(np.float32))


def dataset(device=DEV, **kw):
    from yolov5_amd.dataloaders import ValLoader

    ims, labels = vd.val_dataset()
    return ValLoader([torch.from_numpy(im).to(device) for im in ims], labels, img_size=vd.IMG_SIZE, batch_size=vd.BATCH, stride=vd.STRIDE, **kw)


def check_loader_golden(device=DEV):
    g = np.load(GOLD)
    loader = dataset(device, pad=vd.PAD)
    np.testing.assert_array_equal(loader.order, g["order"])
    np.testing.assert_array_equal(loader.shapes, g["shapes"])
    np.testing.assert_array_equal(loader.batch, g["batch"])
    np.testing.assert_array_equal(loader.batch_shapes, g["batch_shapes"])
    for k, lb in enumerate(loader.labels):
        np.testing.assert_array_equal(lb, g[f"labels{k}"])
    assert len(loader) == 3
    for _ in range(2):                                            # re-iterable: the second pass gives the same batches
        nb = 0
        for b, (imgs, targets, paths, shapes) in enumerate(loader):
            assert imgs.dtype == torch.uint8 and np.array_equal(imgs.cpu().numpy(), g[f"img{b}"]), b
            assert targets.dtype == torch.float32 and tuple(targets.shape) == g[f"lab{b}"].shape
            np.testing.assert_array_equal(targets.numpy(), g[f"lab{b}"])
            assert paths == [f"image{i}" for i in g[f"paths{b}"]]
            flat = np.array([[h0, w0, rh, rw, dw, dh] for (h0, w0), ((rh, rw), (dw, dh)) in shapes], np.float64)
            np.testing.assert_array_equal(flat, g[f"shp{b}"])
            nb += 1
        assert nb == 3 and imgs.shape[0] == 1                     # the last batch is short


def check_single_cls(device=DEV):
    a, b = dataset(device, single_cls=True), dataset(device)
    assert all((lb[:, 0] == 0).all() for lb in a.labels)
    for (_, ta, _, _), (_, tb, _, _) in zip(a, b):
        assert (ta[:, 1] == 0).all() and torch.equal(ta[:, 2:], tb[:, 2:]) and torch.equal(ta[:, 0], tb[:, 0]) and tb[:, 1].any()


def check_square_mode(device=DEV):
    """rect=False, pad=0 (`val.py --task speed`) against SegValLoader's image half: S = 128 shrinks no image of the tiny polygon dataset (the
    default path of SegValLoader), S = 64 shrinks some (SegValLoader(area=True))."""
    from yolov5_amd.dataloaders import SegValLoader, ValLoader, _resized_hw, labels_from_segments

    ims, classes, segments = sd.polygon_dataset(6, seed=3, tiny=True)
    labels = [labels_from_segments(c, sg) for c, sg in zip(classes, segments)]
    t = [torch.from_numpy(im).to(device) for im in ims]
    for S, area, shrinks in ((128, False, False), (64, True, True)):
        assert any(_resized_hw(*im.shape[:2], S)[0] < im.shape[0] for im in ims) == shrinks
        det = ValLoader(t, labels, img_size=S, batch_size=4, rect=False, pad=0.0)
        seg = SegValLoader(t, labels, segments, img_size=S, batch_size=4, area=area)
        assert len(det) == len(seg) == 2 and not hasattr(det, "batch_shapes")
        for (im_d, tg_d, paths_d, shapes_d), (im_s, _tg, paths_s, shapes_s, _m) in zip(det, seg):
            assert tuple(im_d.shape[2:]) == (S, S) and torch.equal(im_d, im_s)
            assert paths_d == paths_s and shapes_d == shapes_s and tg_d.shape[1] == 6


def _cm(nc, device):
    from yolov5_amd.metrics import ConfusionMatrix

    return ConfusionMatrix(nc, vd.CONF, vd.IOU_THRES)


def _feed(cm, det, lab, device):
    cm.process_batch(None if det is None else torch.from_numpy(det).to(device), torch.from_numpy(lab).to(device))


def check_cm_case(name, device=DEV):
    nc, det, lab = vd.cm_case(name)
    cm = _cm(nc, device)
    _feed(cm, det, lab, device)
    m = cm.matrix
    assert m.dtype == np.float64 and m.shape == (nc + 1, nc + 1) and cm.nc == nc
    np.testing.assert_array_equal(m, np.load(GOLD)[f"cm_{name}"])


def check_cm_accumulated(device=DEV):
    g = np.load(GOLD)
    acc = {}
    for name in vd.CM_CASES:
        nc, det, lab = vd.cm_case(name)
        _feed(acc.setdefault(nc, _cm(nc, device)), det, lab, device)
    assert sorted(acc) == [1, 3, 5, 80]
    for nc, cm in acc.items():
        np.testing.assert_array_equal(cm.matrix, g[f"cm_all_{nc}"])
    with pytest.raises(NotImplementedError):
        acc[3].plot()


def check_cm_batch(device=DEV):
    """`update` on a padded batch == the per-image `process_batch` calls of val.py:289-309 on `predn` of match_batch(predn=True) and the
    de-letterboxed labels; with the loader's shapes and with None."""
    from yolov5_amd.metrics import match_batch

    out, counts, targets, shapes, nc = vd.batch_case()
    out_t, cnt_t, tg_t = torch.from_numpy(out).to(device), torch.from_numpy(counts).to(device), torch.from_numpy(targets).to(device)
    iouv = torch.linspace(0.5, 0.95, 10)
    for shp in (shapes, None):
        cm = _cm(nc, device)
        cm.update(out_t, cnt_t, tg_t, shp)
        _, predn = match_batch(out_t, cnt_t, tg_t, shp, iouv.to(device), predn=True)
        per = _cm(nc, device)
        for si in range(out.shape[0]):
            lab = torch.from_numpy(targets[targets[:, 0] == si, 1:])
            n = int(counts[si])
            if n == 0:
                if len(lab):
                    per.process_batch(None, lab[:, 0].to(device))                               # val.py:293
                continue
            if not len(lab):
                continue                                                                         # val.py:303: nothing is counted
            half = lab[:, 3:5] / 2
            box = torch.cat((lab[:, 1:3] - half, lab[:, 1:3] + half), 1)                         # xywh2xyxy, then scale_boxes in fp32
            if shp is not None:
                (h0, w0), ((gain, _), (px, py)) = shp[si]
                g32, pad = torch.tensor(gain, dtype=torch.float32), torch.tensor([px, py, px, py], dtype=torch.float32)
                box = (box - pad) / g32
                box[:, [0, 2]] = box[:, [0, 2]].clamp(0, w0)
                box[:, [1, 3]] = box[:, [1, 3]].clamp(0, h0)
            det = torch.cat((predn[si, :n].cpu(), out_t[si, :n, 4:6].cpu()), 1)
            per.process_batch(det.to(device), torch.cat((lab[:, :1], box), 1).to(device))
        m = cm.matrix
        np.testing.assert_array_equal(m, per.matrix)
        assert m[:, :nc].sum() == len(targets) and m[:nc, :nc].sum() > 0 and m[nc, :nc].sum() >= (targets[:, 0] == 1).sum()


@pytest.mark.parametrize("name", list(FACTORS))
def test_area_kernel_equals_restatement(name):
    check_factor(name)


def test_ragged_batch_all_dtypes_and_repeatable():
    check_ragged()


def test_loader_matches_reference_golden():
    check_loader_golden()


def test_single_cls_zeroes_the_class_column():
    check_single_cls()


def test_square_mode_equals_seg_val_loader_images():
    check_square_mode()


@pytest.mark.parametrize("name", list(vd.CM_CASES))
def test_confusion_matrix_case_equals_reference(name):
    check_cm_case(name)


def test_confusion_matrix_accumulates_like_reference():
    check_cm_accumulated()


def test_confusion_matrix_batch_form_equals_per_image_calls():
    check_cm_batch()


# ---- the restatement itself (CPU only) ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in FACTORS if n != "2x2"])
def test_restatement_within_fp32_bound_of_exact_area_mean(name):
    """|restated - exact fp64 mean| <= 0.5 + 255 * (nx + ny + 4) * 2^-23 per pixel: the final rounding to a byte plus the fp32 rounding of the
    nx products / sums of a row, the ny of the column, and the four roundings of the weights and their normalisation.  General path and the
    integer path that is not 2x2."""
    h0, w0, nh, nw = FACTORS[name]
    nx, ny = vd.tap_counts(w0, nw), vd.tap_counts(h0, nh)
    bound = 0.5 + 255.0 * (nx[None, :, None] + ny[:, None, None] + 4) * 2.0 ** -23
    for kind in ("random", "white", "checker"):
        im = vd.pattern(kind, h0, w0, seed=9)
        err = np.abs(vd.resize_area(im, (nw, nh)).astype(np.float64) - vd.area_mean_exact(im, (nw, nh)))
        assert (err <= bound).all(), (kind, float(err.max()))


def test_restatement_2x2_rule_is_exact():
    im = vd.pattern("random", 20, 24, seed=2)
    a = im.astype(np.int64)
    exp = (a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2
    assert np.array_equal(vd.resize_area(im, (12, 10)), exp.astype(np.uint8))
    chk = vd.resize_area(vd.pattern("checker", 20, 24), (12, 10))
    assert (chk == 128).all()                                     # (0 + 255 + 255 + 0 + 2) >> 2: the half-way case rounds up
