"""GPU (-m gpu): the detection validation data path on the MI355X -- the twins of tests/test_emu_val_data.py (the INTER_AREA launch against
the NumPy restatement to the byte, ValLoader against the reference-generated golden, ConfusionMatrix against the reference's matrices,
integer-exact), then val_loop.run and train_loop.train fed by ValLoader end to end on yolov5n."""
import numpy as np
import pytest
import torch

from oracle import yolo_oracle as yo
from tests import test_emu_val_data as twin
from tests import val_data_ref as vd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.mark.parametrize("name", list(twin.FACTORS))
def test_area_kernel_equals_restatement(name, dev):
    twin.check_factor(name, dev)


def test_ragged_batch_all_dtypes_and_repeatable(dev):
    twin.check_ragged(dev)


def test_loader_matches_reference_golden(dev):
    twin.check_loader_golden(dev)


def test_single_cls_zeroes_the_class_column(dev):
    twin.check_single_cls(dev)


def test_square_mode_equals_seg_val_loader_images(dev):
    twin.check_square_mode(dev)


@pytest.mark.parametrize("name", list(vd.CM_CASES))
def test_confusion_matrix_case_equals_reference(name, dev):
    twin.check_cm_case(name, dev)


def test_confusion_matrix_accumulates_like_reference(dev):
    twin.check_cm_accumulated(dev)


def test_confusion_matrix_batch_form_equals_per_image_calls(dev):
    twin.check_cm_batch(dev)


@pytest.fixture(scope="module")
def model(dev):
    from yolov5_amd.yolo import DetectionModel

    cfg = yo.model_cfg("yolov5n")
    m = DetectionModel("yolov5n.yaml")
    m.load_state_dict(yo.det_state_dict(cfg, 0, fused=False))    # conditioned random weights
    m.hyp = dict(yo.HYP_SCRATCH_LOW)
    return m.to(dev)


def test_val_loop_on_val_loader_with_confusion_matrix(model, dev):
    """val_loop.run over the 9-image rect dataset: finite results, seen == 9 (one matrix column entry per label, in either branch), and the
    run without a confusion matrix returns identical metrics."""
    from yolov5_amd import val_loop
    from yolov5_amd.metrics import ConfusionMatrix

    loader = twin.dataset(dev, pad=vd.PAD)
    nc = 80
    cm = ConfusionMatrix(nc)
    res, maps, _ = val_loop.run(model.eval(), loader, half=True, nc=nc, confusion_matrix=cm)
    assert np.isfinite(np.asarray(res, np.float64)).all() and np.isfinite(maps).all()
    n_labels = sum(len(lb) for lb in loader.labels)
    m = cm.matrix
    print(f"\n[val data] results {[round(float(v), 4) for v in res]}; confusion: {int(m[:nc, :nc].sum())} matched, {int(m[nc, :nc].sum())} missed, "
          f"{int(m[:nc, nc].sum())} background of {n_labels} labels")
    assert m[:, :nc].sum() == n_labels
    seen = sum(imgs.shape[0] for imgs, *_ in loader)
    assert seen == 9
    res2, maps2, _ = val_loop.run(model.eval(), loader, half=True, nc=nc)
    assert res2 == res and np.array_equal(maps2, maps)


def test_train_loop_validates_on_val_loader(model, dev):
    from yolov5_amd import train_loop
    from yolov5_amd.dataloaders import MosaicLoader

    ims, labels = vd.val_dataset()
    t = [torch.from_numpy(im).to(dev) for im in ims]
    loader = MosaicLoader(t, labels, img_size=vd.IMG_SIZE, batch_size=vd.BATCH, seed=3)
    out = train_loop.train(model.train(), loader, epochs=1, batch_size=vd.BATCH, nbs=vd.BATCH, val_loader=twin.dataset(dev, pad=vd.PAD))
    row = np.asarray(out["results"][-1], np.float64)
    assert row.shape == (7,) and np.isfinite(row).all()
