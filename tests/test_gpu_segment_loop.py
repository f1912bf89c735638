"""GPU (-m gpu): yolov5_amd.segment_loop.predict (segment/predict.py:139-173) against the seams it is composed of.
  * boxes: detect()'s on the same model.  detect() runs NMS without mask coefficients (nm = 0), so it is given the same network behind a
    wrapper that returns only the 5 + nc detection columns of the prediction; NMS never reads the coefficient columns, so rows must agree.
  * masks, retina_masks=False: process_mask per image on the letterboxed boxes (predict.py:172), bit for bit.
  * masks, retina_masks=True: the restatement of process_mask_native (tests/mask_native_ref.py, pinned to the reference) on the rounded boxes
    the loop returns (predict.py:169-170), under that module's acceptance rule."""
import numpy as np
import pytest
import torch

from tests import mask_native_ref as mr
from tests.test_gpu_seg_val import _conditioned

pytestmark = pytest.mark.gpu

SIZES = [(240, 320), (300, 200), (128, 128), (90, 400)]
KW = dict(imgsz=320, conf_thres=0.1, iou_thres=0.45, max_det=50)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev):
    return _conditioned("yolov5n-seg", dev).eval()


@pytest.fixture(scope="module")
def images():
    rng = np.random.default_rng(17)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SIZES]


class _BoxesOnly(torch.nn.Module):
    """The segmentation network as a plain detector: the prediction without its mask-coefficient columns."""

    def __init__(self, m, nm):
        super().__init__()
        self.m, self.nm = m, nm

    def forward(self, x):
        return self.m(x)[0][..., :-self.nm].contiguous()


def _seams(model, images, bs, dev):
    """Per image (NMS rows in letterboxed pixels, prototypes), batched exactly as predict() batches."""
    from yolov5_amd.augmentations import letterbox_batch
    from yolov5_amd.general import non_max_suppression

    out = []
    for b0 in range(0, len(images), bs):
        frames = [torch.from_numpy(im).to(dev) for im in images[b0:b0 + bs]]
        x, _ = letterbox_batch(frames, (320, 320), auto=False, stride=32, dtype=torch.float32)
        with torch.no_grad():
            pred, proto = model(x)[:2]
        rows = non_max_suppression(pred, KW["conf_thres"], KW["iou_thres"], max_det=KW["max_det"], nm=proto.shape[1])
        out += [(r.clone(), proto[i].clone()) for i, r in enumerate(rows)]
    return out


@pytest.mark.parametrize("bs", [4, 3])
@pytest.mark.parametrize("retina", [False, True])
def test_predict_equals_detect_boxes_and_seam_masks(model, images, retina, bs, dev):
    from yolov5_amd.detect_loop import detect
    from yolov5_amd.segment import process_mask
    from yolov5_amd.segment_loop import predict

    got = predict(model, images, retina_masks=retina, batch_size=bs, **KW)
    boxes = detect(_BoxesOnly(model, 32), images, batch_size=bs, **KW)
    seams = _seams(model, images, bs, dev)
    assert len(got) == len(images)
    counts = [int(d.shape[0]) for d, _ in got]
    print(f"\n[segment_loop] retina_masks={retina} batch_size={bs}: detections per image {counts}")
    assert max(counts) > 5
    assert sum(int(m.sum()) for _, m in got) > 1000   # the conditioned model's masks cover much of their boxes
    for (det, masks), ref_det, (rows, proto), (h0, w0) in zip(got, boxes, seams, SIZES):
        k = det.shape[0]
        assert det.device.type == "cpu" and det.dtype == torch.float32 and tuple(det.shape) == (k, 6)
        assert torch.equal(det, ref_det)
        assert rows.shape[0] == k and torch.equal(det[:, 4:], rows[:, 4:6].cpu())
        assert masks.device.type == "cuda" and masks.dtype == torch.float32
        if not retina:
            assert tuple(masks.shape) == (k, 320, 320)
            if k:
                assert torch.equal(masks, process_mask(proto, rows[:, 6:], rows[:, :4], (320, 320), upsample=True))
        else:
            assert tuple(masks.shape) == (k, h0, w0)
            if k:
                bits, v64, band = mr.reference_of(proto.cpu().numpy(), rows[:, 6:].cpu().numpy(), det[:, :4].numpy(), (h0, w0))
                mr.accept(masks.cpu().numpy(), bits, v64, band, f"predict retina {h0}x{w0} bs={bs}")


def test_predict_mask_dtypes_empty_images_and_model_check(model, images, dev):
    from yolov5_amd.segment_loop import predict

    f = predict(model, images, retina_masks=True, **KW)
    for dt in (torch.uint8, torch.bool):
        o = predict(model, images, retina_masks=True, mask_dtype=dt, **KW)
        for (d0, m0), (d1, m1) in zip(f, o):
            assert m1.dtype == dt and torch.equal(d0, d1) and torch.equal(m1.to(torch.float32), m0)
    # nothing passes the threshold: (0, 6) boxes and (0, H, W) masks at the right sizes
    for retina in (False, True):
        o = predict(model, images, retina_masks=retina, **dict(KW, conf_thres=1.0))
        for (d, m), (h0, w0) in zip(o, SIZES):
            assert tuple(d.shape) == (0, 6) and tuple(m.shape) == ((0, h0, w0) if retina else (0, 320, 320)) and m.device.type == "cuda"
    with pytest.raises(RuntimeError, match="segmentation model"):
        predict(_BoxesOnly(model, 32), images, **KW)
