"""CPU: host logic of the classification task -- ClassificationModel's structure against the reference's (tests/golden/classify.npz), the
planner, reshape_classifier_output, what is refused, pickling and the reference-pickled checkpoint, and classify_val.run's bookkeeping and the
predict loop on emulator logits (the `_lib.use_test_library` seam routes CPU tensors to the host-compiled kernels)."""
import copy
import os
import pickle

import numpy as np
import pytest
import torch

from tests import classify_ref as cr
from tests.hipemu import backend as emu_backend
from yolov5_amd import classify_loop, classify_val, common, torch_utils
from yolov5_amd.engine import build_plan_spec
from yolov5_amd.yolo import ClassificationModel, DetectionModel

G = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture()
def emu_seam():
    emu_backend.install()
    yield
    emu_backend.uninstall()


def cls_model(nc=cr.MODEL_NC):
    m = ClassificationModel(model=DetectionModel("yolov5n.yaml"), nc=nc, cutoff=10)
    m.load_state_dict(cr.cls_state_dict("yolov5n", nc))
    return m.eval()


@pytest.mark.parametrize("wrapped", [False, True])
def test_structure_matches_the_reference(wrapped):
    det = DetectionModel("yolov5n.yaml")
    src = common.DetectMultiBackend(det, device=torch.device("cpu"), fuse=False) if wrapped else det
    m = ClassificationModel(model=src, nc=10, cutoff=10)
    head = m.model[-1]
    assert len(m.model) == 10 and isinstance(head, common.Classify) and head.f == -1 and head.i == 9 and head.type == "models.common.Classify"
    assert head.conv.conv.in_channels == 256 and head.conv.conv.out_channels == 1280 and head.linear.out_features == 10
    assert isinstance(head.pool, torch.nn.AdaptiveAvgPool2d) and isinstance(head.drop, torch.nn.Dropout) and head.drop.p == 0.0
    assert m.save == [] and m.nc == 10 and torch.equal(m.stride, det.stride)
    assert list(m.state_dict().keys()) == str(cr.golden()["keys"]).split("\n")
    m.load_state_dict(cr.cls_state_dict())   # the reference's keys and shapes


def test_classify_refuses_what_is_not_built():
    with pytest.raises(NotImplementedError):
        common.Classify(64, 10, g=2)
    c = common.Classify(64, 10)
    with pytest.raises(NotImplementedError, match="list"):
        c([torch.zeros(1, 32, 2, 2), torch.zeros(1, 32, 2, 2)])
    with pytest.raises(NotImplementedError):
        ClassificationModel(cfg="yolov5s-cls.yaml")
    m = cls_model()
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(NotImplementedError, match="training"):
        m.train()(x)
    with pytest.raises(NotImplementedError, match="augment"):
        m.eval()(x, augment=True)
    with pytest.raises(NotImplementedError, match="augment"):
        common.DetectMultiBackend(m, device=torch.device("cpu"))(x, augment=True)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="GPU"):   # no CPU fall-back
            m.eval()(x)


def test_planner_accepts_a_classify_last_layer():
    spec = build_plan_spec(cls_model(), 2, 3, 96, 64)
    kinds = [o["op"] for o in spec.ops]
    assert kinds[-2:] == ["conv", "classify_head"] and spec.ops[-2]["name"] == "9.Classify.conv"
    assert spec.outputs == {"logits": dict(shape=(2, cr.MODEL_NC))}
    head = spec.ops[-1]
    assert head["x"] == spec.ops[-2]["y"] and (head["x"].H, head["x"].W, head["x"].C) == (3, 2, 1280) and head["nc"] == cr.MODEL_NC
    # fp16 plans keep the fused Bottleneck forms of the backbone
    fused = build_plan_spec(cls_model(), 2, 3, 64, 64, fuse_bneck=True)
    assert any(o["op"] == "bneck" for o in fused.ops) and fused.ops[-1]["op"] == "classify_head"


def test_reshape_classifier_output():
    m = cls_model()
    old = m.model[-1].linear
    torch_utils.reshape_classifier_output(m, cr.MODEL_NC)
    assert m.model[-1].linear is old                     # already n outputs: untouched
    m._engines["stale"] = object()
    torch_utils.reshape_classifier_output(m, 3)
    lin = m.model[-1].linear
    assert lin is not old and (lin.in_features, lin.out_features) == (1280, 3) and m.nc == 3 and not m._engines
    with pytest.raises(NotImplementedError):
        torch_utils.reshape_classifier_output(DetectionModel("yolov5n.yaml"), 3)


def test_pickle_deepcopy_and_dtype_moves_keep_the_model(emu_seam):
    m = cls_model()
    x = cr.model_input("sq")
    want = m(x)
    assert m._engines
    for clone in (copy.deepcopy(m), pickle.loads(pickle.dumps(m))):
        assert not clone._engines and torch.equal(clone(x), want)
    a, b = m(x), m(x)
    assert a.data_ptr() != b.data_ptr() and torch.equal(a, b)   # fresh tensor per call
    h = copy.deepcopy(m)
    h(x)
    h.half()
    assert not h._engines                                    # engine invalidation on a dtype move
    assert h(x.half()).dtype == torch.float16
    with torch.no_grad():
        m.model[-1].linear.weight.mul_(0.5)                  # an in-place edit is picked up by refresh_weights
        m.model[-1].linear.bias.zero_()
    got = m(x)
    assert not torch.equal(got, want)
    ref = cls_model()
    with torch.no_grad():
        ref.model[-1].linear.weight.mul_(0.5)
        ref.model[-1].linear.bias.zero_()
    assert torch.equal(got, ref(x))


def test_reference_pickled_checkpoint_loads_and_pickles_back(emu_seam, tmp_path):
    from yolov5_amd import checkpoint
    from yolov5_amd.experimental import attempt_load

    g = np.load(os.path.join(G, "ckpt_ref_cls_tiny.npz"))
    m = attempt_load(os.path.join(G, "ckpt_ref_cls_tiny.pt"), device="cpu")
    assert isinstance(m, ClassificationModel) and isinstance(m.model[-1], common.Classify)
    assert list(m.state_dict().keys()) == str(g["keys"]).split("\n")
    got = m(cr.model_input("sq")).numpy()
    np.testing.assert_allclose(got, g["logits"], rtol=1e-4, atol=1e-4)
    path = str(tmp_path / "cls.pt")
    checkpoint.save_checkpoint(path, m, epoch=0)
    with open(path, "rb") as f:
        blob = f.read()
    assert b"models.yolo" in blob and b"ClassificationModel" in blob and b"yolov5_amd" not in blob
    back = attempt_load(path, device="cpu")
    # (the file holds fp16 weights like the reference's, here of the FUSED model: the same logits up to that rounding)
    np.testing.assert_allclose(back(cr.model_input("sq")).numpy(), got, atol=5e-3)


@pytest.mark.parametrize("k", [0, 1])
def test_val_run_bookkeeping_matches_the_reference(emu_seam, k):
    """classify/val.py of the reference over three batches (2, 2, 1 images): per-batch mean loss then / n_batches, a last short batch, the
    verbose per-class rows -- on emulator logits.  The loss is compared within the fp32 whole-model bound (1e-4, tests/test_emu_model.py)."""
    g = cr.golden()
    labels = torch.from_numpy(g["val_labels"])
    batches = cr.val_inputs()
    loader = [(b, labels[2 * i:2 * i + len(b)]) for i, b in enumerate(batches)]
    m = cls_model()
    eps = (0.0, 0.1)[k]
    top1, top5, loss = classify_val.run(m, loader, criterion=torch_utils.smartCrossEntropyLoss(eps), verbose=True)
    want = g[f"val_triple_{k}"]
    assert (top1, top5) == pytest.approx(tuple(want[:2]), abs=1e-6)
    assert loss == pytest.approx(want[2], rel=1e-4, abs=1e-4)
    rows = np.array([[r[1], r[2], r[3]] for r in classify_val.run.rows], np.float64)
    np.testing.assert_allclose(rows, g[f"val_rows_{k}"], rtol=5e-3, equal_nan=True)   # (the golden rows are the reference's 3-digit log lines)
    # a plain callable as criterion gives the same loss; none gives 0
    t = classify_val.run(m, loader, criterion=lambda y, lab: torch.nn.functional.cross_entropy(y.float(), lab, label_smoothing=eps))
    assert t[:2] == (top1, top5) and t[2] == pytest.approx(loss, rel=1e-5)
    assert classify_val.run(m, loader)[2] == 0


def test_predict_loop_equals_the_composition_of_its_seams(emu_seam):
    from yolov5_amd.augmentations import CenterCrop, IMAGENET_MEAN, IMAGENET_STD, ToTensor, classify_transforms

    assert (IMAGENET_MEAN, IMAGENET_STD) == (cr.IMAGENET_MEAN, cr.IMAGENET_STD)
    frames = [torch.from_numpy(np.ascontiguousarray(cr.source(n)[0])) for n in ("rect", "down", "up")]
    m = cls_model()
    res, probs = classify_loop.predict(m, frames, imgsz=64, topk=3)
    x = classify_transforms(64)(frames)
    assert x.shape == (3, 3, 64, 64) and x.dtype == torch.float32
    for i, f in enumerate(frames):
        assert np.array_equal(x[i].numpy(), cr.transform_restated(f.numpy(), 64))
    top5, p, _ = torch_utils.classify_post(m(x))
    assert torch.equal(probs, p)
    for i, (idx, pr) in enumerate(res):
        assert torch.equal(idx, top5[i, :3].long()) and torch.equal(pr, p[i, idx])
    # the reference's two transform classes on their own: the crop is the restated resize, ToTensor the exact / 255
    c = CenterCrop(32)(frames[0])
    assert np.array_equal(c.numpy(), cr.center_crop_resize(frames[0].numpy(), 32))
    t = ToTensor()(c)
    assert torch.equal(t, torch.from_numpy(np.ascontiguousarray(c.numpy().transpose(2, 0, 1)[::-1])).float() / 255.0)
