"""Writes tests/golden/classify.npz (and tests/golden/ckpt_ref_cls_tiny.pt) from the UNMODIFIED reference, imported read-only through
oracle.ref_shim on torch-CPU.  Needs the reference checkout; no test runs this.

    python scripts/make_golden_classify.py

  tf_{case}            (3, 32, 32) fp32: the reference's CenterCrop(32) and ToTensor() (utils/augmentations.py:304-341) on tests/classify_ref.source(case),
                       then Normalize.  The shim stubs torchvision, so this script applies Normalize's published `sub(mean).div(std)` in fp32 itself, and
                       cv2.resize is the project's restatement (oracle/thirdparty.py): both are parity unpinned in the project's sense.
  keys                 state-dict keys of the reference's ClassificationModel(model=DetectionModel(yolov5n), nc=10, cutoff=10), newline-joined
  logits64_{sq,rect}   the reference model in float64 on tests/classify_ref.model_input(...), weights tests/classify_ref.cls_state_dict()
  logits16_{sq,rect}   the reference's own `.half()` forward on the CPU (its error from logits64 is the noise the fp16 plan is held to, times two)
  s_logits64           yolov5s-cls shape (nc = 10) at 224 x 224, batch 2, float64
  val_labels, val_triple_{0,1}, val_rows_{0,1}
                       classify/val.py `run` (model=, dataloader=, criterion=smartCrossEntropyLoss(eps)) of the fp32 reference model over three batches
                       (2, 2, 1 images): labels, (top1, top5, loss) and the verbose per-class rows (images, top1, top5; NaN for an absent class) for
                       label smoothing 0 and 0.1
"""
import copy
import logging
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402
from tests import classify_ref as cr  # noqa: E402


def ref_model(ns, name, nc):
    m = ns.yolo.ClassificationModel(model=ns.yolo.DetectionModel(os.path.join(ns.root, f"models/{name}.yaml")), nc=nc, cutoff=10)
    m.load_state_dict(cr.cls_state_dict(name, nc))
    return m.eval()


def main():
    ns = ref_shim.load()
    out = {}
    mean = torch.tensor(cr.IMAGENET_MEAN, dtype=torch.float32).view(3, 1, 1)
    std = torch.tensor(cr.IMAGENET_STD, dtype=torch.float32).view(3, 1, 1)
    crop, tot = ns.augmentations.CenterCrop(cr.S), ns.augmentations.ToTensor()
    for name in cr.TRANSFORM_CASES:
        im, _ = cr.source(name)
        t = tot(crop(im))
        assert t.dtype == torch.float32 and tuple(t.shape) == (3, cr.S, cr.S)
        out[f"tf_{name}"] = t.sub(mean).div(std).numpy()
        assert np.array_equal(out[f"tf_{name}"], cr.transform_restated(im, cr.S)), name

    m = ref_model(ns, "yolov5n", cr.MODEL_NC)
    assert len(m.model) == 10 and type(m.model[-1]).__name__ == "Classify" and m.model[-1].f == -1 and m.model[-1].i == 9
    out["keys"] = np.array("\n".join(m.state_dict().keys()))
    with torch.no_grad():
        for key in cr.MODEL_INPUTS:
            x = cr.model_input(key)
            ref = copy.deepcopy(m).double()(x.double()).numpy()     # (copies: .half() would round the weights every later result is made with)
            half = copy.deepcopy(m).half()(x.half()).float().numpy()
            out[f"logits64_{key}"], out[f"logits16_{key}"] = ref, half.astype(np.float16)
            err = np.abs(half - ref)
            s = -np.sort(-ref, axis=1)[:, :6]
            print(key, "logits", ref.min(), ref.max(), "half forward error max", err.max(), "mean", err.mean(), "smallest top-6 gap", (s[:, :-1] - s[:, 1:]).min())
        ms = ref_model(ns, "yolov5s", cr.MODEL_NC)
        xs = torch.from_numpy(cr.detgen.uniform((2, 3, 224, 224), 0.0, 1.0, name="img", seed=5))
        out["s_logits64"] = ms.double()(xs.double()).numpy()
        print("yolov5s-cls 224", out["s_logits64"].min(), out["s_logits64"].max())

        # classify/val.py on a three-batch loader; labels placed at chosen ranks of the reference's own ranking (hits, top-5 hits and misses)
        batches = cr.val_inputs()
        rank = torch.cat([m(b) for b in batches]).argsort(1, descending=True)
        labels = torch.stack([rank[i, r] for i, r in enumerate((0, 3, 7, 0, 5))])
        out["val_labels"] = labels.numpy().astype(np.int64)
        cwd = os.getcwd()
        os.chdir(ns.root)
        try:
            import classify.val as cval
        finally:
            os.chdir(cwd)
        cval.TQDM = lambda it, *a, **k: it
        rows = []
        handler = logging.Handler()
        handler.emit = lambda rec: rows.append(rec.getMessage())
        cval.LOGGER.addHandler(handler)
        cval.LOGGER.setLevel(logging.INFO)
        m.names = {i: f"class{i}" for i in range(cr.MODEL_NC)}
        loader = types.SimpleNamespace(dataset=types.SimpleNamespace(root=types.SimpleNamespace(stem="val"), samples=list(range(5))))

        class Loader:
            dataset = loader.dataset

            def __len__(self):
                return len(batches)

            def __iter__(self):
                return iter((b, labels[2 * i:2 * i + len(b)]) for i, b in enumerate(batches))

        for k, eps in enumerate((0.0, 0.1)):
            rows.clear()
            top1, top5, loss = cval.run(model=m, dataloader=Loader(), criterion=ns.torch_utils.smartCrossEntropyLoss(eps), verbose=True)
            out[f"val_triple_{k}"] = np.array([top1, top5, float(loss)], np.float64)
            per = [r.split() for r in rows if r.split() and r.split()[0].startswith("class")]
            assert len(per) == cr.MODEL_NC, rows
            out[f"val_rows_{k}"] = np.array([[float(v) for v in r[1:4]] for r in per], np.float64)
            print("val eps", eps, out[f"val_triple_{k}"])
        cval.LOGGER.removeHandler(handler)

    path = os.path.join(ROOT, "tests", "golden", "classify.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))

    # a tiny classification checkpoint pickled under the REFERENCE's class paths (models.yolo.ClassificationModel, models.common.Classify),
    # fp16 like train.py's, following tests/golden/ckpt_ref_tiny.pt; its own fp32 logits on model_input("sq") for the loading test
    from oracle.make_golden import TINY_CFG, load_det_weights
    torch.manual_seed(0)
    det = ns.yolo.DetectionModel(copy.deepcopy(TINY_CFG))
    load_det_weights(det, 11)
    tiny = ns.yolo.ClassificationModel(model=det, nc=4, cutoff=10)
    sd = tiny.state_dict()
    for k, v in cr.cls_state_dict("yolov5n", 4).items():
        if k.startswith("model.9.linear") or (k.startswith("model.9.") and sd[k].shape == v.shape):
            sd[k] = v
    tiny.load_state_dict(sd)
    tiny.names = {i: f"class{i}" for i in range(4)}
    ckpt = {"epoch": 1, "best_fitness": 0.5, "model": copy.deepcopy(tiny).half(), "ema": None, "updates": 3, "optimizer": None, "opt": {"imgsz": 64},
            "git": None, "date": "2026-01-01T00:00:00"}
    cpath = os.path.join(ROOT, "tests", "golden", "ckpt_ref_cls_tiny.pt")
    torch.save(ckpt, cpath)
    mm = torch.load(cpath, map_location="cpu", weights_only=False)["model"].float().fuse().eval()
    with torch.no_grad():
        z = mm(cr.model_input("sq"))
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "ckpt_ref_cls_tiny.npz"), logits=z.numpy(), keys=np.array("\n".join(mm.state_dict().keys())))
    print(cpath, os.path.getsize(cpath), z.shape)


if __name__ == "__main__":
    main()
