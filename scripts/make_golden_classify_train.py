"""Writes tests/golden/classify_train.npz from the UNMODIFIED reference, imported read-only through oracle.ref_shim on torch-CPU.  Needs the
reference checkout; no test runs this.

    python scripts/make_golden_classify_train.py

Model: the reference's ClassificationModel(model=DetectionModel(yolov5n), nc=10, cutoff=10) with tests/classify_ref.cls_state_dict() weights, train
mode, Dropout 0 (the reference's Dropout streams cannot be reproduced).  Inputs and labels: tests/classify_train_ref.py.

  (a) one step in float64 on step_input() with STEP_LABELS
      a_logits, a_loss0, a_loss1      logits; smartCrossEntropyLoss(0) and (0.1) of them (the gradients below are those of the 0.1 loss)
      names                           parameter names, newline-joined, in named_parameters() order
      a_norm (P), a_proj (P, 4)       per parameter: L2 norm of the gradient and its inner products with classify_train_ref.projections(name, numel)
      a_grad_{name}                   the whole gradient for the names of classify_train_ref.FULL_GRADS
      a_rm, a_rv                      the head BatchNorm's running statistics after the step (model.9.conv.bn)
  (b) the same step by the reference's own fp32 model (b32_*) and, where CPU torch runs it, by `.half()` (b16_*; b16_ok = 0 otherwise): their
      distance from (a) is the noise scale of the reference itself
  (c) a 3-epoch x 2-batch trajectory on classify_ref.val_inputs()[:2] with TRAJ_LABELS: the reference's model, smart_optimizer, ModelEMA,
      smartCrossEntropyLoss(0.1) and linear schedule in the order of classify/train.py:200-252 (no AMP on the CPU: GradScaler is disabled there),
      with SGD and with Adam, in float64 and in float32:
      c_{SGD,Adam}_{64,32}_losses (6), _lr (3: optimizer.param_groups[0]["lr"] behind each scheduler.step()), _bias, _ema_bias (final linear.bias)
"""
import copy
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402
from tests import classify_ref as cr  # noqa: E402
from tests import classify_train_ref as ct  # noqa: E402


def ref_model(ns):
    m = ns.yolo.ClassificationModel(model=ns.yolo.DetectionModel(os.path.join(ns.root, "models/yolov5n.yaml")), nc=cr.MODEL_NC, cutoff=10)
    m.load_state_dict(cr.cls_state_dict("yolov5n", cr.MODEL_NC))
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    for p in m.parameters():
        p.requires_grad = True
    return m.train()


def one_step(ns, m, x, labels):
    logits = m(x)
    loss0 = ns.torch_utils.smartCrossEntropyLoss(0.0)(logits.float() if logits.dtype == torch.float16 else logits, labels)
    loss1 = ns.torch_utils.smartCrossEntropyLoss(0.1)(logits.float() if logits.dtype == torch.float16 else logits, labels)
    loss1.backward()
    out = dict(logits=logits.detach().double().numpy(), loss0=float(loss0), loss1=float(loss1))
    names, norms, proj = [], [], []
    for n, p in m.named_parameters():
        g = p.grad.detach().double().numpy().ravel()
        names.append(n)
        norms.append(np.linalg.norm(g))
        proj.append(ct.projections(n, g.size) @ g)
        if n in ct.FULL_GRADS:
            out["grad_" + n] = p.grad.detach().double().numpy()
    out["norm"], out["proj"], out["names"] = np.array(norms), np.array(proj), names
    bn = m.model[9].conv.bn
    out["rm"], out["rv"] = bn.running_mean.detach().double().numpy(), bn.running_var.detach().double().numpy()
    return out


def trajectory(ns, name, dtype):
    m = ref_model(ns).to(dtype)
    batches = [b.to(dtype) for b in cr.val_inputs()[:2]]
    labels = [torch.tensor(l, dtype=torch.int64) for l in ct.TRAJ_LABELS]
    epochs = ct.TRAJ_EPOCHS
    optimizer = ns.torch_utils.smart_optimizer(m, name, ct.TRAJ_ARGS["lr0"], momentum=0.9, decay=ct.TRAJ_ARGS["decay"])
    lrf = 0.01
    scheduler = torch.optim.lr_scheduler.LambdaLR(optimizer, lr_lambda=lambda x: (1 - x / epochs) * (1 - lrf) + lrf)
    ema = ns.torch_utils.ModelEMA(m)
    criterion = ns.torch_utils.smartCrossEntropyLoss(label_smoothing=ct.TRAJ_ARGS["label_smoothing"])
    losses, lrs = [], []
    for _ in range(epochs):
        m.train()
        for x, y in zip(batches, labels):
            loss = criterion(m(x), y)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(m.parameters(), max_norm=10.0)
            optimizer.step()
            optimizer.zero_grad()
            ema.update(m)
            losses.append(float(loss))
        scheduler.step()
        lrs.append(optimizer.param_groups[0]["lr"])
    return dict(losses=np.array(losses), lr=np.array(lrs), bias=m.model[9].linear.bias.detach().double().numpy(),
                ema_bias=ema.ema.model[9].linear.bias.detach().double().numpy())


def main():
    ns = ref_shim.load()
    out = {}
    x, labels = ct.step_input(), torch.tensor(ct.STEP_LABELS, dtype=torch.int64)
    a = one_step(ns, ref_model(ns).double(), x.double(), labels)
    out["names"] = np.array("\n".join(a.pop("names")))
    for k, v in a.items():
        out["a_" + k] = np.asarray(v)
    b = one_step(ns, ref_model(ns), x, labels)
    b.pop("names")
    for k, v in b.items():
        out["b32_" + k] = np.asarray(v)
    rel = lambda u, v: float(np.linalg.norm(u - v) / np.linalg.norm(v))
    print("fp32 reference vs fp64: loss", abs(b["loss1"] - a["loss1"]) / a["loss1"], "worst norm", np.abs(b["norm"] / a["norm"] - 1).max(),
          "stored gradients", {n: rel(b["grad_" + n], a["grad_" + n]) for n in ct.FULL_GRADS})
    try:
        h = one_step(ns, ref_model(ns).half(), x.half(), labels)
        h.pop("names")
        for k, v in h.items():
            out["b16_" + k] = np.asarray(v)
        out["b16_ok"] = np.array(1)
        print("half reference vs fp64: loss", abs(h["loss1"] - a["loss1"]) / a["loss1"], "worst norm", np.abs(h["norm"] / a["norm"] - 1).max(),
              "stored gradients", {n: rel(h["grad_" + n], a["grad_" + n]) for n in ct.FULL_GRADS})
    except RuntimeError as e:   # CPU torch without a half kernel for some op of the step
        out["b16_ok"] = np.array(0)
        print("half reference step not available on this CPU torch:", e)

    for name in ("SGD", "Adam"):
        t64, t32 = trajectory(ns, name, torch.float64), trajectory(ns, name, torch.float32)
        for tag, t in (("64", t64), ("32", t32)):
            for k, v in t.items():
                out[f"c_{name}_{tag}_{k}"] = v
        dev = {k: float(np.abs(t32[k] - t64[k]).max()) for k in ("losses", "bias", "ema_bias")}
        # the trajectory test allows 4 x these; were the two runs bit-equal at this size, the test takes the project's rtol 1e-4 instead
        print(name, "losses", t64["losses"], "lr", t64["lr"], "largest deviation of the fp32 run from the fp64 run", dev,
              "(zero: bit-equal)" if not any(dev.values()) else "")

    path = os.path.join(ROOT, "tests", "golden", "classify_train.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
