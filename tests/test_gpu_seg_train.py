"""GPU: segmentation training -- model.train(); (p, proto) = model(imgs); loss, items = ComputeLoss(model, overlap=True)((p, proto), targets,
masks); loss.backward() (segment/train.py:355,381,391) -- against torch autograd over the CPU oracle's Segment forward plus the restated
segmentation loss (tests/seg_loss_ref.py), and train_loop.train on a small synthetic segmentation set."""
import numpy as np
import pytest
import torch

from oracle import detgen, yolo_oracle as yo
from tests import seg_loss_ref as sr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _model(name, dev):
    from yolov5_amd.yolo import SegmentationModel

    cfg = yo.model_cfg(name)
    sd = yo.det_state_dict(cfg, 0, fused=False)
    m = SegmentationModel(name + ".yaml")
    m.load_state_dict(sd)
    m.hyp = dict(yo.HYP_SCRATCH_LOW)
    return m.to(dev).train(), cfg, sd


def _data(B, S, per, seed):
    x = torch.from_numpy(detgen.uniform((B, 3, S, S), 0.0, 1.0, name="simg", seed=seed))
    t = detgen.synth_targets(B, per, seed=seed)
    t[:, 4:6] += 0.05
    masks = sr._masks(t, B, S // 4, S // 4, True, seed)
    return x, torch.from_numpy(t), torch.from_numpy(masks)


def _step(m, x, t, masks, dev):
    from yolov5_amd.segment_loss import ComputeLoss

    for q in m.parameters():
        q.grad = None
    p, proto = m(x.to(dev))
    loss, items = ComputeLoss(m, overlap=True)((p, proto), t.to(dev), masks.to(dev))
    loss.backward()
    torch.cuda.synchronize()
    return p, proto, loss, items


def test_fp32_seg_training_plan_exact_gradients_vs_oracle_autograd(dev):
    m, cfg, sd = _model("yolov5n-seg", dev)
    B, S = 4, 128
    x, t, masks = _data(B, S, 5, 9)
    p, proto, loss, items = _step(m, x, t, masks, dev)
    assert isinstance(p, list) and len(p) == 3 and p[0].dtype == torch.float32 and p[0].shape == (B, 3, S // 8, S // 8, 117)
    assert proto.shape == (B, 32, S // 4, S // 4) and proto.dtype == torch.float32
    sdo, leaves = {}, {}
    for k, v in sd.items():
        sdo[k] = v.clone()
        if v.dtype.is_floating_point and not k.endswith(("running_mean", "running_var", "anchors")):
            sdo[k] = v.clone().requires_grad_(True)
            leaves[k] = sdo[k]
    rp, rproto = yo.model_forward(cfg, sdo, x, training=True, bn_batch_stats=True)
    rloss, ritems = sr.seg_loss(rp, rproto, t, masks, 80, True, anchors=yo.model_anchors(cfg))
    rloss.backward()
    for a, b in zip(p, rp):
        np.testing.assert_allclose(a.detach().cpu().numpy(), b.detach().numpy(), rtol=1e-3, atol=1e-3)
    np.testing.assert_allclose(proto.detach().cpu().numpy(), rproto.detach().numpy(), rtol=1e-3, atol=1e-3)
    np.testing.assert_allclose(loss.item(), rloss.item(), rtol=1e-4)
    np.testing.assert_allclose(items.cpu().numpy(), ritems.numpy(), rtol=1e-4, atol=1e-7)
    worst = 0.0
    for n, q in m.named_parameters():
        assert q.grad is not None, n
        a, b = q.grad.cpu().flatten().double(), leaves[n].grad.flatten().double()
        rel = float((a - b).norm() / (b.norm() + 1e-30))
        worst = max(worst, rel)
        assert rel < 1e-3, (n, rel)
    assert any(n.startswith("model.24.proto") for n in leaves)
    for name, mod in m.named_modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            np.testing.assert_allclose(mod.running_var.cpu().numpy(), sdo[name + ".running_var"].numpy(), rtol=1e-4, atol=1e-6)
            np.testing.assert_allclose(mod.running_mean.cpu().numpy(), sdo[name + ".running_mean"].numpy(), rtol=1e-4, atol=1e-6)
    print(f"\n[seg train fp32] yolov5n-seg bs={B} {S}^2: loss {loss.item():.6f} vs oracle {rloss.item():.6f}; worst relative L2 over "
          f"{len(leaves)} parameter gradients {worst:.2e}")


def test_fp16_seg_training_plan_within_envelope_of_fp32_plan(dev):
    """yolov5s-seg, 16 x 640^2: the fp16 (AMP) plan's loss and every parameter gradient against the fp32 plan on the same weights / batch.
    fp16 storage of the activations makes the step a discontinuous function of its inputs (see test_gpu_train.py), so the bound is an
    envelope: loss within 2e-2, median relative L2 over the parameters < 0.35, every gradient finite with cosine > 0.5."""
    m, cfg, sd = _model("yolov5s-seg", dev)
    B, S = 16, 640
    x, t, masks = _data(B, S, 6, 11)
    _, _, l32, i32 = _step(m, x, t, masks, dev)
    g32 = {n: q.grad.float().cpu().clone() for n, q in m.named_parameters()}
    m.load_state_dict(sd)  # the fp32 step moved the BatchNorm running statistics only; restore them
    _, proto16, l16, i16 = _step(m, x.half(), t, masks, dev)
    assert proto16.dtype == torch.float16
    assert np.isfinite(l16.item()) and abs(l16.item() / l32.item() - 1) < 2e-2
    np.testing.assert_allclose(i16.float().cpu().numpy(), i32.cpu().numpy(), rtol=5e-2, atol=1e-4)
    rels, worst_cos = [], 1.0
    for n, q in m.named_parameters():
        a, b = q.grad.float().cpu().flatten().double(), g32[n].flatten().double()
        assert torch.isfinite(a).all(), n
        rels.append(float((a - b).norm() / (b.norm() + 1e-30)))
        cos = float(a @ b / (a.norm() * b.norm() + 1e-30))
        worst_cos = min(worst_cos, cos)
        assert cos > 0.5, (n, cos)
    med = float(np.median(rels))
    print(f"\n[seg train fp16] yolov5s-seg bs={B} {S}^2: loss {l16.item():.5f} vs fp32 plan {l32.item():.5f}; gradient relative L2 median "
          f"{med:.3f}, max {max(rels):.3f}; worst cosine {worst_cos:.3f}")
    assert med < 0.35


def test_train_loop_segmentation_lseg_falls(dev):
    """train_loop.train on a Segment model: (imgs, targets, paths, shapes, masks) batches, the segmentation loss with overlap=True,
    four loss items per step; lseg falls over the epochs, the scaler stays finite, val_loader raises (mask mAP is not implemented)."""
    from yolov5_amd import train_loop

    m, cfg, sd = _model("yolov5n-seg", dev)
    B, S, nb = 4, 128, 4
    batches = []
    for k in range(nb):
        x, t, masks = _data(B, S, 3, 30 + k)
        batches.append(((x * 255).round().to(torch.uint8), t, None, None, masks))
    with pytest.raises(NotImplementedError):
        train_loop.train(m, batches, epochs=1, val_loader=batches)
    m, cfg, sd = _model("yolov5n-seg", dev)
    hyp = dict(train_loop.HYP_SCRATCH_LOW)
    out = train_loop.train(m, batches, hyp=hyp, epochs=6, nbs=B, ema=True)
    losses = out["losses"]
    assert losses.shape == (6 * nb, 4) and torch.isfinite(losses).all()
    lseg = out["mloss"][:, 1]
    print(f"\n[seg train_loop] lseg per epoch {[round(float(v), 5) for v in lseg]}; scale {out['scaler'].scale}")
    assert lseg[-1] < 0.9 * lseg[0]
    assert np.isfinite(float(out["scaler"].scale)) and out["scaler"].scale > 0
