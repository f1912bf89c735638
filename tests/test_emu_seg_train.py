"""CPU: the training plan of a Segment model (Proto output, dproto back into proto.cv3 and the shared P3 feature) on the HIP emulator, fp32,
against torch autograd over the CPU oracle's Segment forward (a tiny model: oracle/make_golden.py:TINY_CFG with a Segment head)."""
import copy

import numpy as np
import torch

from oracle import detgen, yolo_oracle as yo
from tests.hipemu.backend import EmuBackend
from yolov5_amd.train_engine import TrainEngine
from yolov5_amd.yolo import SegmentationModel


def _seg_cfg():
    from oracle.make_golden import TINY_CFG

    cfg = copy.deepcopy(TINY_CFG)
    f, n, _, args = cfg["head"][-1]
    cfg["head"][-1] = [f, n, "Segment", list(args[:2]) + [8, 16]]
    return cfg


def test_fp32_seg_training_plan_vs_oracle_autograd():
    cfg = _seg_cfg()
    sd = yo.det_state_dict(cfg, 4, fused=False)
    m = SegmentationModel(copy.deepcopy(cfg))
    m.load_state_dict(sd)
    m.train()
    B, S = 2, 64
    x = torch.from_numpy(detgen.uniform((B, 3, S, S), 0.0, 1.0, name="img", seed=4))
    eng = TrainEngine(m, (B, 3, S, S), "cpu", backend=EmuBackend(), dtype=torch.float32)
    outs = [eng.be.to_torch(o) for o in eng.forward(x)]
    assert eng.seg and len(outs) == 4 and outs[-1].shape == (B, 8, S // 4, S // 4)
    sdo, leaves = {}, {}
    for k, v in sd.items():
        sdo[k] = v.clone()
        if v.dtype.is_floating_point and not k.endswith(("running_mean", "running_var", "anchors")):
            sdo[k] = v.clone().requires_grad_(True)
            leaves[k] = sdo[k]
    rp, rproto = yo.model_forward(cfg, sdo, x, training=True, bn_batch_stats=True)
    ref = list(rp) + [rproto]
    for a, b in zip(outs, ref):
        np.testing.assert_allclose(a.numpy(), b.detach().numpy(), rtol=2e-4, atol=2e-4)
    rs = [torch.from_numpy(detgen.uniform(tuple(b.shape), -1, 1, name=f"sup{i}", seed=5)) for i, b in enumerate(ref)]
    sum((b * r).sum() for b, r in zip(ref, rs)).backward()
    grads = eng.backward(rs)
    names = [n for n, _ in m.named_parameters()]
    assert any(".proto." in n for n in names)
    for n, g in zip(names, grads):
        rg = leaves[n].grad
        rel = float((g.double() - rg.double()).norm() / (rg.double().norm() + 1e-30))
        assert rel < 1e-3, (n, rel)
