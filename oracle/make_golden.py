"""TEST INFRASTRUCTURE ONLY -- never imported by the product path (yolov5_amd/).

Generates tests/golden/*.npz by running the UNMODIFIED reference (imported from /root/reference via
oracle/ref_shim.py) on deterministic synthetic inputs (oracle/detgen.py).  Run in the build container:

    python -m oracle.make_golden            # rewrites tests/golden/

Inputs and weights are NOT stored: they are regenerated from (name, seed) by detgen on any machine.
Only expected outputs (full when small, strided samples + float64 checksums when large, or quantized with a
recorded error bound that the tests subtract from their tolerance: gen_crosscheck) are committed.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

from . import detgen, ref_shim

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")


def load_det_weights(model, seed=0):
    """Overwrite every parameter/buffer of a reference model with detgen values (anchors kept)."""
    sd = model.state_dict()
    new = detgen.fill_state_dict(sd, seed)
    for k, v in new.items():
        if v is not None:
            sd[k] = torch.from_numpy(v).to(sd[k].dtype)
    model.load_state_dict(sd)
    return model


def summarize(t: np.ndarray, stride: int):
    flat = t.reshape(-1, t.shape[-1]).astype(np.float64)
    return {"rows": t.reshape(-1, t.shape[-1])[::stride].astype(np.float32),
            "sum": np.array([flat.sum(), np.abs(flat).sum(), (flat * flat).sum()])}


def gen_forward(ns, name, yaml_rel, hw, bs, seed, row_stride, seg=False):
    torch.manual_seed(0)
    Model = ns.yolo.SegmentationModel if seg else ns.yolo.DetectionModel
    m = Model(os.path.join(ns.root, yaml_rel))
    load_det_weights(m, seed)
    m.eval()
    x = torch.from_numpy(detgen.uniform((bs, 3, hw, hw), 0.0, 1.0, name="img", seed=seed))
    out = {"nparams": np.array(sum(p.numel() for p in m.parameters()))}
    with torch.no_grad():
        y = m(x)
        z_unfused = y[0].numpy()
        raws = y[2] if seg else y[1]
        m.fuse()
        y2 = m(x)
    z_fused = y2[0].numpy()
    out["anchors"] = m.model[-1].anchors.numpy()
    out["stride"] = m.model[-1].stride.numpy()
    if row_stride == 1:
        out["z_unfused"] = z_unfused
        out["z_fused"] = z_fused
        for i, r in enumerate(raws):
            out[f"raw{i}"] = r.numpy()
    else:
        s = summarize(z_unfused, row_stride)
        out["z_unfused_rows"], out["z_unfused_sum"] = s["rows"], s["sum"]
        s = summarize(z_fused, row_stride)
        out["z_fused_rows"], out["z_fused_sum"] = s["rows"], s["sum"]
    out["row_stride"] = np.array(row_stride)
    if seg:
        proto = y2[1].numpy()
        out["proto_sum"] = np.array([proto.astype(np.float64).sum(), np.abs(proto.astype(np.float64)).sum()])
        out["proto_sample"] = proto[:, :, ::5, ::5]
    # Detect grid / anchor_grid exactly as the reference cached them (yolo.py:117-128)
    det = m.model[-1]
    for i in range(det.nl):
        out[f"grid{i}"] = det.grid[i][0, 0].numpy()
        out[f"anchor_grid{i}"] = det.anchor_grid[i][0, :, 0, 0].numpy()
    np.savez_compressed(os.path.join(OUT, f"fwd_{name}.npz"), **out)
    print("fwd", name, z_fused.shape, float(np.abs(z_fused - z_unfused).max()))
    return m


def head_affine_from_logits(raws, nc, obj=(-2.5, 1.0), cls=(-1.0, 0.7), xy=(0.0, 1.0), wh=(0.0, 0.7)):
    """Per (anchor, output) affine that gives the objectness / class LOGITS of a random-init head a trained-looking spread: measured
    mean / std over all positions of the raw (bs, na, ny, nx, no) maps -> target N(mean, std) for the box (anchor-sized boxes
    instead of pixel-thin ones), objectness and class rows; mask-coefficient rows untouched.
    Round 3 targets: objectness N(-2.5, 1) and class N(-1, 0.7).  The round-2 targets (objectness N(-6, 2), class N(-1.5, 1.5)) selected
    candidates 2.5 sigma out in a heavy-tailed distribution -- exactly the positions where the feature norm, hence EVERY logit, is inflated:
    on candidate rows the class logits had std 4.9, 7-22 classes per row sat above 0.99 and the top-1 / top-2 gap was 2e-5, so the class
    argmax was a coin flip at fp16 resolution (38 % of the reference's own fp16 detections changed class).
    Returns [(scale (na*no,), shift (na*no,))] per level, logit_new = scale * logit_old + shift."""
    out = []
    for r in raws:
        na, no = r.shape[1], r.shape[4]
        m = r.mean(dim=(0, 2, 3)).double()                      # (na, no)
        sd = r.std(dim=(0, 2, 3)).double().clamp_min(1e-6)
        scale = torch.ones(na, no, dtype=torch.float64)
        shift = torch.zeros(na, no, dtype=torch.float64)
        for cols, (tm, ts) in ((slice(0, 2), xy), (slice(2, 4), wh), (slice(4, 5), obj), (slice(5, 5 + nc), cls)):
            scale[:, cols] = ts / sd[:, cols]
            shift[:, cols] = tm - m[:, cols] * scale[:, cols]
        out.append((scale.reshape(-1).float(), shift.reshape(-1).float()))
    return out


def gen_detset(ns, name, yaml_rel, hw, bs, seed, row_stride, seg=False, conf=0.25, iou=0.45, max_det=1000, bn_gamma_scale=0.2, cal_scenes=0):
    """BASELINE configs C2 / C4 / C5 at their real resolution: the REFERENCE's fused fp32 forward and its own non_max_suppression
    on a conditioned network (detgen.condition_state_dict: BatchNorm statistics calibrated on the input, head logits spread) ->
    strided z rows + checksums, the statistics / head affine that were applied (the tests apply the same ones) and the detections per image (the detection-set agreement target for the fp16 HIP path)."""
    torch.manual_seed(0)
    Model = ns.yolo.SegmentationModel if seg else ns.yolo.DetectionModel
    m = Model(os.path.join(ns.root, yaml_rel))
    load_det_weights(m, seed)
    det = m.model[-1]
    x = torch.from_numpy(detgen.scene((bs, 3, hw, hw), seed=seed))
    out = {}
    with torch.no_grad():
        # BatchNorm calibration: one train-mode pass with momentum 1 -> running statistics := batch statistics of this input
        bns = [b for b in m.modules() if isinstance(b, torch.nn.BatchNorm2d)]
        for b in bns:
            b.momentum = 1.0
            b.weight.mul_(bn_gamma_scale)   # ordered regime (detgen.condition_state_dict): the tests apply the same factor
        out["bn_gamma_scale"] = np.array(bn_gamma_scale, dtype=np.float64)
        m.train()
        # cal_scenes > 0 (yolov5x, round 4): the statistics are those of the fixture image AND `cal_scenes` unrelated scenes (generator seed
        # 2000 + seed; the tests' own extra images use 1000 + seed).  Statistics of ONE image let any other scene drive some fp16 activation of
        # this 200-layer stack past 65504, so the bs = 16 plan test could only run shifted copies of the fixture image (parity 2).
        xc = x if not cal_scenes else torch.cat([x, torch.from_numpy(detgen.scene((cal_scenes, 3, hw, hw), seed=2000 + seed))], 0)
        out["cal_scenes"] = np.array(cal_scenes)
        m(xc)
        m.eval()
        out["bn_mean"] = torch.cat([b.running_mean.flatten() for b in bns]).numpy().astype(np.float32)
        out["bn_var"] = torch.cat([b.running_var.flatten() for b in bns]).numpy().astype(np.float32)
        y0 = m(x)
        aff = head_affine_from_logits(y0[2] if seg else y0[1], det.nc)
        for i, (mi, (sc, sh)) in enumerate(zip(det.m, aff)):
            new_b = (mi.bias.detach().float() * sc + sh).float()      # logit_new = sc * (w x + b) + sh
            mi.weight.mul_(sc.view(-1, 1, 1, 1))
            mi.bias.copy_(new_b)
            out[f"head_scale{i}"], out[f"head_bias{i}"] = sc.numpy(), new_b.numpy()
        m.fuse()
        y = m(x)
    z = y[0]
    out.update(row_stride=np.array(row_stride), shape=np.array(z.shape))
    sm = summarize(z.numpy(), row_stride)
    out["z_rows"], out["z_sum"] = sm["rows"], sm["sum"]
    nm = det.nm if seg else 0
    if seg:
        proto = y[1].numpy()
        out["proto_sum"] = np.array([proto.astype(np.float64).sum(), np.abs(proto.astype(np.float64)).sum()])
        out["proto_sample"] = proto[:, :, ::5, ::5]
    with ref_shim.oracle_nms_mode():
        res = ns.general.non_max_suppression(z.clone(), conf, iou, max_det=max_det, nm=nm)
    for i, r in enumerate(res):
        out[f"det{i}"] = r.numpy().astype(np.float32)
    out["nms"] = np.array([conf, iou, max_det], dtype=np.float64)
    # The same reference model in float64 (the "truth" both fp32 implementations are measured against: deep nets amplify
    # accumulation-order noise beyond 1e-4) and in float16 (what `model.half()` computes on torch-CPU: fp32 accumulation, fp16
    # storage -- the envelope an fp16 implementation of this network can be held to).
    import copy

    with torch.no_grad():
        z64 = copy.deepcopy(m).double()(x.double())[0]
        z16 = copy.deepcopy(m).half()(x.half())[0].float()
    out["z64_rows"] = z64.numpy().reshape(-1, z64.shape[-1])[::row_stride]
    out["z16_rows"] = z16.numpy().reshape(-1, z16.shape[-1])[::row_stride]
    with ref_shim.oracle_nms_mode():
        res16 = ns.general.non_max_suppression(z16.clone(), conf, iou, max_det=max_det, nm=nm)  # (fp32 arithmetic on the fp16 values)
    for i, r in enumerate(res16):
        out[f"det16_{i}"] = r.numpy().astype(np.float32)
    np.savez_compressed(os.path.join(OUT, f"detset_{name}.npz"), **out)
    print("detset", name, tuple(z.shape), [int(r.shape[0]) for r in res], [int(r.shape[0]) for r in res16],
          "fp32 vs fp64 max", float((z.double() - z64).abs().max()), "fp16 vs fp32 max", float((z16 - z).abs().max()))


def gen_fuse(ns):
    from torch import nn

    conv = nn.Conv2d(8, 16, 3, 1, 1, bias=False)
    bn = nn.BatchNorm2d(16)
    bn.eps = 1e-3
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(detgen.uniform((16, 8, 3, 3), -0.5, 0.5, name="fw")))
        bn.weight.copy_(torch.from_numpy(detgen.uniform((16,), 0.5, 1.5, name="fg")))
        bn.bias.copy_(torch.from_numpy(detgen.uniform((16,), -0.5, 0.5, name="fb")))
        bn.running_mean.copy_(torch.from_numpy(detgen.uniform((16,), -0.5, 0.5, name="fm")))
        bn.running_var.copy_(torch.from_numpy(detgen.uniform((16,), 0.5, 1.5, name="fv")))
        f = ns.torch_utils.fuse_conv_and_bn(conv, bn)
    np.savez_compressed(os.path.join(OUT, "fuse.npz"), w=f.weight.detach().numpy(), b=f.bias.detach().numpy())


NMS_CASES = {
    # name: (pred kwargs, nms kwargs)
    "default": (dict(bs=2, n=3000, no=85, obj_pow=8, seed=1), dict(conf_thres=0.25, iou_thres=0.45, max_det=1000)),
    "sparse": (dict(bs=3, n=2000, no=85, obj_pow=64, seed=2), dict(conf_thres=0.25, iou_thres=0.45, max_det=300)),
    "val_multilabel": (dict(bs=2, n=600, no=15, obj_pow=2, seed=3),
                       dict(conf_thres=0.001, iou_thres=0.6, multi_label=True, max_det=300)),
    "agnostic": (dict(bs=2, n=1500, no=85, obj_pow=4, seed=4), dict(conf_thres=0.25, iou_thres=0.45, agnostic=True, max_det=300)),
    "classes": (dict(bs=2, n=1500, no=85, obj_pow=4, seed=5), dict(conf_thres=0.25, iou_thres=0.45, classes=[0, 3, 17, 79], max_det=300)),
    "maxdet": (dict(bs=2, n=4000, no=85, obj_pow=2, seed=6), dict(conf_thres=0.1, iou_thres=0.45, max_det=50)),
    "masks": (dict(bs=2, n=1500, no=117, obj_pow=4, seed=7), dict(conf_thres=0.25, iou_thres=0.45, max_det=300, nm=32)),
    "ties": (dict(bs=2, n=3000, no=85, obj_pow=2, seed=8), dict(conf_thres=0.25, iou_thres=0.45, max_det=1000)),
    "empty": (dict(bs=2, n=500, no=85, obj_pow=64, seed=9), dict(conf_thres=0.999, iou_thres=0.45, max_det=300)),
    "clustered": (dict(bs=2, n=3000, no=85, obj_pow=3, seed=10), dict(conf_thres=0.25, iou_thres=0.45, max_det=300)),
    "clustered_agn": (dict(bs=2, n=3000, no=85, obj_pow=3, seed=10),
                      dict(conf_thres=0.25, iou_thres=0.45, max_det=300, agnostic=True)),
}


def nms_case_pred(name):
    kw, _ = NMS_CASES[name]
    p = detgen.synth_predictions(kw["bs"], kw["n"], kw["no"], obj_pow=kw["obj_pow"], seed=kw["seed"])
    if name == "ties":  # quantise obj and cls so that obj*cls products tie often (fp16-like behaviour)
        p[..., 4:] = np.round(p[..., 4:] * 16) / 16
    if name.startswith("clustered"):  # heavy overlap: boxes drawn around 12 centres so that NMS suppresses a lot
        c = detgen.uniform((12, 2), 80, 560, name="centres", seed=kw["seed"])
        idx = detgen.integers((kw["bs"], kw["n"]), 0, 12, name="cidx", seed=kw["seed"])
        p[..., 0:2] = c[idx] + (p[..., 0:2] / 640.0 - 0.5) * 30.0
        p[..., 2:4] = 60.0 + (p[..., 2:4] - 4.0) * 0.4
    return p


def gen_nms(ns):
    out = {}
    with ref_shim.oracle_nms_mode():
        for name, (kw, nkw) in NMS_CASES.items():
            p = torch.from_numpy(nms_case_pred(name))
            res = ns.general.non_max_suppression(p.clone(), **nkw)
            for i, r in enumerate(res):
                out[f"{name}_{i}"] = r.numpy().astype(np.float32)
            print("nms", name, [int(r.shape[0]) for r in res])
    np.savez_compressed(os.path.join(OUT, "nms.npz"), **out)


APPENDIX_A_TARGETS = np.array([[0, 5, .50, .50, .10, .20], [0, 7, .013, .98, .05, .05],
                               [0, 1, .30625, .70, .40, .40]], dtype=np.float32)


def loss_case(name):
    """(p list as np arrays, targets np) for the named loss fixture."""
    if name == "appendix_a":  # zero logits at 640^2, bs=1
        p = [np.zeros((1, 3, s, s, 85), dtype=np.float32) for s in (80, 40, 20)]
        return p, APPENDIX_A_TARGETS.copy()
    if name == "synthetic":  # bs=4 at 256^2 -> grids 32/16/8, 8 targets per image + boundary cases
        p = [detgen.uniform((4, 3, s, s, 85), -3.0, 3.0, name=f"p{s}", seed=11) for s in (32, 16, 8)]
        t = detgen.synth_targets(4, 8, seed=11)
        extra = np.array([[1, 2, 0.5, 0.5, 0.25, 0.25],       # exact integer grid coordinates on every level
                          [2, 3, 0.015, 0.985, 0.06, 0.05],    # near borders: gxy>1 guards + clamp
                          [3, 4, 0.999, 0.001, 0.10, 0.12],
                          [0, 5, 0.515625, 0.484375, 0.3, 0.02],  # extreme aspect: fails anchor_t on some anchors
                          [0, 6, 0.25, 0.75, 0.9, 0.9]], dtype=np.float32)
        return p, np.concatenate((t, extra), 0)
    if name == "no_targets":
        p = [detgen.uniform((2, 3, s, s, 85), -3.0, 3.0, name=f"q{s}", seed=12) for s in (16, 8, 4)]
        return p, np.zeros((0, 6), dtype=np.float32)
    raise KeyError(name)


def gen_loss(ns):
    import yaml

    torch.manual_seed(0)
    m = ns.yolo.DetectionModel(os.path.join(ns.root, "models/yolov5s.yaml"))
    with open(os.path.join(ns.root, "data/hyps/hyp.scratch-low.yaml")) as f:
        m.hyp = yaml.safe_load(f)
    cl = ns.loss.ComputeLoss(m)
    out = {"anchors": m.model[-1].anchors.numpy()}
    for name in ("appendix_a", "synthetic", "no_targets"):
        pn, tn = loss_case(name)
        p = [torch.from_numpy(a).clone().requires_grad_(True) for a in pn]
        t = torch.from_numpy(tn)
        tcls, tbox, indices, anch = cl.build_targets(p, t)
        loss, items = cl(p, t)
        loss.backward()
        out[f"{name}_loss"] = loss.detach().numpy()
        out[f"{name}_items"] = items.numpy()
        for i in range(3):
            out[f"{name}_idx{i}"] = torch.stack(indices[i]).numpy() if indices[i][0].numel() else np.zeros((4, 0), np.int64)
            out[f"{name}_tbox{i}"] = tbox[i].numpy()
            out[f"{name}_tcls{i}"] = tcls[i].numpy()
            out[f"{name}_anch{i}"] = anch[i].numpy()
            g = p[i].grad.numpy()
            if g.size > 400000:
                out[f"{name}_grad{i}_sum"] = np.array([g.astype(np.float64).sum(), np.abs(g.astype(np.float64)).sum()])
                nz = np.argwhere(np.abs(g[..., :4]).sum(-1) > 0)[:64]
                out[f"{name}_grad{i}_nzidx"] = nz
                out[f"{name}_grad{i}_nzrows"] = g[tuple(nz.T)] if len(nz) else np.zeros((0, 85), np.float32)
            else:
                out[f"{name}_grad{i}"] = g
        print("loss", name, loss.item(), items.tolist(), [int(ix[0].numel()) for ix in indices])
    np.savez_compressed(os.path.join(OUT, "loss.npz"), **out)
    # focal loss (hyp fl_gamma = 1.5, loss.py:120-122 -> FocalLoss :77-98) with label smoothing 0.1 on the synthetic case: loss, items, gradients
    fo = {}
    m.hyp = dict(m.hyp, fl_gamma=1.5, label_smoothing=0.1)
    clf = ns.loss.ComputeLoss(m)
    pn, tn = loss_case("synthetic")
    p = [torch.from_numpy(a).clone().requires_grad_(True) for a in pn]
    loss, items = clf(p, torch.from_numpy(tn))
    loss.backward()
    fo["loss"], fo["items"] = loss.detach().numpy(), items.numpy()
    for i in range(3):
        gq = p[i].grad.numpy()
        fo[f"grad{i}_sum"] = np.array([gq.astype(np.float64).sum(), np.abs(gq.astype(np.float64)).sum()])
        nz = np.argwhere(np.abs(gq[..., :4]).sum(-1) > 0)[:64]
        fo[f"grad{i}_nzidx"] = nz
        fo[f"grad{i}_nzrows"] = gq[tuple(nz.T)]
        fo[f"grad{i}_obj_head"] = gq[0, 0, :4, :8, 4].copy()   # objectness gradients of cells without targets too
    print("loss focal", loss.item(), items.tolist())
    np.savez_compressed(os.path.join(OUT, "loss_focal.npz"), **fo)


def gen_mask(ns):
    protos = torch.from_numpy(detgen.uniform((32, 40, 40), -1.0, 1.0, name="protos", seed=13))
    coef = torch.from_numpy(detgen.uniform((7, 32), -1.0, 1.0, name="coef", seed=13))
    xy1 = detgen.uniform((7, 2), 0, 90, name="bx1", seed=13)
    wh = detgen.uniform((7, 2), 8, 70, name="bwh", seed=13)
    boxes = torch.from_numpy(np.concatenate((xy1, xy1 + wh), 1))
    m0 = ns.seg_general.process_mask(protos, coef, boxes, (160, 160), upsample=False)
    m1 = ns.seg_general.process_mask(protos, coef, boxes, (160, 160), upsample=True)
    np.savez_compressed(os.path.join(OUT, "mask.npz"), m_noup=np.packbits(m0.numpy().astype(bool)),
                        m_up=np.packbits(m1.numpy().astype(bool)), shape_noup=np.array(m0.shape), shape_up=np.array(m1.shape))
    print("mask", m0.shape, m1.shape, float(m1.float().mean()))


def gen_scale_boxes(ns):
    b = detgen.uniform((20, 4), -20, 660, name="sb", seed=14)
    o = ns.general.scale_boxes((640, 640), torch.from_numpy(b.copy()), (1080, 810)).numpy()
    o2 = ns.general.scale_boxes((384, 640), torch.from_numpy(b.copy()), (720, 1280)).numpy()
    np.savez_compressed(os.path.join(OUT, "scale_boxes.npz"), a=o, b=o2)


def optim_grad(name, shape, step):
    """Deterministic synthetic gradient of parameter `name` at optimizer step `step` (shared with tests/test_emu_optim.py)."""
    return detgen.uniform(tuple(shape), -0.05, 0.05, name="g:" + name, seed=100 + step)


def gen_optim(ns):
    """utils/torch_utils.py:257-290 smart_optimizer + :343-369 ModelEMA of the REFERENCE on yolov5n, three steps of
    (synthetic gradients -> GradScaler-style unscale -> clip_grad_norm_(10.0) -> optimizer.step() -> ema.update(model)),
    train.py:413-421.  Stores strided samples + float64 checksums of every parameter / EMA tensor after step 3."""
    torch.manual_seed(0)
    m = ns.yolo.DetectionModel(os.path.join(ns.root, "models/yolov5n.yaml"))
    load_det_weights(m, 0)
    m.train()
    opt = ns.torch_utils.smart_optimizer(m, "SGD", 0.01, 0.937, 5e-4)
    ema = ns.torch_utils.ModelEMA(m, tau=4)   # short ramp so that three updates move the average visibly
    out = {"group_sizes": np.array([len(g["params"]) for g in opt.param_groups]),
           "group_decay": np.array([g["weight_decay"] for g in opt.param_groups]), "norms": []}
    S = 512.0
    for step in range(3):
        for i, g in enumerate(opt.param_groups):
            g["lr"] = 0.01 * (1.0 + 0.5 * i) / (1 + step)
        for k, p in m.named_parameters():
            p.grad = torch.from_numpy(optim_grad(k, p.shape, step)) * S
        for p in m.parameters():                      # scaler.unscale_
            p.grad.mul_(1.0 / S)
        out["norms"].append(float(torch.nn.utils.clip_grad_norm_(m.parameters(), max_norm=10.0)))
        opt.step()
        ema.update(m)
    out["norms"] = np.array(out["norms"])
    esd = ema.ema.state_dict()
    for k, p in m.state_dict().items():
        if not p.dtype.is_floating_point:
            continue
        a, e = p.detach().numpy().ravel(), esd[k].detach().float().numpy().ravel()
        out["p:" + k] = np.concatenate([a[::97], [a.astype(np.float64).sum()]]).astype(np.float64)
        out["e:" + k] = np.concatenate([e[::97], [e.astype(np.float64).sum()]]).astype(np.float64)
    np.savez_compressed(os.path.join(OUT, "optim.npz"), **out)


METRIC_CASES = {  # name: (images, labels per image, detections per label, false positives per image, classes, jitter px, seed)
    "sparse": dict(bs=3, nl=6, per=2, nfp=20, nc=5, jit=6.0, seed=21),
    "crowd": dict(bs=2, nl=40, per=5, nfp=60, nc=3, jit=10.0, seed=22),
    "full": dict(bs=4, nl=30, per=8, nfp=60, nc=80, jit=4.0, seed=23),
    "nolabel": dict(bs=2, nl=0, per=0, nfp=15, nc=4, jit=1.0, seed=24),
    "dups": dict(bs=2, nl=5, per=3, nfp=4, nc=2, jit=0.0, seed=25),  # jitter 0: exact duplicates, IoU ties
}
METRIC_SHAPES = [((480, 640), ((0.8, 0.8), (0.0, 64.0))), ((1080, 810), ((0.5925926, 0.5925926), (80.0, 0.0))),
                 ((300, 400), ((1.6, 1.6), (0.0, 80.0))), ((640, 640), ((1.0, 1.0), (0.0, 0.0)))]  # shapes[si] = (shape0, ratio_pad)


def metrics_case(name, max_det=300):
    """Synthetic validation batch: targets (M,6) [img, cls, cx, cy, w, h] in letterboxed 640x640 pixels (val.py:274) and
    NMS-shaped output rows (bs, max_det, 6) + counts: jittered copies of the labels (some with a wrong class) plus random
    false positives, ordered by descending confidence like non_max_suppression's output."""
    kw = METRIC_CASES[name]
    bs, nl, per, nfp, nc, seed = kw["bs"], kw["nl"], kw["per"], kw["nfp"], kw["nc"], kw["seed"]
    t = detgen.synth_targets(bs, nl, nc, seed=seed) if nl else np.zeros((0, 6), np.float32)
    if name == "crowd":  # heavy overlap between labels: centres squeezed into a band
        t[:, 2:4] = 0.4 + 0.2 * t[:, 2:4]
    t[:, 2:] *= np.float32(640)
    det = np.zeros((bs, max_det, 6), np.float32)
    cnt = np.zeros((bs,), np.int32)
    for si in range(bs):
        lab = t[t[:, 0] == si]
        rows = []
        if nl:
            j = detgen.uniform((nl, per, 4), -1.0, 1.0, name=f"jit{si}", seed=seed) * np.float32(kw["jit"])
            flip = detgen.uniform((nl, per), 0, 1, name=f"flip{si}", seed=seed) < 0.15
            for l in range(nl):
                for k in range(per):
                    cx, cy, w, h = lab[l, 2:6] + j[l, k] * np.array([1, 1, 0.5, 0.5], np.float32)
                    c = (lab[l, 1] + 1) % nc if flip[l, k] else lab[l, 1]
                    rows.append([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2, 0.0, c])
        fp = detgen.uniform((nfp, 4), 0, 1, name=f"fp{si}", seed=seed)
        fc = detgen.integers((nfp,), 0, nc, name=f"fpc{si}", seed=seed)
        for k in range(nfp):
            cx, cy, w, h = fp[k, 0] * 640, fp[k, 1] * 640, 8 + fp[k, 2] * 120, 8 + fp[k, 3] * 120
            rows.append([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2, 0.0, float(fc[k])])
        rows = np.array(rows, np.float32).reshape(-1, 6)
        conf = detgen.uniform((rows.shape[0],), 0.001, 1.0, name=f"conf{si}", seed=seed)
        rows[:, 4] = conf
        rows = rows[np.argsort(-conf, kind="stable")][:max_det]
        det[si, :rows.shape[0]] = rows
        cnt[si] = rows.shape[0]
    shapes = [METRIC_SHAPES[(si + seed) % len(METRIC_SHAPES)] for si in range(bs)]
    return det, cnt, t, shapes


def gen_metrics(ns):
    """val.py:282-307 + utils/metrics.py ap_per_class run by the reference's own functions on metrics_case batches."""
    out = {}
    iouv = torch.linspace(0.5, 0.95, 10)  # val.py:222
    stats = []
    for name in METRIC_CASES:
        det, cnt, t, shapes = metrics_case(name)
        targets = torch.from_numpy(t)
        for si in range(det.shape[0]):
            pred = torch.from_numpy(det[si, :cnt[si]].copy())
            labels = targets[targets[:, 0] == si, 1:]
            shape, ratio_pad = shapes[si]
            # direct process_batch on the letterboxed-space boxes (no de-letterbox)
            lab_xyxy = torch.cat((labels[:, 0:1], ns.general.xywh2xyxy(labels[:, 1:5])), 1)
            c0 = ns.metrics.process_batch(pred, lab_xyxy, iouv) if labels.shape[0] else torch.zeros(pred.shape[0], 10, dtype=torch.bool)
            # val.py:296-307
            predn = pred.clone()
            ns.general.scale_boxes((640, 640), predn[:, :4], shape, ratio_pad)
            correct = torch.zeros(pred.shape[0], 10, dtype=torch.bool)
            if labels.shape[0]:
                tbox = ns.general.xywh2xyxy(labels[:, 1:5])
                ns.general.scale_boxes((640, 640), tbox, shape, ratio_pad)
                correct = ns.metrics.process_batch(predn, torch.cat((labels[:, 0:1], tbox), 1), iouv)
            out[f"{name}_{si}_direct"] = np.packbits(c0.numpy())
            out[f"{name}_{si}_correct"] = np.packbits(correct.numpy())
            out[f"{name}_{si}_predn"] = predn[:, :4].numpy()
            stats.append((correct.numpy(), pred[:, 4].numpy(), pred[:, 5].numpy(), labels[:, 0].numpy()))
            print("metrics", name, si, int(pred.shape[0]), int(labels.shape[0]), correct.sum(0).tolist())
    tp, conf, pcls, tcls = (np.concatenate(x, 0) for x in zip(*stats))
    res = ns.metrics.ap_per_class(tp, conf, pcls, tcls, plot=False, names={})
    for k, v in zip(("tp", "fp", "p", "r", "f1", "ap", "cls"), res):
        out["ap_" + k] = np.asarray(v)
    print("ap_per_class", res[5].mean(0)[[0, -1]], res[5].shape)
    np.savez_compressed(os.path.join(OUT, "metrics.npz"), **out)


LETTERBOX_CASES = {  # name: ((h0, w0), kwargs of letterbox)
    "up": ((75, 100), dict(new_shape=128, auto=False)),
    "down": ((300, 200), dict(new_shape=128, auto=False)),
    "half": ((256, 192), dict(new_shape=128, auto=False)),  # exact 2x down-scale: cv2 re-routes INTER_LINEAR to INTER_AREA
    "pad_only": ((96, 128), dict(new_shape=128, auto=False)),
    "auto": ((90, 150), dict(new_shape=(96, 160), auto=True, stride=32)),
    "fill": ((60, 110), dict(new_shape=128, auto=False, scaleFill=True)),
    "noscaleup": ((50, 70), dict(new_shape=128, auto=False, scaleup=False)),
}
LETTERBOX_GEOMETRY = [((h, w), dict(new_shape=ns_, auto=a, scaleFill=f, scaleup=u, stride=st))
                      for (h, w) in [(480, 640), (1080, 810), (375, 500), (333, 500), (1280, 960), (427, 640), (640, 640), (17, 1000), (720, 1280)]
                      for ns_ in [640, (384, 640), 1280, 320]
                      for (a, f, u, st) in [(False, False, True, 32), (True, False, True, 32), (False, True, True, 32), (True, False, False, 64)]]


def letterbox_image(name):
    (h, w), _ = LETTERBOX_CASES[name]
    return detgen.integers((h, w, 3), 0, 256, name="lb_" + name, seed=51).astype(np.uint8)


def gen_letterbox(ns):
    """utils/augmentations.py letterbox (unmodified) on top of the restated cv2.resize / copyMakeBorder (oracle/thirdparty.py):
    pins the geometry and the padding; the resize arithmetic itself stays parity-unpinned."""
    out = {}
    for name, (_, kw) in LETTERBOX_CASES.items():
        im, ratio, pad = ns.augmentations.letterbox(letterbox_image(name), **kw)
        out[name] = im
        out[name + "_meta"] = np.array([ratio[0], ratio[1], pad[0], pad[1]], np.float64)
        print("letterbox", name, im.shape, ratio, pad)
    geo = []
    for (h, w), kw in LETTERBOX_GEOMETRY:
        im, ratio, pad = ns.augmentations.letterbox(np.zeros((h, w, 3), np.uint8), **kw)
        top = int(np.argmax((im[:, im.shape[1] // 2, 0] != 114))) if (im[:, :, 0] != 114).any() else -1
        left = int(np.argmax((im[im.shape[0] // 2, :, 0] != 114))) if (im[:, :, 0] != 114).any() else -1
        rows = int((im[:, im.shape[1] // 2, 0] != 114).sum())
        cols = int((im[im.shape[0] // 2, :, 0] != 114).sum())
        geo.append([im.shape[0], im.shape[1], ratio[0], ratio[1], pad[0], pad[1], top, left, rows, cols])
    out["geometry"] = np.array(geo, np.float64)
    np.savez_compressed(os.path.join(OUT, "letterbox.npz"), **out)


def gen_augment(ns):
    """The reference's own `LoadImagesAndLabels.__getitem__` (mosaic branch: load_mosaic -> random_perspective -> augment_hsv -> flips ->
    CHW / RGB) + `collate_fn` on a synthetic 6-image dataset, one batch per seed, with Python's / numpy's generators seeded so that
    oracle/augment_oracle.py:reference_draws reproduces the draws.  The dataset object is a bare namespace carrying exactly the
    attributes those methods read (no files, no cache)."""
    import types

    import utils.dataloaders as dl

    from . import augment_oracle as ao, thirdparty as tp

    dl.xywhn2xyxy, dl.xyxy2xywhn = tp.xywhn2xyxy, tp.xyxy2xywhn
    s = 96
    ims, labs = ao.synthetic_dataset(6, seed=3)
    hyp = dict(ao.HYP_AUG, degrees=5.0, shear=2.0, flipud=0.3)  # exercise rotation / shear / up-down flip too
    cls = dl.LoadImagesAndLabels
    ds = types.SimpleNamespace(img_size=s, mosaic=True, augment=True, hyp=hyp, mosaic_border=[-s // 2, -s // 2], rect=False,
                               indices=list(range(len(ims))), labels=[lb.astype(np.float32).copy() for lb in labs],
                               segments=[[] for _ in ims], ims=[None] * len(ims), im_files=[f"im{i}" for i in range(len(ims))],
                               npy_files=[types.SimpleNamespace(exists=lambda: False)] * len(ims), albumentations=lambda im, lb: (im, lb))
    ds.load_mosaic = types.MethodType(cls.load_mosaic, ds)

    def load_image(self, i):  # dataloaders.py:770-790 with cv2.imread replaced by the in-memory image
        im = ims[i]
        h0, w0 = im.shape[:2]
        r = self.img_size / max(h0, w0)
        if r != 1:
            im = dl.cv2.resize(im, (math.ceil(w0 * r), math.ceil(h0 * r)), interpolation=dl.cv2.INTER_LINEAR)
        return im, (h0, w0), im.shape[:2]

    import math
    import random

    ds.load_image = types.MethodType(load_image, ds)
    out = {"s": np.array(s)}
    for seed in (1, 2, 3, 4):
        batch = []
        for index in (seed % 6, (seed + 3) % 6):
            random.seed(seed * 10 + index)
            np.random.seed(seed * 10 + index)
            im, lab, _, _ = cls.__getitem__(ds, index)
            batch.append((im, lab, "", None))
        imb, labb, _, _ = cls.collate_fn(batch)
        out[f"img{seed}"], out[f"lab{seed}"] = imb.numpy(), labb.numpy()
        print("augment", seed, tuple(imb.shape), tuple(labb.shape))
    np.savez_compressed(os.path.join(OUT, "augment.npz"), **out)

    # hyp['mosaic'] = 0.5: the gate of dataloaders.py:701 sends about half of the samples down the letterbox branch (:710-733: load_image,
    # letterbox(auto=False, scaleup=True), float-pad labels, random_perspective with border (0, 0)); batches of three so that both branches meet
    ds.hyp = dict(hyp, mosaic=0.5)
    out = {"s": np.array(s)}
    for seed in (11, 12, 13, 14):
        batch, gates = [], []
        for index in (seed % 6, (seed + 2) % 6, (seed + 4) % 6):
            random.seed(seed * 10 + index)
            gates.append(random.random() < 0.5)
            random.seed(seed * 10 + index)
            np.random.seed(seed * 10 + index)
            im, lab, _, _ = cls.__getitem__(ds, index)
            batch.append((im, lab, "", None))
        imb, labb, _, _ = cls.collate_fn(batch)
        out[f"img{seed}"], out[f"lab{seed}"], out[f"mosaic{seed}"] = imb.numpy(), labb.numpy(), np.array(gates)
        print("augment mixed", seed, gates, tuple(imb.shape), tuple(labb.shape))
    np.savez_compressed(os.path.join(OUT, "augment_mixed.npz"), **out)

    # hyp['mixup'] = 0.5 (data/hyps/hyp.scratch-med.yaml has 0.1): dataloaders.py:707-708 blends a second mosaic into about half of the samples
    ds.hyp = dict(hyp, mixup=0.5)
    out = {"s": np.array(s)}
    for seed in (21, 22, 23, 24):
        batch = []
        for index in (seed % 6, (seed + 2) % 6, (seed + 4) % 6):
            random.seed(seed * 10 + index)
            np.random.seed(seed * 10 + index)
            im, lab, _, _ = cls.__getitem__(ds, index)
            batch.append((im, lab, "", None))
        imb, labb, _, _ = cls.collate_fn(batch)
        out[f"img{seed}"], out[f"lab{seed}"] = imb.numpy(), labb.numpy()
        print("augment mixup", seed, tuple(imb.shape), tuple(labb.shape))
    np.savez_compressed(os.path.join(OUT, "augment_mixup.npz"), **out)


TINY_CFG = {  # a 0.13 M-parameter YOLOv5 (reference schema, models/yolov5n.yaml with width 0.125): checkpoint fixtures stay small
    "nc": 80, "depth_multiple": 0.33, "width_multiple": 0.125,
    "anchors": [[10, 13, 16, 30, 33, 23], [30, 61, 62, 45, 59, 119], [116, 90, 156, 198, 373, 326]],
    "backbone": [[-1, 1, "Conv", [64, 6, 2, 2]], [-1, 1, "Conv", [128, 3, 2]], [-1, 3, "C3", [128]], [-1, 1, "Conv", [256, 3, 2]],
                 [-1, 6, "C3", [256]], [-1, 1, "Conv", [512, 3, 2]], [-1, 9, "C3", [512]], [-1, 1, "Conv", [1024, 3, 2]],
                 [-1, 3, "C3", [1024]], [-1, 1, "SPPF", [1024, 5]]],
    "head": [[-1, 1, "Conv", [512, 1, 1]], [-1, 1, "nn.Upsample", ["None", 2, "nearest"]], [[-1, 6], 1, "Concat", [1]],
             [-1, 3, "C3", [512, False]], [-1, 1, "Conv", [256, 1, 1]], [-1, 1, "nn.Upsample", ["None", 2, "nearest"]],
             [[-1, 4], 1, "Concat", [1]], [-1, 3, "C3", [256, False]], [-1, 1, "Conv", [256, 3, 2]], [[-1, 14], 1, "Concat", [1]],
             [-1, 3, "C3", [512, False]], [-1, 1, "Conv", [512, 3, 2]], [[-1, 10], 1, "Concat", [1]], [-1, 3, "C3", [1024, False]],
             [[17, 20, 23], 1, "Detect", ["nc", "anchors"]]],
}


def gen_ckpt(ns):
    """A checkpoint exactly as the reference's train.py:469-488 writes it -- pickled REFERENCE classes (models.yolo.DetectionModel,
    models.common.Conv, ...), fp16 -- of the tiny model above, plus what the reference computes from it after
    models/experimental.py:attempt_load's steps (float, fuse, eval): tests load the file into the yolov5_amd classes."""
    import copy
    from copy import deepcopy

    torch.manual_seed(0)
    m = ns.yolo.DetectionModel(copy.deepcopy(TINY_CFG))
    load_det_weights(m, 11)
    m.names = {i: f"class{i}" for i in range(80)}
    opt = ns.torch_utils.smart_optimizer(m, "SGD", 0.01, 0.937, 5e-4)
    ckpt = {"epoch": 3, "best_fitness": 0.25, "model": deepcopy(m).half(), "ema": None, "updates": 7, "optimizer": opt.state_dict(),
            "opt": {"imgsz": 64, "batch_size": 2}, "git": None, "date": "2026-01-01T00:00:00"}
    path = os.path.join(OUT, "ckpt_ref_tiny.pt")
    torch.save(ckpt, path)
    mm = torch.load(path, map_location="cpu", weights_only=False)["model"].float().fuse().eval()
    x = torch.from_numpy(detgen.uniform((2, 3, 64, 64), 0.0, 1.0, name="img", seed=11))
    with torch.no_grad():
        z, raw = mm(x)
    np.savez_compressed(os.path.join(OUT, "ckpt_ref_tiny.npz"), z=z.numpy(), raw0=raw[0].numpy(), nparams=np.array(sum(p.numel() for p in mm.parameters())))
    print("ckpt", os.path.getsize(path), tuple(z.shape))


XC_LABELS = [np.array([[2, 100.0, 120.0, 40.0, 60.0], [7, 300.5, 310.25, 80.0, 20.0]], np.float32), np.zeros((0, 5), np.float32),
             np.array([[0, 50.0, 60.0, 30.0, 30.0]], np.float32)]


def xc_metrics_batches():
    """The four (detections, labels) batches of tests/test_oracle_vs_reference.py::test_process_batch_and_ap_match_live_reference (seed 77)."""
    rng = np.random.default_rng(77)
    out = []
    for _ in range(4):
        m = int(rng.integers(1, 25))
        lab = np.zeros((m, 5), np.float32)
        lab[:, 0] = rng.integers(0, 4, m)
        xy = rng.uniform(0, 500, (m, 2)); wh = rng.uniform(10, 140, (m, 2))
        lab[:, 1:3], lab[:, 3:5] = xy, xy + wh
        pick = rng.integers(0, m, 90)
        det = np.zeros((90, 6), np.float32)
        det[:, :4] = lab[pick, 1:] + rng.normal(0, 5, (90, 4))
        det[:, 4] = np.sort(rng.uniform(0, 1, 90))[::-1]
        det[:, 5] = np.where(rng.uniform(0, 1, 90) < 0.8, lab[pick, 0], rng.integers(0, 4, 90))
        out.append((det, lab))
    return out


def xc_train_setup():
    """Data, weights and schedule of test_training_loop_restatement_matches_reference_pieces: (cfg, imgs, targets per image, bs, epochs, hyp)."""
    import copy

    from . import train_oracle as to

    imgs, tpi = to.synthetic_set(8, 64, per_img=2, seed=6)
    return copy.deepcopy(TINY_CFG), imgs, tpi, 4, 3, dict(to.HYP)


XC_PARTS = {"loss": ("loss_", "ab_"), "tta": ("tta_",), "metrics": ("nms", "pb_", "ap_"), "train": ("train_",)}  # tests/golden/crosscheck_<part>.npz
XC_TTA_Q = 1e-5     # quantization steps of the two large outputs, well below the tolerances their tests apply (1e-5 + 1e-5 |z|, 2e-5 + 2e-3 |w|)
XC_TRAIN_Q = 4e-6


def xc_quantize(ref, base, q):
    """ref (float32) as integer steps of q above base: (k int32, the largest |base + k q - ref| in float64).  A test that holds a value to
    atol + rtol |ref| holds it to (atol - (1 + rtol) err) + rtol |base + k q| instead: passing that implies the original bound exactly."""
    d = (ref.astype(np.float64) - base) / q
    assert np.abs(d).max() < 2 ** 31 - 1
    k = np.round(d).astype(np.int32)
    return k, np.array(np.abs(base + k.astype(np.float64) * q - ref.astype(np.float64)).max() if k.size else 0.0)


def _i4_planes(a):
    """int32 array -> its four byte planes, (4, last axis, ...): the high planes of small steps are runs of 0x00 / 0xff that zlib packs away."""
    b = np.ascontiguousarray(np.moveaxis(a.astype("<i4"), -1, 0))
    return np.ascontiguousarray(np.moveaxis(b.view(np.uint8).reshape(b.shape + (4,)), -1, 0))


def _i4_unplanes(p):
    b = np.ascontiguousarray(np.moveaxis(p, 0, -1)).view("<i4").reshape(p.shape[1:])
    return np.moveaxis(b, 0, -1)


def load_crosscheck(out_dir=OUT):
    """The reference outputs gen_crosscheck stored, one dict over all crosscheck_<part>.npz files."""
    G = {}
    for part in XC_PARTS:
        with np.load(os.path.join(out_dir, f"crosscheck_{part}.npz")) as f:
            G.update({k[:-3] if k.endswith("#i4") else k: _i4_unplanes(f[k]) if k.endswith("#i4") else f[k] for k in f.files})
    return G


def gen_crosscheck(ns):
    """tests/golden/crosscheck_<part>.npz: what the unmodified reference computes on the inputs of tests/test_oracle_vs_reference.py (inputs that
    differ from the other fixtures) -- ComputeLoss.build_targets / loss / input gradients (yolov5s), four autobalance calls, the TTA forward (yolov5n),
    NMS with and without a-priori labels, process_batch / ap_per_class, and three epochs of the train.py loop on the tiny model (per-iteration loss
    items, final parameters and EMA).  Everything is stored exactly but the TTA output and the trained weights: those are quantized (xc_quantize;
    the weights as steps above the seeded initial weights, the EMA as steps above the final weights) with the bound the tests subtract."""
    import math

    import yaml

    from . import yolo_oracle as yo

    G = {}
    with open(os.path.join(ns.root, "data/hyps/hyp.scratch-low.yaml")) as f:
        hyp_low = yaml.safe_load(f)

    # ComputeLoss: build_targets, the loss and its input gradients
    torch.manual_seed(0)
    m = ns.yolo.DetectionModel(os.path.join(ns.root, "models/yolov5s.yaml"))
    m.hyp = dict(hyp_low)
    cl = ns.loss.ComputeLoss(m)
    G["loss_anchors"] = m.model[-1].anchors.clone().numpy()
    p = [torch.from_numpy(detgen.uniform((3, 3, s, s, 85), -3.0, 3.0, name=f"v{s}", seed=31)).requires_grad_(True) for s in (24, 12, 6)]
    t = torch.from_numpy(detgen.synth_targets(3, 11, seed=31))
    tcls, tbox, idx, anch = cl.build_targets(p, t)
    for i in range(3):
        G[f"loss_idx{i}"] = torch.stack(list(idx[i])).numpy()
        G[f"loss_tcls{i}"], G[f"loss_tbox{i}"], G[f"loss_anch{i}"] = tcls[i].numpy(), tbox[i].numpy(), anch[i].numpy()
    loss, items = cl(p, t)
    loss.backward()
    G["loss_loss"], G["loss_items"] = loss.detach().numpy(), items.numpy()
    for i in range(3):
        G[f"loss_grad{i}"] = p[i].grad.numpy()

    # ComputeLoss(autobalance=True): losses and the balance list after each of four calls
    m = ns.yolo.DetectionModel(os.path.join(ns.root, "models/yolov5s.yaml"), ch=3, nc=80)
    m.hyp = dict(hyp_low)
    cl = ns.loss.ComputeLoss(m, autobalance=True)
    G["ab_ssi"], G["ab_anchors"] = np.array(cl.ssi), m.model[-1].anchors.clone().numpy()
    for step in range(4):
        p = [torch.from_numpy(detgen.uniform((2, 3, s, s, 85), -3.0, 3.0, name=f"ab{s}", seed=40 + step)) for s in (16, 8, 4)]
        t = torch.from_numpy(detgen.synth_targets(2, 6, seed=40 + step))
        loss, items = cl(p, t)
        G[f"ab_loss{step}"], G[f"ab_items{step}"], G[f"ab_balance{step}"] = loss.numpy(), items.numpy(), np.array(cl.balance, np.float64)

    # TTA forward
    torch.manual_seed(0)
    m = ns.yolo.DetectionModel(os.path.join(ns.root, "models/yolov5n.yaml"))
    m.load_state_dict(yo.det_state_dict(yo.model_cfg("yolov5n"), 3, fused=False))
    m.eval()
    x = torch.from_numpy(detgen.uniform((2, 3, 96, 128), 0.0, 1.0, name="tta", seed=5))
    with torch.no_grad():
        G["tta_k"], G["tta_err"] = xc_quantize(m(x, augment=True)[0].numpy(), 0.0, XC_TTA_Q)
    G["tta_q"] = np.array(XC_TTA_Q)

    # NMS, plain and with a-priori labels
    pred = detgen.synth_predictions(2, 1500, 85, obj_pow=3, seed=41)
    with ref_shim.oracle_nms_mode():
        for i, r in enumerate(ns.general.non_max_suppression(torch.from_numpy(pred), 0.25, 0.45, max_det=300)):
            G[f"nms_{i}"] = r.numpy()
    pred = detgen.synth_predictions(3, 800, 15, obj_pow=3, seed=43)
    for ml in (False, True):
        with ref_shim.oracle_nms_mode():
            out = ns.general.non_max_suppression(torch.from_numpy(pred), 0.25, 0.45, labels=[torch.from_numpy(lb) for lb in XC_LABELS], multi_label=ml,
                                                 max_det=300)
        for i, r in enumerate(out):
            G[f"nmslab{int(ml)}_{i}"] = r.numpy()

    # process_batch / ap_per_class
    iouv = torch.linspace(0.5, 0.95, 10)
    stats = []
    for i, (det, lab) in enumerate(xc_metrics_batches()):
        ref = ns.metrics.process_batch(torch.from_numpy(det), torch.from_numpy(lab), iouv).numpy()
        G[f"pb_{i}"] = ref
        stats.append((ref, det[:, 4], det[:, 5], lab[:, 0]))
    tp, conf, pcls, tcls = (np.concatenate(v, 0) for v in zip(*stats))
    for i, a in enumerate(ns.metrics.ap_per_class(tp, conf, pcls, tcls, plot=False, names={})):
        G[f"ap_{i}"] = np.asarray(a, np.float64)

    # train.py:234-248,372-434 on the tiny model: DetectionModel (train mode), ComputeLoss, smart_optimizer, ModelEMA
    cfg, imgs, tpi, bs, epochs, h = xc_train_setup()
    torch.manual_seed(0)
    m = ns.yolo.DetectionModel(cfg)
    load_det_weights(m, 9)
    init = yo.det_state_dict(cfg, 9, fused=False)   # what the test regenerates: must be the reference model's starting point, bit for bit
    for k, v in m.state_dict().items():
        if v.dtype.is_floating_point and not k.endswith("anchors"):
            assert torch.equal(init[k].to(v.dtype), v), k
    nbs, nb = 64, 2
    accumulate = max(round(nbs / bs), 1)
    h["weight_decay"] *= bs * accumulate / nbs
    opt = ns.torch_utils.smart_optimizer(m, "SGD", h["lr0"], h["momentum"], h["weight_decay"])
    lf = lambda x: ((1 - math.cos(x * math.pi / epochs)) / 2) * (h["lrf"] - 1) + 1  # noqa: E731  one_cycle(1, lrf, epochs)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lf)
    ema = ns.torch_utils.ModelEMA(m)
    m.hyp = h
    cl = ns.loss.ComputeLoss(m)
    nw = max(round(h["warmup_epochs"] * nb), 100)
    last, losses = -1, []
    for epoch in range(epochs):
        m.train()
        opt.zero_grad()
        for i in range(nb):
            ids = list(range(i * bs, (i + 1) * bs))
            ni = i + nb * epoch
            x = imgs[ids].float() / 255
            t = torch.cat([torch.cat((torch.full((len(tpi[j]), 1), float(k)), tpi[j][:, 1:]), 1) for k, j in enumerate(ids)], 0)
            if ni <= nw:
                accumulate = max(1, np.interp(ni, [0, nw], [1, nbs / bs]).round())
                for j, g in enumerate(opt.param_groups):
                    g["lr"] = np.interp(ni, [0, nw], [h["warmup_bias_lr"] if j == 0 else 0.0, g["initial_lr"] * lf(epoch)])
                    g["momentum"] = np.interp(ni, [0, nw], [h["warmup_momentum"], h["momentum"]])
            loss, items = cl(m(x), t)
            loss.backward()
            if ni - last >= accumulate:
                torch.nn.utils.clip_grad_norm_(m.parameters(), max_norm=10.0)
                opt.step()
                opt.zero_grad()
                ema.update(m)
                last = ni
            losses.append(items.detach().clone())
        sched.step()
    G["train_losses"], G["train_updates"] = torch.stack(losses).numpy(), np.array(ema.updates)
    G["train_q"], err = np.array(XC_TRAIN_Q), 0.0
    esd = ema.ema.state_dict()
    for k, v in m.state_dict().items():
        if v.dtype.is_floating_point and not k.endswith("anchors"):
            base = init[k].numpy().astype(np.float64)
            G[f"train_sd:{k}"], e1 = xc_quantize(v.numpy(), base, XC_TRAIN_Q)
            G[f"train_ema:{k}"], e2 = xc_quantize(esd[k].numpy(), base + G[f"train_sd:{k}"] * XC_TRAIN_Q, XC_TRAIN_Q)
            err = max(err, float(e1), float(e2))
    G["train_err"] = np.array(err)
    for part, prefixes in XC_PARTS.items():
        path = os.path.join(OUT, f"crosscheck_{part}.npz")
        planes = lambda v: v.dtype == np.int32 and v.size >= 1 << 16   # noqa: E731  (the TTA output; not the many small weight tensors)
        np.savez_compressed(path, **{(k + "#i4" if planes(v) else k): (_i4_planes(v) if planes(v) else v) for k, v in G.items() if k.startswith(prefixes)})
        print("crosscheck", part, os.path.getsize(path))
    L = load_crosscheck()
    assert L.keys() == G.keys() and all(L[k].dtype == G[k].dtype and np.array_equal(L[k], G[k]) for k in G)


def main():
    os.makedirs(OUT, exist_ok=True)
    ns = ref_shim.load()
    torch.set_num_threads(os.cpu_count() or 1)
    if len(sys.argv) > 1 and sys.argv[1] == "loss":  # only the ComputeLoss fixtures
        gen_loss(ns)
        return
    if len(sys.argv) > 1 and sys.argv[1] == "augment":
        gen_augment(ns)
        return 0
    if len(sys.argv) > 1 and sys.argv[1] == "ckpt":
        gen_ckpt(ns)
        return 0
    if len(sys.argv) > 1 and sys.argv[1] == "crosscheck":
        gen_crosscheck(ns)
        return 0
    if len(sys.argv) > 1 and sys.argv[1] == "detset_x":  # only the yolov5x fixture
        gen_detset(ns, "yolov5x_1280", "models/yolov5x.yaml", 1280, 1, 4, 397, bn_gamma_scale=0.07, cal_scenes=3)
        return 0
    if len(sys.argv) > 1 and sys.argv[1] == "detset":  # only the full-resolution fixtures (the rest is unchanged)
        gen_detset(ns, "yolov5s_640", "models/yolov5s.yaml", 640, 2, 3, 97, bn_gamma_scale=0.2)
        gen_detset(ns, "yolov5x_1280", "models/yolov5x.yaml", 1280, 1, 4, 397, bn_gamma_scale=0.07, cal_scenes=3)
        gen_detset(ns, "yolov5s-seg_640", "models/segment/yolov5s-seg.yaml", 640, 2, 5, 97, seg=True, bn_gamma_scale=0.1)
        return 0
    gen_fuse(ns)
    gen_forward(ns, "yolov5n_64", "models/yolov5n.yaml", 64, 2, 0, 1)
    gen_forward(ns, "yolov5s_320", "models/yolov5s.yaml", 320, 2, 1, 41)
    gen_forward(ns, "yolov5n-seg_64", "models/segment/yolov5n-seg.yaml", 64, 2, 2, 1, seg=True)
    gen_detset(ns, "yolov5s_640", "models/yolov5s.yaml", 640, 2, 3, 97, bn_gamma_scale=0.2)                                   # C2 shape class
    gen_detset(ns, "yolov5x_1280", "models/yolov5x.yaml", 1280, 1, 4, 397, bn_gamma_scale=0.07, cal_scenes=3)                 # C4
    gen_detset(ns, "yolov5s-seg_640", "models/segment/yolov5s-seg.yaml", 640, 2, 5, 97, seg=True, bn_gamma_scale=0.1)         # C5
    gen_nms(ns)
    gen_loss(ns)
    gen_mask(ns)
    gen_scale_boxes(ns)
    gen_optim(ns)
    gen_metrics(ns)
    gen_letterbox(ns)
    gen_ckpt(ns)
    gen_augment(ns)
    gen_crosscheck(ns)
    sizes = {f: os.path.getsize(os.path.join(OUT, f)) for f in sorted(os.listdir(OUT))}
    print(sizes, sum(sizes.values()))


if __name__ == "__main__":
    sys.exit(main())
