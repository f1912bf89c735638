"""Shared inputs and acceptance rules of the classification tests (tests/test_emu_classify.py, tests/test_classify_host.py,
tests/test_gpu_classify.py) and of scripts/make_golden_classify.py, which writes tests/golden/classify.npz from the unmodified reference.

  * transform: seeded uint8 HWC BGR sources (row stride wider than 3 * w0) of TRANSFORM_CASES at S = 32, the ToTensor + Normalize table built
    with the reference's two fp32 expressions, and `transform_restated`, the chain on oracle.thirdparty.cv2_resize (cv2 is absent: the resize is
    the project's restatement, "parity unpinned" in the project's sense, as is Normalize, whose published sub(mean).div(std) is applied in fp32).
  * head / post: float64 restatements with the forward error bound of fp32 summation in any order, per output.
  * whole model: a seeded conditioning of the Classify weights on top of oracle.yolo_oracle.det_state_dict's backbone, and the tie-free rule for
    comparing top-5 rankings.
"""
import os

import numpy as np
import torch

from oracle import detgen, thirdparty as tp, yolo_oracle as yo

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "classify.npz")
U24 = 2.0 ** -24   # unit roundoff of fp32

IMAGENET_MEAN = (0.485, 0.456, 0.406)   # utils/augmentations.py:15-16 (RGB)
IMAGENET_STD = (0.229, 0.224, 0.225)

S = 32
TRANSFORM_CASES = {"rect": (37, 53), "down": (64, 48), "identity": (32, 40), "up": (20, 31), "area2": (97, 64), "odd_top": (33, 32),
                   "odd_left": (32, 35), "m1": (1, 7)}


def golden():
    return np.load(GOLDEN, allow_pickle=False)


def source(name, shape=None, pad=5):
    """(view (h0, w0, 3) uint8 BGR whose rows are `stride` = 3 * w0 + pad bytes apart, stride)."""
    h0, w0 = shape or TRANSFORM_CASES[name]
    seed = sum(ord(c) for c in name) * 7919 + h0 * 131 + w0
    rs = np.random.RandomState(seed % (2 ** 31))
    stride = 3 * w0 + pad
    buf = rs.randint(0, 256, size=(h0, stride), dtype=np.uint8)
    # smooth part so that the interpolation has structure, noise on top
    yy, xx = np.mgrid[0:h0, 0:w0]
    for c in range(3):
        buf[:, c:3 * w0:3] = ((np.sin(yy * (0.21 + 0.05 * c)) + np.cos(xx * (0.17 + 0.03 * c))) * 60 + 128 + rs.randint(-20, 21, size=(h0, w0))).clip(0, 255)
    return buf[:, :3 * w0].reshape(h0, w0, 3), stride


def lut():
    """(3, 256) fp32: ToTensor's `im.float(); im /= 255.0` then Normalize's `sub(mean).div(std)` in fp32, channel order RGB."""
    u = torch.arange(256, dtype=torch.uint8).float()
    u /= 255.0
    mean = torch.tensor(IMAGENET_MEAN, dtype=torch.float32).view(3, 1)
    std = torch.tensor(IMAGENET_STD, dtype=torch.float32).view(3, 1)
    return u.expand(3, 256).clone().sub_(mean).div_(std).contiguous()


def center_crop_resize(im, size):
    """CenterCrop(size) of utils/augmentations.py:304-320 on the restated cv2.resize."""
    imh, imw = im.shape[:2]
    m = min(imh, imw)
    top, left = (imh - m) // 2, (imw - m) // 2
    return tp.cv2_resize(np.ascontiguousarray(im[top:top + m, left:left + m]), (size, size), interpolation=1)


def transform_restated(im, size):
    """(3, size, size) fp32: CenterCrop -> ToTensor -> Normalize, as classify_transforms(size) composes them."""
    r = center_crop_resize(im, size)
    t = torch.from_numpy(np.ascontiguousarray(r.transpose((2, 0, 1))[::-1])).float()
    t /= 255.0
    mean = torch.tensor(IMAGENET_MEAN, dtype=torch.float32).view(3, 1, 1)
    std = torch.tensor(IMAGENET_STD, dtype=torch.float32).view(3, 1, 1)
    return t.sub_(mean).div_(std).numpy()


# ---- head ------------------------------------------------------------------------------------------------------------------------------------
HEAD_SHAPES = [(3, 49, 1280, 1000), (1, 1, 64, 1), (2, 6, 1280, 10), (5, 4, 1280, 5), (2, 9, 1280, 1003)]


def head_inputs(B, HW, C, nc, dtype, ld=None, seed=0):
    """x (B, HW, ld) with the C channels in front (the rest is a sentinel no kernel may read into the result), w (nc, C), bias (nc) fp32."""
    rs = np.random.RandomState(1000 + seed + B * 7 + HW * 13 + C + nc * 3)
    ld = ld or C
    x = np.full((B, HW, ld), 77.0, dtype)
    v = rs.standard_normal((B, HW, C))
    x[:, :, :C] = (v / (1.0 + np.exp(-v))).astype(dtype)   # SiLU outputs, like the Conv's
    w = (rs.standard_normal((nc, C)) / np.sqrt(C)).astype(dtype)
    bias = (rs.standard_normal(nc) * 0.5).astype(np.float32)
    return x, w, bias


def head_ref(x, w, bias, C):
    """float64 logits and the per-output bound: (HW + C + 8) * 2^-24 * sum of the absolute values of the terms (+ half an fp16 ulp of the
    result when the output is fp16)."""
    B, HW, _ = x.shape
    x64, w64, b64 = x[:, :, :C].astype(np.float64), w.astype(np.float64), bias.astype(np.float64)
    pooled = x64.sum(1) / HW
    ref = b64[None] + pooled @ w64.T
    mag = np.abs(b64)[None] + (np.abs(x64).sum(1) / HW) @ np.abs(w64).T
    bound = (HW + C + 8) * U24 * mag
    if x.dtype == np.float16:
        bound = bound + np.spacing((np.abs(ref) + bound).astype(np.float16)).astype(np.float64) / 2
    return ref, bound


# ---- post ------------------------------------------------------------------------------------------------------------------------------------
POST_NC = (1, 4, 5, 10, 1000)
POST_B = (1, 7)


def post_inputs(B, nc, dtype, seed=0):
    """logits (B, nc) with a row of deliberate ties and a row of equal values when B allows, labels (B,) int32."""
    rs = np.random.RandomState(2000 + seed + B * 31 + nc)
    z = rs.standard_normal((B, nc)).astype(dtype)
    if B > 2 and nc > 1:
        z[1, :] = np.asarray(rs.randint(-2, 3, size=nc), dtype) * dtype(0.5)   # many ties
        z[2, :] = dtype(0.25)                                                   # all equal
    labels = rs.randint(0, nc, size=B).astype(np.int32)
    return z, labels


def post_ref(z, labels, eps):
    """(top5 (B, 5) stable descending argsort padded with -1, probs64, their bound, row_loss64, its bound) from the fp32-widened logits."""
    z32 = z.astype(np.float32)
    B, nc = z32.shape
    z64 = z32.astype(np.float64)
    order = np.argsort(-z32, axis=1, kind="stable")[:, :5]
    top5 = np.full((B, 5), -1, np.int32)
    top5[:, :order.shape[1]] = order
    mx = z64.max(1, keepdims=True)
    e = np.exp(z64 - mx)
    se = e.sum(1, keepdims=True)
    probs = e / se
    pb = (nc + 8) * U24 * probs
    lse = (mx + np.log(se))[:, 0]
    zy = z64[np.arange(B), labels]
    loss = (1 - eps) * (lse - zy) + eps * (lse - z64.mean(1))
    lb = (nc + 8) * U24 * ((1 - eps) * (np.abs(lse) + np.abs(zy)) + eps * (np.abs(lse) + np.abs(z64).sum(1) / nc))
    return top5, probs, pb, loss, lb


# ---- whole model -----------------------------------------------------------------------------------------------------------------------------
MODEL_NC = 10
MODEL_INPUTS = {"sq": (2, 3, 64, 64), "rect": (3, 3, 96, 64)}   # (3, 3, 96, 64): a 3 x 2 feature map, HW = 6


def cls_state_dict(name="yolov5n", nc=MODEL_NC, seed=0):
    """State dict of ClassificationModel(model=DetectionModel(name), nc=nc, cutoff=10): det_state_dict's backbone (layers 0..8) and a seeded,
    well-conditioned Classify head (layer 9) -- activations of order one into the pool, logits of order one with clear gaps between them."""
    cfg = yo.model_cfg(name)
    sd = {k: v for k, v in yo.det_state_dict(cfg, seed, fused=False).items() if int(k.split(".")[1]) < 9}
    ch = sd["model.8.cv3.conv.weight"].shape[0]
    rs = np.random.RandomState(4242 + seed)
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    sd["model.9.conv.conv.weight"] = f(rs.standard_normal((1280, ch, 1, 1)) / np.sqrt(ch))
    sd["model.9.conv.bn.weight"] = f(rs.uniform(0.8, 1.2, 1280))
    sd["model.9.conv.bn.bias"] = f(rs.standard_normal(1280) * 0.3)
    sd["model.9.conv.bn.running_mean"] = f(rs.standard_normal(1280) * 0.1)
    sd["model.9.conv.bn.running_var"] = f(rs.uniform(0.5, 1.5, 1280))
    sd["model.9.conv.bn.num_batches_tracked"] = torch.tensor(0, dtype=torch.long)
    sd["model.9.linear.weight"] = f(rs.standard_normal((nc, 1280)) * (2.0 / np.sqrt(1280)))
    sd["model.9.linear.bias"] = f(rs.standard_normal(nc) * 0.5)
    return sd


def model_input(key, seed=0):
    return torch.from_numpy(detgen.uniform(MODEL_INPUTS[key], 0.0, 1.0, name="img", seed=seed + len(key)))


def val_inputs():
    """Three batches (2, 2, 1 images) of the classify/val.py fixture."""
    x = torch.cat([model_input("sq", 1), model_input("sq", 2), model_input("sq", 3)[:1]])
    return [x[0:2], x[2:4], x[4:5]]


def tie_free_rows(ref64, allowed):
    """Rows whose top-6 values of the fp64 logits are more than 2 * `allowed` apart: only there is the ranking decided by the reference itself and
    not by the error that is allowed.  A condition on the fixture, not a measurement -- the caller asserts that no row is left out."""
    s = -np.sort(-ref64, axis=1)[:, :6]
    gaps = s[:, :-1] - s[:, 1:]
    return (gaps > 2 * allowed).all(1)


def assert_top5_matches(got, ref64, allowed, what):
    rows = tie_free_rows(ref64, allowed)
    assert rows.all(), f"{what}: rows {np.nonzero(~rows)[0].tolist()} of the fixture have top-6 gaps within twice the allowed error {allowed}"
    want = np.argsort(-ref64, axis=1, kind="stable")[:, :5]
    g = np.argsort(-np.asarray(got, np.float64), axis=1, kind="stable")[:, :5]
    assert np.array_equal(g, want), what
