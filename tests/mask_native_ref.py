"""Shared by the process_mask_native tests: the named cases, their seeded inputs, a torch restatement of utils/segment/general.py:54-76 with
the compute dtype as a parameter, and the acceptance rule for mask bits.

The fp32 restatement is pinned bit for bit to the reference's own function by tests/golden/mask_native.npz (tests/test_mask_native_ref.py).
A kernel result is accepted against it when, per case,
  * at most 1e-4 of the pixels differ (the project's cap for process_mask, tests/test_emu_mask.py), and
  * every differing pixel has an fp64 pre-threshold value within `band` of 0.5, band = 4 x max|v_fp32 - v_fp64| over that case, computed from
    the restatement alone.  The factor 4 covers the kernel's different summation order, its expf and the FMA contraction of the four-tap blend.
A wrong window, tap or crop moves whole rows or columns and fails both."""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import detgen

SEED = 21
N = 7
# name: (c, mh, mw, h0, w0, window rows, window columns)
CASES = {
    "up": (8, 24, 40, 75, 130, 23, 40),        # window one row short of the plane: int(pad) and int(mh - pad) truncate differently
    "down": (8, 24, 40, 17, 29, 23, 40),       # scale > 1
    "tall": (8, 24, 40, 131, 52, 24, 9),       # side padding
    "same": (8, 24, 40, 24, 40, 24, 40),       # identity
    "strip": (8, 24, 40, 7, 300, 1, 40),       # one-row window
    "wide16": (8, 24, 40, 96, 160, 24, 40),    # fully vectorisable rows
    "g_port": (32, 40, 40, 270, 202, 40, 29),  # portrait
    "g_land": (32, 40, 40, 202, 270, 29, 40),  # landscape
}
PROTO_DTYPES = ("f32", "f16")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mask_native.npz")


def window(mh, mw, shape):
    """general.py:68-71: rows [top, bottom) and columns [left, right) of the prototype plane that is resized."""
    gain = min(mh / shape[0], mw / shape[1])
    pad = (mw - shape[1] * gain) / 2, (mh - shape[0] * gain) / 2
    return int(pad[1]), int(pad[0]), int(mh - pad[1]), int(mw - pad[0])


def make_inputs(tag, c, mh, mw, h0, w0, n=N, proto_dtype="f32"):
    """protos (c, mh, mw) in (-1, 1) (float16 when proto_dtype == "f16"), coefficients (n, c) in (-1, 1), boxes (n, 4) rounded xyxy in the
    image's pixels; box 0 is the whole image, box 1 is empty (x2 = x1)."""
    protos = detgen.uniform((c, mh, mw), -1.0, 1.0, name=f"{tag}_protos", seed=SEED)
    coef = detgen.uniform((n, c), -1.0, 1.0, name=f"{tag}_coef", seed=SEED)
    size = np.array([w0, h0], np.float32)
    xy1 = detgen.uniform((n, 2), 0.0, 0.5, name=f"{tag}_xy1", seed=SEED) * size
    wh = detgen.uniform((n, 2), 0.05, 0.5, name=f"{tag}_wh", seed=SEED) * size
    boxes = np.round(np.concatenate((xy1, xy1 + wh), 1)).astype(np.float32)
    boxes[0] = (0, 0, w0, h0)
    boxes[1, 2] = boxes[1, 0]
    if proto_dtype == "f16":
        protos = protos.astype(np.float16)
    return protos, coef, boxes


def inputs(name, proto_dtype="f32"):
    c, mh, mw, h0, w0, _, _ = CASES[name]
    return make_inputs(name, c, mh, mw, h0, w0, proto_dtype=proto_dtype) + ((h0, w0),)


def process_mask_native(protos, masks_in, bboxes, shape, dtype=torch.float32):
    """Restatement of general.py:54-76 computing in `dtype`.  Returns (bits (n, h0, w0) bool, pre-threshold values in `dtype`)."""
    c, mh, mw = protos.shape
    masks = (masks_in.to(dtype) @ protos.to(dtype).view(c, -1)).sigmoid().view(-1, mh, mw)
    top, left, bottom, right = window(mh, mw, shape)
    masks = masks[:, top:bottom, left:right]
    masks = F.interpolate(masks[None], tuple(shape), mode="bilinear", align_corners=False)[0]
    b = bboxes.to(dtype)
    x1, y1, x2, y2 = (b[:, k, None, None] for k in range(4))
    r = torch.arange(shape[1], dtype=dtype)[None, None, :]
    cc = torch.arange(shape[0], dtype=dtype)[None, :, None]
    vals = masks * ((r >= x1) * (r < x2) * (cc >= y1) * (cc < y2))
    return vals > 0.5, vals


def reference_of(protos, coef, boxes, shape):
    """(fp32 bits, fp64 values, band) of one set of numpy inputs."""
    t = [torch.from_numpy(np.ascontiguousarray(a).astype(np.float32)) for a in (protos, coef, boxes)]
    bits, v32 = process_mask_native(*t, shape, torch.float32)
    _, v64 = process_mask_native(*t, shape, torch.float64)
    band = 4.0 * float((v32.double() - v64).abs().max())
    return bits.numpy(), v64.numpy(), band


@functools.lru_cache(maxsize=None)
def reference(name, proto_dtype="f32"):
    """Computed once per case and shared; callers must not modify the arrays."""
    out = reference_of(*inputs(name, proto_dtype))
    for a in out[:2]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def golden(name, proto_dtype="f32"):
    """The reference's own bits (scripts/make_golden_mask_native.py)."""
    with np.load(GOLDEN) as g:
        shape = tuple(g[f"{name}_{proto_dtype}_shape"])
        a = np.unpackbits(g[f"{name}_{proto_dtype}"])[: int(np.prod(shape))].reshape(shape).astype(bool)
    a.setflags(write=False)
    return a


def accept(got, ref_bits, v64, band, what=""):
    """The acceptance rule of the module docstring; prints the figures before it asserts."""
    got = np.asarray(got)
    assert got.shape == ref_bits.shape, (what, got.shape, ref_bits.shape)
    assert set(np.unique(got).tolist()) <= {0, 1}, what
    diff = got.astype(bool) != ref_bits
    nd = int(diff.sum())
    far = float(np.abs(v64[diff] - 0.5).max()) if nd else 0.0
    print(f"[mask_native] {what}: {nd} of {diff.size} pixels differ, farthest from 0.5: {far:.3e}, band {band:.3e}")
    assert nd <= 1e-4 * diff.size, f"{what}: {nd} of {diff.size} pixels differ"
    assert far <= band, f"{what}: a differing pixel has fp64 value {far:.3e} from 0.5, band {band:.3e}"


def accept_case(got, name, proto_dtype="f32", what=""):
    """Against the golden (the reference's bits), band from the restatement."""
    _, v64, band = reference(name, proto_dtype)
    accept(got, golden(name, proto_dtype), v64, band, what or f"{name}/{proto_dtype}")
