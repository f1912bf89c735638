"""CPU: the classification kernels (yolov5_amd/csrc/classify.h, classify_data.h) on the HIP emulator through their C entries, and the whole
ClassificationModel plan on EmuBackend, against tests/golden/classify.npz (written from the unmodified reference by
scripts/make_golden_classify.py) under the rules of tests/classify_ref.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import classify_ref as cr
from tests.hipemu.backend import EmuBackend
from tests.hipemu.emu import aligned, emu, ptr
from yolov5_amd import _lib
from yolov5_amd.engine import Engine
from yolov5_amd.yolo import ClassificationModel, DetectionModel

GUARD = 64
BAD, UNSUP, WS = -1, -2, -4


def _dt(a):
    return _lib.Y5_F16 if a.dtype == np.float16 else _lib.Y5_F32


# ---- transform -------------------------------------------------------------------------------------------------------------------------------
def run_transform(names, f16=False, S=cr.S):
    """One launch for the sources `names`; checks the guard elements around the output and that every output element was written."""
    lib = emu()
    jobs = aligned((len(names),), np.dtype([("src", np.uint64), ("h0", np.int32), ("w0", np.int32), ("stride", np.int32), ("r", np.int32)]))
    keep = []
    for i, n in enumerate(names):
        im, stride = cr.source(n)
        assert stride > 3 * im.shape[1] and (im.shape[0] == 1 or im.strides[0] == stride)
        keep.append(im)
        jobs[i] = (im.ctypes.data, im.shape[0], im.shape[1], stride, 0)
    lut = aligned((3, 256), np.float32); lut[...] = cr.lut().numpy()
    dt = np.float16 if f16 else np.float32
    n = len(names) * 3 * S * S
    sent = dt(-77.5)
    buf = aligned((GUARD + n + GUARD,), dt, sent)   # (GUARD elements = a multiple of 16 bytes: the output stays aligned)
    out = buf[GUARD:GUARD + n]
    rc = lib.y5_classify_transform_batch(ptr(jobs), len(names), S, ptr(lut), ptr(out), _dt(buf), None)
    assert rc == 0, lib.y5_last_error()
    assert (buf[:GUARD] == sent).all() and (buf[GUARD + n:] == sent).all(), "a store outside the output"
    assert (out != sent).all(), "an output element was not written"
    return out.reshape(len(names), 3, S, S).copy()


@pytest.mark.parametrize("name", list(cr.TRANSFORM_CASES))
def test_emu_transform_fp32_bit_equal_to_reference_golden(name):
    g = cr.golden()
    got = run_transform([name])[0]
    assert got.dtype == np.float32 and np.array_equal(got, g[f"tf_{name}"])
    h0, w0 = cr.TRANSFORM_CASES[name]
    m = min(h0, w0)
    if name == "odd_top":
        assert (h0 - m) // 2 == 0 and (h0 - m) % 2 == 1
    if name == "area2":
        assert m == 2 * cr.S
    half = run_transform([name], f16=True)[0]
    assert half.dtype == np.float16 and np.array_equal(half, got.astype(np.float16))   # numpy rounds to nearest even, like .half()


@pytest.mark.parametrize("f16", [False, True])
def test_emu_transform_ragged_batch_equals_single_calls(f16):
    names = list(cr.TRANSFORM_CASES)
    batch = run_transform(names, f16)
    for i, n in enumerate(names):
        assert np.array_equal(batch[i], run_transform([n], f16)[0]), n


def test_emu_transform_size_that_is_no_multiple_of_the_vector():
    """S = 19: the scalar tail of every row, against the restatement."""
    got = run_transform(["rect", "up"], S=19)
    for i, n in enumerate(("rect", "up")):
        assert np.array_equal(got[i], cr.transform_restated(cr.source(n)[0], 19))


def test_emu_transform_bad_arguments():
    lib = emu()
    im, stride = cr.source("rect")
    jobs = aligned((1,), np.dtype([("src", np.uint64), ("h0", np.int32), ("w0", np.int32), ("stride", np.int32), ("r", np.int32)]))
    jobs[0] = (im.ctypes.data, im.shape[0], im.shape[1], stride, 0)
    lut = aligned((3, 256), np.float32); lut[...] = cr.lut().numpy()
    out = aligned((3 * 32 * 32,), np.float32, -77.5)

    def call(**kw):
        a = dict(jobs=ptr(jobs), B=1, S=32, lut=ptr(lut), dst=ptr(out), dt=_lib.Y5_F32)
        a.update(kw)
        return lib.y5_classify_transform_batch(a["jobs"], a["B"], a["S"], a["lut"], a["dst"], a["dt"], None)

    assert call() == 0
    for kw in (dict(jobs=None), dict(lut=None), dict(dst=None), dict(B=0), dict(B=65536), dict(S=0), dict(dt=_lib.Y5_U8), dict(dt=_lib.Y5_I32),
               dict(dst=C.c_void_p(out.ctypes.data + 4))):
        assert call(**kw) == BAD, kw
        assert b"classify_transform_batch" in lib.y5_last_error()
    assert call(S=1 << 20) == UNSUP
    # a job whose stride is narrower than its row is not read: its image stays unwritten
    out[...] = -77.5
    jobs[0]["stride"] = 3 * im.shape[1] - 1
    assert call() == 0 and (out == -77.5).all()


# ---- head ------------------------------------------------------------------------------------------------------------------------------------
def run_head(x, w, bias, C_, nc, form, ldo=None):
    lib = emu()
    B, HW, ld = x.shape
    ldo = ldo or nc
    X = aligned(x.shape, x.dtype); X[...] = x
    Wt = aligned(w.shape, w.dtype); Wt[...] = w
    Bi = aligned(bias.shape, np.float32); Bi[...] = bias
    sent = x.dtype.type(-9.5)
    out = aligned((B, ldo), x.dtype, sent)
    nbytes = lib.y5_classify_head_workspace_bytes(B, C_)
    assert nbytes == B * C_ * 4
    ws = aligned((nbytes + 64,), np.uint8, 0xA5)
    rc = lib.y5_classify_head(ptr(X), _dt(x), B, HW, C_, ld, ptr(Wt), ptr(Bi), nc, ptr(out), ldo, form, ptr(ws), nbytes, None)
    assert rc == 0, lib.y5_last_error()
    assert (ws[nbytes:] == 0xA5).all(), "a store behind the workspace"
    assert (out[:, nc:] == sent).all(), "a store behind a logits row"
    return out[:, :nc].copy()


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("dtype", [np.float16, np.float32])
@pytest.mark.parametrize("shape", cr.HEAD_SHAPES + [(2, 6, 1280, 10, 1288)])
def test_emu_head_within_fp32_summation_bound(shape, dtype, form):
    B, HW, C_, nc = shape[:4]
    ld = shape[4] if len(shape) > 4 else None
    x, w, bias = cr.head_inputs(B, HW, C_, nc, dtype, ld)
    got = run_head(x, w, bias, C_, nc, form, ldo=nc + 3 if ld else None)
    ref, bound = cr.head_ref(x, w, bias, C_)
    err = np.abs(got.astype(np.float64) - ref)
    print(f"head {shape} {np.dtype(dtype).name} form {form}: max err / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all(), (err / bound).max()


@pytest.mark.parametrize("form", [0, 1, 2])
@pytest.mark.parametrize("dtype", [np.float16, np.float32])
def test_emu_head_batch_equals_single_rows_bit_for_bit(dtype, form):
    B, HW, C_, nc = 5, 4, 1280, 5
    x, w, bias = cr.head_inputs(B, HW, C_, nc, dtype)
    batch = run_head(x, w, bias, C_, nc, form)
    for b in range(B):
        assert np.array_equal(batch[b:b + 1], run_head(x[b:b + 1], w, bias, C_, nc, form)), b
    # ... and a row's result does not depend on its position in the batch
    assert np.array_equal(run_head(x[::-1].copy(), w, bias, C_, nc, form), batch[::-1])


def test_emu_head_bad_arguments():
    lib = emu()
    B, HW, C_, nc = 2, 6, 64, 10
    x, w, bias = cr.head_inputs(B, HW, C_, nc, np.float32)
    X = aligned(x.shape, np.float32); X[...] = x
    Wt = aligned(w.shape, np.float32); Wt[...] = w
    Bi = aligned(bias.shape, np.float32); Bi[...] = bias
    out = aligned((B, nc), np.float32)
    ws = aligned((B * C_ * 4,), np.uint8)

    def call(**kw):
        a = dict(x=ptr(X), dt=_lib.Y5_F32, B=B, HW=HW, C=C_, ld=C_, w=ptr(Wt), bias=ptr(Bi), nc=nc, out=ptr(out), ldo=nc, form=2, ws=ptr(ws), nb=B * C_ * 4)
        a.update(kw)
        return lib.y5_classify_head(a["x"], a["dt"], a["B"], a["HW"], a["C"], a["ld"], a["w"], a["bias"], a["nc"], a["out"], a["ldo"], a["form"], a["ws"],
                                    a["nb"], None)

    assert call() == 0 and call(form=1, ws=None, nb=0) == 0
    for kw in (dict(x=None), dict(w=None), dict(bias=None), dict(out=None), dict(dt=_lib.Y5_U8), dict(B=0), dict(HW=0), dict(C=0), dict(nc=0), dict(ld=C_ - 8),
               dict(ldo=nc - 1), dict(form=3), dict(form=-1), dict(x=C.c_void_p(X.ctypes.data + 4)), dict(w=C.c_void_p(Wt.ctypes.data + 8))):
        assert call(**kw) == BAD, kw
        assert b"classify_head" in lib.y5_last_error()
    for kw in (dict(C=60, ld=60), dict(ld=C_ + 2), dict(C=8200, ld=8200), dict(B=65536)):
        assert call(**kw) == UNSUP, kw
    for kw in (dict(ws=None), dict(nb=B * C_ * 4 - 1), dict(ws=C.c_void_p(ws.ctypes.data + 4))):
        assert call(**kw) == WS, kw
    assert lib.y5_classify_head_workspace_bytes(0, 8) == 0


# ---- post ------------------------------------------------------------------------------------------------------------------------------------
def run_post(z, labels=None, eps=0.0, probs=True, ld=None):
    lib = emu()
    B, nc = z.shape
    ld = ld or nc
    Z = aligned((B, ld), z.dtype, 99.0); Z[:, :nc] = z
    top5 = aligned((B + 1, 5), np.int32, -7)
    P = aligned((B * nc + 8,), np.float32, -3.5) if probs else None
    L = aligned((B + 4,), np.float32, -3.5)
    lab = None
    if labels is not None:
        lab = aligned((B,), np.int32); lab[...] = labels
    rc = lib.y5_classify_post(ptr(Z), _dt(z), B, nc, ld, ptr(lab), eps, ptr(top5), ptr(P), ptr(L), None)
    assert rc == 0, lib.y5_last_error()
    assert (top5[B] == -7).all() and (L[B:] == -3.5).all() and (P is None or (P[B * nc:] == -3.5).all())
    return top5[:B].copy(), None if P is None else P[:B * nc].reshape(B, nc).copy(), L[:B].copy()


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
@pytest.mark.parametrize("B", cr.POST_B)
@pytest.mark.parametrize("nc", cr.POST_NC)
def test_emu_post_top5_exact_probs_and_loss_within_bound(nc, B, dtype):
    z, labels = cr.post_inputs(B, nc, dtype)
    for eps in (0.0, 0.1):
        want5, p64, pb, l64, lb = cr.post_ref(z, labels, eps)
        top5, probs, loss = run_post(z, labels, eps, ld=nc + 3)
        assert np.array_equal(top5, want5), (top5, want5)
        ep, el = np.abs(probs - p64), np.abs(loss - l64)
        print(f"post nc {nc} B {B} {np.dtype(dtype).name} eps {eps}: probs err / bound {(ep / pb).max():.3f}, loss err / bound {(el / lb).max():.3f}")
        assert (ep <= pb).all() and (el <= lb).all()
    if B > 2 and nc > 5:
        assert len(set(z[1].tolist())) <= 5 and (top5[2] == np.arange(5)).all()   # the tie rows did what they are there for
    # labels absent: row_loss untouched; probs optional
    top5b, none, loss = run_post(z, None, 0.1, probs=False)
    assert none is None and (loss == -3.5).all() and np.array_equal(top5b, want5)


def test_emu_post_bad_arguments():
    lib = emu()
    z, labels = cr.post_inputs(7, 10, np.float32)
    Z = aligned(z.shape, np.float32); Z[...] = z
    lab = aligned((7,), np.int32); lab[...] = labels
    top5, P, L = aligned((7, 5), np.int32), aligned((7, 10), np.float32), aligned((7,), np.float32)

    def call(**kw):
        a = dict(z=ptr(Z), dt=_lib.Y5_F32, B=7, nc=10, ld=10, lab=ptr(lab), eps=0.1, top5=ptr(top5), P=ptr(P), L=ptr(L))
        a.update(kw)
        return lib.y5_classify_post(a["z"], a["dt"], a["B"], a["nc"], a["ld"], a["lab"], a["eps"], a["top5"], a["P"], a["L"], None)

    assert call() == 0 and call(P=None, L=None, lab=None) == 0
    for kw in (dict(z=None), dict(top5=None), dict(dt=_lib.Y5_U8), dict(B=0), dict(nc=0), dict(ld=9), dict(eps=-0.1), dict(eps=1.5),
               dict(eps=float("nan")), dict(z=C.c_void_p(Z.ctypes.data + 2)), dict(top5=C.c_void_p(top5.ctypes.data + 2)), dict(P=C.c_void_p(P.ctypes.data + 1))):
        assert call(**kw) == BAD, kw
        assert b"classify_post" in lib.y5_last_error()
    assert call(nc=40000, ld=40000) == UNSUP


# ---- whole model -----------------------------------------------------------------------------------------------------------------------------
def cls_model(fused, name="yolov5n"):
    m = ClassificationModel(model=DetectionModel(name + ".yaml"), nc=cr.MODEL_NC, cutoff=10)
    m.load_state_dict(cr.cls_state_dict(name))
    m.eval()
    return m.fuse() if fused else m


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("key", list(cr.MODEL_INPUTS))
def test_emu_yolov5n_cls_fp32_matches_reference_fp64(key, fused):
    g = cr.golden()
    x = cr.model_input(key)
    eng = Engine(cls_model(fused), tuple(x.shape), torch.float32, "cpu", backend=EmuBackend())
    assert any(n.startswith("classify_head:") for n in eng.op_names) and "z" not in eng.outputs
    got = np.asarray(eng(x)["logits"])
    ref = g[f"logits64_{key}"]
    assert got.shape == ref.shape == (x.shape[0], cr.MODEL_NC)
    print(f"fp32 plan {key} fused={fused}: max error {np.abs(got - ref).max():.3e}")
    np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-4)
    cr.assert_top5_matches(got, ref, 1e-4 + 1e-4 * np.abs(ref).max(), f"top-5 {key}")


@pytest.mark.parametrize("key", list(cr.MODEL_INPUTS))
def test_emu_yolov5n_cls_fp16_within_twice_the_reference_half_forward(key):
    """The plan's max error from the reference's fp64 logits is at most 2x that of the reference's own `.half()` forward (measured by
    scripts/make_golden_classify.py on the CPU: 3.4e-4 max on `sq`, 5.1e-4 on `rect`)."""
    g = cr.golden()
    x = cr.model_input(key).half()
    m = cls_model(True).half()
    eng = Engine(m, tuple(x.shape), torch.float16, "cpu", backend=EmuBackend())
    assert eng._stem is not None   # the fp16 plan keeps the fused stem of the backbone
    got = np.asarray(eng(x)["logits"]).astype(np.float64)
    ref = g[f"logits64_{key}"]
    noise = np.abs(g[f"logits16_{key}"].astype(np.float64) - ref).max()
    err = np.abs(got - ref).max()
    print(f"fp16 plan {key}: max error {err:.3e}, reference half forward {noise:.3e}")
    assert err <= 2 * noise, (err, noise)
    cr.assert_top5_matches(got, ref, 2 * noise, f"top-5 {key} fp16")
