"""CPU: y5_process_mask_native_batch (yolov5_amd/csrc/mask_native.h) on the HIP emulator, through the C entry point: every case of
tests/mask_native_ref.CASES against the reference-generated golden (tests/golden/mask_native.npz) under the acceptance rule of
tests/mask_native_ref.py, the project's own paths against each other bit for bit, guard bytes around every image's block, and every
bad-argument path."""
import ctypes as C

import numpy as np
import pytest

from tests import mask_native_ref as mr
from tests.hipemu.emu import aligned, emu, ptr
from yolov5_amd import _lib

GUARD = 64          # guard elements before the first block, between blocks and after the last
SENT_U8, SENT_F32 = 0xA5, -7.25


def _rows(coef, boxes, c):
    """Coefficient / box rows embedded in wider rows, like det[:, 6:] / det[:, :4] of the NMS output (ld = 6 + c + 3)."""
    n = coef.shape[0]
    ld = 6 + c + 3
    det = aligned((max(n, 1), ld), np.float32, 9.0)
    if n:
        det[:, :4] = boxes
        det[:, 6:6 + c] = coef
    return det, ld


def run_native(protos, items, shapes, u8):
    """protos (B, c, mh, mw); items[i] = (coef (n, c), boxes (n, 4)); shapes[i] = (h0, w0).  Returns the per-image (n, h0, w0) arrays after
    checking that nothing outside the images' blocks was written."""
    lib = emu()
    B, c, mh, mw = protos.shape
    P = aligned(protos.shape, protos.dtype); P[...] = protos
    vec = 16 if u8 else 4
    imgs = (_lib.MaskNativeImg * B)()
    keep, spans = [], []
    off = GUARD
    for i, ((coef, boxes), (h0, w0)) in enumerate(zip(items, shapes)):
        top, left, bottom, right = mr.window(mh, mw, (h0, w0))
        det, ld = _rows(coef, boxes, c)
        keep.append(det)
        n = coef.shape[0]
        im = imgs[i]
        im.masks_in, im.boxes, im.ld_m, im.ld_b, im.n = det.ctypes.data + 24, det.ctypes.data, ld, ld, n
        im.h0, im.w0, im.top, im.left, im.ch, im.cw, im.out_off = h0, w0, top, left, bottom - top, right - left, off
        spans.append((off, n, h0, w0))
        off += -(-n * h0 * w0 // vec) * vec + GUARD
    sent = SENT_U8 if u8 else SENT_F32
    out = aligned((off,), np.uint8 if u8 else np.float32, sent)
    rc = lib.y5_process_mask_native_batch(ptr(P), _lib.Y5_F16 if protos.dtype == np.float16 else _lib.Y5_F32, B, c, mh, mw, imgs, ptr(out), off,
                                          _lib.Y5_U8 if u8 else _lib.Y5_F32, None)
    assert rc == 0, lib.y5_last_error()
    untouched = np.ones(off, bool)
    res = []
    for o, n, h0, w0 in spans:
        untouched[o:o + n * h0 * w0] = False
        res.append(out[o:o + n * h0 * w0].reshape(n, h0, w0).copy())
    assert (out[untouched] == sent).all(), "a store outside the images' blocks"
    assert all((r != sent).all() for r in res), "an output pixel was not written"
    return res


def run_case(name, pd, u8):
    protos, coef, boxes, shape = mr.inputs(name, pd)
    return run_native(protos[None], [(coef, boxes)], [shape], u8)[0]


@pytest.mark.parametrize("pd", mr.PROTO_DTYPES)
@pytest.mark.parametrize("name", list(mr.CASES))
def test_emu_native_cases_vs_reference_golden(name, pd):
    f = run_case(name, pd, False)
    assert f.dtype == np.float32
    mr.accept_case(f, name, pd, f"emu {name}/{pd}/f32")
    u = run_case(name, pd, True)
    assert u.dtype == np.uint8
    mr.accept_case(u, name, pd, f"emu {name}/{pd}/u8")
    assert np.array_equal(u, f.astype(np.uint8))   # U8 bits == F32 bits


@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("pd", mr.PROTO_DTYPES)
def test_emu_native_ragged_batch_equals_single_calls(pd, u8):
    """`up`, an image without detections, `down`: one call for the three images against three single-image calls, bit for bit."""
    pu, cu, bu, su = mr.inputs("up", pd)
    pdn, cd, bd, sd = mr.inputs("down", pd)
    empty = (np.zeros((0, 8), np.float32), np.zeros((0, 4), np.float32))
    protos = np.stack([pu, pu[::-1].copy(), pdn])
    got = run_native(protos, [(cu, bu), empty, (cd, bd)], [su, (33, 57), sd], u8)
    assert got[1].shape == (0, 33, 57)
    assert np.array_equal(got[0], run_case("up", pd, u8))
    assert np.array_equal(got[2], run_case("down", pd, u8))
    # all images empty: nothing is launched, nothing is written
    none = run_native(protos, [empty, empty, empty], [su, (33, 57), sd], u8)
    assert [m.shape for m in none] == [(0,) + su, (0, 33, 57), (0,) + sd]


def test_emu_native_direct_taps_when_the_source_region_exceeds_lds():
    """An image much smaller than its window (scale 8): the source region of the one tile is the whole 160 x 160 window, more than the LDS of a
    launch holds, so the tile evaluates its four taps directly -- the same value function, checked against the restatement like the others."""
    c, mh, mw, h0, w0 = 8, 160, 160, 20, 20
    for pd in mr.PROTO_DTYPES:
        protos, coef, boxes = mr.make_inputs("direct", c, mh, mw, h0, w0, n=3, proto_dtype=pd)
        assert mr.window(mh, mw, (h0, w0)) == (0, 0, 160, 160)
        bits, v64, band = mr.reference_of(protos, coef, boxes, (h0, w0))
        f = run_native(protos[None], [(coef, boxes)], [(h0, w0)], False)[0]
        u = run_native(protos[None], [(coef, boxes)], [(h0, w0)], True)[0]
        mr.accept(f, bits, v64, band, f"emu direct/{pd}")
        assert np.array_equal(u, f.astype(np.uint8))


def test_emu_native_boxes_read_as_given():
    """Fractional, negative and oversized boxes are compared as they are: x1 <= X < x2 and y1 <= Y < y2 on the float values."""
    protos, coef, _, shape = mr.inputs("up")
    boxes = np.array([[10.5, 3.2, 70.1, 60.0], [-5, -5, 500, 500], [129, 74, 130, 75], [30.2, 30, 30.8, 31], [64, 0, 65, 75], [0, 63.5, 130, 64.5],
                      [np.nan, 0, 50, 50]], np.float32)
    bits, v64, band = mr.reference_of(protos, coef, boxes, shape)
    assert not bits[3].any() and not bits[6].any() and bits[:3].any()
    for u8 in (False, True):
        mr.accept(run_native(protos[None], [(coef, boxes)], [shape], u8)[0], bits, v64, band, f"emu boxes u8={u8}")


def test_emu_native_bad_arguments():
    lib = emu()
    protos, coef, boxes, (h0, w0) = mr.inputs("up")
    c, mh, mw = protos.shape
    P = aligned(protos.shape, np.float32); P[...] = protos
    det, ld = _rows(coef, boxes, c)
    n = coef.shape[0]
    out = aligned((n * h0 * w0 + 4,), np.float32, SENT_F32)
    good = dict(masks_in=det.ctypes.data + 24, boxes=det.ctypes.data, ld_m=ld, ld_b=ld, n=n, h0=h0, w0=w0, top=0, left=0, ch=23, cw=40, out_off=0)

    def call(img=None, **kw):
        a = dict(protos=ptr(P), pdt=_lib.Y5_F32, B=1, c=c, mh=mh, mw=mw, imgs=True, out=ptr(out), elems=n * h0 * w0, odt=_lib.Y5_F32)
        a.update(kw)
        imgs = (_lib.MaskNativeImg * 1)()
        for k, v in dict(good, **(img or {})).items():
            setattr(imgs[0], k, v)
        return lib.y5_process_mask_native_batch(a["protos"], a["pdt"], a["B"], a["c"], a["mh"], a["mw"], imgs if a["imgs"] else None, a["out"],
                                                a["elems"], a["odt"], None)

    BAD, UNSUP = -1, -2
    assert call() == 0 and (out[: n * h0 * w0] != SENT_F32).all() and (out[n * h0 * w0:] == SENT_F32).all()
    for kw in (dict(protos=None), dict(imgs=False), dict(out=None), dict(B=0), dict(c=0), dict(c=257), dict(mh=0), dict(mw=0), dict(elems=-1),
               dict(pdt=_lib.Y5_U8), dict(odt=_lib.Y5_F16), dict(odt=_lib.Y5_I32), dict(elems=n * h0 * w0 - 1),
               dict(out=C.c_void_p(out.ctypes.data + 4))):
        assert call(**kw) == BAD, kw
        assert b"process_mask_native_batch" in lib.y5_last_error()
    for img in (dict(n=-1), dict(masks_in=None), dict(boxes=None), dict(ld_m=c - 1), dict(ld_b=3), dict(h0=0), dict(w0=0), dict(w0=-3),
                dict(ch=0), dict(cw=0), dict(ch=-1), dict(top=-1), dict(left=-1), dict(top=2), dict(ch=25), dict(left=1), dict(cw=41),
                dict(out_off=-4), dict(out_off=2), dict(out_off=4)):
        assert call(img=img) == BAD, img
    assert call(img=dict(h0=1 << 24, w0=1 << 24, n=1 << 20), elems=1 << 62) == UNSUP   # more tiles than a grid holds
    # an image without instances is not looked at any further, and an all-empty batch needs no output
    assert call(img=dict(n=0, masks_in=None, boxes=None, h0=0, w0=0, ch=0, cw=0), out=None, elems=0) == 0
