"""TEST INFRASTRUCTURE ONLY: case tables, references and ONE runner per kernel for the three launches that read the caller's NCHW batch -- the fused
front (yolov5_amd/csrc/conv_front.h, y5_conv_front_fwd: 0.Conv + 1.Conv + 2.C3.cv1+cv2) and the NCHW stem with and without its epilogue
(csrc/conv_stem.h, y5_conv_stem_fwd / y5_conv_stem_fwd_raw).  Every runner takes a backend of tests/train_glue_ref.py, so tests/test_emu_front_parity.py
(the kernels compiled for the host, a reduced table) and tests/test_gpu_front.py (the device library, the full tables) run the same cases through the same code.

Rules every case follows: the image lies between NaN guards (the stem reads it through plain pointers: a read outside the image poisons the result);
outputs are slabs with a pixel stride larger than the payload, a non-zero channel offset, the sentinel around the payload AND in TAIL pixels behind the
last one (a wave tile dealt past the end of the batch lands there); inputs are signed, all biases are non-zero (a stem pixel outside the stem image
computed as SiLU(b0) instead of 1.Conv's zero padding shows up); filter columns a kernel must not read hold NaN.

References are float64 on the operands as stored:
    A  raw stem on small integers: every partial sum is an integer below 2048, the result is exact in any order -> bit equality;
    B  stem: r = SiLU(v); |got - r| <= max(2^-11 |r|, 2^-24) + 1.1 g S + 2^-18 |r|, g = 4 x max(torch fp32 CPU conv2d against float64 in units of S, 2^-22);
    C  front: the float64 chain with t0 and t1 rounded to fp16 where the three-launch form stores them, rtol 5e-3 / atol 5e-3;
    D  the same launch under another deal of tiles to workgroups, or at another batch position: bit equality."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import torch
import torch.nn.functional as F

from tests.train_glue_ref import F16, F32, SENT, Guarded, Slab, _seed, assert_bits_equal, ok
from yolov5_amd import _lib
from yolov5_amd.packing import pack_conv_weight, pack_stem_weight

TAIL = 128                                   # sentinel pixels behind the last output pixel (four wave tiles of the stem)
SUM_FLOOR, SUM_FACTOR = 2.0 ** -22, 4.0      # the yardstick of DESIGN.md 4.1a / 4.1b
SILU_SLOPE, EXP_RCP = 1.1, 2.0 ** -18        # |SiLU'| <= 1.0998; __expf + v_rcp_f32 at |v| <= 16
V_MAX = 16.0
MBS_GPU = (1, 2, 5, 7, 8, 9, 16, 0, 10000)   # 9: G &= ~7; 10 000: the clamp to the tile count
MBS_EMU = (1, 2, 0)

# (B, H, W, C2, max_blocks)
STEM_CASES = [
    (1, 2, 64, 8, 1),        # OH = 1: every row is a border row
    (2, 6, 128, 16, 0),      # small base case
    (3, 34, 192, 40, 3),     # C2 tail inside Npad 64; 153 wave tiles: not a multiple of 4, 39 workgroup tiles on 3 workgroups
    (1, 10, 64, 48, 1),      # one workgroup walks everything
    (4, 64, 256, 32, 3),     # 512 wave tiles on 3 workgroups: the rings reach steady state and drain
    (2, 64, 64, 64, 0),      # Npad 64, full channel count
    (1, 22, 192, 8, 1),      # 33 wave tiles in 9 workgroup tiles on one workgroup: the partial tile must be the LAST step of its owner
]
STEM_BENCH = (8, 640, 640, 32, 0)            # GPU only: the benchmark's geometry at a small batch
STEM_SCHED = (4, 64, 256, 32, 0)
# the host build: at most 64 wave tiles; the C2 tail / odd wave-tile count and the Npad-64 ring at sizes it walks in a second
STEM_CASES_EMU = [STEM_CASES[0], STEM_CASES[1], (1, 10, 192, 40, 3), STEM_CASES[3], (3, 4, 64, 64, 1), STEM_CASES[5], STEM_CASES[6]]
STEM_SCHED_EMU = (2, 16, 256, 32, 0)


def _nhwc(t):
    return np.ascontiguousarray(t.permute(0, 2, 3, 1).numpy())


def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


def _bias(rng, n):
    """Non-zero: 0.1 <= |b| <= 0.5."""
    return (rng.uniform(0.1, 0.5, size=n) * rng.choice([-1.0, 1.0], size=n)).astype(F32)


def _image(rng, shape, kind):
    if kind == "int":
        return rng.choice(np.array([-3, -2, -1, 1, 2, 3], F32), size=shape).astype(F16)
    return rng.uniform(0.0 if kind == "image" else -1.0, 1.0, size=shape).astype(F32).astype(F16)


def _filter(rng, shape, fan_in):
    """He-scaled, already on the fp16 grid."""
    return (rng.standard_normal(shape) * (2.0 / fan_in) ** 0.5).astype(F32).astype(F16).astype(F32)


def _t(a):
    """A tensor of its own (the shared inputs are read-only arrays)."""
    return torch.from_numpy(np.array(a))


def _t64(a):
    return torch.from_numpy(np.array(a, np.float64))


def _r16(t):
    """Round to fp16 and back, as a store to HBM between two launches does."""
    return t.to(torch.float16).to(t.dtype)


# ---- the stem ------------------------------------------------------------------------------------------------------------------------------------------
def stem_reference(x, w, b):
    """float64 conv (+ bias) as NHWC; with a bias also S, torch's fp32 result before the activation and its error in units of S."""
    v = F.conv2d(_t64(x), _t64(w), None if b is None else _t64(b), 2, 2)
    if b is None:
        return _nhwc(v), None, None, None
    S = F.conv2d(_t64(x).abs(), _t64(w).abs(), _t64(b).abs(), 2, 2)
    t32 = F.conv2d(_t(x).float(), _t(w), _t(b), 2, 2)
    et = float(((t32.double() - v).abs() / S).max())
    return _nhwc(v), _nhwc(S), _nhwc(F.silu(t32)), et


@functools.lru_cache(maxsize=3)
def stem_inputs(shape, kind):
    """shape = (B, H, W, C2); kind 'int' (part A), 'signed' or 'image' (part B).  Read-only, shared by every test of the shape."""
    B, H, W, C2 = shape
    rng = _seed("stem", shape, kind)
    x = _image(rng, (B, 3, H, W), kind)
    if kind == "int":
        w, b = rng.integers(-2, 3, size=(C2, 3, 6, 6)).astype(F32), None
    else:
        w, b = _filter(rng, (C2, 3, 6, 6), 108), _bias(rng, C2)
    v, S, t32, et = stem_reference(x, w, b)
    if kind == "int":
        assert np.abs(v).max() <= 648
    else:
        assert np.abs(v).max() <= V_MAX, "the bound on __expf + v_rcp_f32 was derived for |v| <= 16"
    return _frozen(x, w, b, v, S, t32) + (et,)


class StemRun:
    """The operands of one stem geometry on the backend; launch() gives the payload of a fresh output slab after the sentinel checks."""

    def __init__(self, be, shape, x, w, b):
        self.be, self.shape = be, shape
        B, H, W, C2 = shape
        wp, bp, self.npad = pack_stem_weight(_t(w), None if b is None else _t(b))
        self.x = Guarded(be, (B, 3, H, W), F16, x, fill=np.nan, guard=3 * W + 64)   # two rows above / below the image and more
        self.w = Guarded(be, wp.shape, F16, wp.numpy(), fill=np.nan)
        self.b = None if b is None else be.put(bp.numpy())
        self.npix, self.ldy, self.off = B * (H // 2) * (W // 2), C2 + 16, 8

    def slab(self):
        return Slab(self.be, self.npix + TAIL, self.shape[3], self.ldy, self.off, F16)

    def call(self, out, mb, **kw):
        B, H, W, C2 = self.shape
        a = dict(x=self.x.p, B=B, H=H, W=W, w=self.w.p, C2=C2, npad=self.npad, y=out.p, ldy=self.ldy)
        a.update(kw)
        if self.b is None:
            return self.be.lib.y5_conv_stem_fwd_raw(a["x"], a["B"], a["H"], a["W"], a["w"], a["C2"], a["npad"], a["y"], a["ldy"], mb, self.be.stream)
        return self.be.lib.y5_conv_stem_fwd(a["x"], a["B"], a["H"], a["W"], a["w"], self.be.ptr(self.b), a["C2"], a["npad"], a["y"], a["ldy"], mb,
                                            self.be.stream)

    def launch(self, mb, what="stem"):
        B, H, W, C2 = self.shape
        out = self.slab()
        ok(self.be, self.call(out, mb))
        got = out.read(f"{what} output")
        assert np.all(got[self.npix:] == SENT), f"{what}: pixels behind the end of the batch were written"
        return got[:self.npix].reshape(B, H // 2, W // 2, C2)


def run_stem_exact(be, case):
    """A: y5_conv_stem_fwd_raw on integers, bit for bit."""
    x, w, _, v, _, _, _ = stem_inputs(case[:4], "int")
    got = StemRun(be, case[:4], x, w, None).launch(case[4], f"stem raw {case}")
    assert_bits_equal(got, v.astype(F16), f"y5_conv_stem_fwd_raw {case}")


def check_stem(got, v, S, t32, et, tag):
    """B's bound per element; prints and returns (worst kernel / tolerance, kernel / torch in units of S)."""
    r = v / (1.0 + np.exp(-v))
    err = np.abs(got.astype(np.float64) - r)
    assert not np.isnan(err).any(), f"{tag}: NaN in the output (a read outside the image, or a pixel never written)"
    rnd = np.maximum(2.0 ** -11 * np.abs(r), 2.0 ** -24)
    g = SUM_FACTOR * max(et, SUM_FLOOR)
    tol = rnd + SILU_SLOPE * g * S + EXP_RCP * np.abs(r)
    frac = float((err / tol).max())
    ek = float((np.maximum(err - rnd - EXP_RCP * np.abs(r), 0.0) / (SILU_SLOPE * S)).max())
    same16 = float(np.mean(got != r.astype(F16))), float(np.mean(t32.astype(F16) != r.astype(F16)))
    print(f"\n[{tag}] worst kernel / tolerance {frac:.3f}; accumulation error {ek:.2e} S, torch fp32 {et:.2e} S, kernel / torch "
          f"{ek / max(et, SUM_FLOOR):.2f} (bound {SUM_FACTOR:g}); differs from fp16(ref) in {same16[0]:.2%} of the elements, torch fp32 in {same16[1]:.2%}")
    bad = err > tol
    assert not bad.any(), f"{tag}: {int(bad.sum())} of {bad.size} elements beyond the bound, worst {frac:.2f} x, first at {np.argwhere(bad)[0].tolist()}"
    return frac, ek / max(et, SUM_FLOOR)


def run_stem_parity(be, case, kind="signed"):
    """B: y5_conv_stem_fwd against SiLU(float64 conv + bias)."""
    x, w, b, v, S, t32, et = stem_inputs(case[:4], kind)
    got = StemRun(be, case[:4], x, w, b).launch(case[4], f"stem {case}")
    return check_stem(got, v, S, t32, et, f"stem {case} {kind}")


def run_stem_schedule(be, case, raw, mbs):
    """D: the output bits do not depend on the grid."""
    x, w, b = stem_inputs(case[:4], "int" if raw else "signed")[:3]
    r = StemRun(be, case[:4], x, w, b)
    first = r.launch(mbs[0])
    assert np.abs(first.astype(F32)).max() > 0
    for mb in mbs[1:]:
        assert_bits_equal(r.launch(mb), first, f"stem{' raw' if raw else ''} {case[:4]} max_blocks {mb} against max_blocks {mbs[0]}")


def _batch_copies(rng, shape, kind):
    """B = 5 images, the first one again at positions 1 and B - 1."""
    x = _image(rng, shape, kind)
    x[1], x[-1] = x[0], x[0]
    return x


def run_stem_batch(be, shape, raw):
    """D: the same image at batch positions 0, 1 and B - 1."""
    assert shape[0] == 5
    B, H, W, C2 = shape
    rng = _seed("stem batch", shape, raw)
    x = _batch_copies(rng, (B, 3, H, W), "int" if raw else "signed")
    w = rng.integers(-2, 3, size=(C2, 3, 6, 6)).astype(F32) if raw else _filter(rng, (C2, 3, 6, 6), 108)
    got = StemRun(be, shape, x, w, None if raw else _bias(rng, C2)).launch(0)
    assert_bits_equal(got[1], got[0], "stem: image 1 against image 0")
    assert_bits_equal(got[-1], got[0], "stem: image B - 1 against image 0")
    assert not np.array_equal(got[2], got[0])


# ---- the front -----------------------------------------------------------------------------------------------------------------------------------------
def fc(B, H, W, c1=64, c3=64, split=32, act1=1, act2=1, mb=0, kpad1=None, kpad2=None, kind="signed"):
    return (B, H, W, c1, c3, split, act1, act2, mb, kpad1, kpad2, kind)


FRONT_SHAPES = [(1, 64, 64), (2, 192, 192), (2, 64, 448), (1, 256, 64)]      # one tile; 18 tiles, one with neighbours on all sides; 7 per image (G < 8)
FRONT_BENCH = fc(2, 640, 640)                                                 # the benchmark's own shape at a small batch
FRONT_CASES = [fc(*s) for s in FRONT_SHAPES] + [
    fc(2, 192, 192, kind="image"),
    # the other three builds (Npad1, Npad2); Kpad2 = 64 > Npad1 = 32 in two of them
    fc(2, 192, 192, c1=32, c3=32, split=16), fc(1, 256, 64, c1=64, c3=32, split=16), fc(2, 64, 448, c1=32, c3=64, split=32),
    # channel tails: the partial last block takes the vmcnt(0) path
    fc(2, 192, 192, c1=56, c3=48, split=16, mb=3), fc(1, 256, 64, c1=24, c3=16, split=8, mb=1),
    # split_n: everything to y2, everything to y (y2 = NULL), 8, and 24 of 48 (the lanes of one store instruction go to different outputs)
    fc(2, 64, 448, split=0, mb=2), fc(2, 192, 192, split=64), fc(1, 256, 64, split=8), fc(2, 192, 192, c1=56, c3=48, split=24),
    fc(2, 192, 192, act1=0, mb=5), fc(1, 256, 64, act2=0),
    # filter rows wider than the kernel reads (NaN behind column 288 / Npad1) and as tight as it accepts
    fc(1, 256, 64, kpad1=352, kpad2=128, mb=1), fc(2, 64, 448, c1=32, c3=32, split=16, kpad1=288, kpad2=32),
]
FRONT_SCHED = fc(2, 192, 192)
# the host build: up to 4 tiles, every build, both tails, every split form, both activations off
FRONT_CASES_EMU = [
    fc(1, 64, 64), fc(1, 128, 128, mb=1), fc(1, 64, 64, kind="image"), fc(1, 64, 128, c1=32, c3=32, split=16, mb=1), fc(1, 64, 64, c1=64, c3=32, split=16),
    fc(1, 128, 64, c1=32, c3=64, split=0, mb=1), fc(2, 64, 64, c1=56, c3=48, split=24, mb=1), fc(1, 64, 64, c1=24, c3=16, split=8), fc(1, 64, 64, split=64),
    fc(1, 64, 64, act1=0, split=8), fc(1, 64, 64, act2=0), fc(1, 64, 128, kpad1=352, kpad2=128, mb=1),
]
FRONT_SCHED_EMU = fc(1, 128, 128)


def front_chain(x, ws, act1, act2, dtype):
    """The three layers in `dtype` with t0 and t1 rounded to fp16 where the three-launch form stores them; the result is NOT rounded."""
    w0, b0, w1, b1, w2, b2 = (_t(a).to(dtype) for a in ws)
    t0 = _r16(F.silu(F.conv2d(_t(x).to(dtype), w0, b0, 2, 2)))
    t1 = F.conv2d(t0, w1, b1, 2, 1)
    t1 = _r16(F.silu(t1) if act1 else t1)
    r = F.conv2d(t1, w2, b2)
    return _nhwc(F.silu(r) if act2 else r)


def front_weights(rng, c1, c3):
    return _frozen(_filter(rng, (32, 3, 6, 6), 108), _bias(rng, 32), _filter(rng, (c1, 32, 3, 3), 288), _bias(rng, c1),
                   _filter(rng, (c3, c1, 1, 1), c1), _bias(rng, c3))


@functools.lru_cache(maxsize=4)
def front_inputs(key):
    """key = (B, H, W, c1, c3, act1, act2, kind) -> x, weights, float64 chain, torch fp32 chain.  Read-only, shared by every case of the key."""
    B, H, W, c1, c3, act1, act2, kind = key
    rng = _seed("front", key)
    x = _image(rng, (B, 3, H, W), kind)
    ws = front_weights(rng, c1, c3)
    ref = front_chain(x, ws, act1, act2, torch.float64)
    t32 = front_chain(x, ws, act1, act2, torch.float32)
    return _frozen(x)[0], ws, _frozen(ref)[0], _frozen(t32)[0]


def _key(case):
    B, H, W, c1, c3, _, act1, act2, _, _, _, kind = case
    return (B, H, W, c1, c3, act1, act2, kind)


def _widen(wp, k_read, kpad):
    """A packed filter with row pitch `kpad`: the first k_read columns are what the kernel reads, NaN behind them."""
    out = np.full((wp.shape[0], kpad), np.nan, F16)
    out[:, :k_read] = wp[:, :k_read]
    return out


class FrontRun:
    def __init__(self, be, case, x, ws):
        self.be, self.case = be, case
        B, H, W, c1, c3, split, _, _, _, kpad1, kpad2, _ = case
        w0, b0, w1, b1, w2, b2 = (_t(a) for a in ws)
        w0p, b0p, n0 = pack_stem_weight(w0, b0)
        w1p, b1p, _, K1, self.N1 = pack_conv_weight(w1, b1, torch.float16)
        w2p, b2p, _, K2, self.N2 = pack_conv_weight(w2, b2, torch.float16)
        assert n0 == 32 and K1 == 320 and K2 >= self.N1
        self.K1, self.K2 = kpad1 or K1, kpad2 or K2
        w1p = _widen(w1p.numpy(), 288, self.K1)
        w2p = _widen(w2p.numpy(), self.N1, self.K2)
        self.x = Guarded(be, (B, 3, H, W), F16, x, fill=np.nan, guard=3 * W + 64)
        self.w = [Guarded(be, a.shape, F16, a, fill=np.nan) for a in (w0p.numpy(), w1p, w2p)]
        self.b = [be.put(a.numpy()) for a in (b0p, b1p, b2p)]
        self.npix = B * (H // 4) * (W // 4)
        self.ldy, self.ld2 = split + 16, (c3 - split) + 24

    def slabs(self):
        c3, split = self.case[4:6]
        y = Slab(self.be, self.npix + TAIL, split, self.ldy, 8, F16)
        y2 = Slab(self.be, self.npix + TAIL, c3 - split, self.ld2, 16, F16) if split < c3 else None
        return y, y2

    def call(self, sy, sy2, mb, **kw):
        B, H, W, c1, c3, split, act1, act2 = self.case[:8]
        a = dict(x=self.x.p, B=B, H=H, W=W, c0=32, c1=c1, N1=self.N1, K1=self.K1, c3=c3, N2=self.N2, K2=self.K2, y=None if sy is None else sy.p, ldy=self.ldy,
                 y2=None if sy2 is None else sy2.p, ld2=self.ld2 if sy2 is not None else 0, split=split)
        a.update(kw)
        be = self.be
        return be.lib.y5_conv_front_fwd(a["x"], a["B"], a["H"], a["W"], self.w[0].p, be.ptr(self.b[0]), a["c0"], self.w[1].p, be.ptr(self.b[1]), a["c1"],
                                        a["N1"], a["K1"], act1, self.w[2].p, be.ptr(self.b[2]), a["c3"], a["N2"], a["K2"], act2, a["y"], a["ldy"], a["y2"],
                                        a["ld2"], a["split"], mb, be.stream)

    def launch(self, mb, what="front"):
        B, H, W, _, c3, split = self.case[:6]
        y, y2 = self.slabs()
        ok(self.be, self.call(y, y2, mb))
        parts = [s.read(f"{what} {'y2' if i else 'y'}") for i, s in enumerate((y, y2)) if s is not None]
        for p in parts:
            assert np.all(p[self.npix:] == SENT), f"{what}: pixels behind the end of the batch were written"
        return np.concatenate([p[:self.npix] for p in parts], axis=1).reshape(B, H // 4, W // 4, c3)


def ulp16(a):
    """Spacing of fp16 at |a| (subnormal spacing below 2^-14)."""
    e = np.floor(np.log2(np.maximum(np.abs(a), 2.0 ** -14)))
    return 2.0 ** (e - 10)


def check_front(got, ref, t32, tag):
    """C: rtol 5e-3 / atol 5e-3 against the float64 chain, beside the reference-side yardstick."""
    g64 = got.astype(np.float64)
    assert not np.isnan(g64).any(), f"{tag}: NaN in the output (a pixel never written, or a filter column that must not be read)"
    err = np.abs(g64 - ref)
    E = float(np.abs(t32.astype(np.float64) - ref).max())
    yard = float((err / (ulp16(ref) + 4.0 * E)).max())
    r16 = ref.astype(F16)
    print(f"\n[{tag}] worst |kernel - ref| {err.max():.3e} = {float((err / (5e-3 + 5e-3 * np.abs(ref))).max()):.3f} of the tolerance, {yard:.2f} x (ulp16(ref) + 4 E) "
          f"with E = {E:.2e}; differs from fp16(ref) in {float(np.mean(got != r16)):.2%} of the elements, torch's fp32 chain in "
          f"{float(np.mean(t32.astype(F16) != r16)):.2%}")
    np.testing.assert_allclose(g64, ref, rtol=5e-3, atol=5e-3, err_msg=tag)
    return yard


def run_front_parity(be, case):
    x, ws, ref, t32 = front_inputs(_key(case))
    got = FrontRun(be, case, x, ws).launch(case[8], f"front {case}")
    return check_front(got, ref, t32, f"front {case}")


def run_front_schedule(be, case, mbs):
    x, ws = front_inputs(_key(case))[:2]
    r = FrontRun(be, case, x, ws)
    first = r.launch(mbs[0])
    for mb in mbs[1:]:
        assert_bits_equal(r.launch(mb), first, f"front {case[:3]} max_blocks {mb} against max_blocks {mbs[0]}")


def run_front_batch(be, case):
    assert case[0] == 5
    rng = _seed("front batch", case)
    x = _batch_copies(rng, (5, 3) + case[1:3], "signed")
    got = FrontRun(be, case, x, front_weights(rng, case[3], case[4])).launch(case[8])
    assert_bits_equal(got[1], got[0], "front: image 1 against image 0")
    assert_bits_equal(got[-1], got[0], "front: image B - 1 against image 0")
    assert not np.array_equal(got[2], got[0])


# ---- E. repeatability under load (GPU only) ------------------------------------------------------------------------------------------------------------
def _repeat(be, launch, buffers, runs=40):
    """`launch` 40 times into sentinel-filled `buffers`, alternating with a 64 MiB copy on a second stream; every run bit-identical to the first.
    Returns the first run's buffers."""
    side = torch.cuda.Stream(be.dev)
    junk_a = torch.empty(64 << 20, dtype=torch.uint8, device=be.dev)
    junk_b = torch.empty_like(junk_a)
    first = None
    for it in range(runs):
        for h in buffers:
            h.fill_(SENT)
        if it % 2:
            with torch.cuda.stream(side):
                junk_b.copy_(junk_a)
        ok(be, launch())
        torch.cuda.synchronize(be.dev)
        if first is None:
            first = [h.clone() for h in buffers]
        else:
            for h, f in zip(buffers, first):
                assert torch.equal(h.view(torch.int16), f.view(torch.int16)), \
                    f"run {it} differs from run 0 in {int((h.view(torch.int16) != f.view(torch.int16)).sum())} elements"
    torch.cuda.synchronize(be.dev)
    return first


def run_stem_repeat(be):
    """The stem at the benchmark's geometry (STEM_BENCH, 8 x 3 x 640 x 640); the first run is held to B on its first and last image."""
    shape = STEM_BENCH[:4]
    x, w, b, v, S, t32, et = stem_inputs(shape, "signed")
    r = StemRun(be, shape, x, w, b)
    out = r.slab()
    first = _repeat(be, lambda: r.call(out, 0), [out.h])[0]
    out.h.copy_(first)
    got = out.read("stem repeat")[:r.npix].reshape(v.shape)
    for i in (0, -1):
        check_stem(got[i], v[i], S[i], t32[i], et, f"stem repeat, image {i}")


def run_front_repeat(be):
    """The front at 4 x 3 x 640 x 640, (64, 64) build, default grid: FRONT_BENCH's two images twice, so that the first and the last image have FRONT_BENCH's
    reference; the first run is held to C on them."""
    x2, ws, ref, t32 = front_inputs(_key(FRONT_BENCH))
    case = fc(4, 640, 640)
    r = FrontRun(be, case, np.concatenate([x2, x2]), ws)
    y, y2 = r.slabs()
    first = _repeat(be, lambda: r.call(y, y2, 0), [y.h, y2.h])
    y.h.copy_(first[0])
    y2.h.copy_(first[1])
    got = np.concatenate([s.read("front repeat")[:r.npix] for s in (y, y2)], axis=1).reshape((4,) + ref.shape[1:])
    check_front(got[0], ref[0], t32[0], "front repeat, image 0")
    check_front(got[-1], ref[1], t32[1], "front repeat, image B - 1")


# ---- G. refusals ---------------------------------------------------------------------------------------------------------------------------------------
BAD, UNS = _lib.Y5_ERR_BAD_ARG, _lib.Y5_ERR_UNSUPPORTED


def _untouched(slab, what):
    got = slab.read(what)
    assert np.all(got == SENT), f"{what}: the refused call wrote its output"


def run_front_refusals(be):
    """Every refusal of front.hip that tests/test_emu_front.py does not reach: the status, the message, and nothing written."""
    case = fc(1, 64, 128, split=32)
    rng = _seed("front refusals")
    r = FrontRun(be, case, _image(rng, (1, 3, 64, 128), "signed"), front_weights(rng, 64, 64))
    y, y2 = r.slabs()
    ok(be, r.call(y, y2, 0))
    probes = [
        (dict(W=96), UNS, b"W % 64"), (dict(N1=96), UNS, b"3x3 layer"), (dict(K1=280), UNS, b"3x3 layer"), (dict(K2=56), UNS, b"pointwise layer"),
        (dict(ldy=r.ldy + 4), BAD, b"multiples of 8"), (dict(ld2=r.ld2 + 4), BAD, b"multiples of 8"),
        (dict(x=be.ptr(r.x.h, r.x.lo * 2 + 2)), BAD, b"16-byte aligned"), (dict(y="shift"), BAD, b"16-byte aligned"),
        (dict(y2=None), BAD, b"needs y2"),
    ]
    for kw, status, msg in probes:
        y, y2 = r.slabs()
        if kw.get("y") == "shift":
            kw = dict(y=be.ptr(y.h, (y.off + 1) * 2))
        rc = r.call(y, y2, 0, **kw)
        err = be.lib.y5_last_error()
        assert rc == status and msg in err, f"front {sorted(kw)}: status {rc}, {err!r}; expected {status} with {msg!r}"
        _untouched(y, f"front refusal {sorted(kw)}: y")
        _untouched(y2, f"front refusal {sorted(kw)}: y2")


def run_stem_refusals(be):
    rng = _seed("stem refusals")
    shape = (1, 8, 128, 16)
    for raw in (False, True):
        r = StemRun(be, shape, _image(rng, (1, 3, 8, 128), "signed"), _filter(rng, (16, 3, 6, 6), 108), None if raw else _bias(rng, 16))
        name = b"conv_stem_raw" if raw else b"conv_stem"
        ok(be, r.call(r.slab(), 0))
        probes = [
            (dict(H=7), UNS, b"even H"), (dict(W=96), UNS, b"W % 64"), (dict(C2=12), UNS, b"multiple of 8"), (dict(C2=72, npad=64), UNS, b"<= 64"),
            (dict(C2=72, npad=96), UNS, b"<= 64"), (dict(ldy=r.ldy + 4), UNS, b"multiple of 8"), (dict(x=be.ptr(r.x.h, r.x.lo * 2 + 2)), BAD, b"16-byte aligned"),
            (dict(y="shift"), BAD, b"16-byte aligned"),
        ]
        for kw, status, msg in probes:
            out = r.slab()
            if kw.get("y") == "shift":
                kw = dict(y=be.ptr(out.h, (out.off + 1) * 2))
            rc = r.call(out, 0, **kw)
            err = be.lib.y5_last_error()
            assert rc == status and msg in err and err.startswith(name + b":"), f"stem {sorted(kw)}: status {rc}, {err!r}; expected {status} with {msg!r}"
            _untouched(out, f"stem refusal {sorted(kw)}")


# ---- G. the size guards (GPU only) ---------------------------------------------------------------------------------------------------------------------
BIG_B, BIG_HW = 873, 640        # 873 x 3 x 640 x 640: 2 145 484 800 bytes < 2^31 - 1, 1 072 742 400 elements < 2^30 - 1; 874 images are over both


def _big_image(be, B, last):
    """(B, 3, 640, 640) fp16 on the device between NaN guards: zeros, the last image = `last`."""
    n, guard = B * 3 * BIG_HW * BIG_HW, 3 * BIG_HW + 64
    flat = torch.zeros(guard + n + guard, dtype=torch.float16, device=be.dev)
    flat[:guard] = float("nan")
    flat[guard + n:] = float("nan")
    flat[guard + n - last.size:guard + n] = _t(last.reshape(-1)).to(be.dev)
    return flat, C.c_void_p(flat.data_ptr() + guard * 2)


def _big_slab(be, npix, Cc, ld, off):
    h = torch.full((npix + TAIL, ld), SENT, dtype=torch.float16, device=be.dev)
    return h, C.c_void_p(h.data_ptr() + off * 2)


def _big_read(h, npix, Cc, off, img_pix, what):
    """Sentinel checks on the device; the first and the last image's payload come to the host."""
    torch.cuda.synchronize()
    assert bool((h[:, :off] == SENT).all()) and bool((h[:, off + Cc:] == SENT).all()), f"{what}: columns around the payload were written"
    assert bool((h[npix:] == SENT).all()), f"{what}: pixels behind the end of the batch were written"
    return h[:img_pix, off:off + Cc].cpu().numpy(), h[npix - img_pix:npix, off:off + Cc].cpu().numpy()


def run_stem_size_guard(be, over):
    """An input just under 2^30 elements runs and its LAST image is right by B (offsets are int arithmetic cast to unsigned); just over, refused."""
    B = BIG_B + (1 if over else 0)
    assert (B * 3 * BIG_HW * BIG_HW >= 0x3fffffff) == over
    shape = (1, BIG_HW, BIG_HW, 8)
    x, w, b, v, S, t32, et = stem_inputs(shape, "signed")
    wp, bp, npad = pack_stem_weight(_t(w), _t(b))
    xbuf, xp = _big_image(be, B, x)
    wd, bd = wp.to(be.dev), bp.to(be.dev)
    img = (BIG_HW // 2) ** 2
    h, yp = _big_slab(be, B * img, 8, 16, 8)
    rc = be.lib.y5_conv_stem_fwd(xp, B, BIG_HW, BIG_HW, C.c_void_p(wd.data_ptr()), C.c_void_p(bd.data_ptr()), 8, npad, yp, 16, 0, be.stream)
    if over:
        assert rc == UNS and b"exceeds 2^30" in be.lib.y5_last_error(), (rc, be.lib.y5_last_error())
        torch.cuda.synchronize()
        assert bool((h == SENT).all()), "the refused call wrote its output"
        return
    ok(be, rc)
    head, last = _big_read(h, B * img, 8, 8, img, "stem under 2^30 elements")
    check_stem(last.reshape(v.shape[1:]), v[0], S[0], t32[0], et, "stem under 2^30 elements, last image")
    # an all-zero image: SiLU(bias) in the interior
    bias_out = (b.astype(np.float64) / (1.0 + np.exp(-b.astype(np.float64))))
    assert np.abs(head.reshape(v.shape[1:])[8, 8].astype(np.float64) - bias_out).max() <= 2.0 ** -10


def run_front_size_guard(be, over):
    """An input just under 2^31 bytes runs and its LAST image is right by C; just over, refused."""
    B = BIG_B + (1 if over else 0)
    assert (B * 3 * BIG_HW * BIG_HW * 2 >= 0x7fffffff) == over
    case = fc(1, BIG_HW, BIG_HW, c1=24, c3=16, split=16)
    x, ws, ref, t32 = front_inputs(_key(case))
    r = FrontRun(be, case, x, ws)          # the filters and biases; its own one-image input is not used
    xbuf, xp = _big_image(be, B, x)
    img = (BIG_HW // 4) ** 2
    h, yp = _big_slab(be, B * img, 16, 32, 8)
    rc = r.call(None, None, 0, x=xp, B=B, y=yp, ldy=32, y2=None, ld2=0)
    if over:
        assert rc == UNS and b"exceeds 2^31" in be.lib.y5_last_error(), (rc, be.lib.y5_last_error())
        torch.cuda.synchronize()
        assert bool((h == SENT).all()), "the refused call wrote its output"
        return
    ok(be, rc)
    _, last = _big_read(h, B * img, 16, 8, img, "front under 2^31 bytes")
    check_front(last.reshape(ref.shape[1:]), ref[0], t32[0], "front under 2^31 bytes, last image")
