"""TEST INFRASTRUCTURE ONLY: every op kind of the C-side execution plan (yolov5_amd/csrc/core.hip, y5_plan_*) against the direct entry point it
launches.  One case per kind: fixed inputs, the direct call (y5_X_fwd, y5_nchw_to_nhwc, ...) into one set of output buffers, y5_plan_add_X + y5_plan_run
into a second set, and the two sets equal bit for bit -- a plan op only carries arguments, so any difference is an argument that travelled wrong.  Every
runner takes a backend of tests/train_glue_ref.py: tests/test_emu_plan_ops.py (the kernels compiled for the host) and tests/test_gpu_plan_ops.py (the
device library) run the same cases through the same code.

Rules every case follows: the smallest shape its entry point accepts; every scalar argument differs from its neighbours in the argument list where the
entry point allows it (ldx != ldy != ld2, Kpad1 != Kpad2, C3 != C, both values of act3 / add, split_n set), so that two swapped fields cannot cancel;
output buffers hold a sentinel first and are compared WHOLE (payload and everything around it).

On the same plans: y5_plan_rebind_output moves every output the plan may re-point (main output, second output, objectness plane) and nothing else --
the address of an input, a Bottleneck's bias2 among them, is refused with "no op writes that pointer"; the setters (y5_plan_set_input / _set_anchors /
_set_obj_hint / _set_conv_cfg) act exactly like a direct call with the new value and are refused on every other kind; y5_plan_add_nop keeps indices; a
side-branch op gives the same bits; a captured range (GPU) gives the same bits."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from tests import front_ref as fr
from tests.train_glue_ref import F16, F32, SENT, U8, Guarded, _seed, _vals, assert_bits_equal, ok
from yolov5_amd import _lib
from yolov5_amd.packing import pack_conv_weight

BAD = _lib.Y5_ERR_BAD_ARG
DT16, DT32, DTU8 = _lib.Y5_F16, _lib.Y5_F32, _lib.Y5_U8


def _sent(shape, dtype=F16):
    return np.full(shape, SENT, dtype)


def _filter(rng, c2, c1, k):
    """He-scaled filter and a non-zero bias, fp32 torch tensors."""
    w = rng.standard_normal((c2, c1, k, k)).astype(F32) * (2.0 / (c1 * k * k)) ** 0.5
    b = (rng.uniform(0.1, 0.5, size=c2) * rng.choice([-1.0, 1.0], size=c2)).astype(F32)
    return torch.from_numpy(w), torch.from_numpy(b)


class Case:
    """One op kind: `inputs` (every address the op only reads), fresh() (the initial content of its output buffers), direct(p) and add(plan, p) with
    p = the output addresses.  second / hint: index in fresh() of the second re-pointable output / shape and dtype of the objectness plane."""
    kind, second, hint, reads_input, is_conv = "", None, None, False, False

    def __init__(self, be):
        self.be, self.lib, self.keep, self.inputs = be, be.lib, [], []

    def dev(self, a):
        """An input on the backend; its address is remembered as one that no op writes."""
        h = self.be.put(np.ascontiguousarray(a))
        self.keep.append(h)
        p = self.be.ptr(h)
        self.inputs.append(p)
        return p

    def packed(self, w, b, widen=0):
        """Packed fp16 filter (optionally with a row pitch `widen` columns wider, zeros behind the columns the pack holds) + bias on the backend."""
        wp, bp, _, K, N = pack_conv_weight(w, b, torch.float16)
        wp = wp.numpy()
        if widen:
            wide = np.zeros((wp.shape[0], K + widen), F16)
            wide[:, :K] = wp
            wp, K = wide, K + widen
        return self.dev(wp), self.dev(bp.numpy()), K, N

    @property
    def st(self):
        return self.be.stream


class Conv(Case):
    """1x1 64 -> 64 with the split store: channels [0, 32) to y, [32, 64) to y2."""
    kind, second, is_conv = "conv", 1, True

    def __init__(self, be):
        super().__init__(be)
        rng = _seed("plan conv")
        self.npix = 1 * 4 * 8
        self.w, self.b, K, N = self.packed(*_filter(rng, 64, 64, 1))
        self.x = self.dev(_vals(rng, (self.npix, 72), F16, -1.0, 1.0))
        self.d = _lib.ConvDesc(dtype=DT16, B=1, H=4, W=8, C1=64, ldx=72, OH=4, OW=8, C2=64, ldy=40, KH=1, KW=1, SH=1, SW=1, PH=0, PW=0, act=1, Kpad=K, Npad=N,
                               ldr=0, ld2=48, cfg=-1, max_blocks=0, split_n=32)

    def fresh(self):
        return [_sent((self.npix, 40)), _sent((self.npix, 48))]

    def direct(self, p):
        return self.lib.y5_conv2d_fwd(C.byref(self.d), self.x, self.w, self.b, None, p[0], p[1], self.st)

    def add(self, plan, p):
        return self.lib.y5_plan_add_conv(plan, C.byref(self.d), self.x, self.w, self.b, None, p[0], p[1])


class ToNhwc(Case):
    kind, reads_input = "to_nhwc", True
    B, Cc, H, W, ld, scale = 2, 3, 5, 7, 8, 1.0 / 255.0

    def __init__(self, be):
        super().__init__(be)
        n = self.B * self.Cc * self.H * self.W
        self.x = self.dev((np.arange(n) * 7 % 256).astype(U8))
        self.x_alt = self.dev((np.arange(n) * 11 % 256).astype(U8))

    def fresh(self):
        return [_sent((self.B, self.H, self.W, self.ld))]

    def direct(self, p, x=None):
        return self.lib.y5_nchw_to_nhwc(x or self.x, DTU8, p[0], DT16, self.B, self.Cc, self.H, self.W, self.ld, self.scale, self.st)

    def add(self, plan, p):
        return self.lib.y5_plan_add_nchw_to_nhwc(plan, self.x, DTU8, p[0], DT16, self.B, self.Cc, self.H, self.W, self.ld, self.scale)


class ToNchw(Case):
    kind = "to_nchw"
    B, Cc, H, W, ld = 2, 3, 5, 7, 8

    def __init__(self, be):
        super().__init__(be)
        self.x = self.dev(_vals(_seed("plan to_nchw"), (self.B * self.H * self.W, self.ld), F32))

    def fresh(self):
        return [_sent((self.B, self.Cc, self.H, self.W), F32)]

    def direct(self, p):
        return self.lib.y5_nhwc_to_nchw(self.x, DT32, p[0], self.B, self.Cc, self.H, self.W, self.ld, self.st)

    def add(self, plan, p):
        return self.lib.y5_plan_add_nhwc_to_nchw(plan, self.x, DT32, p[0], self.B, self.Cc, self.H, self.W, self.ld)


class SppfFront(Case):
    """SPPF.cv1 (32 -> 64) + the three pools into four slices of the concat buffer."""
    kind = "sppf_front"
    B, H, W, C1, c_, k, ldx, ld = 2, 5, 7, 32, 64, 3, 40, 264

    def __init__(self, be):
        super().__init__(be)
        rng = _seed("plan sppf_front")
        self.w, self.b, self.K, _ = self.packed(*_filter(rng, self.c_, self.C1, 1), widen=8)
        self.x = self.dev(_vals(rng, (self.B * self.H * self.W, self.ldx), F16, -1.0, 1.0))

    def fresh(self):
        return [_sent((self.B * self.H * self.W, self.ld))]

    def direct(self, p):
        return self.lib.y5_sppf_cv1_pool_fwd(self.x, self.ldx, self.w, self.b, self.K, p[0], self.ld, self.B, self.H, self.W, self.C1, self.c_, self.k, 1, self.st)

    def add(self, plan, p):
        return self.lib.y5_plan_add_sppf_cv1_pool(plan, self.x, self.ldx, self.w, self.b, self.K, p[0], self.ld, self.B, self.H, self.W, self.C1, self.c_, self.k, 1)


class SppfPool(Case):
    """In place: slice 0 of the buffer is the input, slices 1..3 are written."""
    kind = "sppf_pool"
    B, H, W, Cc, ld, k = 2, 3, 5, 8, 40, 3

    def __init__(self, be):
        super().__init__(be)
        self.x0 = _vals(_seed("plan sppf_pool"), (self.B * self.H * self.W, self.Cc), F16)

    def fresh(self):
        a = _sent((self.B * self.H * self.W, self.ld))
        a[:, :self.Cc] = self.x0
        return [a]

    def direct(self, p):
        return self.lib.y5_sppf_pool(p[0], DT16, self.B, self.H, self.W, self.Cc, self.ld, self.k, self.st)

    def add(self, plan, p):
        return self.lib.y5_plan_add_sppf_pool(plan, p[0], DT16, self.B, self.H, self.W, self.Cc, self.ld, self.k)


class Upsample(Case):
    kind = "upsample"
    B, H, W, Cc, lds, ldd = 2, 3, 5, 8, 16, 24

    def __init__(self, be):
        super().__init__(be)
        self.x = self.dev(_vals(_seed("plan upsample"), (self.B * self.H * self.W, self.lds), F16))

    def fresh(self):
        return [_sent((self.B * 4 * self.H * self.W, self.ldd))]

    def direct(self, p):
        return self.lib.y5_upsample2x(self.x, DT16, p[0], self.B, self.H, self.W, self.Cc, self.lds, self.ldd, self.st)

    def add(self, plan, p):
        return self.lib.y5_plan_add_upsample2x(plan, self.x, DT16, p[0], self.B, self.H, self.W, self.Cc, self.lds, self.ldd)


class Copy(Case):
    kind = "copy"
    npix, Cc, lds, ldd = 7, 8, 16, 24

    def __init__(self, be):
        super().__init__(be)
        self.x = self.dev(_vals(_seed("plan copy"), (self.npix, self.lds), F16))

    def fresh(self):
        return [_sent((self.npix, self.ldd))]

    def direct(self, p):
        return self.lib.y5_copy_slice(self.x, DT16, p[0], self.npix, self.Cc, self.lds, self.ldd, self.st)

    def add(self, plan, p):
        return self.lib.y5_plan_add_copy_slice(plan, self.x, DT16, p[0], self.npix, self.Cc, self.lds, self.ldd)


def _anchors(vals):
    return (C.c_float * len(vals))(*vals)


class Decode(Case):
    """fp16 logits -> fp32 z (so that dt != zdt) + the raw copy; the objectness plane has z's dtype."""
    kind, second = "decode", 1
    B, ny, nx, na, no, nm, ld, stride, row_off = 2, 3, 5, 3, 7, 2, 24, 8.0, 4
    nrows = 4 + 3 * 15 + 11
    hint = ((B, nrows), F32)

    def __init__(self, be):
        super().__init__(be)
        self.x = self.dev(_vals(_seed("plan decode"), (self.B * self.ny * self.nx, self.ld), F16, -2.0, 2.0))
        self.anchors, self.anchors_alt = _anchors([10.0, 13.0, 16.0, 30.0, 33.0, 23.0]), _anchors([30.0, 61.0, 62.0, 45.0, 59.0, 119.0])

    def fresh(self):
        return [_sent((self.B, self.nrows, self.no), F32), _sent((self.B * self.na * self.ny * self.nx * self.no + 8,))]

    def direct(self, p, anchors=None, hint=None):
        return self.lib.y5_detect_decode_hint(self.x, DT16, self.B, self.ny, self.nx, self.na, self.no, self.nm, self.ld, self.stride, anchors or self.anchors,
                                              p[0], DT32, self.nrows, self.row_off, p[1], hint, self.st)

    def add(self, plan, p):
        return self.lib.y5_plan_add_detect_decode(plan, self.x, DT16, self.B, self.ny, self.nx, self.na, self.no, self.nm, self.ld, self.stride, self.anchors,
                                                  p[0], DT32, self.nrows, self.row_off, p[1])


class Head(Case):
    """The fused Detect head on the 8 x 16 grid of tests/test_emu_head.py (128 -> 3 x 85)."""
    kind = "head"
    B, ny, nx, ldx, stride, row_off = 1, 8, 16, 136, 8.0, 8
    nrows = 8 + 3 * 128 + 16
    hint = ((B, nrows), F16)

    def __init__(self, be):
        super().__init__(be)
        rng = _seed("plan head")
        w = torch.from_numpy(rng.uniform(-0.25, 0.25, size=(255, 128, 1, 1)).astype(F32))
        b = torch.from_numpy(rng.uniform(-2.0, 1.0, size=255).astype(F32))
        self.w, self.b, K, N = self.packed(w, b)
        self.x = self.dev(_vals(rng, (self.B * self.ny * self.nx, self.ldx), F16, -1.0, 1.0))
        self.d = _lib.ConvDesc(dtype=DT16, B=self.B, H=self.ny, W=self.nx, C1=128, ldx=self.ldx, OH=self.ny, OW=self.nx, C2=256, ldy=256, KH=1, KW=1, SH=1, SW=1,
                               PH=0, PW=0, act=0, Kpad=K, Npad=N, ldr=0, ld2=0, cfg=56, max_blocks=0)
        self.anchors, self.anchors_alt = _anchors([10.0, 13.0, 16.0, 30.0, 33.0, 23.0]), _anchors([30.0, 61.0, 62.0, 45.0, 59.0, 119.0])

    def fresh(self):
        return [_sent((self.B, self.nrows, 85))]

    def direct(self, p, anchors=None, hint=None):
        return self.lib.y5_detect_head_fwd_hint(C.byref(self.d), self.x, self.w, self.b, self.ny, self.nx, self.stride, anchors or self.anchors, p[0], self.nrows,
                                                self.row_off, hint, self.st)

    def add(self, plan, p):
        return self.lib.y5_plan_add_detect_head(plan, C.byref(self.d), self.x, self.w, self.b, self.ny, self.nx, self.stride, self.anchors, p[0], self.nrows,
                                                self.row_off)


class Bneck(Case):
    """(C, B, H, W, add): 32 and 64 channels on one 4 x 8 tile, 128 channels on a few pixels."""
    SHAPES = {"bneck32": (32, 1, 4, 8, 1), "bneck64": (64, 1, 4, 8, 0), "bneck128": (128, 1, 3, 5, 1)}

    def __init__(self, be, kind):
        super().__init__(be)
        self.kind = kind
        self.Cc, self.B, self.H, self.W, self.add_ = Cc, B, H, W, _ = self.SHAPES[kind]
        rng = _seed("plan", kind)
        self.ldx, self.ldy = Cc + 8, Cc + 16
        self.w1, self.b1, self.K1, _ = self.packed(*_filter(rng, Cc, Cc, 1), widen=24)
        self.w2, self.b2, self.K2, _ = self.packed(*_filter(rng, Cc, Cc, 3))
        self.x = self.dev(_vals(rng, (B * H * W, self.ldx), F16, -1.0, 1.0))

    def fresh(self):
        return [_sent((self.B * self.H * self.W, self.ldy))]

    def args(self, p):
        return (self.x, self.ldx, self.w1, self.b1, self.K1, self.w2, self.b2, self.K2, p[0], self.ldy, self.B, self.H, self.W, self.Cc, self.add_)

    def direct(self, p):
        return self.lib.y5_bottleneck_fwd(*self.args(p), 0, self.st)

    def add(self, plan, p):
        return self.lib.y5_plan_add_bottleneck(plan, *self.args(p))


class BneckCv3(Case):
    """(C3, act3, add): the last Bottleneck of a 32-channel C3 + its cv3 (64 -> C3)."""
    SHAPES = {"bneck_cv3_a": (48, 0, 1), "bneck_cv3_b": (64, 1, 0)}
    Cc, B, H, W, ldx, ld2 = 32, 1, 4, 8, 40, 48

    def __init__(self, be, kind):
        super().__init__(be)
        self.kind = kind
        self.C3, self.act3, self.add_ = self.SHAPES[kind]
        self.ldo = self.C3 + 24
        rng = _seed("plan", kind)
        self.w1, self.b1, self.K1, _ = self.packed(*_filter(rng, 32, 32, 1), widen=24)
        self.w2, self.b2, self.K2, _ = self.packed(*_filter(rng, 32, 32, 3))
        self.w3, self.b3, self.K3, _ = self.packed(*_filter(rng, self.C3, 64, 1), widen=8)
        npix = self.B * self.H * self.W
        self.x = self.dev(_vals(rng, (npix, self.ldx), F16, -1.0, 1.0))
        self.y2 = self.dev(_vals(rng, (npix, self.ld2), F16, -1.0, 1.0))

    def fresh(self):
        return [_sent((self.B * self.H * self.W, self.ldo))]

    def args(self, p):
        return (self.x, self.ldx, self.w1, self.b1, self.K1, self.w2, self.b2, self.K2, self.y2, self.ld2, self.w3, self.b3, self.K3, self.C3, self.act3, p[0],
                self.ldo, self.B, self.H, self.W, self.Cc, self.add_)

    def direct(self, p):
        return self.lib.y5_bottleneck_cv3_fwd(*self.args(p), 0, self.st)

    def add(self, plan, p):
        return self.lib.y5_plan_add_bottleneck_cv3(plan, *self.args(p))


class K3pw(Case):
    """Conv(32, 64, 3, 2) + a pointwise layer with 48 outputs, 16 of them to y and 32 to y2, no activation behind it."""
    kind, second = "k3pw", 1
    B, H, W, c3, split, ldy, ld2, act2 = 1, 8, 16, 48, 16, 24, 40, 0

    def __init__(self, be):
        super().__init__(be)
        rng = _seed("plan k3pw")
        self.w1, self.b1, K1, N1 = self.packed(*_filter(rng, 64, 32, 3))
        self.w2, self.b2, self.K2, self.N2 = self.packed(*_filter(rng, self.c3, 64, 1), widen=64)
        self.x = self.dev(_vals(rng, (self.B * self.H * self.W, 40), F16, -1.0, 1.0))
        self.d = _lib.ConvDesc(dtype=DT16, B=self.B, H=self.H, W=self.W, C1=32, ldx=40, OH=self.H // 2, OW=self.W // 2, C2=64, ldy=64, KH=3, KW=3, SH=2, SW=2,
                               PH=1, PW=1, act=1, Kpad=K1, Npad=N1, ldr=0, ld2=0, cfg=34, max_blocks=0)
        self.npix = self.B * (self.H // 2) * (self.W // 2)

    def fresh(self):
        return [_sent((self.npix, self.ldy)), _sent((self.npix, self.ld2))]

    def args(self, p):
        return (C.byref(self.d), self.x, self.w1, self.b1, self.w2, self.b2, self.c3, self.N2, self.K2, self.act2, p[0], self.ldy, p[1], self.ld2, self.split)

    def direct(self, p):
        return self.lib.y5_conv_k3pw_fwd(*self.args(p), self.st)

    def add(self, plan, p):
        return self.lib.y5_plan_add_conv_k3pw(plan, *self.args(p))


class Front(Case):
    """The fused front on one 64 x 64 image: 56 real 3x3 channels, 48 pointwise outputs split 16 | 32, wider filter rows, no activation behind the 1x1."""
    kind, second, reads_input = "front", 1, True
    CASE = fr.fc(1, 64, 64, c1=56, c3=48, split=16, act1=1, act2=0, kpad1=352, kpad2=128)

    def __init__(self, be):
        super().__init__(be)
        rng = _seed("plan front")
        B, H, W, c1, c3 = self.CASE[:5]
        self.r = fr.FrontRun(be, self.CASE, fr._image(rng, (B, 3, H, W), "signed"), fr.front_weights(rng, c1, c3))
        self.alt = Guarded(be, (B, 3, H, W), F16, fr._image(rng, (B, 3, H, W), "signed"), fill=np.nan, guard=3 * W + 64)
        self.x, self.x_alt = self.r.x.p, self.alt.p
        self.inputs = [self.x] + [w.p for w in self.r.w] + [be.ptr(b) for b in self.r.b]

    def fresh(self):
        return [_sent((self.r.npix, self.r.ldy)), _sent((self.r.npix, self.r.ld2))]

    def args(self, p, x):
        r, be = self.r, self.be
        B, H, W, c1, c3, split, act1, act2 = self.CASE[:8]
        return (x, B, H, W, r.w[0].p, be.ptr(r.b[0]), 32, r.w[1].p, be.ptr(r.b[1]), c1, r.N1, r.K1, act1, r.w[2].p, be.ptr(r.b[2]), c3, r.N2, r.K2, act2, p[0],
                r.ldy, p[1], r.ld2, split)

    def direct(self, p, x=None):
        return self.lib.y5_conv_front_fwd(*self.args(p, x or self.x), 0, self.st)

    def add(self, plan, p):
        return self.lib.y5_plan_add_conv_front(plan, *self.args(p, self.x))


class Stem(Case):
    """The NCHW stem on the smallest row of front_ref.STEM_CASES."""
    kind, reads_input = "stem", True
    SHAPE = fr.STEM_CASES[0][:4]

    def __init__(self, be):
        super().__init__(be)
        rng = _seed("plan stem")
        B, H, W, C2 = self.SHAPE
        self.r = fr.StemRun(be, self.SHAPE, fr._image(rng, (B, 3, H, W), "signed"), fr._filter(rng, (C2, 3, 6, 6), 108), fr._bias(rng, C2))
        self.alt = Guarded(be, (B, 3, H, W), F16, fr._image(rng, (B, 3, H, W), "signed"), fill=np.nan, guard=3 * W + 64)
        self.x, self.x_alt = self.r.x.p, self.alt.p
        self.inputs = [self.x, self.r.w.p, be.ptr(self.r.b)]

    def fresh(self):
        return [_sent((self.r.npix, self.r.ldy))]

    def args(self, p, x):
        B, H, W, C2 = self.SHAPE
        return (x, B, H, W, self.r.w.p, self.be.ptr(self.r.b), C2, self.r.npad, p[0], self.r.ldy)

    def direct(self, p, x=None):
        return self.lib.y5_conv_stem_fwd(*self.args(p, x or self.x), 0, self.st)

    def add(self, plan, p):
        return self.lib.y5_plan_add_conv_stem(plan, *self.args(p, self.x))


# the fourteen op kinds that launch something; Bottleneck at its three channel counts, Bottleneck + cv3 at both values of act3 / add
CASES = {"conv": Conv, "to_nhwc": ToNhwc, "to_nchw": ToNchw, "sppf_front": SppfFront, "sppf_pool": SppfPool, "upsample": Upsample, "copy": Copy,
         "decode": Decode, "head": Head, "k3pw": K3pw, "front": Front, "stem": Stem,
         **{k: (lambda be, k=k: Bneck(be, k)) for k in Bneck.SHAPES}, **{k: (lambda be, k=k: BneckCv3(be, k)) for k in BneckCv3.SHAPES}}
KINDS = list(CASES)
INPUT_KINDS = ("stem", "to_nhwc", "front")     # y5_plan_set_input
ANCHOR_KINDS = ("decode", "head")              # y5_plan_set_anchors, y5_plan_set_obj_hint


# ---- buffers and plans ---------------------------------------------------------------------------------------------------------------------------------
class Outs:
    """A fresh set of a case's output buffers on the backend."""

    def __init__(self, case):
        self.be, self.init = case.be, case.fresh()
        self.h = [self.be.put(a) for a in self.init]
        self.p = [self.be.ptr(h) for h in self.h]

    def read(self):
        return [self.be.get(h) for h in self.h]

    def assert_equal(self, other, what):
        for k, (a, b) in enumerate(zip(self.read(), other.read())):
            assert_bits_equal(a, b, f"{what}: output {k}")

    def assert_untouched(self, k, what):
        assert_bits_equal(self.read()[k], self.init[k], f"{what}: output {k} was written")

    def assert_written(self, what):
        for k, a in enumerate(self.read()):
            assert a.tobytes() != self.init[k].tobytes(), f"{what}: output {k} was not written"


def _plane(be, shape_dtype):
    a = _sent(*shape_dtype)
    h = be.put(a)
    return a, h, be.ptr(h)


class Plan:
    def __init__(self, be):
        self.be, self.lib = be, be.lib
        self.p = C.c_void_p(be.lib.y5_plan_create())

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.lib.y5_plan_destroy(self.p)

    def run(self, first=0, last=None):
        ok(self.be, self.lib.y5_plan_run_range(self.p, first, self.size() if last is None else last, self.be.stream))

    def size(self):
        return self.lib.y5_plan_size(self.p)


def refused(be, rc, msg, what):
    err = be.lib.y5_last_error()
    assert rc == BAD and msg in err, f"{what}: status {rc}, {err!r}; expected {BAD} with {msg!r}"


def _direct(case, **kw):
    o = Outs(case)
    ok(case.be, case.direct(o.p, **kw))
    return o


# ---- the runners ---------------------------------------------------------------------------------------------------------------------------------------
def run_parity(be, kind):
    """Direct call against plan op, then on the same plan: every re-pointable output moves, no input does, and the setters that are not this kind's are refused."""
    case = CASES[kind](be)
    lib = be.lib
    ref = _direct(case)
    ref.assert_written(f"{kind} direct")
    with Plan(be) as plan:
        got = Outs(case)
        ok(be, case.add(plan.p, got.p))
        assert plan.size() == 1
        ok(be, lib.y5_plan_run(plan.p, be.stream))
        got.assert_equal(ref, f"{kind}: y5_plan_run against the direct call")

        # rebinding: one output at a time moves to a new buffer; the old one keeps its initial content
        cur = got
        movable = [0] + ([case.second] if case.second is not None else [])
        assert len(movable) == len(cur.p)
        for k in movable:
            new = Outs(case)
            ok(be, lib.y5_plan_rebind_output(plan.p, 0, 1, cur.p[k], new.p[k]))
            for h, a in zip(cur.h, cur.init):
                _refill(be, h, a)  # the initial content again, so that a run that still reaches the old address shows
            plan.run()
            assert_bits_equal(new.read()[k], ref.read()[k], f"{kind}: output {k} after y5_plan_rebind_output")
            cur.assert_untouched(k, f"{kind}: the buffer output {k} was moved away from")
            for j in movable:
                if j != k:
                    assert_bits_equal(cur.read()[j], ref.read()[j], f"{kind}: output {j}, which did not move")
                    new.assert_untouched(j, f"{kind}: output {j} of the new set, which the plan was not pointed at")
            ok(be, lib.y5_plan_rebind_output(plan.p, 0, 1, new.p[k], cur.p[k]))   # and back
        spare = Outs(case)
        for p in case.inputs:
            refused(be, lib.y5_plan_rebind_output(plan.p, 0, 1, p, spare.p[0]), b"no op writes that pointer", f"{kind}: rebinding an input")
        refused(be, lib.y5_plan_rebind_output(plan.p, 0, 1, spare.p[0], cur.p[0]), b"no op writes that pointer", f"{kind}: rebinding an unknown address")
        plan.run()
        cur.assert_equal(ref, f"{kind}: after the refused calls")

        # the setters of other kinds
        if not case.reads_input:
            refused(be, lib.y5_plan_set_input(plan.p, 0, spare.p[0]), b"op does not read the model input", f"{kind}: y5_plan_set_input")
        if case.hint is None:
            refused(be, lib.y5_plan_set_obj_hint(plan.p, 0, spare.p[0]), b"not a Detect decode / fused head op", f"{kind}: y5_plan_set_obj_hint")
            refused(be, lib.y5_plan_set_anchors(plan.p, 0, _anchors([1.0] * 6), 6), b"op has no anchors", f"{kind}: y5_plan_set_anchors")
        if not case.is_conv:
            refused(be, lib.y5_plan_set_conv_cfg(plan.p, 0, 0), b"not a convolution op", f"{kind}: y5_plan_set_conv_cfg")
        refused(be, lib.y5_plan_set_input(plan.p, 1, spare.p[0]), b"bad op index", f"{kind}: y5_plan_set_input past the end")
        plan.run()
        cur.assert_equal(ref, f"{kind}: after the refused setters")


def _refill(be, h, a):
    if isinstance(h, np.ndarray):
        h[...] = a
    else:
        h.copy_(torch.from_numpy(a))


def run_set_input(be, kind):
    case = CASES[kind](be)
    ref = _direct(case, x=case.x_alt)
    with Plan(be) as plan:
        got = Outs(case)
        ok(be, case.add(plan.p, got.p))
        ok(be, be.lib.y5_plan_set_input(plan.p, 0, case.x_alt))
        plan.run()
        got.assert_equal(ref, f"{kind}: y5_plan_set_input against the direct call on the other input")
        assert any(a.tobytes() != b.tobytes() for a, b in zip(ref.read(), _direct(case).read())), "the two inputs give the same output"


def run_anchors_and_hint(be, kind):
    """y5_plan_set_obj_hint / y5_plan_set_anchors against the direct call with the plane / the new anchors; the plane is re-pointable."""
    case = CASES[kind](be)
    lib = be.lib
    h_ref = _plane(be, case.hint)
    ref = _direct(case, hint=h_ref[2])
    assert be.get(h_ref[1]).tobytes() != h_ref[0].tobytes()
    with Plan(be) as plan:
        got, h_got = Outs(case), _plane(be, case.hint)
        ok(be, case.add(plan.p, got.p))
        plan.run()
        got.assert_equal(ref, f"{kind}: without a plane")
        ok(be, lib.y5_plan_set_obj_hint(plan.p, 0, h_got[2]))
        plan.run()
        got.assert_equal(ref, f"{kind}: with a plane")
        assert_bits_equal(be.get(h_got[1]), be.get(h_ref[1]), f"{kind}: the objectness plane against the direct call")
        # the plane moves like an output
        h_new = _plane(be, case.hint)
        ok(be, lib.y5_plan_rebind_output(plan.p, 0, 1, h_got[2], h_new[2]))
        _refill(be, h_got[1], h_got[0])
        plan.run()
        assert_bits_equal(be.get(h_new[1]), be.get(h_ref[1]), f"{kind}: the objectness plane after y5_plan_rebind_output")
        assert_bits_equal(be.get(h_got[1]), h_got[0], f"{kind}: the plane that was moved away from")
        # new anchors
        h_alt = _plane(be, case.hint)
        alt = _direct(case, anchors=case.anchors_alt, hint=h_alt[2])
        assert alt.read()[0].tobytes() != ref.read()[0].tobytes()
        for n in (0, 17):
            refused(be, lib.y5_plan_set_anchors(plan.p, 0, case.anchors_alt, n), b"plan_set_anchors: bad args", f"{kind}: y5_plan_set_anchors n = {n}")
        ok(be, lib.y5_plan_set_anchors(plan.p, 0, case.anchors_alt, 6))
        plan.run()
        got.assert_equal(alt, f"{kind}: y5_plan_set_anchors against the direct call with the new anchors")
        assert_bits_equal(be.get(h_new[1]), be.get(h_alt[1]), f"{kind}: the objectness plane after y5_plan_set_anchors")
        ok(be, lib.y5_plan_set_anchors(plan.p, 0, case.anchors, 2))   # the first anchor only
        mixed = _anchors(list(case.anchors)[:2] + list(case.anchors_alt)[2:])
        plan.run()
        got.assert_equal(_direct(case, anchors=mixed), f"{kind}: y5_plan_set_anchors with n = 2")


def run_nop_and_ranges(be):
    """[nop, upsample, nop, copy]: indices count the no-ops, a range runs its ops only; and the two launches as a range with the second on the side branch."""
    up, cp = Upsample(be), Copy(be)
    lib = be.lib
    r_up, r_cp = _direct(up), _direct(cp)
    with Plan(be) as plan:
        o_up, o_cp = Outs(up), Outs(cp)
        ok(be, lib.y5_plan_add_nop(plan.p))
        ok(be, up.add(plan.p, o_up.p))
        ok(be, lib.y5_plan_add_nop(plan.p))
        ok(be, cp.add(plan.p, o_cp.p))
        assert plan.size() == 4
        plan.run(0, 1)
        plan.run(2, 3)
        o_up.assert_untouched(0, "a no-op range")
        o_cp.assert_untouched(0, "a no-op range")
        plan.run(1, 3)
        o_up.assert_equal(r_up, "range [1, 3)")
        o_cp.assert_untouched(0, "range [1, 3)")
        refused(be, lib.y5_plan_rebind_output(plan.p, 0, 3, o_cp.p[0], o_up.p[0]), b"no op writes that pointer", "rebinding outside the op's range")
        ok(be, lib.y5_plan_set_branch(plan.p, 3, 1))
        refused(be, lib.y5_plan_set_branch(plan.p, 3, 2), b"plan_set_branch", "branch 2")
        refused(be, lib.y5_plan_set_branch(plan.p, 4, 1), b"plan_set_branch", "branch of op 4")
        plan.run()
        o_cp.assert_equal(r_cp, "the copy on the side branch")
        o_up.assert_equal(r_up, "the upsample in front of a side branch")
    with Plan(be) as plan:     # the two-op range proper: branch 0, then the second op on branch 1, into fresh buffers
        a_up, a_cp, b_up, b_cp = Outs(up), Outs(cp), Outs(up), Outs(cp)
        ok(be, up.add(plan.p, a_up.p))
        ok(be, cp.add(plan.p, a_cp.p))
        plan.run(0, 2)
        ok(be, lib.y5_plan_set_branch(plan.p, 1, 1))
        ok(be, lib.y5_plan_rebind_output(plan.p, 0, 2, a_up.p[0], b_up.p[0]))
        ok(be, lib.y5_plan_rebind_output(plan.p, 0, 2, a_cp.p[0], b_cp.p[0]))
        plan.run(0, 2)
        b_up.assert_equal(a_up, "branch 1 against branch 0: op 0")
        b_cp.assert_equal(a_cp, "branch 1 against branch 0: op 1")
        a_up.assert_equal(r_up, "branch 0 against the direct call")


def run_capture(be):
    """GPU only: the two-op range with a side branch as a captured graph, and y5_plan_set_conv_cfg on either side of a capture."""
    up, cp, cv = Upsample(be), Copy(be), Conv(be)
    lib = be.lib
    r_up, r_cp = _direct(up), _direct(cp)
    with Plan(be) as plan:
        o_up, o_cp, o_cv = Outs(up), Outs(cp), Outs(cv)
        ok(be, up.add(plan.p, o_up.p))
        ok(be, cp.add(plan.p, o_cp.p))
        ok(be, cv.add(plan.p, o_cv.p))
        ok(be, lib.y5_plan_set_branch(plan.p, 1, 1))
        ok(be, lib.y5_plan_set_conv_cfg(plan.p, 2, 2))
        ok(be, lib.y5_plan_set_conv_cfg(plan.p, 2, -1))
        refused(be, lib.y5_plan_launch_graph(plan.p, be.stream), b"plan not captured", "launch before capture")
        ok(be, lib.y5_plan_capture_range(plan.p, 0, 2, be.stream))
        for o in (o_up, o_cp):       # the capture's own eager run wrote them
            _refill(be, o.h[0], o.init[0])
        ok(be, lib.y5_plan_launch_graph(plan.p, be.stream))
        o_up.assert_equal(r_up, "captured range: op 0")
        o_cp.assert_equal(r_cp, "captured range: op 1 (side branch)")
        o_cv.assert_untouched(0, "captured range [0, 2): op 2")
        refused(be, lib.y5_plan_set_conv_cfg(plan.p, 2, 2), b"the plan has captured graphs", "y5_plan_set_conv_cfg after a capture")
