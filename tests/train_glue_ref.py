"""TEST INFRASTRUCTURE ONLY: case tables, references and ONE runner per kernel family for the memory-bound kernels between the convolutions of the
training path -- train-mode BatchNorm + SiLU forward / backward with their statistics passes (yolov5_amd/csrc/bn_kernels.h), the gradient-routing and
layout kernels (csrc/train_misc.hip, csrc/misc_kernels.h) and the SPPF pooling chain.  Every runner takes a backend, so tests/test_emu_train_glue.py (the
kernels compiled for the host, small shapes) and tests/test_gpu_train_glue.py (the device library, the full tables) run the same cases through the same code.

Rules every case follows: a buffer is wider than its payload and is reached through a channel offset where the entry takes a slice; pad columns, the
columns before the slice and the guards around flat buffers hold a sentinel that must survive the call (inputs: NaN, so that a read outside the payload
poisons the result); the strides within one call are pairwise different, so that two swapped strides cannot cancel.

References: pure data movement is numpy indexing, compared bit for bit; the small sums are restated in their documented order (fp16) or drawn on a dyadic
grid where every fp32 sum is exact (fp32), compared bit for bit; BatchNorm is float64 numpy, in chunks over the pixels."""
from __future__ import annotations

import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
import torch.nn.functional as F

from yolov5_amd import _lib

F16, F32, U8 = np.float16, np.float32, np.uint8
SENT = -777.0          # sentinel of output buffers (exact in fp16); input buffers are padded with NaN
SENT_U8 = 0xAB
_DT = {np.dtype(F16): _lib.Y5_F16, np.dtype(F32): _lib.Y5_F32, np.dtype(U8): _lib.Y5_U8}


def y5_dtype(dtype):
    return _DT[np.dtype(dtype)]


# ---- backends ----------------------------------------------------------------------------------------------------------------------------------------
class EmuBackend:
    """Host arrays (256-byte aligned) handed to the kernels compiled for the host."""
    name, stream = "emu", None

    def __init__(self):
        from tests.hipemu.emu import emu

        self.lib = emu()

    def put(self, a):
        from tests.hipemu.emu import aligned

        b = aligned(a.shape, a.dtype)
        b[...] = a
        return b

    def ptr(self, h, byte_off=0):
        return C.c_void_p(h.ctypes.data + byte_off)

    def get(self, h):
        return h.copy()

    def equal(self, a, b):
        return a.tobytes() == b.tobytes()


class GpuBackend:
    """torch device tensors (the caching allocator aligns to 512 bytes) handed to yolov5_amd._lib on the current stream."""
    name = "gpu"

    def __init__(self, dev):
        self.lib, self.dev = _lib.lib(), dev

    @property
    def stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def put(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def ptr(self, h, byte_off=0):
        return C.c_void_p(h.data_ptr() + byte_off)

    def get(self, h):
        torch.cuda.synchronize(self.dev)
        return h.cpu().numpy()

    def equal(self, a, b):
        torch.cuda.synchronize(self.dev)
        return torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def ok(be, rc):
    assert rc == 0, be.lib.y5_last_error().decode(errors="replace")


def bits(a):
    return np.ascontiguousarray(a).view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def assert_bits_equal(got, ref, what=""):
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    bad = bits(got) != bits(ref)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at {np.argwhere(bad)[0].tolist()}"


def _same_fill(a, fill):
    return bool(np.all(a == fill)) if fill == fill else bool(np.all(np.isnan(a)))


class Slab:
    """(npix, ld) buffer whose payload is the channel slice [:, off:off + C]; the entry receives the slice's address."""

    def __init__(self, be, npix, Cc, ld, off, dtype, data=None, fill=SENT):
        assert ld >= off + Cc and ld > Cc
        host = np.full((npix, ld), fill, dtype)
        if data is not None:
            host[:, off:off + Cc] = np.asarray(data).reshape(npix, Cc)
        self.be, self.Cc, self.ld, self.off, self.fill = be, Cc, ld, off, fill
        self.h = be.put(host)
        self.p = be.ptr(self.h, off * host.dtype.itemsize)

    def read(self, what="slab"):
        """The payload; asserts that everything around it still holds the sentinel."""
        a = self.be.get(self.h)
        assert _same_fill(a[:, :self.off], self.fill), f"{what}: the columns before the slice were written"
        assert _same_fill(a[:, self.off + self.Cc:], self.fill), f"{what}: the pad columns were written"
        return a[:, self.off:self.off + self.Cc]


class Guarded:
    """Contiguous payload of `shape` between two sentinel guards; `shift` extra elements in front move the base address off its 16-byte alignment."""

    def __init__(self, be, shape, dtype, data=None, fill=SENT, guard=64, shift=0):
        n = int(np.prod(shape))
        host = np.full((guard + shift + n + guard,), fill, dtype)
        if data is not None:
            host[guard + shift:guard + shift + n] = np.asarray(data).reshape(-1)
        self.be, self.shape, self.n, self.lo, self.fill = be, tuple(shape), n, guard + shift, fill
        self.h = be.put(host)
        self.p = be.ptr(self.h, self.lo * host.dtype.itemsize)

    def read(self, what="buffer"):
        a = self.be.get(self.h)
        assert _same_fill(a[:self.lo], self.fill) and _same_fill(a[self.lo + self.n:], self.fill), f"{what}: a guard was written"
        return a[self.lo:self.lo + self.n].reshape(self.shape)


def _seed(*key):
    """Deterministic across processes (no str hash)."""
    s = 1469598103934665603
    for ch in repr(key).encode():
        s = ((s ^ ch) * 1099511628211) % (1 << 63)
    return np.random.default_rng(s)


def _vals(rng, shape, dtype, lo=-4.0, hi=4.0):
    return rng.uniform(lo, hi, size=shape).astype(np.float32).astype(dtype)


def _dyadic(rng, shape):
    """fp32 multiples of 2^-10 in [-1, 1]: every sum of a few thousand of them is exact in fp32."""
    return (rng.integers(-1024, 1025, size=shape).astype(np.float32) / np.float32(1024.0)).astype(np.float32)


def _vec(dtype):
    return 16 // np.dtype(dtype).itemsize


def _strides(dtype, Cc, n):
    """Slice offset (one 16-byte vector) and n pairwise different pixel strides, all multiples of 16 bytes and wider than the payload."""
    v = _vec(dtype)
    return v, [v + Cc + (k + 1) * v for k in range(n)]


# ---- 1. pure data movement ---------------------------------------------------------------------------------------------------------------------------
# (dtype, B, H, W, C, big): odd H / W, one / three / 32 vectors per pixel, a single pixel, and the benchmark's P4 -> P3 upsample (bs 64)
MOVE_CASES = [(dt, 2, 3, 5, c, False) for dt in (F16, F32) for c in (8, 24, 256)] + [(F16, 1, 1, 1, 8, False), (F32, 3, 1, 7, 24, False),
                                                                                      (F16, 64, 40, 40, 256, True)]


def run_upsample2x(be, case):
    dtype, B, H, W, Cc, _ = case
    off, (lds, ldd) = _strides(dtype, Cc, 2)
    x = _vals(_seed("up", case), (B, H, W, Cc), dtype)
    src = Slab(be, B * H * W, Cc, lds, off, dtype, x, fill=np.nan)
    dst = Slab(be, B * 4 * H * W, Cc, ldd, off, dtype)
    ok(be, be.lib.y5_upsample2x(src.p, y5_dtype(dtype), dst.p, B, H, W, Cc, lds, ldd, be.stream))
    assert_bits_equal(dst.read("upsample2x dst").reshape(B, 2 * H, 2 * W, Cc), x.repeat(2, 1).repeat(2, 2), "y5_upsample2x")


def run_copy_slice(be, case):
    dtype, B, H, W, Cc, _ = case
    npix = B * H * W
    off, (lds, ldd) = _strides(dtype, Cc, 2)
    x = _vals(_seed("cp", case), (npix, Cc), dtype)
    src = Slab(be, npix, Cc, lds, off, dtype, x, fill=np.nan)
    dst = Slab(be, npix, Cc, ldd, off, dtype)
    ok(be, be.lib.y5_copy_slice(src.p, y5_dtype(dtype), dst.p, npix, Cc, lds, ldd, be.stream))
    assert_bits_equal(dst.read("copy_slice dst"), x, "y5_copy_slice")


# (src dtype, dst dtype, scale, C, ld): all six pairs x both scales x channel counts / strides incl. C == ld and ld = 64 (the launcher's maximum)
NCHW_CASES = [(s, d, sc, c, ld) for s in (U8, F16, F32) for d in (F16, F32) for sc in (1.0 / 255.0, 1.0)
              for c, ld in ((1, 4), (3, 8), (8, 64), (3, 4), (8, 8))]


def run_nchw_to_nhwc(be, case):
    sdt, ddt, scale, Cc, ld = case
    B, H, W = 2, 9, 15
    n = B * Cc * H * W
    if sdt is U8:
        x = (np.arange(n) * 7 % 256).astype(U8).reshape(B, Cc, H, W)   # 7 is coprime to 256: every byte value occurs
        assert len(np.unique(x)) == 256
    else:
        x = _vals(_seed("nchw", case), (B, Cc, H, W), sdt, -255.0, 255.0)
    src = Guarded(be, x.shape, sdt, x, fill=SENT_U8 if sdt is U8 else np.nan)
    dst = Guarded(be, (B, H, W, ld), ddt)
    ok(be, be.lib.y5_nchw_to_nhwc(src.p, y5_dtype(sdt), dst.p, y5_dtype(ddt), B, Cc, H, W, ld, scale, be.stream))
    ref = np.zeros((B, H, W, ld), ddt)                                  # pad channels are written as +0
    # ONE rounding: the fp32 value of the element times the fp32 scale, then to the destination type
    ref[..., :Cc] = (x.astype(np.float32) * np.float32(scale)).astype(ddt).transpose(0, 2, 3, 1)
    assert_bits_equal(dst.read("nchw_to_nhwc dst"), ref, "y5_nchw_to_nhwc")


# (dtype, B, H, W, C): C not a multiple of 8, a slice at an offset inside a wider buffer
NHWC_NCHW_CASES = [(F16, 2, 5, 7, 13), (F32, 2, 5, 7, 3), (F16, 1, 4, 4, 24), (F32, 1, 3, 3, 13)]


def run_nhwc_to_nchw(be, case):
    dtype, B, H, W, Cc = case
    off, ld = 5, Cc + 5 + 6
    x = _vals(_seed("nhwc", case), (B, H, W, Cc), dtype)
    src = Slab(be, B * H * W, Cc, ld, off, dtype, x, fill=np.nan)
    dst = Guarded(be, (B, Cc, H, W), dtype)
    ok(be, be.lib.y5_nhwc_to_nchw(src.p, y5_dtype(dtype), dst.p, B, Cc, H, W, ld, be.stream))
    assert_bits_equal(dst.read("nhwc_to_nchw dst"), np.ascontiguousarray(x.transpose(0, 3, 1, 2)), "y5_nhwc_to_nchw")


# (B, npix, na, no, ld, shift, big) and the dispatch path each direction takes (train_misc.hip: nhwc_to_raw is tiled iff ld % 8 == 0, na <= 8 and both
# pointers are 16-byte aligned; raw_to_nhwc iff ld % 8 == 0, aligned and 64 * no < 65536)
RAW_CASES = [
    (2, 11, 3, 7, 24, 0, False),        # tiled / tiled
    (2, 11, 3, 7, 22, 0, False),        # ld % 8 != 0: fallback / fallback
    (1, 13, 9, 5, 48, 0, False),        # na = 9: fallback / tiled
    (2, 11, 3, 7, 24, 1, False),        # base addresses 2 bytes past a 16-byte boundary (legal for fp16): fallback / fallback
    (1, 3, 1, 1024, 1032, 0, False),    # 64 * no >= 65536: tiled / fallback
    (2, 6400, 3, 117, 352, 0, True),    # yolov5s-seg's head (no = 5 + 80 + 32) at P3 of 640 x 640: tiled / tiled
]


def run_raw(be, case, f32=False):
    """y5_nhwc_to_raw / y5_raw_to_nhwc (fp16), or y5_train_glue_f32 ops 0 / 1 with the same table in fp32."""
    B, npix, na, no, ld, shift, _ = case
    dtype = F32 if f32 else F16
    shift = 0 if f32 else shift
    rng = _seed("raw", case, f32)
    lg = np.full((B, npix, ld), np.nan, dtype)
    lg[..., :na * no] = _vals(rng, (B, npix, na * no), dtype)
    src = Guarded(be, lg.shape, dtype, lg, fill=np.nan, shift=shift)
    raw = Guarded(be, (B, na, npix, no), dtype, shift=shift)
    if f32:
        ok(be, be.lib.y5_train_glue_f32(0, src.p, raw.p, B, npix, na, no, ld, 0, 0, be.stream))
    else:
        ok(be, be.lib.y5_nhwc_to_raw(src.p, raw.p, B, npix, na, no, ld, be.stream))
    ref = np.ascontiguousarray(lg[..., :na * no].reshape(B, npix, na, no).transpose(0, 2, 1, 3))
    assert_bits_equal(raw.read("nhwc_to_raw dst"), ref, "nhwc_to_raw")
    # and back: the padding channels of dlogits are zeroed
    dr = _vals(rng, (B, na, npix, no), dtype)
    dsrc = Guarded(be, dr.shape, dtype, dr, fill=np.nan, shift=shift)
    dlg = Guarded(be, (B, npix, ld), dtype, shift=shift)
    if f32:
        ok(be, be.lib.y5_train_glue_f32(1, dsrc.p, dlg.p, B, npix, na, no, ld, 0, 0, be.stream))
    else:
        ok(be, be.lib.y5_raw_to_nhwc(dsrc.p, dlg.p, B, npix, na, no, ld, be.stream))
    ref = np.zeros((B, npix, ld), dtype)
    ref[..., :na * no] = dr.transpose(0, 2, 1, 3).reshape(B, npix, na * no)
    assert_bits_equal(dlg.read("raw_to_nhwc dst"), ref, "raw_to_nhwc")


def run_memset_zero(be, nbytes=1001, shift=3):
    buf = Guarded(be, (nbytes,), U8, fill=SENT_U8, shift=shift)   # an odd count at an odd address
    ok(be, be.lib.y5_memset_zero(buf.p, nbytes, be.stream))
    assert not buf.read("memset_zero").any()


# ---- 2. exactly specified arithmetic -----------------------------------------------------------------------------------------------------------------
# (B, H, W, C, big): destination geometry; C in vectors of 8 for the fp16 entries.  The fp32 twins take any C (table below).
SUM_CASES = [(2, 3, 5, 8, False), (1, 1, 1, 24, False), (2, 5, 3, 256, False), (3, 7, 1, 24, False), (64, 40, 40, 128, True)]
SUM_CASES_F32 = [(2, 3, 5, 6, False), (1, 1, 1, 3, False), (2, 5, 3, 16, False), (3, 7, 1, 13, False)]   # C not a multiple of 4 among them


def _sum_strides(f32, Cc):
    if f32:                                  # scalar kernels: any offset, any stride
        return 3, [Cc + 3 + 2, Cc + 3 + 5]
    return _strides(F16, Cc, 2)


def run_upsample2x_bwd(be, case, acc, f32=False):
    """gsrc(b,h,w,:) (+)= the 2x2 block of gup, summed in fp32 in the documented order: the destination first when accumulating, then
    (dy, dx) = (0,0), (0,1), (1,0), (1,1); rounded to the storage type once."""
    B, H, W, Cc, _ = case
    dtype = F32 if f32 else F16
    off, (ld_up, ld_src) = _sum_strides(f32, Cc)
    rng = _seed("upb", case, acc, f32)
    gup = _dyadic(rng, (B, 2 * H, 2 * W, Cc)) if f32 else _vals(rng, (B, 2 * H, 2 * W, Cc), F16)
    d0 = _dyadic(rng, (B, H, W, Cc)) if f32 else _vals(rng, (B, H, W, Cc), F16)
    src = Slab(be, B * 4 * H * W, Cc, ld_up, off, dtype, gup, fill=np.nan)
    dst = Slab(be, B * H * W, Cc, ld_src, off, dtype, d0)
    if f32:
        ok(be, be.lib.y5_train_glue_f32(2, src.p, dst.p, B, H, W, Cc, ld_up, ld_src, acc, be.stream))
    else:
        ok(be, be.lib.y5_upsample2x_bwd(src.p, dst.p, B, H, W, Cc, ld_up, ld_src, acc, be.stream))
    got = dst.read("upsample2x_bwd dst").reshape(B, H, W, Cc)
    if f32:   # dyadic operands: every fp32 sum is exact, so the result EQUALS the float64 sum
        ref = (d0.astype(np.float64) if acc else 0.0) + sum(gup[:, dy::2, dx::2].astype(np.float64) for dy in (0, 1) for dx in (0, 1))
        assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), ref), "train_glue_f32 op 2"
    else:
        s = d0.astype(np.float32) if acc else np.zeros((B, H, W, Cc), np.float32)
        for dy in (0, 1):
            for dx in (0, 1):
                s = s + gup[:, dy::2, dx::2].astype(np.float32)
        assert_bits_equal(got, s.astype(F16), "y5_upsample2x_bwd")


def run_add_slice(be, case, acc, f32=False):
    """dst (+)= src: accumulate = 0 is a copy (bit-exact), accumulate = 1 one fp32 add rounded to the storage type once."""
    B, H, W, Cc, _ = case
    npix = B * H * W
    dtype = F32 if f32 else F16
    off, (lds, ldd) = _sum_strides(f32, Cc)
    rng = _seed("add", case, acc, f32)
    x = _dyadic(rng, (npix, Cc)) if f32 else _vals(rng, (npix, Cc), F16)
    d0 = _dyadic(rng, (npix, Cc)) if f32 else _vals(rng, (npix, Cc), F16)
    src = Slab(be, npix, Cc, lds, off, dtype, x, fill=np.nan)
    dst = Slab(be, npix, Cc, ldd, off, dtype, d0)
    if f32:
        ok(be, be.lib.y5_train_glue_f32(3, src.p, dst.p, B, H, W, Cc, lds, ldd, acc, be.stream))
    else:
        ok(be, be.lib.y5_add_slice(src.p, dst.p, npix, Cc, lds, ldd, acc, be.stream))
    got = dst.read("add_slice dst")
    if f32:
        ref = x.astype(np.float64) + (d0.astype(np.float64) if acc else 0.0)
        assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), ref), "train_glue_f32 op 3"
    else:
        assert_bits_equal(got, (x.astype(np.float32) + d0.astype(np.float32)).astype(F16) if acc else x, "y5_add_slice")


# (B, H, W, C): y5_train_glue_f32 op 4 (one thread per (image, channel)); planes smaller than / larger than the 5 x 5 window, C not a multiple of 4
SPPF_BWD_F32_CASES = [(2, 7, 6, 6), (1, 3, 4, 3), (2, 11, 9, 13), (1, 1, 1, 4)]


def run_sppf_bwd_f32(be, case, k=5):
    """Backward of SPPF's three chained MaxPool2d(k, 1, k // 2) in the [x | y1 | y2 | y3] buffers against float64 torch autograd.  The activations sit
    on a coarse grid, so windows hold ties and torch's first-maximum rule decides; the gradients are dyadic, so every fp32 sum is exact."""
    B, H, W, Cc = case
    rng = _seed("sppfb", case)
    x = rng.integers(0, 4, size=(B, H, W, Cc)).astype(np.float64)
    g = _dyadic(rng, (B, H, W, 4 * Cc))
    xt = torch.from_numpy(x).permute(0, 3, 1, 2).requires_grad_(True)
    ys = [xt]
    for _ in range(3):
        ys.append(F.max_pool2d(ys[-1], k, 1, k // 2))
    gt = torch.from_numpy(g.astype(np.float64)).permute(0, 3, 1, 2)
    sum((y * gt[:, i * Cc:(i + 1) * Cc]).sum() for i, y in enumerate(ys)).backward()
    ref = xt.grad.permute(0, 2, 3, 1).numpy()
    act = torch.cat([y.detach() for y in ys], 1).permute(0, 2, 3, 1).numpy().astype(np.float32)
    off, ld_act, ld_grad = 3, 4 * Cc + 3 + 2, 4 * Cc + 3 + 5
    a = Slab(be, B * H * W, 4 * Cc, ld_act, off, F32, act, fill=np.nan)
    gr = Slab(be, B * H * W, 4 * Cc, ld_grad, off, F32, g)
    ok(be, be.lib.y5_train_glue_f32(4, a.p, gr.p, B, H, W, Cc, ld_act, ld_grad, k, be.stream))
    got = gr.read("sppf_pool_bwd grad").reshape(B, H, W, 4 * Cc)[..., :Cc]
    assert np.array_equal(got.astype(np.float64), ref), "train_glue_f32 op 4"


# ---- 3. SPPF pooling chain, forward ------------------------------------------------------------------------------------------------------------------
# (dtype, Y5_SPPF_GV or None, B, H, W, C, ld, off, big) -> the instantiation y5_sppf_pool selects (misc.hip: the width is halved until C * es divides by
# 16 * gv and three planes fit in 150 KiB; planes of 3200 < H*W <= 4800 pixels take the direct k x k form, one vector wide)
SPPF_CASES = (
    [(F16, gv, 2, 7, 5, 64, 4 * 64 + 24, 8, False) for gv in (1, 2, 4, 8)] +        # <half8, gv, separable>
    [(F32, gv, 2, 7, 5, 32, 4 * 32 + 12, 4, False) for gv in (1, 2, 4, 8)] +        # <float4, gv, separable>
    [(F16, 8, 1, 6, 9, 24, 4 * 24 + 16, 8, False),                                  # 48 bytes per pixel: 8 falls back to one vector
     (F16, None, 1, 60, 56, 8, 4 * 8 + 16, 8, False),                               # <half8, 1, direct>: 3360 pixels
     (F32, None, 1, 60, 56, 4, 4 * 4 + 8, 4, False),                                # <float4, 1, direct>
     (F16, 2, 1, 40, 40, 16, 4 * 16 + 8, 8, False),                                 # separable build, more than 2048 vectors: its generic-index loop
     (F16, None, 64, 20, 20, 256, 1024, 0, True),                                   # the benchmark's SPPF at bs 64: C = 256 inside ld = 1024, default width 4
     (F16, None, 16, 40, 40, 640, 4 * 640 + 8, 0, True)])                           # yolov5x's SPPF at 1280 x 1280: width 2, generic-index loop
SPPF_UNSUPPORTED = (F16, None, 1, 70, 70, 8, 4 * 8 + 16, 8, False)                  # 4900 pixels x 32 bytes > 150 KiB: refused, nothing is launched


def run_sppf_pool(be, case, setenv, k=5, unsupported=False):
    """setenv(value or None) sets / clears Y5_SPPF_GV (the launcher reads it at every call)."""
    dtype, gv, B, H, W, Cc, ld, off, _ = case
    setenv(gv)
    npix = B * H * W
    x = _vals(_seed("sppf", case), (B, H, W, Cc), dtype)
    if ld == 4 * Cc:                       # the benchmark's buffer has no pad columns: guards around it instead
        host = np.full((npix, ld), SENT, dtype)
        host[:, :Cc] = x.reshape(npix, Cc)
        buf = Guarded(be, (npix, ld), dtype, host)
        rd = lambda: buf.read("sppf buffer")
    else:
        host = np.full((npix, 4 * Cc), SENT, dtype)
        host[:, :Cc] = x.reshape(npix, Cc)
        buf = Slab(be, npix, 4 * Cc, ld, off, dtype, host)
        rd = lambda: buf.read("sppf buffer")
    rc = be.lib.y5_sppf_pool(buf.p, y5_dtype(dtype), B, H, W, Cc, ld, k, be.stream)
    if unsupported:
        assert rc == _lib.Y5_ERR_UNSUPPORTED and b"does not fit in LDS" in be.lib.y5_last_error()
        assert_bits_equal(rd(), host, "sppf buffer after the refusal")
        return
    ok(be, rc)
    t = torch.from_numpy(x.astype(np.float32)).permute(0, 3, 1, 2)   # max is exact in any precision
    ref = [t]
    for _ in range(3):
        ref.append(F.max_pool2d(ref[-1], k, 1, k // 2))
    ref = torch.cat(ref, 1).permute(0, 2, 3, 1).numpy().astype(dtype).reshape(npix, 4 * Cc)
    assert_bits_equal(rd(), ref, "y5_sppf_pool")


# ---- 4. BatchNorm family against float64 -------------------------------------------------------------------------------------------------------------
EPS, MOMENTUM = 1e-3, 0.03
TOL = {np.dtype(F16): dict(rtol=5e-3, atol=5e-3), np.dtype(F32): dict(rtol=1e-4, atol=1e-5)}         # y, dz (tests/test_emu_bn.py, test_gpu_train_ops.py)
# saved mean / running mean, saved invstd / running variance: the running-statistics tolerances of test_gpu_train_ops.py::test_bn_silu_fwd_bwd (fp16) and of
# tests/test_emu_bn.py (fp32)
TOL_MEAN = {np.dtype(F16): dict(rtol=1e-4, atol=1e-5), np.dtype(F32): dict(rtol=1e-5, atol=1e-6)}
TOL_VAR = {np.dtype(F16): dict(rtol=1e-3, atol=1e-5), np.dtype(F32): dict(rtol=1e-4, atol=1e-6)}
SUM_FLOOR, SUM_FACTOR = 2.0 ** -22, 4.0

_POOL = ThreadPoolExecutor(8)


def _chunks(n, step=1 << 15):
    return [(i, min(i + step, n)) for i in range(0, n, step)]


def _pmap(fn, n):
    return list(_POOL.map(lambda c: fn(*c), _chunks(n)))


class BnRef:
    """float64 train-mode BatchNorm + SiLU (+ residual) and its closed-form backward on (npix, C) arrays of the storage type, in chunks over the pixels.
    npix = 1 is the formula itself: variance 0, invstd = 1 / sqrt(eps), running variance updated with the biased value (torch refuses the shape)."""

    def __init__(self, z, dy, res, gamma, beta):
        self.z, self.dy, self.res = z, dy, res
        n = self.n = z.shape[0]
        g = self.g = gamma.astype(np.float64)
        b = self.b = beta.astype(np.float64)

        def p1(lo, hi):
            zz = z[lo:hi].astype(np.float64)
            return zz.sum(0), np.abs(zz).sum(0), (zz * zz).sum(0)
        r = _pmap(p1, n)
        self.sum_z, self.abs_z, self.sum_zz = (sum(t[i] for t in r) for i in range(3))
        mean = self.mean = self.sum_z / n

        def p2(lo, hi):
            d = z[lo:hi].astype(np.float64) - mean
            return (d * d).sum(0)
        var = self.var = sum(_pmap(p2, n)) / n                  # two passes: no cancellation in the reference
        self.invstd = 1.0 / np.sqrt(var + EPS)
        self.running_mean = (1 - MOMENTUM) * 0.0 + MOMENTUM * mean
        self.running_var = (1 - MOMENTUM) * 1.0 + MOMENTUM * (var * n / (n - 1) if n > 1 else var)

        def p3(lo, hi):
            zh, u, sg = self._fwd(lo, hi)
            dyy = dy[lo:hi].astype(np.float64)
            dv = dyy * sg * (1.0 + u * (1.0 - sg))
            t = dv * zh
            return dv.sum(0), np.abs(dv).sum(0), t.sum(0), np.abs(t).sum(0), dyy.sum(0), np.abs(dyy).sum(0)
        r = _pmap(p3, n)
        self.dbeta, self.abs_dbeta, self.dgamma, self.abs_dgamma, self.sum_dy, self.abs_dy = (sum(t[i] for t in r) for i in range(6))

    def _fwd(self, lo, hi):
        zh = (self.z[lo:hi].astype(np.float64) - self.mean) * self.invstd
        u = self.g * zh + self.b
        return zh, u, 1.0 / (1.0 + np.exp(-u))

    def y(self, lo, hi):
        _, u, sg = self._fwd(lo, hi)
        return u * sg + (self.res[lo:hi].astype(np.float64) if self.res is not None else 0.0)

    def dz(self, lo, hi):
        zh, u, sg = self._fwd(lo, hi)
        dv = self.dy[lo:hi].astype(np.float64) * sg * (1.0 + u * (1.0 - sg))
        return self.g * self.invstd * (dv - self.dbeta / self.n - zh * self.dgamma / self.n)

    def worst(self, which, got, rtol, atol):
        """max |got - ref| / (atol + rtol |ref|): <= 1 is what assert_allclose(rtol, atol) accepts; inf if anything is not finite."""
        fn = self.y if which == "y" else self.dz

        def part(lo, hi):
            ref, gg = fn(lo, hi), got[lo:hi].astype(np.float64)
            if not np.isfinite(gg).all():
                return np.inf
            return float((np.abs(gg - ref) / (atol + rtol * np.abs(ref))).max())
        return max(_pmap(part, self.n))


def _norm_err(got, ref, absref):
    """Worst channel of |got - ref| / sum of the absolute terms."""
    return float((np.abs(np.asarray(got, np.float64) - ref) / np.maximum(absref, 1e-300)).max())


def torch_fp32(z, dy, res, gamma, beta):
    """torch's own fp32 CPU result on the same inputs: y, and the sums the kernels are measured against (None where torch refuses the shape)."""
    zt = torch.from_numpy(z.astype(np.float32)).requires_grad_(True)
    dyt = torch.from_numpy(dy.astype(np.float32))
    out = dict(sum_z=zt.detach().sum(0).numpy(), sum_zz=(zt.detach() * zt.detach()).sum(0).numpy(), sum_dy=dyt.sum(0).numpy(), y=None, dgamma=None, dbeta=None)
    if z.shape[0] > 1:
        gt, bt = torch.from_numpy(gamma).requires_grad_(True), torch.from_numpy(beta).requires_grad_(True)
        y = F.silu(F.batch_norm(zt, torch.zeros(z.shape[1]), torch.ones(z.shape[1]), gt, bt, True, MOMENTUM, EPS))
        y.backward(dyt)
        if res is not None:
            y = y.detach() + torch.from_numpy(res.astype(np.float32))
        out.update(y=y.detach().numpy(), dgamma=gt.grad.numpy(), dbeta=bt.grad.numpy())
    return out


def bn_cases(full):
    """(dtype, C, npix, residual, big).  C: the one-vector minimum, vector counts that do not divide 256 (24, 80; 1280: one pixel row per workgroup, 96 idle
    threads), the 256-vector limit.  npix: 1, around the 64-per-workgroup split, past the 1024-workgroup cap (65 536 + 77), and the benchmark's first
    layer at bs 16 (16 x 320 x 320 = 1 638 400 pixels at C = 32: 1600 pixels per workgroup, long per-thread fp32 chains)."""
    cases = []
    for dtype, cs in ((F16, (8, 24, 80, 1280, 2048)), (F32, (4, 24, 80, 1024))):
        for i, c in enumerate(cs):
            for j, n in enumerate((1, 63, 65)):
                cases.append((dtype, c, n, (i + j) % 2 == 1, False))
        cases.append((dtype, cs[0], 65536 + 77, True, False))
        if full:
            cases += [(dtype, 24, 65536 + 77, False, True), (dtype, 80, 65536 + 77, True, True), (dtype, 32, 16 * 320 * 320, dtype is F16, True)]
    if full:
        cases.append((F16, 1280, 65536 + 77, False, True))
    return cases


def bn_inputs(case, ratio=None):
    """z, dy, res (storage type, (npix, C)), gamma, beta.  ratio = r: z = sigma * randn + r * sigma per channel (the conditioning sweep)."""
    dtype, Cc, npix, use_res, _ = case
    rng = _seed("bn", case, ratio)
    zf = rng.standard_normal((npix, Cc), np.float32)
    if ratio is None:
        zf = zf * np.float32(1.5) + np.float32(0.5)
    else:
        sigma = np.linspace(0.5, 2.0, Cc, dtype=np.float32)
        zf = sigma * zf + np.float32(ratio) * sigma
    z = zf.astype(dtype)
    dy = rng.uniform(-1, 1, (npix, Cc)).astype(np.float32).astype(dtype)
    res = rng.uniform(-1, 1, (npix, Cc)).astype(np.float32).astype(dtype) if use_res else None
    gamma = rng.uniform(0.5, 1.5, Cc).astype(np.float32)
    beta = rng.uniform(-0.5, 0.5, Cc).astype(np.float32)
    return z, dy, res, gamma, beta


def run_bn(be, case, ratio=None, assert_tol=True, tag="bn"):
    """Every BatchNorm entry on one case: the fused forward / backward, y5_channel_sum, y5_bn_stats, and SyncBatchNorm's split entries with one rank.
    Asserts pads, bit-identity (split == fused, second launch == first) and -- unless assert_tol is False -- the tolerances; returns the figures."""
    dtype, Cc, npix, use_res, _ = case
    lib, dt, st = be.lib, y5_dtype(dtype), be.stream
    z, dy, res, gamma, beta = bn_inputs(case, ratio)
    off, (ldz, ldy, ldr, ld_dy, ld_dz) = _strides(dtype, Cc, 5)
    Z = Slab(be, npix, Cc, ldz, off, dtype, z, fill=np.nan)
    DY = Slab(be, npix, Cc, ld_dy, off, dtype, dy, fill=np.nan)
    R = Slab(be, npix, Cc, ldr, off, dtype, res, fill=np.nan) if use_res else None
    rp = R.p if R else None
    g, b = be.put(gamma), be.put(beta)
    nws = lib.y5_bn_workspace_bytes(Cc, npix)
    ws = be.put(np.full((nws,), 0xFF, U8))           # NaN patterns: every partial that is read must have been written

    def f32s(n, fill=np.nan):
        return [be.put(np.full((Cc,), fill, np.float32)) for _ in range(n)]

    def stats():
        return [be.put(np.zeros(Cc, np.float32)), be.put(np.ones(Cc, np.float32))] + f32s(2)

    def fused():
        Y, DZ = Slab(be, npix, Cc, ldy, off, dtype), Slab(be, npix, Cc, ld_dz, off, dtype)
        rm, rv, sm, si = stats()
        dg, db = f32s(2)
        ok(be, lib.y5_bn_silu_fwd(Z.p, dt, npix, Cc, ldz, be.ptr(g), be.ptr(b), EPS, MOMENTUM, be.ptr(rm), be.ptr(rv), be.ptr(sm), be.ptr(si), rp,
                                  ldr if use_res else 0, Y.p, ldy, be.ptr(ws), nws, st))
        ok(be, lib.y5_bn_silu_bwd(DY.p, ld_dy, Z.p, ldz, dt, npix, Cc, be.ptr(g), be.ptr(b), be.ptr(sm), be.ptr(si), DZ.p, ld_dz, be.ptr(dg), be.ptr(db),
                                  be.ptr(ws), nws, st))
        return [Y.h, DZ.h, rm, rv, sm, si, dg, db], Y, DZ

    first, Y, DZ = fused()
    cs = f32s(1)[0]
    ok(be, lib.y5_channel_sum(DY.p, dt, npix, Cc, ld_dy, be.ptr(cs), be.ptr(ws), nws, st))
    # SyncBatchNorm's split entries with ONE rank (count_total = npix, the sums untouched)
    sums = be.put(np.full((2 * Cc,), np.nan, np.float64))
    ok(be, lib.y5_bn_stats(Z.p, dt, npix, Cc, ldz, be.ptr(sums), be.ptr(ws), nws, st))
    Y2, DZ2 = Slab(be, npix, Cc, ldy, off, dtype), Slab(be, npix, Cc, ld_dz, off, dtype)
    rm2, rv2, sm2, si2 = stats()
    dg2, db2 = f32s(2)
    ok(be, lib.y5_bn_silu_fwd_from_sums(Z.p, dt, npix, Cc, ldz, be.ptr(g), be.ptr(b), EPS, MOMENTUM, be.ptr(rm2), be.ptr(rv2), be.ptr(sm2), be.ptr(si2),
                                        be.ptr(sums), npix, rp, ldr if use_res else 0, Y2.p, ldy, st))
    ok(be, lib.y5_bn_bwd_stats(DY.p, ld_dy, Z.p, ldz, dt, npix, Cc, be.ptr(g), be.ptr(b), be.ptr(sm2), be.ptr(si2), be.ptr(dg2), be.ptr(db2), be.ptr(ws),
                               nws, st))
    ok(be, lib.y5_bn_silu_bwd_from_sums(DY.p, ld_dy, Z.p, ldz, dt, npix, Cc, be.ptr(g), be.ptr(b), be.ptr(sm2), be.ptr(si2), be.ptr(dg2), be.ptr(db2),
                                        npix, DZ2.p, ld_dz, st))
    names = ("y", "dz", "running_mean", "running_var", "save_mean", "save_invstd", "dgamma", "dbeta")
    for nm, u, v in zip(names, first, [Y2.h, DZ2.h, rm2, rv2, sm2, si2, dg2, db2]):
        assert be.equal(u, v), f"{tag} {case}: split entries with one rank differ from the fused entries in {nm}"
    del Y2, DZ2
    second, Yb, DZb = fused()
    for nm, u, v in zip(names, first, second):
        assert be.equal(u, v), f"{tag} {case}: a second launch differs in {nm}"
    del second, Yb, DZb

    y, dz = Y.read("y"), DZ.read("dz")                      # (pads checked here)
    ref = BnRef(z, dy, res, gamma, beta)
    tol = TOL[np.dtype(dtype)]
    fig = dict(y=ref.worst("y", y, **tol), dz=ref.worst("dz", dz, **tol))
    tf = torch_fp32(z, dy, res, gamma, beta)
    if tf["y"] is not None:
        fig["y_torch"] = ref.worst("y", tf["y"], **tol)
    _, _, rm, rv, sm, si, dg, db = (be.get(h) for h in first)
    sums_h = be.get(sums)
    ksum = dict(dbeta=(db, ref.dbeta, ref.abs_dbeta, tf["dbeta"]), dgamma=(dg, ref.dgamma, ref.abs_dgamma, tf["dgamma"]),
                channel_sum=(be.get(cs), ref.sum_dy, ref.abs_dy, tf["sum_dy"]),
                stats_z=(sums_h[:Cc], ref.sum_z, ref.abs_z, tf["sum_z"]), stats_zz=(sums_h[Cc:], ref.sum_zz, ref.sum_zz, tf["sum_zz"]))
    for nm, (got, r64, a64, t32) in ksum.items():
        ek = _norm_err(got, r64, a64)
        et = _norm_err(t32, r64, a64) if t32 is not None else 0.0
        fig[nm] = (ek, et, ek / max(et, SUM_FLOOR))
    print(f"\n[{tag}] {np.dtype(dtype).name} C={Cc} npix={npix} res={int(use_res)}" + (f" r={ratio}" if ratio is not None else "") +
          f" | y {fig['y']:.3g} (torch fp32 {fig.get('y_torch', float('nan')):.3g}) dz {fig['dz']:.3g} of tol | " +
          " ".join(f"{nm} {fig[nm][0]:.2e}/{fig[nm][1]:.2e}={fig[nm][2]:.2f}" for nm in ksum))
    assert np.isfinite(fig["y"]) and np.isfinite(fig["dz"]), f"{tag} {case}: non-finite output"
    if not assert_tol:
        return fig
    assert fig["y"] <= 1.0, f"{tag} {case}: y is {fig['y']:.3g} x its tolerance"
    assert fig["dz"] <= 1.0, f"{tag} {case}: dz is {fig['dz']:.3g} x its tolerance"
    tm, tv = TOL_MEAN[np.dtype(dtype)], TOL_VAR[np.dtype(dtype)]
    np.testing.assert_allclose(sm, ref.mean, **tm)
    np.testing.assert_allclose(rm, ref.running_mean, **tm)
    np.testing.assert_allclose(si, ref.invstd, **tv)
    np.testing.assert_allclose(rv, ref.running_var, **tv)
    if ratio is not None:     # the 4x yardstick presumes that kernel and torch differ in summation ORDER only; under a large mean torch's two-pass variance
        return fig            # and the single-pass one differ in conditioning too (dgamma inherits invstd's error), so the sweep prints the ratios
    for nm in ksum:
        assert fig[nm][2] <= SUM_FACTOR, f"{tag} {case}: {nm} normalised error {fig[nm][0]:.3g}, torch fp32 {fig[nm][1]:.3g}, ratio {fig[nm][2]:.2f}"
    return fig


# ---- 5. conditioning of the single-pass variance -----------------------------------------------------------------------------------------------------
COND_RATIOS = (0, 4, 16, 64, 256)
COND_ASSERT_UP_TO = 16


def cond_cases(npix_list):
    return [(dtype, 16, n, False, False) for dtype in (F32, F16) for n in npix_list]


def run_bn_conditioning(be, case, ratio):
    """z = sigma * randn + r * sigma per channel.  r <= 16: the tolerances of part 4.  r = 64, 256: figures only (finite, pads untouched) -- the
    documented limit of var = E[z^2] - mean^2 from fp32 partial sums."""
    return run_bn(be, case, ratio=ratio, assert_tol=ratio <= COND_ASSERT_UP_TO, tag="bn-cond")
