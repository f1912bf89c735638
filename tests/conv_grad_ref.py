"""TEST INFRASTRUCTURE ONLY: case tables, references and ONE runner per kernel family for the two parts of a training step that sit around the
convolution kernels -- the filter repack kernels of yolov5_amd/csrc/train_misc.hip (y5_pack_conv_weight, y5_pack_dgrad_weight, y5_unpack_conv_wgrad and
the multi-filter walker y5_filter_jobs, kinds 0-3, fp16 / fp32 destination) and the data-gradient launches of train_engine._bwd_conv (sub-filter packed ON
THE DEVICE -> one y5_conv2d_fwd per parity class with output placement -> dx).  Every runner takes a backend of tests/train_glue_ref.py, so
tests/test_emu_conv_grad.py (host build, small shapes) and tests/test_gpu_conv_grad.py (device library, full tables) run the same code.

Repack: the reference is numpy fancy indexing of the documented layouts followed by astype(float16); both sides round to nearest even, every comparison
is bit for bit.  Sources are guarded with NaN (a read outside the filter poisons the result), destinations with a sentinel before and after.

Data gradient: float64 torch.nn.grad.conv2d_input on the operands as stored, plus the initial dx.  Tolerance per element:
    fp16: one rounding of the result, max(2^-11 |ref|, 2^-24); WITH a residual a second one of the convolution part alone (conv_igemm.h's epilogue
          rounds the accumulator to fp16 into its LDS scratch row, then adds the fp16 residual in fp32 and rounds again: two roundings);
    plus g * S, S = the float64 sum of the absolute products of that element, g = 4 x (torch's own fp32 CPU conv2d_input against float64 on the same
    operands, in units of S, floor 2^-22) -- the yardstick of 4.1a.  fp32 launches get g * S alone."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import torch

from tests.train_glue_ref import F16, F32, SENT, Guarded, _seed, assert_bits_equal, ok, y5_dtype
from yolov5_amd import _lib
from yolov5_amd.packing import round_up
from yolov5_amd.train_ops import _axis_classes

BAD_ARG, UNSUPPORTED = _lib.Y5_ERR_BAD_ARG, _lib.Y5_ERR_UNSUPPORTED
MT_CH = 1024          # elements per chunk of y5_filter_jobs_kernel
MT_GRID = 2048        # its grid cap

# ======================================================================================================================================================
# A. filter repack
# ======================================================================================================================================================
# fp32 values whose fp16 rounding is an edge: beyond the largest finite value (65504; 65520 is the tie that rounds to inf), subnormals and the ties
# around the smallest one (2^-25 rounds to even = 0), both zeros
SPECIALS = np.array([70000.0, -70000.0, 65520.0, 65519.996, 65504.0, -65520.0, 1e30, 3e-8, 2.0 ** -25, np.nextafter(np.float32(2.0 ** -25), np.float32(1)),
                     6e-8, 1e-5, -1e-5, 6.1e-5, 0.0, -0.0, -1e-30, 2.0 ** -24 * 1.5, 2.0 ** -24 * 2.5], np.float32)


def _to_f16(a):
    with np.errstate(over="ignore"):
        return a.astype(F16)


def taps_of(k, s, p):
    """The (th, tw) tap sets of every data-gradient parity class of a k x k stride-s pad-p convolution (train_ops._axis_classes; the taps do not
    depend on the image size)."""
    ax = [t for _, t, _, _ in _axis_classes(k, s, p, 64)]
    return [(tuple(th), tuple(tw)) for th in ax for tw in ax]


def spec(kind, c2, c1, kh, kw, view=None, th=(), tw=(), f32=False, kpad_extra=0, npad_extra=0):
    """(kind, C2, C1, KH, KW, view, Kpad, Npad, th, tw, f32) with the padding rules of train_engine._alloc_conv: Kpad = K rounded up to 64, Npad = rows
    rounded up to 32.  view = C1_view (kinds 0, 2) / C2_view (kind 1)."""
    if kind == 3:
        return (3, c2, 3, 6, 6, 0, 144, round_up(c2, 32) + npad_extra, (), (), False)
    if kind == 1:
        view = round_up(c2, 8) if view is None else view
        return (1, c2, c1, kh, kw, view, round_up(len(th) * len(tw) * view, 64) + kpad_extra, round_up(c1, 32) + npad_extra, tuple(th), tuple(tw), f32)
    view = c1 if view is None else view
    return (kind, c2, c1, kh, kw, view, round_up(kh * kw * view, 64) + kpad_extra, round_up(c2, 32) + npad_extra, (), (), f32)


def total_of(sp):
    kind, c2, c1, kh, kw, _, Kpad, Npad = sp[:8]
    return c2 * c1 * kh * kw if kind == 2 else Npad * Kpad


@functools.lru_cache(None)
def model_convs(name):
    """(C2, C1, k, s, p) of every nn.Conv2d of the model, in module order -- read from the model."""
    from yolov5_amd.yolo import DetectionModel

    out = []
    for m in DetectionModel(f"{name}.yaml").modules():
        if isinstance(m, torch.nn.Conv2d):
            c2, c1, kh, kw = m.weight.shape
            assert kh == kw and m.stride[0] == m.stride[1] and m.padding[0] == m.padding[1] and m.groups == 1
            out.append((c2, c1, kh, m.stride[0], m.padding[0]))
    return out


def conv_specs(c2, c1, k, s, p):
    """What one training step issues for one convolution (train_engine._run_jobs): the forward pack, the unpack of its weight gradient and one
    data-gradient sub-filter per parity class; the 3-channel stem has the NHWC view of 4 channels, its own kind-3 layout and no data gradient."""
    if c1 == 3:
        return [spec(0, c2, 3, k, k, view=4), spec(3, c2, 3, k, k), spec(2, c2, 3, k, k, view=4)]
    return [spec(0, c2, c1, k, k), spec(2, c2, c1, k, k)] + [spec(1, c2, c1, k, k, th=th, tw=tw) for th, tw in taps_of(k, s, p)]


def model_specs(name, distinct):
    convs = model_convs(name)
    if distinct:
        convs = list(dict.fromkeys(convs))
    return [sp for cv in convs for sp in conv_specs(*cv)]


# the cases beyond the model's own geometries
EXTRA_SPECS = (
    [spec(0, 32, 3, 6, 6, view=8), spec(2, 32, 3, 6, 6, view=8), spec(0, 64, 3, 6, 6, view=4), spec(3, 64, 3, 6, 6), spec(3, 40, 3, 6, 6, npad_extra=32)] +   # the stem
    [spec(1, 255, 128, 1, 1, view=256, th=(0,), tw=(0,)), spec(0, 255, 128, 1, 1), spec(2, 255, 128, 1, 1)] +                # Detect: 255 outputs in a 256 view
    [spec(0, 64, 40, 1, 1), spec(2, 64, 40, 1, 1), spec(0, 16, 8, 1, 1, kpad_extra=64)] +                                    # 1 x 1 with Kpad > K
    [spec(1, 48, 40, 3, 3, th=th, tw=tw) for th, tw in taps_of(3, 2, 1) + taps_of(3, 1, 1)] +                                # 1x1, 1x2, 2x1, 2x2 taps; flipped order
    [spec(1, 16, 8, 6, 6, th=th, tw=tw) for th, tw in taps_of(6, 2, 2)] +                                                    # 6 x 6 s2 p2: 3 x 3 taps per class
    [spec(0, 40, 24, 3, 3, f32=True), spec(1, 40, 24, 3, 3, th=(2, 0), tw=(1,), f32=True), spec(1, 255, 16, 1, 1, view=256, th=(0,), tw=(0,), f32=True)])
assert taps_of(3, 2, 1) == [((1,), (1,)), ((1,), (2, 0)), ((2, 0), (1,)), ((2, 0), (2, 0))] and taps_of(3, 1, 1) == [((2, 1, 0), (2, 1, 0))]
BIG_SPECS = [spec(0, 640, 640, 3, 3), spec(2, 8, 8, 1, 1)]   # yolov5x's 3 x 3 (3 686 400 elements), then 64 elements: the walker's largest step down


def _interleave(specs):
    """Round-robin over the kinds, so that neighbouring jobs are of different kinds."""
    by = {k: [s for s in specs if s[0] == k] for k in (0, 1, 2, 3)}
    out = []
    while any(by.values()):
        for k in (0, 1, 2, 3):
            if by[k]:
                out.append(by[k].pop(0))
    return out


def jobs_table(full):
    """The y5_filter_jobs table.  full: every convolution of yolov5s as a step issues it + the extra cases, with yolov5x's 3 x 3 in the middle followed
    by a 64-element job.  Reduced (host build): yolov5n's distinct geometries instead of yolov5s.  Asserted: more than 2048 chunks (workgroups wrap),
    a job below 1024 elements directly after the largest, totals that are / are not multiples of 1024, every kind next to another kind."""
    specs = _interleave(model_specs("yolov5s" if full else "yolov5n", distinct=not full) + list(EXTRA_SPECS))
    half = len(specs) // 2
    specs = specs[:half] + (BIG_SPECS if full else [max(specs, key=total_of), spec(2, 8, 8, 1, 1)]) + specs[half:]
    tot = [total_of(s) for s in specs]
    assert sum(-(-t // MT_CH) for t in tot) > MT_GRID
    assert any(a == max(tot) and b < MT_CH for a, b in zip(tot, tot[1:])) and any(t % MT_CH == 0 for t in tot) and any(t % MT_CH for t in tot)
    assert {s[0] for s in specs} == {0, 1, 2, 3} and sum(a[0] != b[0] for a, b in zip(specs, specs[1:])) > len(specs) // 2
    if full:
        assert len(specs) >= 194
    return specs


WALKER_SPECS = [spec(2, 8, 8, 1, 1), spec(2, 5, 8, 3, 3), spec(3, 8, 3, 6, 6), spec(2, 8, 8, 1, 1), spec(0, 32, 40, 1, 1)]   # 1 + 1 + 5 + 1 + 2 chunks


def repack_ref(sp, src):
    """Expected destination of one spec from its source array, by fancy indexing of the layouts documented at the kernels."""
    kind, c2, c1, kh, kw, view, Kpad, Npad, th, tw, f32 = sp
    if kind == 2:      # gw[n][c][kh][kw] = dw[n][(kh*KW + kw)*C1v + c]
        n, c, i, j = np.indices((c2, c1, kh, kw), sparse=True)
        return src[n, (i * kw + j) * view + c]
    out = np.zeros((Npad, Kpad), np.float32)       # rows >= C2 (C1 for kind 1), columns >= K and the view-pad channels are written as +0
    if kind == 0:      # out[n][(kh*KW + kw)*C1v + c] = w[n][c][kh][kw]
        n, c, i, j = np.indices((c2, c1, kh, kw), sparse=True)
        out[n, (i * kw + j) * view + c] = src
    elif kind == 1:    # out[c1][(a*NTW + b)*C2v + c2] = w[c2][c1][th[a]][tw[b]]
        m, n, a, b = np.indices((c2, c1, len(th), len(tw)), sparse=True)
        out[n, (a * len(tw) + b) * view + m] = src[m, n, np.asarray(th)[a], np.asarray(tw)[b]]
    else:              # stem: out[n][(c*6 + kh)*8 + kw] = w[n][c][kh][kw], taps kw = 6, 7 zero
        n, c, i, j = np.indices((c2, 3, 6, 6), sparse=True)
        out[n, (c * 6 + i) * 8 + j] = src
    return out if f32 else _to_f16(out)


def repack_source(sp, rng):
    """fp32 master weights with the rounding edges at the front; for the unpack a packed gradient that is NaN wherever the kernel must not read."""
    kind, c2, c1, kh, kw, view, Kpad, Npad = sp[:8]
    w = rng.standard_normal((c2, c1, kh, kw), np.float32)
    if kind != 2:
        if not sp[10]:
            n = min(len(SPECIALS), w.size)
            w.reshape(-1)[:n] = SPECIALS[:n]
        return w
    dw = np.full((Npad, Kpad), np.nan, np.float32)
    n, c, i, j = np.indices((c2, c1, kh, kw), sparse=True)
    dw[n, (i * kw + j) * view + c] = w
    return dw


class RepackJob:
    def __init__(self, be, sp, tag):
        self.sp = sp
        src = repack_source(sp, _seed("repack", sp, tag))
        self.ref = repack_ref(sp, src)
        self.src = Guarded(be, src.shape, F32, src, fill=np.nan)
        self.dst = Guarded(be, self.ref.shape, self.ref.dtype)

    def row(self, j):
        kind, c2, c1, kh, kw, view, Kpad, Npad, th, tw, f32 = self.sp
        j.src, j.dst, j.total, j.kind = self.src.p.value, self.dst.p.value, total_of(self.sp), kind
        j.C2, j.C1, j.KH, j.KW, j.Kpad, j.Npad, j.nth, j.ntw = c2, c1, kh, kw, Kpad, Npad, len(th), len(tw)
        j.C1_view, j.C2_view = (0, view) if kind == 1 else (view, 0)
        for q, v in enumerate(th):
            j.th[q] = v
        for q, v in enumerate(tw):
            j.tw[q] = v
        j.reserved = 1 if f32 else 0

    def check(self, what):
        assert_bits_equal(self.dst.read(f"{what} {self.sp}"), self.ref, f"{what} {self.sp}")


def _ints(v):
    return (C.c_int * max(len(v), 1))(*v)


def run_single(be, sp):
    """One spec through its single-filter entry point (kinds 0-2, fp16 destination)."""
    kind, c2, c1, kh, kw, view, Kpad, Npad, th, tw, f32 = sp
    assert kind in (0, 1, 2) and not f32
    jb, lib = RepackJob(be, sp, "single"), be.lib
    if kind == 0:
        ok(be, lib.y5_pack_conv_weight(jb.src.p, c2, c1, kh, kw, view, jb.dst.p, Kpad, Npad, be.stream))
    elif kind == 1:
        ok(be, lib.y5_pack_dgrad_weight(jb.src.p, c2, c1, kh, kw, _ints(th), len(th), _ints(tw), len(tw), view, jb.dst.p, Kpad, Npad, be.stream))
    else:
        ok(be, lib.y5_unpack_conv_wgrad(jb.src.p, Kpad, jb.dst.p, c2, c1, kh, kw, view, be.stream))
    jb.check(("y5_pack_conv_weight", "y5_pack_dgrad_weight", "y5_unpack_conv_wgrad")[kind])


def single_specs(specs):
    return [s for s in dict.fromkeys(specs) if s[0] != 3 and not s[10]]


def launch_jobs(be, jobs, max_total):
    arr = (_lib.FilterJob * len(jobs))()
    for j, jb in zip(arr, jobs):
        jb.row(j)
    tab = be.put(np.frombuffer(arr, dtype=np.uint8).copy())
    rc = be.lib.y5_filter_jobs(be.ptr(tab), len(jobs), max_total, be.stream)
    be.get(tab)   # (synchronises; keeps the table alive until the launch is done)
    return rc


def run_jobs(be, specs, slack=0, tag="jobs"):
    """The whole table in ONE y5_filter_jobs launch; max_total = the true maximum + slack (a larger bound only changes the grid)."""
    jobs = [RepackJob(be, sp, (tag, i)) for i, sp in enumerate(specs)]
    ok(be, launch_jobs(be, jobs, max(total_of(s) for s in specs) + slack))
    for i, jb in enumerate(jobs):
        jb.check(f"y5_filter_jobs job {i} of {len(jobs)}")


def run_repack_refusals(be):
    lib, st = be.lib, be.stream
    jb = RepackJob(be, spec(0, 16, 8, 3, 3), "refuse")
    d1 = RepackJob(be, spec(1, 16, 8, 3, 3, th=(0, 2), tw=(1,)), "refuse")
    one, nine = _ints((0,)), _ints(tuple(range(9)))

    def bad(rc, code=BAD_ARG):
        assert rc == code and lib.y5_last_error(), (rc, lib.y5_last_error())
    bad(lib.y5_pack_conv_weight(jb.src.p, 16, 8, 3, 3, 7, jb.dst.p, 128, 32, st))                         # C1_view < C1
    bad(lib.y5_pack_conv_weight(jb.src.p, 16, 8, 3, 3, 8, jb.dst.p, 71, 32, st))                          # Kpad < KH*KW*C1_view = 72
    bad(lib.y5_pack_conv_weight(jb.src.p, 16, 8, 3, 3, 8, jb.dst.p, 128, 15, st))                         # Npad < C2
    bad(lib.y5_unpack_conv_wgrad(jb.src.p, 128, jb.dst.p, 16, 8, 3, 3, 7, st))                            # C1_view < C1
    bad(lib.y5_unpack_conv_wgrad(jb.src.p, 71, jb.dst.p, 16, 8, 3, 3, 8, st))                             # Kpad too small
    bad(lib.y5_pack_dgrad_weight(d1.src.p, 16, 8, 3, 3, nine, 9, one, 1, 16, d1.dst.p, 64 * 9, 32, st))   # nth > 8
    bad(lib.y5_pack_dgrad_weight(d1.src.p, 16, 8, 3, 3, one, 1, nine, 9, 16, d1.dst.p, 64 * 9, 32, st))   # ntw > 8
    bad(lib.y5_pack_dgrad_weight(d1.src.p, 16, 8, 3, 3, one, 0, one, 1, 16, d1.dst.p, 64, 32, st))        # nth < 1
    bad(lib.y5_pack_dgrad_weight(d1.src.p, 16, 8, 3, 3, one, 1, one, 1, 15, d1.dst.p, 64, 32, st))        # C2_view < C2
    bad(lib.y5_pack_dgrad_weight(d1.src.p, 16, 8, 3, 3, _ints((0, 2)), 2, one, 1, 16, d1.dst.p, 31, 32, st))   # Kpad < nth*ntw*C2_view = 32
    bad(lib.y5_pack_dgrad_weight(d1.src.p, 16, 8, 3, 3, one, 1, one, 1, 16, d1.dst.p, 64, 7, st))         # Npad < C1
    arr = (_lib.FilterJob * 1)()
    jb.row(arr[0])
    tab = be.put(np.frombuffer(arr, dtype=np.uint8).copy())
    bad(lib.y5_filter_jobs(be.ptr(tab), 0, 4096, st))
    bad(lib.y5_filter_jobs(be.ptr(tab), 65536, 4096, st))
    bad(lib.y5_filter_jobs(be.ptr(tab), 1, 0, st))
    bad(lib.y5_filter_jobs(None, 1, 4096, st))
    bad(lib.y5_filter_jobs(be.ptr(tab), 1, 2 ** 31 - 1, st), UNSUPPORTED)
    bad(lib.y5_filter_jobs(be.ptr(tab), 1, 2 ** 31, st), UNSUPPORTED)
    for j in (jb, d1):     # nothing was launched
        assert_bits_equal(j.dst.read("refused"), np.full(j.ref.shape, SENT, j.ref.dtype), "destination after the refusals")


# ======================================================================================================================================================
# B. data-gradient launches
# ======================================================================================================================================================
# The ids whose y5_conv2d_fwd takes a launch with output placement -- conv.hip's general implicit-GEMM ranges: 0..13 (kNumIgemm), 22..29 (kRing0 +
# kNumRing), 35..55 (kBig0 + kNumBig).  NOT the streaming pointwise (14..21, 56, 84..87), streaming 3x3 (30..34, 78..83), stream-K (57..60), halo
# (61..77, 90..92), virtual-upsample (88, 89: up_c = 0 here), K-streamed (93, 94) or 8-phase (95, 96) families.  The residual read is the same
# epilogue, so the list with a residual is the same; fp32 has the first four tiles only.
NUM_CFGS = 97
PLACED_IDS = list(range(0, 14)) + list(range(22, 30)) + list(range(35, 56))
PLACED_IDS_RES = list(PLACED_IDS)
PLACED_IDS_F32 = [0, 1, 2, 3]
_PLACEMENT = (UNSUPPORTED, b"output placement needs a general implicit-GEMM configuration")


def expected_refusal(cfg, dtype):
    """(status, fragment of y5_last_error) a placed launch with this id must be refused with; None for the ids that accept."""
    f32 = np.dtype(dtype) == np.dtype(F32)
    if cfg in (PLACED_IDS_F32 if f32 else PLACED_IDS):
        return None
    if cfg in (95, 96):
        return (UNSUPPORTED, b"8-phase configurations need")
    if cfg in (93, 94):
        return (UNSUPPORTED, b"K-streamed pointwise configurations need")
    if cfg in (88, 89):
        return (UNSUPPORTED, b"serve the layers with up_c > 0")
    if f32 and cfg >= 22:
        return (UNSUPPORTED, b"configurations 22 and above are fp16 only")
    if 57 <= cfg <= 60:
        return (UNSUPPORTED, b"stream-K with output placement is not built")
    if f32 and cfg in PLACED_IDS:
        return (BAD_ARG, b"fp32 supports tile configs 0..3 only")
    return _PLACEMENT


# (name, B, H, W, C1, C2, k, s, p, max_blocks): dx is (B, H, W, C1), dz (B, OH, OW, C2) read through a view of round_up(C2, 8) channels
DG_TAILS = ("tails", 2, 20, 18, 72, 64, 3, 2, 1, 0)          # 180 pixels per class (no multiple of any tile height), 72 channels (96 filter rows)
DG_ODD = ("odd", 2, 41, 37, 40, 48, 3, 2, 1, 0)              # classes of 21x19, 21x18, 20x19, 20x18; 48 input channels (BK64 ids: gather-table mode)
DG_VIEW = ("view255", 1, 14, 12, 64, 255, 3, 2, 1, 0)        # 255 of 256 channels of dz: the view-pad channel holds finite garbage
DG_TRAIN = ("train", 2, 160, 160, 32, 64, 3, 2, 1, 8)        # 64 x 80 x 80 -> 32 x 160 x 160, eight persistent workgroups: >= 6 tiles each
DG_TRAIN2 = ("train40", 2, 80, 80, 64, 64, 3, 2, 1, 8)       # 64 x 40 x 40 -> 80 x 80
DG_SMALL = ("small", 1, 7, 5, 16, 16, 3, 2, 1, 0)            # the per-id case of the host build: odd sizes, one tile
DG_MATRIX = [DG_TAILS, DG_ODD, DG_VIEW, DG_TRAIN]
DG_DENSE = [("dense3", 2, 20, 18, 64, 64, 3, 1, 1, 0), ("dense1", 2, 20, 18, 64, 255, 1, 1, 0, 0), ("dense3odd", 1, 9, 11, 24, 40, 3, 1, 1, 0)]
DG_G8 = [("g8k3", 2, 40, 40, 128, 128, 3, 1, 1, 0), ("g8k1", 2, 40, 40, 256, 128, 1, 1, 0, 0)]   # ids 95 / 96: C >= 64, dense, accumulating
DG_EDGES = [DG_SMALL, DG_ODD, DG_VIEW, ("even", 1, 8, 8, 64, 40, 3, 2, 1, 0), ("k6", 1, 10, 8, 8, 16, 6, 2, 2, 0)] + DG_DENSE
SUM_FLOOR, SUM_FACTOR = 2.0 ** -22, 4.0


def dg_classes(case):
    """The parity classes exactly as train_engine._alloc_conv builds them."""
    _, B, H, W, C1, C2, k, s, p, _ = case
    out = []
    for rh, th, padh, nh in _axis_classes(k, s, p, H):
        for rw, tw, padw, nw in _axis_classes(k, s, p, W):
            if nh == 0 or nw == 0:
                continue
            assert th and tw
            out.append(dict(rh=rh, rw=rw, nh=nh, nw=nw, th=th, tw=tw, pad=(padh, padw)))
    return out


@functools.lru_cache(8)
def dg_inputs(case, dtype):
    """w (C2, C1, k, k) fp32 holding values of the storage type, dz (B, OH, OW, C2), dx0 (B, H, W, C1); float64 reference of the convolution part, S and
    torch's fp32 error in units of S."""
    _, B, H, W, C1, C2, k, s, p, _ = case
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    rng = _seed("dgrad", case, np.dtype(dtype).name)
    w = rng.uniform(-0.25, 0.25, (C2, C1, k, k)).astype(np.float32).astype(dtype).astype(np.float32)
    dz = rng.uniform(-1, 1, (B, OH, OW, C2)).astype(np.float32).astype(dtype)
    dx0 = rng.uniform(-1, 1, (B, H, W, C1)).astype(np.float32).astype(dtype)

    def ci(wt, gt):
        return torch.nn.grad.conv2d_input((B, C1, H, W), wt, gt.permute(0, 3, 1, 2), s, p).permute(0, 2, 3, 1).numpy()
    w64, z64 = torch.from_numpy(w).double(), torch.from_numpy(dz.astype(np.float64))
    conv = ci(w64, z64)
    S = ci(w64.abs(), z64.abs())
    t32 = ci(torch.from_numpy(w), torch.from_numpy(dz.astype(np.float32)))
    et = float((np.abs(t32.astype(np.float64) - conv) / np.maximum(S, 1e-300)).max())
    return dict(w=w, dz=dz, dx0=dx0, conv=conv, S=S, et=et, OH=OH, OW=OW)


class DgradRun:
    """Buffers of one data gradient: dz and dx are channel slices at DIFFERENT non-zero offsets of wider buffers with different strides."""

    def __init__(self, be, case, dtype, acc):
        _, B, H, W, C1, C2, k, s, p, _ = case
        self.be, self.case, self.dtype, self.acc = be, case, np.dtype(dtype), acc
        inp = self.inp = dg_inputs(case, dtype)
        epp = 16 // self.dtype.itemsize
        c2s = self.c2s = round_up(C2, 8)
        self.offz, self.ldz = epp, epp + c2s + 2 * epp
        self.offx, self.ldx = 2 * epp, 2 * epp + C1 + 3 * epp
        if self.ldx == self.ldz:
            self.ldx += epp
        rng = _seed("dgbuf", case)
        # dz: finite garbage in the pad columns AND in the view-pad channels [C2, c2s) -- the zero filter rows must cancel it
        hz = rng.uniform(-8, 8, (B, inp["OH"], inp["OW"], self.ldz)).astype(np.float32).astype(dtype)
        hz[..., self.offz:self.offz + C2] = inp["dz"]
        hx = np.full((B, H, W, self.ldx), SENT, dtype)
        hx[..., self.offx:self.offx + C1] = inp["dx0"] if acc else np.nan      # without accumulation every payload element must be WRITTEN
        self.hx0 = hx
        self.dz, self.dx = be.put(hz), be.put(hx)
        self.w = Guarded(be, inp["w"].shape, F32, inp["w"], fill=np.nan)
        self.zb = be.put(np.zeros(round_up(C1, 32), np.float32))
        self.subs = []
        for cl in dg_classes(case):
            Kp, Np = round_up(len(cl["th"]) * len(cl["tw"]) * c2s, 64), round_up(C1, 32)
            cl.update(Kpad=Kp, Npad=Np, wp=Guarded(be, (Np, Kp), dtype))
            self.subs.append(cl)
        self.pack()

    def pack(self):
        """Every sub-filter on the device: y5_pack_dgrad_weight (fp16) / a y5_filter_jobs kind-1 table with the fp32 destination."""
        be, (_, B, H, W, C1, C2, k, s, p, _) = self.be, self.case
        if self.dtype == np.dtype(F16):
            for cl in self.subs:
                ok(be, be.lib.y5_pack_dgrad_weight(self.w.p, C2, C1, k, k, _ints(cl["th"]), len(cl["th"]), _ints(cl["tw"]), len(cl["tw"]), self.c2s,
                                                   cl["wp"].p, cl["Kpad"], cl["Npad"], be.stream))
            return
        arr = (_lib.FilterJob * len(self.subs))()
        for j, cl in zip(arr, self.subs):
            j.src, j.dst, j.total, j.kind, j.reserved = self.w.p.value, cl["wp"].p.value, cl["Npad"] * cl["Kpad"], 1, 1
            j.C2, j.C1, j.KH, j.KW, j.C2_view, j.Kpad, j.Npad, j.nth, j.ntw = C2, C1, k, k, self.c2s, cl["Kpad"], cl["Npad"], len(cl["th"]), len(cl["tw"])
            for q, v in enumerate(cl["th"]):
                j.th[q] = v
            for q, v in enumerate(cl["tw"]):
                j.tw[q] = v
        tab = be.put(np.frombuffer(arr, dtype=np.uint8).copy())
        ok(be, be.lib.y5_filter_jobs(be.ptr(tab), len(self.subs), max(cl["Npad"] * cl["Kpad"] for cl in self.subs), be.stream))
        be.get(tab)

    def launch(self, cfg, only_first=False):
        """One y5_conv2d_fwd per class with the descriptor of train_engine._bwd_conv; returns the first non-zero status."""
        be, (_, B, H, W, C1, C2, k, s, p, mb) = self.be, self.case
        es, dense, inp = self.dtype.itemsize, s == 1, self.inp
        gx = be.ptr(self.dx, self.offx * es)
        for cl in self.subs[:1] if only_first else self.subs:
            d = _lib.ConvDesc(dtype=y5_dtype(self.dtype), B=B, H=inp["OH"], W=inp["OW"], C1=self.c2s, ldx=self.ldz, OH=cl["nh"], OW=cl["nw"], C2=C1,
                              ldy=self.ldx, KH=len(cl["th"]), KW=len(cl["tw"]), SH=1, SW=1, PH=cl["pad"][0], PW=cl["pad"][1], act=0, Kpad=cl["Kpad"],
                              Npad=cl["Npad"], ldr=self.ldx if self.acc else 0, ld2=0, cfg=cfg, max_blocks=mb, out_mul_h=0 if dense else s,
                              out_mul_w=0 if dense else s, out_off_h=cl["rh"], out_off_w=cl["rw"], out_H=0 if dense else H, out_W=0 if dense else W)
            rc = be.lib.y5_conv2d_fwd(C.byref(d), be.ptr(self.dz, self.offz * es), cl["wp"].p, be.ptr(self.zb), gx if self.acc else None, gx, None,
                                      be.stream)
            if rc:
                return rc
        return 0

    def check(self, tag):
        """Pads bit-identical, every payload element written, per-element tolerance; returns (kernel error, torch fp32 error, ratio) in units of S."""
        _, B, H, W, C1, C2, k, s, p, _ = self.case
        inp, f16 = self.inp, self.dtype == np.dtype(F16)
        for cl in self.subs:     # the packed sub-filters: guards intact, rows >= C1 and the view-pad channels zero (bit-exact layout: part A)
            cl["wp"].read(f"{tag}: packed sub-filter")
        got = self.be.get(self.dx)
        lo, hi = self.offx, self.offx + C1
        assert_bits_equal(got[..., :lo], self.hx0[..., :lo], f"{tag}: dx columns before the slice")
        assert_bits_equal(got[..., hi:], self.hx0[..., hi:], f"{tag}: dx pad columns")
        g = got[..., lo:hi].astype(np.float64)
        nan = np.isnan(g)
        assert not nan.any(), f"{tag}: {int(nan.sum())} of {nan.size} dx elements were never written (NaN prefill), first at {np.argwhere(nan)[0].tolist()}"
        ref = inp["conv"] + (inp["dx0"].astype(np.float64) if self.acc else 0.0)
        err = np.abs(g - ref)
        rnd = 0.0
        if f16:
            rnd = np.maximum(2.0 ** -11 * np.abs(ref), 2.0 ** -24)
            if self.acc:   # the epilogue rounds the convolution to fp16 BEFORE it adds the residual: two roundings
                rnd = rnd + np.maximum(2.0 ** -11 * np.abs(inp["conv"]), 2.0 ** -24)
        ek = float((np.maximum(err - rnd, 0.0) / np.maximum(inp["S"], 1e-300)).max())
        ratio = ek / max(inp["et"], SUM_FLOOR)
        return ek, inp["et"], ratio, float((err / np.maximum(rnd + SUM_FACTOR * max(inp["et"], SUM_FLOOR) * inp["S"], 1e-300)).max())


def run_dgrad(be, case, cfg, acc, dtype=F16):
    """Pack, launch every class with configuration `cfg`, check.  A refusal is an error here: the caller names ids that must accept."""
    r = DgradRun(be, case, dtype, acc)
    ok(be, r.launch(cfg))
    tag = f"dgrad {case[0]} {np.dtype(dtype).name} cfg {cfg} acc {int(acc)}"
    ek, et, ratio, frac = r.check(tag)
    print(f"\n[{tag}] kernel {ek:.2e} / torch fp32 {et:.2e} of S = {ratio:.2f} (bound {SUM_FACTOR:g}); worst element at {frac:.2f} of its tolerance")
    assert ratio <= SUM_FACTOR, f"{tag}: accumulation error {ek:.3g} S beyond the roundings, torch fp32 {et:.3g} S, ratio {ratio:.2f} > {SUM_FACTOR:g}"
    return ratio


def run_placed_id(be, case, cfg, dtype, accs=(0, 1), check_acc=None):
    """Ask the library whether id `cfg` takes the placed launches of `case`, without and with the residual.  The answer must be the committed list's;
    a refusal must carry its family's message and launch nothing.  check_acc: the accumulate values whose accepted launches are also verified."""
    exp = expected_refusal(cfg, dtype)
    out = {}
    for acc in accs:
        r = DgradRun(be, case, dtype, acc)
        rc = r.launch(cfg)
        msg = be.lib.y5_last_error() if rc else b""
        tag = f"placed {case[0]} {np.dtype(dtype).name} cfg {cfg} acc {acc}"
        listed = cfg in (PLACED_IDS_F32 if np.dtype(dtype) == np.dtype(F32) else (PLACED_IDS_RES if acc else PLACED_IDS))
        assert (rc == 0) == listed, f"{tag}: the library {'refuses' if rc else 'takes'} an id that the committed list {'holds' if listed else 'lacks'} ({msg})"
        if rc:
            assert exp is not None and rc == exp[0] and exp[1] in msg, f"{tag}: refused with status {rc}, {msg!r}; expected {exp}"
            assert_bits_equal(be.get(r.dx), r.hx0, f"{tag}: dx after the refusal")
        elif check_acc is None or acc in check_acc:
            ek, et, ratio, frac = r.check(tag)
            print(f"\n[{tag}] kernel {ek:.2e} / torch fp32 {et:.2e} of S = {ratio:.2f}; worst element at {frac:.2f} of its tolerance")
            assert ratio <= SUM_FACTOR, f"{tag}: ratio {ratio:.2f} > {SUM_FACTOR:g}"
            out[acc] = ratio
    return out


# ---- the 2^31 probe ------------------------------------------------------------------------------------------------------------------------------------
def big_placed_geometry(over):
    """A placed 1 x 1 launch whose DESTINATION image B * out_H * out_W * ldy * 2 bytes lies just under / just over 2^31 while B * OH * OW = 4050 pixels:
    every 32nd row and column of a 1426^2 (1427^2) image, the last class row / column on the image's last row / column."""
    B, ldy, mul = 2, 264, 32
    side = 1427 if over else 1426
    n = -(-side // mul)
    off = side - 1 - (n - 1) * mul
    nbytes = B * side * side * ldy * 2
    assert (nbytes >= 2 ** 31) == over and 0 <= off < mul and abs(nbytes - 2 ** 31) < 2 ** 22
    return B, side, n, off, mul, ldy


def run_big_placed(be, over, acc):
    """GPU only.  Returns 'ok', 'refused: <message>' or raises; the caller skips if the 2 GiB destination cannot be allocated."""
    B, side, n, off, mul, ldy = big_placed_geometry(over)
    C1, C2 = 64, 256      # launch view: 64 input channels, 256 output channels
    dev = be.dev
    rng = _seed("big", over, acc)
    x = rng.uniform(-1, 1, (B, n, n, C1)).astype(np.float32).astype(F16)
    w = rng.uniform(-0.25, 0.25, (C2, C1)).astype(np.float32).astype(F16)
    dx0 = rng.uniform(-1, 1, (B, n, n, C2)).astype(np.float32).astype(F16)
    buf = torch.full((B, side, side, ldy), SENT, dtype=torch.float16, device=dev)
    sl = (slice(None), slice(off, None, mul), slice(off, None, mul), slice(0, C2))
    if acc:
        buf[sl] = torch.from_numpy(dx0).to(dev)
    wp = be.put(w)
    d = _lib.ConvDesc(dtype=_lib.Y5_F16, B=B, H=n, W=n, C1=C1, ldx=C1, OH=n, OW=n, C2=C2, ldy=ldy, KH=1, KW=1, SH=1, SW=1, PH=0, PW=0, act=0, Kpad=C1,
                      Npad=C2, ldr=ldy if acc else 0, ld2=0, cfg=-1, max_blocks=0, out_mul_h=mul, out_mul_w=mul, out_off_h=off, out_off_w=off,
                      out_H=side, out_W=side)
    xd, zb = be.put(x), be.put(np.zeros(C2, np.float32))
    rc = be.lib.y5_conv2d_fwd(C.byref(d), be.ptr(xd), be.ptr(wp), be.ptr(zb), be.ptr(buf) if acc else None, be.ptr(buf), None, be.stream)
    if rc:
        msg = be.lib.y5_last_error()
        assert over and rc == UNSUPPORTED and msg, (rc, msg)
        torch.cuda.synchronize(dev)
        assert bool((buf == SENT).all()) or acc, "refused, yet the destination was written"
        return "refused: " + msg.decode(errors="replace")
    torch.cuda.synchronize(dev)
    got = buf[sl].cpu().numpy().astype(np.float64)
    conv = x.astype(np.float64).reshape(-1, C1) @ w.astype(np.float64).T
    S = np.abs(x.astype(np.float64)).reshape(-1, C1) @ np.abs(w.astype(np.float64)).T
    ref = conv + (dx0.astype(np.float64).reshape(-1, C2) if acc else 0.0)
    rnd = np.maximum(2.0 ** -11 * np.abs(ref), 2.0 ** -24) + (np.maximum(2.0 ** -11 * np.abs(conv), 2.0 ** -24) if acc else 0.0)
    err = np.abs(got.reshape(-1, C2) - ref)
    worst = float((np.maximum(err - rnd, 0.0) / S).max())
    print(f"\n[big placed over={int(over)} acc={int(acc)}] {B * side * side * ldy * 2} destination bytes, accumulation error {worst:.2e} S")
    assert worst <= SUM_FACTOR * SUM_FLOOR, f"placed image {'over' if over else 'under'} 2^31 bytes: error {worst:.3g} S"   # 64 products: torch fp32 is below the floor
    assert got.reshape(B, n, n, C2)[-1, -1, -1].any(), "the far end of the buffer"
    buf[sl] = SENT          # everything else must still hold the sentinel
    assert bool((buf == SENT).all()), "a pixel outside the class was written"
    return "ok"
