"""TEST INFRASTRUCTURE ONLY: case tables, references and ONE runner per check for the fused Bottlenecks at 32 and 64 channels (yolov5_amd/csrc/conv_bneck.h:
y5_bottleneck_fwd at C = 32 / 64, y5_bottleneck_cv3_fwd at C = 32).  Every runner takes a backend of tests/train_glue_ref.py, so
tests/test_emu_bneck_parity.py (the kernels compiled for the host, the rows of the tables marked for it) and tests/test_gpu_bneck.py (the device
library, the full tables) run the same cases through the same code.

Rules every case follows: x, y2 and the outputs are slabs -- a pixel stride larger than the payload, all strides of a call different, a non-zero channel
offset, NaN in the channels of x / y2 outside the slice, the sentinel around the output payload AND in TAIL pixels behind the last one, outputs compared
whole.  Packed filters have wider row pitches (Kpad1 != Kpad2 != Kpad3) with NaN in the columns the kernel must not read; the third filter and its bias have
the 2 C rows / entries the entry documents (the C = 32 kernel reads all 64 whatever C3 is), NaN in those of channels >= C3.  Inputs are signed, uniform in [-1, 1]; filters He-scaled; every bias
is non-zero (0.1 <= |b| <= 0.5), so a t outside the image computed as SiLU(b1) instead of 0 shows at every border pixel.

    C  the float64 chain on the operands as stored, rounding where the kernel rounds: t = fp16(SiLU(W1 x + b1)), zero outside the image;
       v = SiLU(W2 * t + b2), u = fp16(v), o = fp16(u + x) with add, else o = u; cv3: z = act3(W3 [o ; y2] + b3).  Elementwise
           |got - o| <= ulp16(u) + [add] ulp16(o) + 4 E          cv3: |got - fp16(z)| <= ulp16(z) + 4 E
       with E = the largest |v32 - v64| (cv3: |z32 - z64|) of torch's fp32 CPU chain with the same roundings on the same case (4 = front_ref.SUM_FACTOR):
       a deviation below one fp16 step in front of a rounding moves the result by at most that step plus the deviation, and the fp32 chain's own flips
       of t are inside E.  No NaN; the share of elements whose bits differ from the reference's is at most 4 x the fp32 chain's own share + 0.5 %.
    D  the same launch under another deal of tiles to workgroups, another ring depth, the four-wave form against the aliased eight-wave form, or at
       another batch position: bit equality.
    E  (GPU) 40 runs beside a bandwidth-heavy copy: bit equality, the first run held to C on the first and the last image.
    G  refusals (status, message, nothing written) and one launch on either side of the 2^31-byte guard (GPU).

Measured on the MI355X (__expf, v_rcp_f32) -- worst error in units of the bound; share of elements that differ from the reference: kernel / torch's fp32
chain (rows of one key share their figures: D); the table with E per case is DESIGN.md 4.1d:
    (32, 1, 4, 8, 1)        0.000   0.000 % / 0.195 %        (64, 1, 4, 8, 0)        0.000   0.000 % / 0.098 %
    (32, 3, 12, 40, 1)      0.564   0.009 % / 0.187 %        (64, 3, 20, 40, 1)      0.754   0.128 % / 0.199 %
    (64, 1, 4, 24, 0)       0.538   0.488 % / 1.742 %        (32, 2, 16, 64, 1)      0.568   0.133 % / 0.156 %
    (64, 2, 16, 64, 0)      0.738   0.304 % / 0.662 %        (32, 4, 160, 160, 1)    0.479   0.073 % / 0.124 %
    (64, 4, 80, 80, 1)      0.600   0.124 % / 0.230 %        (64, 4, 80, 80, 0)      0.585   0.456 % / 0.877 %
    cv3 (1, 4, 8, 1, 64, 1)       0.000   0.000 % / 0.049 %  cv3 (3, 12, 40, 1, 48, 0)     0.370   0.200 % / 0.922 %
    cv3 (2, 16, 64, 0, 56, 1)     0.297   0.317 % / 0.928 %  cv3 (2, 8, 16, 0, 8, 1)       0.141   0.146 % / 0.879 %
    cv3 (4, 160, 160, 1, 64, 1)   0.331   0.329 % / 0.556 %  550 x 164 x 248 x 32, first and last image   0.570   0.086 % / 0.141 %
The host build on the rows marked for it: 0.06 to 0.76 of the bound, 0.05 % to 1.63 % against 0.05 % to 1.76 %."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import torch
import torch.nn.functional as F

from tests.front_ref import SUM_FACTOR, TAIL, _big_read, _big_slab, _bias, _filter, _frozen, _image, _repeat, _t, _untouched, _widen, ulp16
from tests.train_glue_ref import F16, F32, SENT, Guarded, Slab, _seed, assert_bits_equal, ok
from yolov5_amd import _lib
from yolov5_amd.packing import pack_conv_weight

BAD, UNS = _lib.Y5_ERR_BAD_ARG, _lib.Y5_ERR_UNSUPPORTED
SHARE_FACTOR, SHARE_SLACK = 4.0, 0.005
MBS_GPU = (1, 2, 5, 7, 8, 9, 16, 0, 10000)   # 9: G &= ~7; 10 000: the clamp to the tile count
MBS_EMU = (1, 2, 8, 0)


def D(depth):
    """Bits 16.. of max_blocks: the ring depth (C = 32: 1 to 3; C = 64: 0 = eight waves with t aliased onto the stage, 1 = four waves)."""
    return depth << 16


# (C, B, H, W, add, max_blocks)
BN_CASES_EMU = (
    [(32, 1, 4, 8, 1, 0), (64, 1, 4, 8, 0, 0)] +                          # one tile, every pixel on the border
    [(32, 3, 12, 40, 1, m) for m in (0, 8, 16, 8 | D(2))] +               # 45 wave tiles on four waves: 12 block tiles, the last partial, on 8 workgroups
    [(64, 3, 20, 40, 1, m) for m in (8, 8 | D(1), 0)] +                   # 75 wave tiles on eight waves: 10 block tiles, the last partial; 0: the library's
    [(64, 1, 4, 24, 0, 0)])                                               # own grid under fewer than 8 slots.  3 wave tiles: fewer than one workgroup's waves
BN_CASES = BN_CASES_EMU + (
    [(32, 2, 16, 64, 1, m) for m in (1 | D(1), 1 | D(2), 5 | D(3))] +     # one to five workgroups walk 16 block tiles: ramp, steady state, drain of every depth
    [(64, 2, 16, 64, 0, m) for m in (1, 1 | D(1), 5 | D(1))])
# the benchmark's geometry at a small batch, default grid: more block tiles than resident workgroups
BN_BENCH = [(32, 4, 160, 160, 1, 0), (64, 4, 80, 80, 1, 0), (64, 4, 80, 80, 0, D(1))]
# C = 32: (B, H, W, add, C3, act3, max_blocks)
CV3_CASES_EMU = [(1, 4, 8, 1, 64, 1, 0), (3, 12, 40, 1, 48, 0, 8)]
CV3_CASES = CV3_CASES_EMU + [(2, 16, 64, 0, 56, 1, 5), (2, 8, 16, 0, 8, 1, 0)]
CV3_BENCH = (4, 160, 160, 1, 64, 1, 0)
SCHED_SHAPE, BATCH_SHAPE, SCHED_C3 = (2, 16, 64), (5, 12, 40), 56
FIX_CASE = (64, 3, 20, 40, 1)                                             # refused under the library's own grid before the fix in launch_bneck


def bn_key(case):
    Cc, B, H, W, add, _ = case
    return (Cc, B, H, W, add, 0, 0)


def cv3_key(case):
    B, H, W, add, C3, act3, _ = case
    return (32, B, H, W, add, C3, act3)


# ---- operands and references ---------------------------------------------------------------------------------------------------------------------------
def weights(rng, Cc, C3):
    ws = (_filter(rng, (Cc, Cc, 1, 1), Cc), _bias(rng, Cc), _filter(rng, (Cc, Cc, 3, 3), 9 * Cc), _bias(rng, Cc))
    if C3:
        ws += (_filter(rng, (C3, 2 * Cc, 1, 1), 2 * Cc), _bias(rng, C3))
    return _frozen(*ws)


@functools.lru_cache(maxsize=6)
def operands(key):
    """key = (C, B, H, W, add, C3, act3), C3 = 0 without cv3 -> x (B, H, W, C) fp16, the filters and biases, y2 or None.  Read-only, shared."""
    Cc, B, H, W, _, C3, _ = key
    rng = _seed("bneck", key)
    x = _image(rng, (B, H, W, Cc), "signed")
    ws = weights(rng, Cc, C3)
    y2 = _image(rng, (B, H, W, Cc), "signed") if C3 else None
    return _frozen(x)[0], ws, _frozen(y2)[0]


def _r16(t):
    """To fp16 and back in ONE rounding from any precision (numpy rounds float64 directly)."""
    return torch.from_numpy(t.numpy().astype(F16).astype(t.numpy().dtype))


def _nhwc(t):
    return np.ascontiguousarray(t.permute(0, 2, 3, 1).numpy())


def chain(x, ws, y2, add, act3, dtype):
    """The chain in `dtype`, rounded where the kernel rounds -> v (before the first output rounding), o, z (cv3, NOT rounded) as NHWC arrays."""
    w = [_t(a).to(dtype) for a in ws]
    xt = _t(x).to(dtype).permute(0, 3, 1, 2)
    t = _r16(F.silu(F.conv2d(xt, w[0], w[1])))
    v = F.silu(F.conv2d(t, w[2], w[3], padding=1))       # zero padding of t: t is zero outside the image
    o = _r16(v)
    if add:
        o = _r16(o + xt)
    z = None
    if y2 is not None:
        z = F.conv2d(torch.cat((o, _t(y2).to(dtype).permute(0, 3, 1, 2)), 1), w[4], w[5])
        z = _nhwc(F.silu(z) if act3 else z)
    return _nhwc(v), _nhwc(o), z


class Ref:
    """ref = the float64 value the output is the fp16 rounding of; tol per element; r32 = the fp32 chain's fp16 output; E."""

    def __init__(self, key):
        x, ws, y2 = operands(key)
        add, C3, act3 = key[4:]
        v64, o64, z64 = chain(x, ws, y2, add, act3, torch.float64)
        v32, o32, z32 = chain(x, ws, y2, add, act3, torch.float32)
        if C3:
            self.E = float(np.abs(z32.astype(np.float64) - z64).max())
            self.ref, self.tol, self.r32 = z64, ulp16(z64) + SUM_FACTOR * self.E, z32.astype(F16)
        else:
            self.E = float(np.abs(v32.astype(np.float64) - v64).max())
            u = v64.astype(F16).astype(np.float64)
            self.ref, self.tol, self.r32 = o64, ulp16(u) + (ulp16(o64) if add else 0.0) + SUM_FACTOR * self.E, o32.astype(F16)
        self.r16 = self.ref.astype(F16)
        _frozen(self.ref, self.tol, self.r32, self.r16)


@functools.lru_cache(maxsize=3)
def reference(key):
    return Ref(key)


def check(got, ref, tag, img=None):
    """C on the whole output or on image `img`; prints and returns (worst error / bound, share of differing elements, the fp32 chain's share)."""
    sel = slice(None) if img is None else img
    r, tol, r16, r32 = ref.ref[sel], ref.tol[sel], ref.r16[sel], ref.r32[sel]
    g64 = got.astype(np.float64)
    assert not np.isnan(g64).any(), f"{tag}: NaN in the output (a pixel never written, or a read outside the slice / the filter columns)"
    err = np.abs(g64 - r16.astype(np.float64))
    frac = float((err / tol).max())
    share, share32 = float(np.mean(got != r16)), float(np.mean(r32 != r16))
    print(f"\n[{tag}] worst |kernel - ref| {err.max():.3e} = {frac:.3f} of the bound, E = {ref.E:.2e}; differs from the reference in {share:.3%} of the "
          f"elements, torch's fp32 chain in {share32:.3%}")
    bad = err > tol
    assert not bad.any(), f"{tag}: {int(bad.sum())} of {bad.size} elements beyond the bound, worst {frac:.2f} x, first at {np.argwhere(bad)[0].tolist()}"
    assert share <= SHARE_FACTOR * share32 + SHARE_SLACK, f"{tag}: {share:.3%} of the elements differ from the reference, torch's fp32 chain in {share32:.3%}"
    return frac, share, share32


# ---- one launch ----------------------------------------------------------------------------------------------------------------------------------------
class Run:
    """The operands of one key on the backend; launch() gives the payload of a fresh output slab after the sentinel checks."""

    def __init__(self, be, key, x, ws, y2=None):
        self.be, self.key = be, key
        Cc, B, H, W, _, C3, _ = key
        self.npix, self.cout = B * H * W, C3 or Cc
        self.ldx, self.ld2, self.ldo = Cc + 24, Cc + 56, self.cout + 16
        self.x = Slab(be, self.npix, Cc, self.ldx, 16, F16, x, fill=np.nan)
        self.y2 = Slab(be, self.npix, Cc, self.ld2, 24, F16, y2, fill=np.nan) if C3 else None
        packs = [pack_conv_weight(_t(ws[i]), _t(ws[i + 1]), torch.float16) for i in range(0, len(ws), 2)]
        self.K = [packs[0][3] + 24, packs[1][3] + 8] + ([packs[2][3] + 40] if C3 else [])
        wide = [_widen(p[0].numpy(), k, kp) for p, k, kp in zip(packs, (Cc, 9 * Cc, 2 * Cc), self.K)]
        bias = [p[1].numpy() for p in packs]
        assert wide[0].shape[0] == Cc and wide[1].shape[0] == Cc
        if C3:          # the 2 C rows and bias entries the entry documents (the kernel reads them all); those of channels >= C3 must not reach the output
            w3, b3 = np.full((2 * Cc, self.K[2]), np.nan, F16), np.full((2 * Cc,), np.nan, F32)
            w3[:C3], b3[:C3] = wide[2][:C3], bias[2][:C3]
            wide[2], bias[2] = w3, b3
        self.w = [Guarded(be, a.shape, F16, a, fill=np.nan) for a in wide]
        self.b = [Guarded(be, a.shape, F32, a, fill=np.nan) for a in bias]

    def slab(self):
        return Slab(self.be, self.npix + TAIL, self.cout, self.ldo, 8, F16)

    def call(self, slab, mb, **kw):
        """The launch into `slab` with the run's own arguments; `kw` replaces any of them by the entry point's names (out = the output pointer)."""
        Cc, B, H, W, add, C3, act3 = self.key
        a = dict(x=self.x.p, ldx=self.ldx, w1=self.w[0].p, b1=self.b[0].p, K1=self.K[0], w2=self.w[1].p, b2=self.b[1].p, K2=self.K[1],
                 out=None if slab is None else slab.p, ldo=self.ldo, B=B, H=H, W=W, C=Cc, add=add)
        if C3:
            a.update(y2=self.y2.p, ld2=self.ld2, w3=self.w[2].p, b3=self.b[2].p, K3=self.K[2], C3=C3, act3=act3)
        a.update(kw)
        lib, st = self.be.lib, self.be.stream
        if C3:
            return lib.y5_bottleneck_cv3_fwd(a["x"], a["ldx"], a["w1"], a["b1"], a["K1"], a["w2"], a["b2"], a["K2"], a["y2"], a["ld2"], a["w3"], a["b3"], a["K3"],
                                             a["C3"], a["act3"], a["out"], a["ldo"], a["B"], a["H"], a["W"], a["C"], a["add"], mb, st)
        return lib.y5_bottleneck_fwd(a["x"], a["ldx"], a["w1"], a["b1"], a["K1"], a["w2"], a["b2"], a["K2"], a["out"], a["ldo"], a["B"], a["H"], a["W"], a["C"],
                                     a["add"], mb, st)

    def payload(self, out, what):
        got = out.read(f"{what} output")
        assert np.all(got[self.npix:] == SENT), f"{what}: pixels behind the end of the batch were written"
        return got[:self.npix].reshape(self.key[1:4] + (self.cout,))

    def launch(self, mb, what="bneck"):
        out = self.slab()
        ok(self.be, self.call(out, mb))
        return self.payload(out, what)


def _run(be, key):
    return Run(be, key, *operands(key))


def run_parity(be, key, mb, tag):
    """C: one launch against the float64 chain."""
    return check(_run(be, key).launch(mb, tag), reference(key), tag)


def run_bn_parity(be, case):
    return run_parity(be, bn_key(case), case[5], f"bneck {case}")


def run_cv3_parity(be, case):
    return run_parity(be, cv3_key(case), case[6], f"bneck+cv3 {case}")


# ---- D. schedule and batch invariance ------------------------------------------------------------------------------------------------------------------
def sched_key(kind, shape=SCHED_SHAPE):
    """kind: 32, 64 or 'cv3'."""
    return (32,) + shape + (1, SCHED_C3, 1) if kind == "cv3" else (kind,) + shape + (1, 0, 0)


def run_schedule(be, kind, mbs):
    """The output bits depend neither on the grid nor (C = 32) on the ring depth nor (C = 64) on the form, four waves or eight with t aliased."""
    r = _run(be, sched_key(kind))
    first = r.launch(mbs[0])
    assert np.abs(first.astype(F32)).max() > 0
    others = list(mbs[1:])
    if kind == 32:
        others += [m | D(d) for d in (2, 3) for m in (mbs[0], mbs[1], 0)]
    elif kind == 64:
        others += [m | D(1) for m in (mbs[0], mbs[1], 0)]
    for mb in others:
        assert_bits_equal(r.launch(mb), first, f"bneck {kind} {SCHED_SHAPE} max_blocks {mb & 0xffff} depth {mb >> 16} against max_blocks {mbs[0]}")


def run_batch(be, kind):
    """The same image at batch positions 0, 1 and B - 1."""
    key = sched_key(kind, BATCH_SHAPE)
    Cc, C3 = key[0], key[5]
    rng = _seed("bneck batch", key)
    x = _image(rng, BATCH_SHAPE + (Cc,), "signed")
    y2 = _image(rng, BATCH_SHAPE + (Cc,), "signed") if C3 else None
    for a in (x, y2):
        if a is not None:
            a[1], a[-1] = a[0], a[0]
    got = Run(be, key, x, weights(rng, Cc, C3), y2).launch(0)
    assert_bits_equal(got[1], got[0], f"bneck {kind}: image 1 against image 0")
    assert_bits_equal(got[-1], got[0], f"bneck {kind}: image B - 1 against image 0")
    assert not np.array_equal(got[2], got[0])


def run_own_grid(be, budget=None, case=FIX_CASE):
    """The library's own grid on FIX_CASE (75 wave tiles on eight waves: a partial last tile, 10 block tiles) with fewer than eight workgroup slots -- on
    the device under y5_set_cu_budget(budget) -- runs, and gives the bits of the explicit grid of 8."""
    r = _run(be, case + (0, 0))
    want = r.launch(8)
    if budget is not None:
        ok(be, be.lib.y5_set_cu_budget(budget))
    try:
        got = r.launch(0, "bneck, the library's own grid")
    finally:
        if budget is not None:
            ok(be, be.lib.y5_set_cu_budget(0))
    assert_bits_equal(got, want, f"bneck {case}: the library's own grid against max_blocks 8")


# ---- E. repeatability under load (GPU only) ------------------------------------------------------------------------------------------------------------
def run_repeat(be, key, tag):
    r, ref = _run(be, key), reference(key)
    out = r.slab()
    first = _repeat(be, lambda: r.call(out, 0), [out.h])[0]
    out.h.copy_(first)
    got = r.payload(out, tag)
    for i in (0, -1):
        check(got[i], ref, f"{tag}, image {i}", img=i)


# ---- G. refusals ---------------------------------------------------------------------------------------------------------------------------------------
def _refused(r, status, msg, mb=0, **kw):
    """The call with `kw` over the run's own arguments: status, message, and neither the output slab nor x written."""
    be, out = r.be, r.slab()
    kw = {k: (v(out) if callable(v) else v) for k, v in kw.items()}
    rc = r.call(out, mb, **kw)
    err = be.lib.y5_last_error()
    what = f"{'bneck+cv3' if r.key[5] else 'bneck'} C = {kw.get('C', r.key[0])} {sorted(kw)} max_blocks {mb}"
    assert rc == status and msg in err, f"{what}: status {rc}, {err!r}; expected {status} with {msg!r}"
    _untouched(out, f"{what}: the output")
    x = operands(r.key)[0]
    assert_bits_equal(r.x.read(f"{what}: x").reshape(x.shape), x, f"{what}: x")


def _shift(r, slab, nbytes):
    return r.be.ptr(slab.h, slab.off * 2 + nbytes)


def run_bn_refusals(be):
    r = _run(be, (32, 3, 12, 40, 1, 0, 0))        # 45 wave tiles, 12 block tiles, the last partial
    r64 = _run(be, FIX_CASE + (0, 0))             # 75 wave tiles on eight waves, 10 block tiles
    ok(be, r.call(r.slab(), 8))
    for run in (r, r64):
        Cc = run.key[0]
        _refused(run, UNS, b"32, 64 and 128 channels", C=48)
        _refused(run, UNS, b"H % 4 == 0 and W % 8 == 0", H=run.key[2] - 2)
        _refused(run, UNS, b"H % 4 == 0 and W % 8 == 0", W=run.key[3] - 4)
        _refused(run, BAD, b"16-byte aligned", x=_shift(run, run.x, 2))
        _refused(run, BAD, b"16-byte aligned", out=lambda o, run=run: _shift(run, o, 2))
        _refused(run, BAD, b"bad strides", ldx=Cc - 8)
        _refused(run, BAD, b"bad strides", ldo=Cc - 8)
        _refused(run, BAD, b"must not overlap x", out=run.x.p, ldo=run.ldx)                          # in place
        _refused(run, BAD, b"must not overlap x", out=_shift(run, run.x, 16), ldo=run.ldx)           # the same pixel stride, channel slices 8 apart
        _refused(run, BAD, b"must not overlap x", out=_shift(run, run.x, -16), ldo=run.ldx)
        _refused(run, BAD, b"must not overlap x", out=run.x.p)                                       # another pixel stride over the same bytes
        _refused(run, UNS, b"unsupported number of stages", mb=D(4 if Cc == 32 else 2))
        for cap in (1, 5, 7):
            _refused(run, UNS, b"a grid cap below 8", mb=cap)
    _refused(r, UNS, b"a grid cap below 8", mb=3 | D(2))
    _refused(r64, UNS, b"a grid cap below 8", mb=7 | D(1))   # four waves: 19 block tiles


def run_cv3_refusals(be):
    r = _run(be, (32, 1, 8, 16, 1, 48, 1))
    ok(be, r.call(r.slab(), 0))
    _refused(r, UNS, b"built for 32-channel", C=64)
    _refused(r, UNS, b"H % 4 == 0 and W % 8 == 0", H=6)
    for c3 in (12, 0, 4, 72):
        _refused(r, BAD, b"output channels", C3=c3)
    _refused(r, BAD, b"output channels", ldo=40)
    _refused(r, BAD, b"bad strides", ld2=24)
    _refused(r, BAD, b"16-byte aligned", y2=_shift(r, r.y2, 2))
    _refused(r, BAD, b"must not overlap x or y2", out=r.x.p, ldo=r.ldx)
    _refused(r, BAD, b"must not overlap x or y2", out=r.x.p)
    _refused(r, BAD, b"must not overlap x or y2", out=r.y2.p, ldo=r.ld2)
    _refused(r, BAD, b"must not overlap x or y2", out=_shift(r, r.y2, -16), ldo=r.ld2, C3=16)   # channels [-8, 8) of y2's slice
    y2 = operands(r.key)[2]
    assert_bits_equal(r.y2.read("bneck+cv3 refusals: y2").reshape(y2.shape), y2, "bneck+cv3 refusals: y2")
    for name in ("x", "w1", "b1", "w2", "b2", "y2", "w3", "b3", "out"):
        _refused(r, BAD, b"null pointer", **{name: None})


# ---- G. the size guard (GPU only) ----------------------------------------------------------------------------------------------------------------------
BIG = (32, 550, 164, 248, 48, 40)      # C, B, H, W, ldx, ldy: 22 369 600 pixels x 96 bytes = 2^31 - 2048 bytes of x; 551 images are over the guard


def run_size_guard(be, over):
    """x just under 2^31 bytes (the largest batch of this image size the guard admits) runs, and its first and LAST image are right by C (byte offsets
    are int arithmetic); one image more is refused."""
    Cc, B, H, W, ldx, ldy = BIG
    B += 1 if over else 0
    assert (B * H * W * ldx * 2 >= 0x7fffffff) == over and (B - 1) * H * W * ldx * 2 < 0x7fffffff
    key = (Cc, 1, H, W, 1, 0, 0)
    x, ws, _ = operands(key)
    r = Run(be, key, x, ws)            # the filters and biases; its own one-image input is not used
    img = H * W
    xb = torch.full((B * img, ldx), float("nan"), dtype=torch.float16, device=be.dev)
    xb[:, 8:8 + Cc] = 0
    one = _t(x.reshape(img, Cc)).to(be.dev)
    xb[:img, 8:8 + Cc] = one
    xb[(B - 1) * img:, 8:8 + Cc] = one
    h, yp = _big_slab(be, B * img, Cc, ldy, 8)
    rc = r.call(None, 0, x=C.c_void_p(xb.data_ptr() + 16), ldx=ldx, out=yp, ldo=ldy, B=B)
    if over:
        assert rc == UNS and b"exceeds 2^31" in be.lib.y5_last_error(), (rc, be.lib.y5_last_error())
        torch.cuda.synchronize()
        assert bool((h == SENT).all()), "the refused call wrote its output"
        return
    ok(be, rc)
    head, last = _big_read(h, B * img, Cc, 8, img, "bneck under 2^31 bytes")
    ref = reference(key)
    check(head.reshape(H, W, Cc), ref, "bneck under 2^31 bytes, first image", img=0)
    check(last.reshape(H, W, Cc), ref, "bneck under 2^31 bytes, last image", img=0)
