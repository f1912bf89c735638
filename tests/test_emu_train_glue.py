"""CPU: the memory-bound kernels between the convolutions of the training path -- BatchNorm + SiLU forward / backward and their statistics passes, the
gradient-routing and layout kernels, the SPPF pooling chain -- compiled for the host on the HIP emulator, on the small cases of tests/train_glue_ref.py
(tests/test_gpu_train_glue.py runs the full tables on the device); plus the argument checks of the BatchNorm entries."""
import ctypes as C

import numpy as np
import pytest

from tests import train_glue_ref as tg
from tests.hipemu.emu import aligned, ptr
from yolov5_amd import _lib


@pytest.fixture(scope="module")
def be():
    return tg.EmuBackend()


def small(cases):
    return [c for c in cases if not c[-1]]


@pytest.fixture
def sppf_gv(monkeypatch):
    return lambda v: monkeypatch.delenv("Y5_SPPF_GV", raising=False) if v is None else monkeypatch.setenv("Y5_SPPF_GV", str(v))


# ---- 1. pure data movement ----
@pytest.mark.parametrize("case", small(tg.MOVE_CASES))
def test_emu_upsample2x(be, case):
    tg.run_upsample2x(be, case)


@pytest.mark.parametrize("case", small(tg.MOVE_CASES))
def test_emu_copy_slice(be, case):
    tg.run_copy_slice(be, case)


@pytest.mark.parametrize("case", tg.NCHW_CASES)
def test_emu_nchw_to_nhwc(be, case):
    tg.run_nchw_to_nhwc(be, case)


@pytest.mark.parametrize("case", tg.NHWC_NCHW_CASES)
def test_emu_nhwc_to_nchw(be, case):
    tg.run_nhwc_to_nchw(be, case)


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("case", small(tg.RAW_CASES))
def test_emu_head_layout(be, case, f32):
    tg.run_raw(be, case, f32)


def test_emu_memset_zero(be):
    tg.run_memset_zero(be)


# ---- 2. exactly specified arithmetic ----
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("case", small(tg.SUM_CASES))
def test_emu_upsample2x_bwd(be, case, acc):
    tg.run_upsample2x_bwd(be, case, acc)


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("case", small(tg.SUM_CASES))
def test_emu_add_slice(be, case, acc):
    tg.run_add_slice(be, case, acc)


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("case", tg.SUM_CASES_F32)
def test_emu_glue_f32_upsample2x_bwd_and_add_slice(be, case, acc):
    tg.run_upsample2x_bwd(be, case, acc, f32=True)
    tg.run_add_slice(be, case, acc, f32=True)


@pytest.mark.parametrize("case", tg.SPPF_BWD_F32_CASES)
def test_emu_glue_f32_sppf_pool_bwd(be, case):
    tg.run_sppf_bwd_f32(be, case)


# ---- 3. SPPF pooling chain ----
@pytest.mark.parametrize("case", small(tg.SPPF_CASES))
def test_emu_sppf_pool(be, case, sppf_gv):
    tg.run_sppf_pool(be, case, sppf_gv)


def test_emu_sppf_pool_refuses_a_plane_beyond_lds(be, sppf_gv):
    tg.run_sppf_pool(be, tg.SPPF_UNSUPPORTED, sppf_gv, unsupported=True)


# ---- 4. BatchNorm family ----
@pytest.mark.parametrize("case", tg.bn_cases(full=False))
def test_emu_bn_family(be, case):
    tg.run_bn(be, case)


# ---- 5. conditioning ----
@pytest.mark.parametrize("ratio", tg.COND_RATIOS)
@pytest.mark.parametrize("case", tg.cond_cases((1600, 102400)))
def test_emu_bn_conditioning(be, case, ratio):
    tg.run_bn_conditioning(be, case, ratio)


# ---- 6. argument checks ----
def _bn_args(dtype, Cc, npix=6):
    v = 16 // np.dtype(dtype).itemsize
    ld = Cc + 4 * v
    a = dict(z=aligned((npix, ld), dtype, 1.0), dy=aligned((npix, ld), dtype, 1.0), r=aligned((npix, ld), dtype, 0.0), y=aligned((npix, ld), dtype, 0.0),
             g=aligned((Cc,), np.float32, 1.0), b=aligned((Cc,), np.float32, 0.0), rm=aligned((Cc,), np.float32, 0.0), rv=aligned((Cc,), np.float32, 1.0),
             sm=aligned((Cc,), np.float32, 0.0), si=aligned((Cc,), np.float32, 1.0), dg=aligned((Cc,), np.float32, 0.0), db=aligned((Cc,), np.float32, 0.0),
             sums=aligned((2 * Cc,), np.float64, 0.0), part=aligned((2 * Cc,), np.float32, 0.0))
    return a, ld, v


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
def test_bn_rejects_bad_strides(be, dtype):
    """A pixel stride below C, or one that is not a multiple of the 16-byte vector, would go straight into vector loads: every entry refuses it on the host,
    naming the stride.  ldr is looked at only when a residual is given."""
    lib, dt, Cc, npix = be.lib, tg.y5_dtype(dtype), 16, 6
    a, ld, v = _bn_args(dtype, Cc, npix)
    p = {k: ptr(x) for k, x in a.items()}
    nws = lib.y5_bn_workspace_bytes(Cc, npix)
    ws = aligned((nws,), np.uint8)

    def fwd(ldz=ld, ldy=ld, ldr=ld, res=True):
        return lib.y5_bn_silu_fwd(p["z"], dt, npix, Cc, ldz, p["g"], p["b"], 1e-3, 0.03, p["rm"], p["rv"], p["sm"], p["si"], p["r"] if res else None, ldr,
                                  p["y"], ldy, ptr(ws), nws, None)

    def fwd_sums(ldz=ld, ldy=ld, ldr=ld, res=True):
        return lib.y5_bn_silu_fwd_from_sums(p["z"], dt, npix, Cc, ldz, p["g"], p["b"], 1e-3, 0.03, p["rm"], p["rv"], p["sm"], p["si"], p["sums"], npix,
                                            p["r"] if res else None, ldr, p["y"], ldy, None)

    def fwd_part(ldz=ld, ldy=ld, ldr=ld, res=True):
        return lib.y5_bn_silu_fwd_from_partials(p["z"], dt, npix, Cc, ldz, p["g"], p["b"], 1e-3, 0.03, p["rm"], p["rv"], p["sm"], p["si"], p["part"], 1,
                                                p["r"] if res else None, ldr, p["y"], ldy, None)

    def bwd(ld_dy=ld, ldz=ld, ld_dz=ld):
        return lib.y5_bn_silu_bwd(p["dy"], ld_dy, p["z"], ldz, dt, npix, Cc, p["g"], p["b"], p["sm"], p["si"], p["y"], ld_dz, p["dg"], p["db"], ptr(ws), nws, None)

    def bwd_sums(ld_dy=ld, ldz=ld, ld_dz=ld):
        return lib.y5_bn_silu_bwd_from_sums(p["dy"], ld_dy, p["z"], ldz, dt, npix, Cc, p["g"], p["b"], p["sm"], p["si"], p["dg"], p["db"], npix, p["y"], ld_dz, None)

    def bwd_stats(ld_dy=ld, ldz=ld):
        return lib.y5_bn_bwd_stats(p["dy"], ld_dy, p["z"], ldz, dt, npix, Cc, p["g"], p["b"], p["sm"], p["si"], p["dg"], p["db"], ptr(ws), nws, None)

    def stats(ldz=ld):
        return lib.y5_bn_stats(p["z"], dt, npix, Cc, ldz, p["sums"], ptr(ws), nws, None)

    def chsum(ld_=ld):
        return lib.y5_channel_sum(p["dy"], dt, npix, Cc, ld_, p["db"], ptr(ws), nws, None)

    entries = [(fwd, ("ldz", "ldy", "ldr")), (fwd_sums, ("ldz", "ldy", "ldr")), (fwd_part, ("ldz", "ldy", "ldr")), (bwd, ("ld_dy", "ldz", "ld_dz")),
               (bwd_sums, ("ld_dy", "ldz", "ld_dz")), (bwd_stats, ("ld_dy", "ldz")), (stats, ("ldz",)), (chsum, ("ld_",))]
    for fn, names in entries:
        assert fn() == 0, lib.y5_last_error()
        for nm in names:
            for bad in (Cc - v, 0, -ld, Cc + 1, ld + v // 2):      # below C (also zero / negative), not a multiple of the vector
                assert fn(**{nm: bad}) == _lib.Y5_ERR_BAD_ARG, (fn.__name__, nm, bad)
                assert nm.rstrip("_").encode() in lib.y5_last_error(), (fn.__name__, nm, lib.y5_last_error())
    for fn in (fwd, fwd_sums, fwd_part):                           # without a residual ldr is not looked at
        assert fn(ldr=0, res=False) == 0 and fn(ldr=3, res=False) == 0, lib.y5_last_error()


def test_bn_refuses_fp32_above_1024_channels(be):
    """More than 256 16-byte vectors per pixel do not fit the workgroup: fp16 ends at C = 2048, fp32 at C = 1024 -- yolov5x's 1280-channel layers cannot
    run the fp32 training plan, and say so instead of computing something."""
    lib = be.lib
    for dtype, Cc in ((np.float32, 1280), (np.float32, 1028), (np.float16, 2056)):
        a, ld, _ = _bn_args(dtype, Cc, 2)
        nws = lib.y5_bn_workspace_bytes(Cc, 2)
        ws = aligned((nws,), np.uint8)
        rc = lib.y5_bn_silu_fwd(ptr(a["z"]), tg.y5_dtype(dtype), 2, Cc, ld, ptr(a["g"]), ptr(a["b"]), 1e-3, 0.03, ptr(a["rm"]), ptr(a["rv"]), ptr(a["sm"]),
                                ptr(a["si"]), None, 0, ptr(a["y"]), ld, ptr(ws), nws, None)
        assert rc == _lib.Y5_ERR_BAD_ARG
        assert lib.y5_last_error() == b"bn: C must be a multiple of 16 bytes, at most 256 vectors"
        rc = lib.y5_channel_sum(ptr(a["dy"]), tg.y5_dtype(dtype), 2, Cc, ld, ptr(a["db"]), ptr(ws), nws, None)
        assert rc == _lib.Y5_ERR_BAD_ARG
