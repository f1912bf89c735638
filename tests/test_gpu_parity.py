"""GPU (-m gpu): parity of the HIP path, called through the C-ABI, against the golden vectors (reference outputs)
and the CPU oracle.  Tolerances: fp32 boxes/logits within 1e-4 relative (north_star); NMS selection bit-exact."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import detgen, yolo_oracle as yo
from oracle.make_golden import NMS_CASES, nms_case_pred

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def test_native_library_is_loaded():
    from yolov5_amd import _lib

    lib = _lib.lib()
    assert lib.y5_version() >= 100
    maps = open("/proc/self/maps").read()
    assert "libyolov5_hip.so" in maps


# ---- conv kernel, direct C-ABI ----------------------------------------------------------------------------
CONV_CASES = [
    # B, H, W, C1, C2, k, s, p, act, residual, up2, cfg, max_blocks, dtype
    (2, 20, 20, 32, 32, 1, 1, 0, 1, False, False, -1, 0, "f16"),
    (2, 23, 17, 32, 64, 3, 1, 1, 1, True, False, -1, 0, "f16"),
    (2, 40, 40, 64, 128, 3, 2, 1, 1, False, False, -1, 0, "f16"),
    (2, 20, 20, 64, 128, 1, 1, 0, 0, False, True, -1, 0, "f16"),
    (1, 9, 9, 16, 16, 3, 1, 1, 1, True, False, -1, 0, "f16"),
    (1, 16, 16, 40, 256, 1, 1, 0, 1, False, False, 3, 0, "f16"),
    (2, 20, 20, 512, 256, 1, 1, 0, 1, False, False, -1, 0, "f16"),
    (2, 20, 20, 256, 512, 3, 1, 1, 1, False, False, 9, 0, "f16"),
    (2, 20, 20, 256, 256, 1, 1, 0, 0, False, False, -1, 0, "f16"),
    (2, 12, 12, 32, 32, 3, 1, 1, 1, True, False, -1, 0, "f32"),
    (1, 14, 10, 4, 32, 3, 2, 1, 1, False, False, -1, 0, "f32"),
    (2, 20, 20, 128, 128, 3, 1, 1, 1, False, False, -1, 0, "f32"),
    (4, 40, 40, 64, 64, 1, 1, 0, 1, False, False, 7, 5, "f16"),     # persistent: 50 one-chunk tiles on 5 workgroups
    (3, 33, 31, 32, 96, 3, 1, 1, 1, True, True, 0, 8, "f16"),
] + [(2, 21, 19, c1, 160, 3, 1, 1, 1, True, False, cfg, 3, "f16") for cfg in list(range(14)) + list(range(22, 30)) + list(range(35, 56)) for c1 in (64, 48)] + [
    # streaming pointwise kernel (conv_pw.h, cfg 14..21): many tiles per wave so the counted-vmcnt ring reaches steady
    # state and drains; LDS-DMA races would show up here as wrong tiles (run on the real machine, not the emulator)
    (16, 40, 40, 32, 32, 1, 1, 0, 1, False, False, 14, 8, "f16"),
    (16, 40, 40, 64, 32, 1, 1, 0, 1, False, False, 15, 8, "f16"),
    (64, 40, 40, 64, 64, 1, 1, 0, 1, False, False, 16, 0, "f16"),
    (16, 40, 40, 64, 64, 1, 1, 0, 1, False, True, 17, 16, "f16"),
    (16, 20, 20, 128, 64, 1, 1, 0, 1, False, False, 18, 8, "f16"),
    (16, 40, 40, 128, 128, 1, 1, 0, 1, False, True, 19, 8, "f16"),
    (64, 20, 20, 128, 120, 1, 1, 0, 1, False, False, 20, 0, "f16"),
    (5, 4, 8, 128, 64, 1, 1, 0, 1, False, False, 21, 1, "f16"),
    (5, 8, 16, 128, 256, 1, 1, 0, 0, False, False, 56, 1, "f16"),  # P3 Detect head shape: split-epilogue pointwise kernel
    (3, 8, 16, 128, 248, 1, 1, 0, 1, False, False, 56, 2, "f16"),
    (16, 80, 80, 128, 256, 1, 1, 0, 0, False, False, 56, 0, "f16"),  # many tiles per wave on the full grid
    (16, 40, 40, 128, 128, 1, 1, 0, 1, False, True, 84, 8, "f16"),    # eight waves per workgroup
    (64, 40, 40, 64, 64, 1, 1, 0, 1, False, False, 85, 0, "f16"),
    (16, 20, 20, 128, 64, 1, 1, 0, 1, False, False, 86, 8, "f16"),
    (16, 80, 80, 128, 256, 1, 1, 0, 0, False, False, 87, 0, "f16"),
    # 256-row tiles with deep rings (cfg 35..39) at deep-layer shapes: many chunks per tile, several tiles per workgroup
    (8, 40, 40, 128, 128, 3, 1, 1, 1, True, False, 35, 16, "f16"),
    (8, 40, 40, 128, 128, 3, 1, 1, 1, False, False, 36, 0, "f16"),
    (8, 20, 20, 256, 256, 3, 1, 1, 1, True, False, 37, 8, "f16"),
    (16, 40, 40, 128, 256, 3, 2, 1, 1, False, False, 38, 0, "f16"),
    (8, 20, 20, 512, 512, 1, 1, 0, 1, False, False, 39, 8, "f16"),
    (8, 20, 20, 512, 256, 1, 1, 0, 1, False, True, 37, 0, "f16"),
    # producer / consumer variants (cfg 40..45): long rings, several tiles per workgroup, tails in M and N
    (8, 40, 40, 128, 128, 3, 1, 1, 1, True, False, 40, 16, "f16"),
    (8, 40, 40, 128, 120, 3, 1, 1, 1, False, False, 41, 0, "f16"),
    (8, 20, 20, 256, 256, 3, 1, 1, 1, True, False, 42, 8, "f16"),
    (16, 40, 40, 128, 256, 3, 2, 1, 1, False, False, 43, 0, "f16"),
    (8, 20, 20, 512, 512, 1, 1, 0, 1, False, False, 44, 8, "f16"),
    (8, 42, 38, 64, 64, 3, 1, 1, 1, True, True, 45, 0, "f16"),
    # high-occupancy variants with aliased epilogue scratch (cfg 46..49): several tiles per workgroup
    (8, 40, 40, 128, 128, 3, 1, 1, 1, True, False, 46, 16, "f16"),
    (8, 40, 40, 128, 120, 3, 1, 1, 1, False, False, 47, 0, "f16"),
    (16, 40, 40, 128, 256, 3, 2, 1, 1, False, False, 48, 24, "f16"),
    (8, 42, 38, 64, 64, 3, 1, 1, 1, True, True, 49, 8, "f16"),
    # streaming 3x3 kernel (conv_k3.h, cfg 30..34)
    (8, 40, 40, 32, 32, 3, 1, 1, 1, True, False, 30, 8, "f16"),
    (8, 40, 40, 32, 32, 3, 1, 1, 1, False, False, 33, 0, "f16"),
    (8, 80, 80, 32, 64, 3, 2, 1, 1, False, False, 31, 8, "f16"),
    (4, 80, 80, 32, 64, 3, 2, 1, 1, False, False, 34, 0, "f16"),
    (8, 40, 40, 64, 64, 3, 1, 1, 1, True, False, 32, 8, "f16"),
    (2, 20, 24, 64, 56, 3, 1, 1, 1, False, False, 32, 0, "f16"),
    (8, 80, 80, 64, 64, 3, 1, 1, 1, True, False, 78, 0, "f16"),     # filter fragments in registers
    (8, 40, 40, 64, 64, 3, 1, 1, 1, False, False, 79, 8, "f16"),
    (8, 80, 80, 64, 64, 3, 1, 1, 1, True, False, 80, 0, "f16"),     # eight waves per workgroup
    (8, 160, 160, 32, 64, 3, 2, 1, 1, False, False, 81, 0, "f16"),
    (8, 80, 80, 32, 32, 3, 1, 1, 1, True, False, 82, 8, "f16"),
    (8, 80, 80, 32, 32, 3, 1, 1, 1, False, False, 83, 0, "f16"),
    # halo-resident 3x3 kernel (conv_h3.h, cfg 61..70): several chunks per tile and several tiles per workgroup so that the counted-vmcnt
    # filter ring, the next-chunk halo prefetch and the cross-tile prologue all reach steady state on the real memory system
    (8, 80, 80, 64, 64, 3, 1, 1, 1, True, False, 62, 16, "f16"),
    (8, 40, 40, 128, 128, 3, 1, 1, 1, True, False, 61, 8, "f16"),
    (8, 40, 40, 128, 120, 3, 1, 1, 1, False, False, 63, 0, "f16"),
    (8, 20, 20, 256, 256, 3, 1, 1, 1, True, False, 64, 8, "f16"),
    (4, 42, 38, 96, 96, 3, 1, 1, 0, False, False, 65, 8, "f16"),
    (8, 80, 80, 64, 64, 3, 1, 1, 1, False, False, 66, 0, "f16"),
    (8, 40, 40, 128, 128, 3, 1, 1, 1, True, False, 67, 8, "f16"),
    (8, 40, 40, 128, 128, 3, 1, 1, 1, False, False, 68, 0, "f16"),
    (8, 20, 20, 256, 256, 3, 1, 1, 1, True, False, 69, 8, "f16"),
    (8, 80, 80, 64, 64, 3, 1, 1, 1, True, False, 70, 24, "f16"),
    (16, 23, 21, 160, 160, 3, 1, 1, 1, True, False, 67, 0, "f16"),
    (8, 40, 40, 128, 128, 3, 1, 1, 1, True, False, 71, 8, "f16"),
    (8, 40, 40, 128, 128, 3, 1, 1, 1, False, False, 72, 0, "f16"),
    (8, 20, 20, 256, 256, 3, 1, 1, 1, True, False, 70, 0, "f16"),
    (8, 40, 40, 128, 128, 3, 1, 1, 1, True, False, 73, 8, "f16"),
    (8, 40, 40, 128, 128, 3, 1, 1, 1, False, False, 73, 0, "f16"),
    (8, 80, 80, 64, 64, 3, 1, 1, 1, True, False, 74, 0, "f16"),
    (8, 20, 20, 256, 256, 3, 1, 1, 1, True, False, 75, 16, "f16"),
    (8, 40, 40, 128, 128, 3, 1, 1, 1, True, False, 76, 0, "f16"),
    (8, 80, 80, 64, 64, 3, 1, 1, 1, True, False, 77, 16, "f16"),
    # halo-resident 3x3 at STRIDE 2 (round 5: the down-sampling layers 3 / 5 / 7 / 18 / 21.Conv at their real shapes, small batch) and the small-tile ids 90..92
    (4, 160, 160, 64, 128, 3, 2, 1, 1, False, False, 90, 0, "f16"),
    (4, 160, 160, 64, 128, 3, 2, 1, 1, False, False, 91, 16, "f16"),
    (8, 80, 80, 128, 256, 3, 2, 1, 1, False, False, 76, 0, "f16"),
    (8, 40, 40, 256, 512, 3, 2, 1, 1, False, False, 92, 8, "f16"),
    (8, 80, 80, 128, 128, 3, 2, 1, 0, False, False, 73, 0, "f16"),
    (3, 41, 37, 64, 96, 3, 2, 1, 1, False, False, 64, 0, "f16"),
    # K-streamed pointwise kernel (conv_pwk.h, ids 93 / 94) at the P4 / P5 shapes of yolov5s and with tails
    (8, 40, 40, 256, 256, 1, 1, 0, 1, False, False, 93, 0, "f16"),
    (8, 20, 20, 1024, 512, 1, 1, 0, 1, False, False, 93, 0, "f16"),
    (8, 40, 40, 256, 128, 1, 1, 0, 1, False, False, 94, 0, "f16"),
    (3, 21, 19, 96, 248, 1, 1, 0, 0, False, False, 93, 0, "f16"),
    (2, 20, 20, 512, 320, 1, 1, 0, 1, False, False, 94, 0, "f16"),
    # 256-row / 8-phase implicit GEMM (conv_g8.h, id 95) at the MFMA-bound shapes of yolov5s (5 / 7 / 21.Conv, SPPF.cv2, Bottleneck.cv2 with residual) at a
    # smaller batch: long K rings across many tiles per workgroup, one tile per workgroup, odd K-tile counts, tails in M and N, a yolov5x channel count
    (8, 80, 80, 128, 256, 3, 2, 1, 1, False, False, 95, 0, "f16"),
    (16, 40, 40, 256, 512, 3, 2, 1, 1, False, False, 95, 0, "f16"),
    (16, 40, 40, 256, 256, 3, 2, 1, 1, False, False, 95, 16, "f16"),
    (16, 20, 20, 1024, 512, 1, 1, 0, 1, False, False, 95, 0, "f16"),
    (16, 20, 20, 256, 256, 3, 1, 1, 1, True, False, 95, 8, "f16"),
    (3, 41, 37, 192, 328, 3, 1, 1, 0, False, False, 95, 24, "f16"),
    (2, 40, 40, 320, 320, 3, 1, 1, 1, True, False, 95, 0, "f16"),
    (4, 40, 40, 64, 256, 1, 1, 0, 1, False, False, 95, 8, "f16"),
    # ... 256 x 128 tiles (id 96): 18 / 21.Conv, Bottleneck.cv2 at P4 / P5, yolov5x channel counts (320, 640: 2.5 and 5 N tiles), tails, short K
    (8, 80, 80, 128, 128, 3, 2, 1, 1, False, False, 96, 0, "f16"),
    (16, 40, 40, 256, 256, 3, 2, 1, 1, False, False, 96, 0, "f16"),
    (16, 20, 20, 256, 256, 3, 1, 1, 1, True, False, 96, 8, "f16"),
    (8, 40, 40, 128, 128, 3, 1, 1, 1, True, False, 96, 16, "f16"),
    (2, 40, 40, 320, 320, 3, 1, 1, 1, True, False, 96, 0, "f16"),
    (2, 20, 20, 640, 640, 3, 1, 1, 1, False, False, 96, 0, "f16"),
    (3, 41, 37, 192, 328, 3, 1, 1, 0, False, False, 96, 24, "f16"),
    (4, 40, 40, 64, 384, 1, 1, 0, 1, False, False, 96, 8, "f16"),
    (8, 20, 20, 128, 136, 1, 1, 0, 1, False, False, 96, 1, "f16"),
    # ... C1 % 64 != 0 (GEN loader: K tiles that span two taps): yolov5x's 80- / 160-channel layers (Bottleneck.cv2 at 320^2 / 160^2 with residual, 1.Conv / 3.Conv
    # at stride 2), yolov5m's 96 / 192, a 1x1 whose last K tile runs past the only tap, several tiles per workgroup, tails
    (2, 160, 160, 80, 80, 3, 1, 1, 1, True, False, 96, 0, "f16"),
    (2, 160, 160, 80, 80, 3, 1, 1, 1, True, False, 95, 0, "f16"),
    (2, 160, 160, 80, 160, 3, 2, 1, 1, False, False, 96, 0, "f16"),
    (4, 80, 80, 160, 160, 3, 1, 1, 1, True, False, 96, 0, "f16"),
    (4, 80, 80, 160, 320, 3, 2, 1, 1, False, False, 95, 0, "f16"),
    (3, 41, 37, 96, 200, 3, 1, 1, 0, False, False, 96, 24, "f16"),
    (3, 41, 37, 96, 200, 3, 1, 1, 0, False, False, 95, 24, "f16"),
    (4, 40, 40, 160, 320, 1, 1, 0, 1, False, False, 96, 8, "f16"),
    (4, 40, 40, 192, 96, 1, 1, 0, 1, False, False, 95, 0, "f16"),
]


@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_matches_torch_fp32_reference(case, dev):
    from yolov5_amd import _lib
    from yolov5_amd.packing import pack_conv_weight

    B, H, W, C1, C2, k, s, p, act, residual, up2, cfg, max_blocks, dt = case
    lib = _lib.lib()
    tdt = torch.float16 if dt == "f16" else torch.float32
    x = torch.from_numpy(detgen.uniform((B, C1, H, W), -1, 1, name="x"))
    w = torch.from_numpy(detgen.uniform((C2, C1, k, k), -1, 1, name="w")) * (2.0 / (C1 * k * k)) ** 0.5
    b = torch.from_numpy(detgen.uniform((C2,), -0.5, 0.5, name="b"))
    if dt == "f16":
        x, w = x.half().float(), w.half().float()
    ldx, ldy = C1 + 8, C2 + 8
    assert cfg is not None and max_blocks is not None
    xd = torch.full((B, H, W, ldx), 7.0, dtype=tdt, device=dev)
    xd[..., :C1] = x.permute(0, 2, 3, 1).to(dev, tdt)
    wp, bp, K, Kpad, Npad = pack_conv_weight(w, b, tdt)
    wp, bp = wp.to(dev), bp.to(dev)
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    y = torch.full((B, OH, OW, ldy), -3.0, dtype=tdt, device=dev)
    res = None
    if residual:
        y[..., :C2] = torch.from_numpy(detgen.uniform((B, OH, OW, C2), -1, 1, name="res")).to(dev, tdt)
        res = y.clone()
    y2 = torch.full((B, 2 * OH, 2 * OW, C2), -5.0, dtype=tdt, device=dev) if up2 else None
    d = _lib.ConvDesc(dtype=_lib.Y5_F16 if dt == "f16" else _lib.Y5_F32, B=B, H=H, W=W, C1=C1, ldx=ldx, OH=OH, OW=OW, C2=C2,
                      ldy=ldy, KH=k, KW=k, SH=s, SW=s, PH=p, PW=p, act=act, Kpad=Kpad, Npad=Npad, ldr=ldy, ld2=C2, cfg=cfg, max_blocks=max_blocks)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rc = lib.y5_conv2d_fwd(C.byref(d), C.c_void_p(xd.data_ptr()), C.c_void_p(wp.data_ptr()), C.c_void_p(bp.data_ptr()),
                           C.c_void_p(y.data_ptr()) if residual else None, C.c_void_p(y.data_ptr()),
                           C.c_void_p(y2.data_ptr()) if up2 else None, st)
    assert rc == 0, lib.y5_last_error()
    torch.cuda.synchronize()
    ref = F.conv2d(x, w, b, s, p)
    if act:
        ref = F.silu(ref)
    ref = ref.permute(0, 2, 3, 1)
    if residual:
        ref = ref + res[..., :C2].float().cpu()
    got = y[..., :C2].float().cpu()
    tol = 2e-2 if dt == "f16" else 2e-5
    torch.testing.assert_close(got, ref, rtol=tol, atol=tol)
    pad = y[..., C2:].float().cpu()
    assert torch.equal(pad, torch.full_like(pad, -3.0) if not residual else res[..., C2:].float().cpu())
    if up2:
        up = y[..., :C2].repeat_interleave(2, 1).repeat_interleave(2, 2)
        assert torch.equal(up, y2)


@pytest.mark.parametrize("B,H,W,c_up,c_hi,C2,cfg,max_blocks", [
    (16, 40, 40, 256, 256, 256, 88, 0),    # yolov5s 13.C3.cv1+cv2 (producer / consumer ring): many tiles per workgroup
    (8, 80, 80, 128, 128, 128, 88, 0),     # yolov5s 17.C3.cv1+cv2
    (8, 80, 80, 128, 128, 128, 89, 0),     # 2-stage BK64 tile
    (4, 38, 42, 64, 192, 96, 88, 16),      # odd tile counts, N tail, source switch after one chunk
    (4, 38, 42, 320, 64, 160, 89, 24),
    (16, 40, 40, 256, 256, 256, 95, 0),    # the 8-phase family's loader (ids 95 / 96) at the same layers
    (8, 80, 80, 128, 128, 128, 96, 0),
    (4, 38, 42, 64, 192, 96, 96, 16),
    (4, 38, 42, 320, 64, 328, 95, 24),
])
def test_conv_virtual_upsample_concat_matches_torch(B, H, W, c_up, c_hi, C2, cfg, max_blocks, dev):
    """Configurations 88 / 89 (conv_igemm.h UP2): the 1x1 convolution behind `nn.Upsample(2, 'nearest')` + `Concat` (models/yolov5s.yaml:36-38,41-43,
    common.py:443-453) reads input channels [0, c_up) from the LOW-resolution tensor; torch on the materialised concat is the reference.  The concat
    buffer's first c_up channels hold NaN: they must never be read."""
    from yolov5_amd import _lib
    from yolov5_amd.packing import pack_conv_weight

    lib = _lib.lib()
    lo = torch.from_numpy(detgen.uniform((B, c_up, H // 2, W // 2), -1, 1, name="lo")).half().float()
    hi = torch.from_numpy(detgen.uniform((B, c_hi, H, W), -1, 1, name="hi")).half().float()
    C1 = c_up + c_hi
    w = (torch.from_numpy(detgen.uniform((C2, C1, 1, 1), -1, 1, name="wu")) * (2.0 / C1) ** 0.5).half().float()
    b = torch.from_numpy(detgen.uniform((C2,), -0.5, 0.5, name="bu"))
    ld_lo, ldx, ldy = c_up + 16, C1 + 8, C2 + 8
    lo_d = torch.full((B, H // 2, W // 2, ld_lo), 9.0, dtype=torch.float16, device=dev)
    lo_d[..., :c_up] = lo.permute(0, 2, 3, 1).to(dev, torch.float16)
    xd = torch.full((B, H, W, ldx), 7.0, dtype=torch.float16, device=dev)
    xd[..., :c_up] = float("nan")
    xd[..., c_up:C1] = hi.permute(0, 2, 3, 1).to(dev, torch.float16)
    wp, bp, K, Kpad, Npad = pack_conv_weight(w, b, torch.float16)
    wp, bp = wp.to(dev), bp.to(dev)
    y = torch.full((B, H, W, ldy), -3.0, dtype=torch.float16, device=dev)
    d = _lib.ConvDesc(dtype=_lib.Y5_F16, B=B, H=H, W=W, C1=C1, ldx=ldx, OH=H, OW=W, C2=C2, ldy=ldy, KH=1, KW=1, SH=1, SW=1, PH=0, PW=0, act=1,
                      Kpad=Kpad, Npad=Npad, ldr=0, ld2=0, cfg=cfg, max_blocks=max_blocks, up_c=c_up, ld_up=ld_lo)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rc = lib.y5_conv2d_fwd(C.byref(d), C.c_void_p(xd.data_ptr()), C.c_void_p(wp.data_ptr()), C.c_void_p(bp.data_ptr()), C.c_void_p(lo_d.data_ptr()),
                           C.c_void_p(y.data_ptr()), None, st)
    assert rc == 0, lib.y5_last_error()
    torch.cuda.synchronize()
    cat = torch.cat((F.interpolate(lo, scale_factor=2, mode="nearest"), hi), 1)
    ref = F.silu(F.conv2d(cat, w, b)).permute(0, 2, 3, 1)
    torch.testing.assert_close(y[..., :C2].float().cpu(), ref, rtol=2e-2, atol=2e-2)
    pad = y[..., C2:].float().cpu()
    assert torch.equal(pad, torch.full_like(pad, -3.0))


@pytest.mark.parametrize("H,C1,C2,k,s,cfg", [(40, 128, 128, 3, 1, 76), (40, 256, 256, 1, 1, 43), (80, 64, 64, 3, 1, 80), (80, 128, 128, 1, 1, 84), (20, 512, 512, 1, 1, 39),
                                             (80, 128, 256, 3, 2, 43), (40, 128, 128, 3, 1, 40)])
def test_conv_unit_scale_and_saturating_activations(H, C1, C2, k, s, cfg, dev):
    """the full-resolution detection-set fixtures are conditioned to small pre-activations (SiLU almost linear).  The per-layer check at
    REALISTIC and LARGE magnitudes lives here: the configurations the yolov5s plan actually selects, pre-activation standard deviation ~1 and ~6
    (SiLU well into both of its asymptotes, fp16 outputs up to ~30), against torch fp32 on the same fp16-rounded operands -- error budget = one fp16
    rounding of the result (2^-10 relative) plus the fp32 accumulation-order noise."""
    from yolov5_amd import _lib
    from yolov5_amd.packing import pack_conv_weight

    lib = _lib.lib()
    B, p = 4, k // 2
    OH = (H + 2 * p - k) // s + 1
    for gain in (1.0, 6.0):
        x = torch.from_numpy(detgen.uniform((B, C1, H, H), -3 ** 0.5, 3 ** 0.5, name="xs", seed=int(gain))).half().float()   # unit variance
        w = (torch.from_numpy(detgen.uniform((C2, C1, k, k), -3 ** 0.5, 3 ** 0.5, name="ws", seed=cfg)) * gain / (C1 * k * k) ** 0.5).half().float()
        b = torch.from_numpy(detgen.uniform((C2,), -0.5, 0.5, name="bs"))
        xd = x.permute(0, 2, 3, 1).contiguous().to(dev, torch.float16)
        wp, bp, K, Kpad, Npad = pack_conv_weight(w, b, torch.float16)
        wp, bp = wp.to(dev), bp.to(dev)
        y = torch.zeros((B, OH, OH, C2), dtype=torch.float16, device=dev)
        d = _lib.ConvDesc(dtype=_lib.Y5_F16, B=B, H=H, W=H, C1=C1, ldx=C1, OH=OH, OW=OH, C2=C2, ldy=C2, KH=k, KW=k, SH=s, SW=s, PH=p, PW=p, act=1,
                          Kpad=Kpad, Npad=Npad, ldr=0, ld2=0, cfg=cfg, max_blocks=0)
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        rc = lib.y5_conv2d_fwd(C.byref(d), C.c_void_p(xd.data_ptr()), C.c_void_p(wp.data_ptr()), C.c_void_p(bp.data_ptr()), None, C.c_void_p(y.data_ptr()), None, st)
        assert rc == 0, lib.y5_last_error()
        torch.cuda.synchronize()
        pre = F.conv2d(x, w, b, s, p)
        ref = F.silu(pre).permute(0, 2, 3, 1)
        assert 0.6 * gain < float(pre.std()) < 1.6 * gain
        got = y.float().cpu()
        err = (got - ref).abs()
        tol = 2.0 ** -10 * ref.abs() + 2e-3 * gain   # one fp16 rounding + accumulation noise / the tanh-like knee of SiLU' <= 1.1
        assert bool((err <= tol).all()), (gain, float(err.max()), float((err / (ref.abs() + 1e-3)).max()))


# ---- whole model ------------------------------------------------------------------------------------------
def _det_model(name, seed):
    from yolov5_amd.yolo import DetectionModel, SegmentationModel

    M = SegmentationModel if "seg" in name else DetectionModel
    m = M(name + ".yaml")
    m.load_state_dict(yo.det_state_dict(yo.model_cfg(name), seed, fused=False))
    return m.eval()


@pytest.mark.parametrize("fused", [False, True])
def test_yolov5n_fp32_vs_reference_golden(fused, dev):
    g = np.load(os.path.join(G, "fwd_yolov5n_64.npz"))
    m = _det_model("yolov5n", 0)
    if fused:
        m.fuse()
    m = m.to(dev)
    x = torch.from_numpy(detgen.uniform((2, 3, 64, 64), 0.0, 1.0, name="img", seed=0)).to(dev)
    z, raw = m(x)
    np.testing.assert_allclose(z.cpu().numpy(), g["z_fused" if fused else "z_unfused"], rtol=1e-4, atol=1e-4)
    for i in range(3):
        assert raw[i].shape == g[f"raw{i}"].shape
        np.testing.assert_allclose(raw[i].cpu().numpy(), g[f"raw{i}"], rtol=1e-4, atol=2e-4)
    # Detect grid/anchor indexing bit-exact (yolo.py:117-128): xy of a zero-logit cell is (ix, iy)*stride exactly
    det = m.model[-1]
    for i, s in enumerate((8, 4, 2)):
        grid, ag = det._make_grid(s, s, i)
        assert np.array_equal(grid[0, 0].cpu().numpy(), g[f"grid{i}"])
        assert np.array_equal(ag[0, :, 0, 0].cpu().numpy(), g[f"anchor_grid{i}"])


def test_yolov5s_fp32_320_vs_reference_golden(dev):
    g = np.load(os.path.join(G, "fwd_yolov5s_320.npz"))
    m = _det_model("yolov5s", 1).fuse().to(dev)
    x = torch.from_numpy(detgen.uniform((2, 3, 320, 320), 0.0, 1.0, name="img", seed=1)).to(dev)
    z = m(x)[0].cpu().numpy()
    rs = int(g["row_stride"])
    np.testing.assert_allclose(z.reshape(-1, 85)[::rs], g["z_fused_rows"], rtol=1e-4, atol=5e-4)
    s = z.astype(np.float64)
    np.testing.assert_allclose([s.sum(), np.abs(s).sum(), (s * s).sum()], g["z_fused_sum"], rtol=1e-5)


def test_yolov5n_seg_fp32_vs_reference_golden(dev):
    g = np.load(os.path.join(G, "fwd_yolov5n-seg_64.npz"))
    m = _det_model("yolov5n-seg", 2).fuse().to(dev)
    x = torch.from_numpy(detgen.uniform((2, 3, 64, 64), 0.0, 1.0, name="img", seed=2)).to(dev)
    z, proto, raw = m(x)
    np.testing.assert_allclose(z.cpu().numpy(), g["z_fused"], rtol=1e-4, atol=2e-4)
    np.testing.assert_allclose(proto.cpu().numpy()[:, :, ::5, ::5], g["proto_sample"], rtol=1e-4, atol=1e-4)


def test_yolov5s_fp16_640_vs_oracle(dev):
    """BASELINE config C2 shape class (bs reduced to 2 so the CPU oracle finishes in seconds)."""
    cfg = yo.model_cfg("yolov5s")
    sd = yo.det_state_dict(cfg, 3, fused=True)
    m = _det_model("yolov5s", 3).fuse().half().to(dev)
    x = torch.from_numpy(detgen.uniform((2, 3, 640, 640), 0.0, 1.0, name="img", seed=3))
    with torch.no_grad():
        ref = yo.model_forward(cfg, sd, x.half().float())[0].numpy()
    z = m(x.half().to(dev))[0].float().cpu().numpy()
    assert z.shape == (2, 25200, 85)
    err_box = np.abs(z[..., :4] - ref[..., :4]).max()
    err_conf = np.abs(z[..., 4:] - ref[..., 4:]).max()
    # utils/general.py:410-435 `check_amp` accepts AMP when the post-NMS *normalised* xywhn rows agree to atol 0.1 (= 64 px at 640^2);
    # this bound is 64x tighter on the raw rows.  The envelope-based fp16 criteria (reference's own model.half() as yardstick,
    # detection-set agreement) at the BASELINE configurations are tests/test_gpu_configs.py.
    assert err_box < 1.0 and err_conf < 3e-2, (err_box, err_conf)
    assert np.abs(z[..., :4] - ref[..., :4]).mean() < 0.05


@pytest.mark.parametrize("shape", [(3, 3, 96, 160), (1, 3, 64, 224), (5, 3, 128, 192), (2, 3, 352, 608), (7, 3, 32, 32)])
def test_rectangular_and_odd_batches_fp16_and_fp32(shape, dev):
    """val.py / detect.py rectangular inference (sizes are multiples of the stride, not of 64; any batch size): every kernel
    family has to take its general fallback somewhere in these shapes (stem needs W % 64 == 0, k3 needs OW % 8 == 0, ...)."""
    cfg = yo.model_cfg("yolov5n")
    sd = yo.det_state_dict(cfg, 5, fused=True)
    x = torch.from_numpy(detgen.uniform(shape, 0.0, 1.0, name="rimg", seed=shape[2] + shape[3]))
    with torch.no_grad():
        ref32 = yo.model_forward(cfg, sd, x)[0].numpy()
        ref16 = yo.model_forward(cfg, sd, x.half().float())[0].numpy()
    m = _det_model("yolov5n", 5).fuse().to(dev)
    z32 = m(x.to(dev))[0].cpu().numpy()
    np.testing.assert_allclose(z32, ref32, rtol=1e-4, atol=2e-4)
    m = m.half()
    z16 = m(x.half().to(dev))[0].float().cpu().numpy()
    assert z16.shape == ref16.shape
    assert np.abs(z16[..., :4] - ref16[..., :4]).max() < 1.0 and np.abs(z16[..., 4:] - ref16[..., 4:]).max() < 3e-2


def test_uint8_input_scaling(dev):
    m = _det_model("yolov5n", 0).fuse().to(dev)
    img = (detgen.uniform((1, 3, 64, 64), 0, 255.99, name="u8img")).astype(np.uint8)
    a = m(torch.from_numpy(img).to(dev))[0].clone()
    b = m((torch.from_numpy(img).float() / 255).to(dev))[0]
    torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-5)


def test_forward_augment_on_gpu_vs_oracle(dev):
    """model(x, augment=True) (models/yolo.py:269-312: scales 1 / 0.83 / 0.67 + left-right flip, _descale_pred, _clip_augmented) on the MI355X:
    y5_scale_img + three plan runs + y5_tta_descale against oracle.forward_augment (pinned to the live reference on CPU); fp32 input tight,
    fp16 input inside the fp16 envelope of the plain forward."""
    m = _det_model("yolov5n", 0).to(dev).eval()
    cfg = yo.model_cfg("yolov5n")
    x = torch.from_numpy(detgen.uniform((2, 3, 96, 128), 0.0, 1.0, name="tta", seed=5))
    with torch.no_grad():
        zo = yo.forward_augment(cfg, yo.det_state_dict(cfg, 0, fused=False), x).numpy()
        z, none = m(x.to(dev), augment=True)
        z16 = m(x.half().to(dev), augment=True)[0]
    assert none is None and tuple(z.shape) == zo.shape
    np.testing.assert_allclose(z.float().cpu().numpy(), zo, rtol=1e-3, atol=2e-3)
    d = np.abs(z16.float().cpu().numpy() - zo)
    assert d[..., :4].max() < 1.0 and d[..., 4:].max() < 3e-2


def test_single_layer_forward_api(dev):
    from yolov5_amd.common import C3, SPPF, Conv

    torch.manual_seed(0)
    for layer, ref_fn in ((Conv(16, 32, 3, 2), None), (C3(32, 32, 2), None), (SPPF(32, 32, 5), None)):
        from yolov5_amd.yolo import initialize_weights

        initialize_weights(layer)  # BN eps=1e-3 as inside a DetectionModel (models/yolo.py:259)
        layer = layer.eval()
        x = torch.rand(2, layer.conv.in_channels if hasattr(layer, "conv") else layer.cv1.conv.in_channels, 16, 16)
        sd = {"model.0." + k: v for k, v in layer.state_dict().items()}
        kind = type(layer).__name__
        with torch.no_grad():
            if kind == "Conv":
                ref = yo._conv(sd, "model.0", x, 3, 2, 1)
            elif kind == "C3":
                ref = yo._c3(sd, "model.0", x, 2, True)
            else:
                ref = yo._sppf(sd, "model.0", x, 5)
        got = layer.to(dev)(x.to(dev)).cpu()
        torch.testing.assert_close(got, ref, rtol=1e-4, atol=1e-4)


# ---- NMS ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(NMS_CASES))
def test_nms_bit_exact_vs_reference_golden(name, dev):
    from yolov5_amd.general import non_max_suppression

    g = np.load(os.path.join(G, "nms.npz"))
    kw, nkw = NMS_CASES[name]
    res = non_max_suppression(torch.from_numpy(nms_case_pred(name)).to(dev), **nkw)
    for i, r in enumerate(res):
        ref = g[f"{name}_{i}"]
        assert tuple(r.shape) == ref.shape, (name, i, r.shape, ref.shape)
        assert np.array_equal(r.cpu().numpy(), ref), (name, i)


def test_nms_full_size_properties_and_oracle_subset(dev):
    """BASELINE size (64, 25200, 85): size-independent properties on every image + oracle equality on 3 images."""
    from yolov5_amd.general import non_max_suppression

    p = detgen.synth_predictions(64, 25200, 85, obj_pow=8, seed=31)
    for dt in (torch.float32, torch.float16):
        pd = torch.from_numpy(p).to(dev, dt)
        out = non_max_suppression(pd, 0.25, 0.45, max_det=1000)
        assert len(out) == 64
        pf = pd.float().cpu().numpy()
        for i in (0, 17, 63):
            ref = yo.non_max_suppression(pf[i:i + 1], 0.25, 0.45, max_det=1000)[0]
            assert np.array_equal(out[i].cpu().numpy(), ref), (dt, i)
        for o in out:
            o = o.cpu().numpy()
            assert o.shape[0] <= 1000 and o.shape[1] == 6
            assert np.all(np.diff(o[:, 4]) <= 0)  # descending confidence
            assert np.all(o[:, 4] > 0.25)
        # idempotence: feeding the kept boxes back (as obj=conf, one-hot cls) keeps all of them
        o = out[5].cpu().numpy()
        q = np.zeros((1, o.shape[0], 85), np.float32)
        q[0, :, 0] = (o[:, 0] + o[:, 2]) / 2; q[0, :, 1] = (o[:, 1] + o[:, 3]) / 2
        q[0, :, 2] = o[:, 2] - o[:, 0]; q[0, :, 3] = o[:, 3] - o[:, 1]
        q[0, :, 4] = 1.0
        q[0, np.arange(o.shape[0]), 5 + o[:, 5].astype(int)] = o[:, 4]
        again = non_max_suppression(torch.from_numpy(q).to(dev), 0.25, 0.45, max_det=1000)[0]
        assert again.shape[0] >= o.shape[0] - 2  # re-derived xyxy may move a box by 1 ulp


def test_nms_val_settings_large_candidate_sets(dev):
    from yolov5_amd.general import non_max_suppression

    p = detgen.synth_predictions(2, 25200, 85, obj_pow=2, seed=33)
    out = non_max_suppression(torch.from_numpy(p).to(dev), 0.001, 0.6, multi_label=False, max_det=300)
    ref = yo.non_max_suppression(p, 0.001, 0.6, multi_label=False, max_det=300)
    for o, r in zip(out, ref):
        assert np.array_equal(o.cpu().numpy(), r)
    p2 = detgen.synth_predictions(1, 6000, 25, obj_pow=1, seed=34)
    out = non_max_suppression(torch.from_numpy(p2).to(dev), 0.001, 0.6, multi_label=True, max_det=300)
    ref = yo.non_max_suppression(p2, 0.001, 0.6, multi_label=True, max_det=300)
    assert np.array_equal(out[0].cpu().numpy(), ref[0])


def test_autoshape_pipeline(dev):
    from yolov5_amd.common import AutoShape

    m = _det_model("yolov5n", 0).fuse().to(dev)
    a = AutoShape(m)
    a.conf = 0.001
    im = (detgen.uniform((96, 128, 3), 0, 255.99, name="autoshape")).astype(np.uint8)
    r = a([im, im[:, ::-1].copy()], size=64)
    assert len(r) == 2 and r.xyxy[0].shape[1] == 6
    assert float(r.xyxy[0][:, [0, 2]].max()) <= 128 and float(r.xyxy[0][:, [1, 3]].max()) <= 96


def test_split_engine_matches_single_plan(dev):
    """engine.SplitEngine (two sub-batch plans on two streams, opt-in Y5_EXPERIMENTAL=split2): same function of the input as one plan."""
    from yolov5_amd.engine import Engine, SplitEngine

    m = _det_model("yolov5n", 2).fuse().half().to(dev)
    x = torch.from_numpy(detgen.uniform((32, 3, 128, 192), 0.0, 1.0, name="simg", seed=4)).half().to(dev)
    with torch.no_grad():
        one = Engine(m, tuple(x.shape), torch.float16, dev, want_raw=True)
        two = SplitEngine(m, tuple(x.shape), torch.float16, dev, want_raw=True, parts=2)
        a = {k: v.float().clone() for k, v in one(x).items()}
        b = {k: v.float().clone() for k, v in two(x).items()}
        b2 = {k: v.float().clone() for k, v in two(x).items()}   # replay (hipGraph of each sub-plan)
    torch.cuda.synchronize()
    assert set(a) == set(b)
    for k in a:
        assert a[k].shape == b[k].shape
        assert torch.equal(b[k], b2[k])
        # tile configurations differ between the batch-32 plan and the batch-16 sub-plans: fp16 accumulation-order noise only
        torch.testing.assert_close(b[k], a[k], rtol=2e-2, atol=2e-2 if k != "z" else 0.5)


# ---- 3x3 s2 Conv + the pointwise convolution behind it as one launch (conv_k3.h PW2) ------------------------------------------------
@pytest.mark.parametrize("B,H,W,c3,split,mb", [(8, 160, 160, 64, 32, 0), (4, 96, 64, 48, 48, 4), (16, 64, 128, 64, 16, 0), (8, 160, 160, 64, 32, 81 << 16)])
def test_conv_k3pw_matches_torch(B, H, W, c3, split, mb, dev):
    """y5_conv_k3pw_fwd (models/yolo.py walking 1.Conv -> 2.C3.cv1+cv2) on the real memory system: many tiles per wave, so the counted-vmcnt ring
    with the second epilogue's stores reaches steady state; reference = torch fp32 on the same fp16 data with the intermediate rounded to fp16."""
    from yolov5_amd import _lib
    from yolov5_amd.packing import pack_conv_weight

    lib = _lib.lib()
    g = torch.Generator().manual_seed(B + H)
    w1 = torch.randn((64, 32, 3, 3), generator=g) * (2.0 / 288) ** 0.5
    b1 = torch.randn(64, generator=g) * 0.3
    w2 = torch.randn((c3, 64, 1, 1), generator=g) * (2.0 / 64) ** 0.5
    b2 = torch.randn(c3, generator=g) * 0.3
    x = torch.randn((B, H, W, 32), generator=g).half()
    w1p, b1p, _, K1, N1 = pack_conv_weight(w1, b1, torch.float16)
    w2p, b2p, _, K2, N2 = pack_conv_weight(w2, b2, torch.float16)
    xd, w1d, b1d, w2d, b2d = (t.to(dev) for t in (x, w1p, b1p, w2p, b2p))
    OH, OW = H // 2, W // 2
    ldy, ld2 = split + 8, (c3 - split) + 8
    y = torch.full((B, OH, OW, ldy), 7.0, dtype=torch.float16, device=dev)
    y2 = torch.full((B, OH, OW, ld2), 7.0, dtype=torch.float16, device=dev) if split < c3 else None
    d = _lib.ConvDesc(dtype=_lib.Y5_F16, B=B, H=H, W=W, C1=32, ldx=32, OH=OH, OW=OW, C2=64, ldy=64, KH=3, KW=3, SH=2, SW=2, PH=1, PW=1, act=1,
                      Kpad=K1, Npad=N1, ldr=0, ld2=0, cfg=(mb >> 16) or -1, max_blocks=mb & 0xffff)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rc = lib.y5_conv_k3pw_fwd(C.byref(d), C.c_void_p(xd.data_ptr()), C.c_void_p(w1d.data_ptr()), C.c_void_p(b1d.data_ptr()), C.c_void_p(w2d.data_ptr()),
                              C.c_void_p(b2d.data_ptr()), c3, N2, K2, 1, C.c_void_p(y.data_ptr()), ldy, C.c_void_p(y2.data_ptr()) if y2 is not None else None,
                              ld2, split, st)
    assert rc == 0, lib.y5_last_error()
    torch.cuda.synchronize()
    t = F.silu(F.conv2d(x.float().permute(0, 3, 1, 2), w1.half().float(), b1, stride=2, padding=1)).half().float()
    ref = F.silu(F.conv2d(t, w2.half().float(), b2)).permute(0, 2, 3, 1)
    torch.testing.assert_close(y[..., :split].float().cpu(), ref[..., :split], rtol=5e-3, atol=5e-3)
    assert bool((y[..., split:] == 7).all())
    if y2 is not None:
        torch.testing.assert_close(y2[..., :c3 - split].float().cpu(), ref[..., split:], rtol=5e-3, atol=5e-3)
        assert bool((y2[..., c3 - split:] == 7).all())


def test_plan_k3pw_fused_equals_unfused_on_gpu(dev, monkeypatch):
    """yolov5s 2 x 3 x 320 x 320 fp16: the plan with 1.Conv + 2.C3.cv1+cv2 as one launch against the plan with two launches (same fp16 intermediate,
    LDS instead of HBM)."""
    from yolov5_amd.yolo import DetectionModel

    cfg = yo.model_cfg("yolov5s")
    sd = yo.det_state_dict(cfg, 0, fused=False)
    x = torch.from_numpy(detgen.uniform((2, 3, 320, 320), 0.0, 1.0, name="img", seed=0)).half().to(dev)
    outs = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("Y5_FUSED_K3PW", mode)
        m = DetectionModel("yolov5s.yaml")
        m.load_state_dict(sd)
        m = m.eval().fuse().half().to(dev)
        outs[mode] = m(x)[0].float().cpu()
        eng = next(iter(m._engines.values()))
        assert any(n.startswith("conv+pw:") for n in eng.op_names) == (mode == "1"), eng.op_names
    u, v = outs["0"], outs["1"]
    assert float((u - v).abs().max()) <= 4e-3 * max(1.0, float(u.abs().max()))


def test_plan_front_fused_equals_unfused_on_gpu(dev, monkeypatch):
    """yolov5s 2 x 3 x 320 x 320 fp16: the plan with 0.Conv + 1.Conv + 2.C3.cv1+cv2 as ONE launch (Y5_FUSED_FRONT=1: taken whenever the library accepts the
    shape, not only when the timing race at plan build picks it) against the plan with the stem and conv+pw launches (same fp16 intermediates, LDS and
    registers instead of HBM)."""
    from yolov5_amd.yolo import DetectionModel

    cfg = yo.model_cfg("yolov5s")
    sd = yo.det_state_dict(cfg, 0, fused=False)
    x = torch.from_numpy(detgen.uniform((2, 3, 320, 320), 0.0, 1.0, name="img", seed=0)).half().to(dev)
    monkeypatch.setenv("Y5_FUSED_K3PW", "1")
    outs = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("Y5_FUSED_FRONT", mode)
        m = DetectionModel("yolov5s.yaml")
        m.load_state_dict(sd)
        m = m.eval().fuse().half().to(dev)
        outs[mode] = m(x)[0].float().cpu()
        eng = next(iter(m._engines.values()))
        assert any(n.startswith("front:") for n in eng.op_names) == (mode == "1"), eng.op_names
    u, v = outs["0"], outs["1"]
    assert float((u - v).abs().max()) <= 4e-3 * max(1.0, float(u.abs().max()))


def test_nms_objectness_hint_from_the_engine(dev):
    """The engine writes an objectness plane beside z (y5_plan_set_obj_hint) and hangs it on the tensor; non_max_suppression(z) then filters through
    the plane.  Same detections, bit for bit, as on a copy of z (no plane: the filter reads the rows), for the conv + decode levels and the fused P3 head;
    an in-place edit of z drops the plane."""
    import bench
    from yolov5_amd.general import non_max_suppression

    model = bench.build_model("yolov5s", dev)
    model.model[-1].export = True
    x = torch.rand((4, 3, 640, 640), generator=torch.Generator().manual_seed(3)).half().to(dev)
    bench.calibrate_head(model, x)
    z = model(x)[0]
    tag = getattr(z, "_y5_obj_hint", None)
    assert tag is not None and tuple(tag[0].shape) == tuple(z.shape[:2])
    assert torch.equal(tag[0], z[..., 4])                       # the plane is z's objectness, bit for bit
    a = non_max_suppression(z, 0.25, 0.45, max_det=1000)        # through the plane
    b = non_max_suppression(z.clone(), 0.25, 0.45, max_det=1000)
    assert sum(len(t) for t in a) > 100
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    c = non_max_suppression(z, 0.001, 0.6, max_det=300, multi_label=True)   # val.py settings: nearly every row passes the plane
    d = non_max_suppression(z.clone(), 0.001, 0.6, max_det=300, multi_label=True)
    for u, v in zip(c, d):
        assert torch.equal(u, v)
    # a LATER forward re-uses the engine's plane: the earlier tensor's tag no longer names the latest forward and its NMS must not look at the plane
    x2 = torch.rand((4, 3, 640, 640), generator=torch.Generator().manual_seed(4)).half().to(dev)
    z2 = model(x2)[0]
    z3 = model(x2)[0]                                            # (two planes, used alternately: the second later forward lands in z's plane)
    live = lambda t: t._y5_obj_hint[3][t._y5_obj_hint[4]] == t._y5_obj_hint[5]
    assert not live(z) and live(z2) and live(z3) and z._y5_obj_hint[0].data_ptr() == z3._y5_obj_hint[0].data_ptr() != z2._y5_obj_hint[0].data_ptr()
    g = non_max_suppression(z, 0.25, 0.45, max_det=1000)
    for u, v in zip(g, b):
        assert torch.equal(u, v)
    h2 = non_max_suppression(z2, 0.25, 0.45, max_det=1000)
    for u, v in zip(h2, non_max_suppression(z2.clone(), 0.25, 0.45, max_det=1000)):
        assert torch.equal(u, v)
    z[0, 0, 4] = 0.0                                             # in-place edit: version counter moves, the plane is ignored from here on
    e = non_max_suppression(z, 0.25, 0.45, max_det=1000)
    f = non_max_suppression(z.clone(), 0.25, 0.45, max_det=1000)
    for u, v in zip(e, f):
        assert torch.equal(u, v)


def test_forward_and_nms_under_inference_mode_on_gpu(dev):
    """the reference's entry points run under torch.inference_mode (utils/torch_utils.py:34-43).  Engine outputs stay ordinary tensors
    (hint tag alive), a caller's inference-tensor copy takes the plain filter; identical detections."""
    import bench
    from yolov5_amd.general import non_max_suppression

    model = bench.build_model("yolov5s", dev)
    model.model[-1].export = True
    x = torch.rand((2, 3, 640, 640), generator=torch.Generator().manual_seed(5)).half().to(dev)
    bench.calibrate_head(model, x)
    with torch.no_grad():
        ref = non_max_suppression(model(x)[0].clone(), 0.25, 0.45, max_det=1000)
    with torch.inference_mode():
        z = model(x)[0]
        assert not z.is_inference() and getattr(z, "_y5_obj_hint", None) is not None
        a = non_max_suppression(z, 0.25, 0.45, max_det=1000)
        zc = z.clone()
        assert zc.is_inference()
        b = non_max_suppression(zc, 0.25, 0.45, max_det=1000)
    assert sum(len(t) for t in ref) > 20
    for u, v, w in zip(ref, a, b):
        assert torch.equal(u, v) and torch.equal(u, w)


def test_plan_bneck_cv3_fused_equals_unfused_on_gpu(dev, monkeypatch):
    """yolov5s 4 x 3 x 320 x 320 fp16: 2.C3's Bottleneck + cv3 as one launch (y5_bottleneck_cv3_fwd, many tiles per wave on the real memory system) against
    the two-launch plan -- same fp16 intermediate (LDS instead of HBM), same k order in the third GEMM."""
    from yolov5_amd.yolo import DetectionModel

    cfg = yo.model_cfg("yolov5s")
    sd = yo.det_state_dict(cfg, 0, fused=False)
    x = torch.from_numpy(detgen.uniform((4, 3, 320, 320), 0.0, 1.0, name="img", seed=1)).half().to(dev)
    outs = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("Y5_FUSED_CV3", mode)
        m = DetectionModel("yolov5s.yaml")
        m.load_state_dict(sd)
        m = m.eval().fuse().half().to(dev)
        outs[mode] = m(x)[0].float().cpu()
        eng = next(iter(m._engines.values()))
        assert any(n.startswith("bneck+cv3:") for n in eng.op_names) == (mode == "1"), eng.op_names
    u, v = outs["0"], outs["1"]
    assert float((u - v).abs().max()) <= 4e-3 * max(1.0, float(u.abs().max()))


@pytest.mark.parametrize("B,H,W,add,ldx,ldy,mb", [(8, 40, 40, True, 256, 128, 0), (8, 40, 40, False, 128, 256, 5 << 16), (3, 23, 37, True, 128, 128, 8),
                                                  (64, 40, 40, True, 256, 256, 0), (2, 80, 80, True, 128, 128, 16 | (5 << 16))])
def test_fused_bottleneck_c128_matches_torch(B, H, W, add, ldx, ldy, mb, dev):
    """y5_bottleneck_fwd at C = 128 (csrc/conv_h3b.h: GEMM-1 phase + halo-resident 3x3 + residual, models/common.py:164-181) through the C-ABI against
    torch fp32 on the same fp16 operands (t rounded to fp16 as the two-launch form stores it); bs = 64 at 40 x 40 is the benchmarked shape
    (two tiles per workgroup: next-tile halo prefetch into dead planes), mb caps the grid so that workgroups walk many tiles."""
    import ctypes as C

    import torch.nn.functional as F

    from yolov5_amd import _lib
    from yolov5_amd.packing import pack_conv_weight

    lib = _lib.lib()
    Cc = 128
    g = torch.Generator().manual_seed(B * 100 + H)
    w1 = torch.randn((Cc, Cc, 1, 1), generator=g) * (2.0 / Cc) ** 0.5
    w2 = torch.randn((Cc, Cc, 3, 3), generator=g) * (2.0 / (9 * Cc)) ** 0.5
    b1, b2 = torch.randn(Cc, generator=g) * 0.3, torch.randn(Cc, generator=g) * 0.3
    w1p, b1p, _, K1, _ = pack_conv_weight(w1, b1, torch.float16)
    w2p, b2p, _, K2, _ = pack_conv_weight(w2, b2, torch.float16)
    w1p, b1p, w2p, b2p = (t.to(dev) for t in (w1p, b1p, w2p, b2p))
    xbuf = torch.randn((B, H, W, ldx), generator=g).half().to(dev)
    ybuf = torch.full((B, H, W, ldy), 7.0, dtype=torch.float16, device=dev)
    st = _lib.stream(dev)
    vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    rc = lib.y5_bottleneck_fwd(vp(xbuf, (ldx - Cc) * 2), ldx, vp(w1p), vp(b1p), K1, vp(w2p), vp(b2p), K2, vp(ybuf), ldy, B, H, W, Cc, int(add), mb, st)
    _lib.check(rc, lib)
    torch.cuda.synchronize()
    xf = xbuf[..., ldx - Cc:].float().permute(0, 3, 1, 2)
    t = F.silu(F.conv2d(xf, w1.half().float().to(dev), b1.to(dev))).half().float()
    ref = F.silu(F.conv2d(t, w2.half().float().to(dev), b2.to(dev), padding=1)).half().float()
    if add:
        ref = (ref + xf).half().float()
    ref = ref.permute(0, 2, 3, 1)
    got = ybuf[..., :Cc].float()
    # torch's GPU conv is a second implementation, not the truth: spot-check a slab against torch-CPU fp32 as well
    cpu = F.silu(F.conv2d(F.silu(F.conv2d(xf[:1].cpu(), w1.half().float(), b1)).half().float(), w2.half().float(), b2, padding=1)).half().float()
    if add:
        cpu = (cpu + xf[:1].cpu()).half().float()
    assert float((got[:1].cpu() - cpu.permute(0, 2, 3, 1)).abs().max()) <= 8e-3
    assert float((got - ref).abs().max()) <= 8e-3, float((got - ref).abs().max())
    assert bool((ybuf[..., Cc:] == 7).all())


def test_plan_bneck128_fused_equals_unfused_on_gpu(dev, monkeypatch):
    """yolov5s 8 x 3 x 640 x 640 fp16: the 128-channel Bottlenecks of 6 / 13 / 20.C3 as conv_h3b.h launches against the two-launch plan."""
    from yolov5_amd.yolo import DetectionModel

    cfg = yo.model_cfg("yolov5s")
    sd = yo.det_state_dict(cfg, 0, fused=False)
    x = torch.from_numpy(detgen.uniform((8, 3, 640, 640), 0.0, 1.0, name="img", seed=1)).half().to(dev)
    outs = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("Y5_FUSED_BNECK128", "force" if mode == "1" else mode)   # (force: below the planner's workgroup-count gate at this batch)
        m = DetectionModel("yolov5s.yaml")
        m.load_state_dict(sd)
        m = m.eval().fuse().half().to(dev)
        outs[mode] = m(x)[0].float().cpu()
        eng = next(iter(m._engines.values()))
        assert sum(n.startswith("bneck128") for n in eng.op_names) == (5 if mode == "1" else 0), eng.op_names   # ("bneck128+cv3:" = the C3-tail form)
    u, v = outs["0"], outs["1"]
    assert float((u - v).abs().max()) <= 4e-3 * max(1.0, float(u.abs().max()))


@pytest.mark.parametrize("B,H,W,add,c3,ldx,ld2,ldo,act3,mb", [(8, 40, 40, True, 256, 256, 256, 256, 1, 0), (64, 40, 40, True, 256, 256, 256, 256, 1, 0),
                                                             (3, 23, 37, False, 248, 128, 136, 264, 0, 8), (2, 80, 80, True, 128, 128, 128, 128, 1, 16)])
def test_fused_bottleneck_cv3_c128_matches_torch(B, H, W, add, c3, ldx, ld2, ldo, act3, mb, dev):
    """y5_bottleneck_cv3_fwd at C = 128 (csrc/conv_h3b.h CV3 form: the last Bottleneck of a C3 + the C3's cv3, models/common.py:232-246, in one launch; the
    Bottleneck's result goes to LDS as fp16 -- the rounding the two-launch form applies when it stores it) through the C-ABI against torch fp32 on the same
    fp16 operands; bs = 64 at 40 x 40 with 256 -> 256 is yolov5s' 6.C3 tail."""
    import ctypes as C

    import torch.nn.functional as F

    from yolov5_amd import _lib
    from yolov5_amd.packing import pack_conv_weight

    lib = _lib.lib()
    Cc = 128
    g = torch.Generator().manual_seed(B * 100 + H + c3)
    w1 = torch.randn((Cc, Cc, 1, 1), generator=g) * (2.0 / Cc) ** 0.5
    w2 = torch.randn((Cc, Cc, 3, 3), generator=g) * (2.0 / (9 * Cc)) ** 0.5
    w3 = torch.randn((c3, 2 * Cc, 1, 1), generator=g) * (2.0 / (2 * Cc)) ** 0.5
    b1, b2, b3 = torch.randn(Cc, generator=g) * 0.3, torch.randn(Cc, generator=g) * 0.3, torch.randn(c3, generator=g) * 0.3
    w1p, b1p, _, K1, _ = pack_conv_weight(w1, b1, torch.float16)
    w2p, b2p, _, K2, _ = pack_conv_weight(w2, b2, torch.float16)
    w3p, b3p, _, K3, _ = pack_conv_weight(w3, b3, torch.float16)
    w1p, b1p, w2p, b2p, w3p, b3p = (t.to(dev) for t in (w1p, b1p, w2p, b2p, w3p, b3p))
    xbuf = torch.randn((B, H, W, ldx), generator=g).half().to(dev)
    y2buf = torch.randn((B, H, W, ld2), generator=g).half().to(dev)
    obuf = torch.full((B, H, W, ldo), 7.0, dtype=torch.float16, device=dev)
    st = _lib.stream(dev)
    vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    rc = lib.y5_bottleneck_cv3_fwd(vp(xbuf, (ldx - Cc) * 2), ldx, vp(w1p), vp(b1p), K1, vp(w2p), vp(b2p), K2, vp(y2buf, (ld2 - Cc) * 2), ld2, vp(w3p), vp(b3p), K3,
                                   c3, act3, vp(obuf), ldo, B, H, W, Cc, int(add), mb, st)
    _lib.check(rc, lib)
    torch.cuda.synchronize()

    def ref_of(xf, y2f, d):
        t = F.silu(F.conv2d(xf, w1.half().float().to(d), b1.to(d))).half().float()
        m = F.silu(F.conv2d(t, w2.half().float().to(d), b2.to(d), padding=1)).half().float()
        if add:
            m = (m + xf).half().float()
        o = F.conv2d(torch.cat((m, y2f), 1), w3.half().float().to(d), b3.to(d))
        return (F.silu(o) if act3 else o).half().float().permute(0, 2, 3, 1)

    xf = xbuf[..., ldx - Cc:].float().permute(0, 3, 1, 2)
    y2f = y2buf[..., ld2 - Cc:].float().permute(0, 3, 1, 2)
    got = obuf[..., :c3].float()
    ref = ref_of(xf, y2f, dev)
    cpu = ref_of(xf[:1].cpu(), y2f[:1].cpu(), "cpu")  # torch's GPU conv is a second implementation, not the truth
    tol = 1.2e-2  # one fp16 ulp of the intermediate moves the 256-term sum by a few 1e-3
    assert float((got[:1].cpu() - cpu).abs().max()) <= tol
    assert float((got - ref).abs().max()) <= tol, float((got - ref).abs().max())
    assert bool((obuf[..., c3:] == 7).all())


def test_plan_bneck128_cv3_fused_equals_unfused_on_gpu(dev, monkeypatch):
    """yolov5s 8 x 3 x 640 x 640 fp16: the C3 tails of layers 6 / 13 / 20 (last Bottleneck + cv3) as one conv_h3b.h launch each (Y5_EXPERIMENTAL=cv3_128) against
    the plan that keeps cv3 its own launch."""
    from yolov5_amd.yolo import DetectionModel

    cfg = yo.model_cfg("yolov5s")
    sd = yo.det_state_dict(cfg, 0, fused=False)
    x = torch.from_numpy(detgen.uniform((8, 3, 640, 640), 0.0, 1.0, name="img", seed=1)).half().to(dev)
    outs = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("Y5_EXPERIMENTAL", "cv3_128" if mode == "1" else "")
        monkeypatch.setenv("Y5_FUSED_BNECK128", "force")   # (below the planner's workgroup-count gate at this batch)
        m = DetectionModel("yolov5s.yaml")
        m.load_state_dict(sd)
        m = m.eval().fuse().half().to(dev)
        outs[mode] = m(x)[0].float().cpu()
        eng = next(iter(m._engines.values()))
        assert sum(n.startswith("bneck128+cv3:") for n in eng.op_names) == (3 if mode == "1" else 0), eng.op_names
    u, v = outs["0"], outs["1"]
    assert float((u - v).abs().max()) <= 4e-3 * max(1.0, float(u.abs().max()))


@pytest.mark.parametrize("B,H,W,C1,c_,k", [(64, 20, 20, 512, 256, 5), (3, 13, 17, 96, 64, 5), (16, 20, 20, 1280, 640, 5), (2, 16, 16, 64, 128, 3)])
def test_sppf_cv1_pool_matches_torch(B, H, W, C1, c_, k, dev):
    """y5_sppf_cv1_pool_fwd (csrc/conv_sppf.h: SPPF.cv1 + the three cascaded max pools in one launch, models/common.py:318-340) through the C-ABI: slice 0
    against torch fp32 on the same fp16 operands, slices 1..3 EXACTLY torch's pools of slice 0; bs 64 x 20 x 20 x 512 -> 256 is yolov5s' 9.SPPF, 1280 -> 640
    yolov5x'."""
    import ctypes as C

    import torch.nn.functional as F

    from yolov5_amd import _lib
    from yolov5_amd.packing import pack_conv_weight

    lib = _lib.lib()
    g = torch.Generator().manual_seed(B + H + C1)
    w = torch.randn((c_, C1, 1, 1), generator=g) * (2.0 / C1) ** 0.5
    b = torch.randn(c_, generator=g) * 0.3
    wp, bp, _, Kpad, _ = pack_conv_weight(w, b, torch.float16)
    wp, bp = wp.to(dev), bp.to(dev)
    x = torch.randn((B, H, W, C1), generator=g).half().to(dev)
    buf = torch.full((B, H, W, 4 * c_ + 8), 7.0, dtype=torch.float16, device=dev)
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    _lib.check(lib.y5_sppf_cv1_pool_fwd(vp(x), C1, vp(wp), vp(bp), Kpad, vp(buf), 4 * c_ + 8, B, H, W, C1, c_, k, 1, _lib.stream(dev)), lib)
    torch.cuda.synchronize()
    xf = x[:2].float().cpu().permute(0, 3, 1, 2)
    ref0 = F.silu(F.conv2d(xf, w.half().float(), b)).half().float().permute(0, 2, 3, 1)
    got = buf[..., :4 * c_].float().cpu()
    assert float((got[:2, ..., :c_] - ref0).abs().max()) <= 8e-3
    cur = got[..., :c_].permute(0, 3, 1, 2)
    for s in range(1, 4):
        cur = F.max_pool2d(cur, k, 1, k // 2)
        assert torch.equal(got[..., s * c_:(s + 1) * c_], cur.permute(0, 2, 3, 1)), s
    assert bool((buf[..., 4 * c_:] == 7).all())


def test_plan_sppf_front_fused_equals_unfused_on_gpu(dev, monkeypatch):
    """yolov5s 8 x 3 x 640 x 640 fp16: 9.SPPF's cv1 + pools as one launch against cv1 + y5_sppf_pool."""
    from yolov5_amd.yolo import DetectionModel

    cfg = yo.model_cfg("yolov5s")
    sd = yo.det_state_dict(cfg, 0, fused=False)
    x = torch.from_numpy(detgen.uniform((8, 3, 640, 640), 0.0, 1.0, name="img", seed=1)).half().to(dev)
    outs = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("Y5_FUSED_SPPF", "force" if mode == "1" else mode)   # (force: below the planner's workgroup-count gate at this batch)
        m = DetectionModel("yolov5s.yaml")
        m.load_state_dict(sd)
        m = m.eval().fuse().half().to(dev)
        outs[mode] = m(x)[0].float().cpu()
        eng = next(iter(m._engines.values()))
        assert any(n.startswith("sppf_front:") for n in eng.op_names) == (mode == "1") and ("sppf_pool" in eng.op_names) == (mode == "0"), eng.op_names
    u, v = outs["0"], outs["1"]
    assert float((u - v).abs().max()) <= 4e-3 * max(1.0, float(u.abs().max()))


@pytest.mark.parametrize("cfg,B,H,C1,C2,k,s", [(95, 64, 40, 256, 512, 3, 2), (96, 64, 40, 256, 256, 3, 2), (95, 64, 40, 256, 256, 1, 1), (96, 64, 80, 128, 128, 3, 2)])
def test_8phase_kernels_are_repeatable_under_load(cfg, B, H, C1, C2, k, s, dev):
    """conv_g8.h hands LDS half-tiles between two wave rows that run one barrier apart; the restage-after-read distances are argued in its header, and a
    violation would show as RARE wrong tiles that depend on timing -- something neither a single parity run nor the host emulator (which runs the rows of a
    workgroup one after the other) can see.  Here the benchmarked shapes run 40 times each, alternating with a bandwidth-heavy copy on a second stream that
    perturbs the memory system's timing, and every output must be BIT-IDENTICAL to the first (the kernel has no atomics: any difference is a race)."""
    from yolov5_amd import _lib
    from yolov5_amd.packing import pack_conv_weight

    lib = _lib.lib()
    g = torch.Generator().manual_seed(cfg + C2)
    x = torch.randn((B, H, H, C1), generator=g).half().to(dev)
    w = torch.randn((C2, C1, k, k), generator=g) * (2.0 / (C1 * k * k)) ** 0.5
    wp, bp, K, Kpad, Npad = pack_conv_weight(w, torch.randn(C2, generator=g) * 0.2, torch.float16)
    wp, bp = wp.to(dev), bp.to(dev)
    p = k // 2
    OH = (H + 2 * p - k) // s + 1
    d = _lib.ConvDesc(dtype=_lib.Y5_F16, B=B, H=H, W=H, C1=C1, ldx=C1, OH=OH, OW=OH, C2=C2, ldy=C2, KH=k, KW=k, SH=s, SW=s, PH=p, PW=p, act=1,
                      Kpad=Kpad, Npad=Npad, ldr=0, ld2=0, cfg=cfg, max_blocks=0)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    side = torch.cuda.Stream(dev)
    junk_a = torch.empty(64 << 20, dtype=torch.uint8, device=dev)
    junk_b = torch.empty_like(junk_a)
    first = None
    for it in range(40):
        y = torch.full((B, OH, OH, C2), -3.0, dtype=torch.float16, device=dev)
        if it % 2:
            with torch.cuda.stream(side):
                junk_b.copy_(junk_a)
        rc = lib.y5_conv2d_fwd(C.byref(d), C.c_void_p(x.data_ptr()), C.c_void_p(wp.data_ptr()), C.c_void_p(bp.data_ptr()), None, C.c_void_p(y.data_ptr()), None, st)
        assert rc == 0, lib.y5_last_error()
        torch.cuda.synchronize()
        if first is None:
            first = y
            ref = F.silu(F.conv2d(x.permute(0, 3, 1, 2).float(), w.half().float().to(dev), bp[:C2], s, p)).permute(0, 2, 3, 1)
            torch.testing.assert_close(y.float(), ref, rtol=2e-2, atol=2e-2)
        else:
            assert torch.equal(y, first), f"run {it} differs from run 0 in {int((y != first).sum())} elements"
