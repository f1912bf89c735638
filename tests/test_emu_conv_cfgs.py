"""The tile every convolution configuration id reports through y5_conv_cfg_info -- (pixels, channels, K bytes per stage) -- pinned as literals: the tuner
(engine.autotune_conv) and the benchmark's op table read these, and an id routed to a neighbouring row of csrc/conv_cfgs.h still computes the right numbers.
Once on the host emulator (no GPU) and once on the real library; neither launches a kernel."""
import ctypes as C

import pytest

from yolov5_amd import _lib

# id: (bm, bn, k_bytes).  Quirks kept on purpose: the eight-wave streaming 3x3 ids 80..83 report 128 pixels, the streaming 3x3 family reports 9 * C1 * 2 bytes.
TILES = {
    0: (128, 32, 64), 1: (128, 64, 64), 2: (128, 128, 64), 3: (128, 256, 64),
    4: (256, 32, 64), 5: (256, 64, 64), 6: (128, 32, 128), 7: (128, 64, 128),
    8: (128, 128, 128), 9: (128, 256, 128), 10: (256, 64, 128), 11: (64, 128, 128),
    12: (256, 128, 128), 13: (256, 32, 128), 14: (128, 32, 64), 15: (128, 32, 128),
    16: (128, 64, 128), 17: (128, 64, 128), 18: (128, 64, 256), 19: (128, 128, 256),
    20: (128, 128, 256), 21: (128, 64, 256), 22: (128, 64, 64), 23: (128, 128, 64),
    24: (128, 256, 64), 25: (256, 64, 64), 26: (128, 64, 128), 27: (128, 128, 128),
    28: (64, 128, 128), 29: (256, 128, 128), 30: (128, 32, 576), 31: (128, 64, 576),
    32: (128, 64, 1152), 33: (128, 32, 576), 34: (128, 64, 576), 35: (256, 128, 64),
    36: (256, 128, 64), 37: (256, 256, 64), 38: (256, 256, 64), 39: (256, 256, 128),
    40: (256, 128, 128), 41: (256, 128, 64), 42: (128, 128, 128), 43: (128, 128, 64),
    44: (128, 256, 64), 45: (128, 64, 128), 46: (128, 128, 64), 47: (128, 64, 64),
    48: (128, 64, 128), 49: (64, 128, 128), 50: (128, 320, 64), 51: (128, 160, 128),
    52: (128, 192, 64), 53: (128, 96, 128), 54: (256, 320, 64), 55: (256, 192, 64),
    56: (128, 256, 256), 57: (128, 128, 128), 58: (256, 256, 128), 59: (256, 128, 128),
    60: (128, 256, 128), 61: (320, 128, 64), 62: (320, 64, 64), 63: (448, 128, 64),
    64: (256, 128, 64), 65: (448, 64, 64), 66: (256, 64, 64), 67: (320, 128, 64),
    68: (448, 128, 64), 69: (256, 128, 64), 70: (256, 128, 64), 71: (512, 128, 64),
    72: (512, 128, 64), 73: (256, 128, 64), 74: (256, 64, 64), 75: (192, 128, 64),
    76: (256, 128, 64), 77: (256, 64, 64), 78: (128, 64, 1152), 79: (128, 64, 1152),
    80: (128, 64, 1152), 81: (128, 64, 576), 82: (128, 32, 576), 83: (128, 32, 576),
    84: (256, 128, 256), 85: (256, 64, 128), 86: (256, 64, 256), 87: (256, 256, 256),
    88: (128, 128, 64), 89: (128, 128, 128), 90: (64, 128, 64), 91: (128, 128, 64),
    92: (128, 128, 64), 93: (256, 256, 64), 94: (256, 128, 64), 95: (256, 256, 128),
    96: (256, 128, 128),
}


def check_cfg_info(lib):
    assert lib.y5_conv_num_cfgs() == 97
    assert sorted(TILES) == list(range(97))
    for cfg, want in TILES.items():
        bm, bn, kb = C.c_int(-1), C.c_int(-1), C.c_int(-1)
        assert lib.y5_conv_cfg_info(cfg, C.byref(bm), C.byref(bn), C.byref(kb)) == _lib.Y5_OK, cfg
        assert (bm.value, bn.value, kb.value) == want, cfg
        assert lib.y5_conv_cfg_info(cfg, None, None, None) == _lib.Y5_OK, cfg   # every out-pointer is optional
    for bad in (-1, 97):
        bm = C.c_int(-1)
        assert lib.y5_conv_cfg_info(bad, C.byref(bm), None, None) == _lib.Y5_ERR_BAD_ARG, bad
        assert bm.value == -1


def test_conv_cfg_info_table_emulated():
    from tests.hipemu.emu import emu

    check_cfg_info(emu())


@pytest.mark.gpu
def test_conv_cfg_info_table_gpu():
    check_cfg_info(_lib.lib())
