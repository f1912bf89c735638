"""CPU (emulator): the fused front and the NCHW stem kernels through the C-ABI on the reduced tables of tests/front_ref.py -- at most four tiles of the
front and 64 wave tiles of the stem: the raw stem on integers bit for bit (A), the stem within its derived bound (B), the front against the float64
chain (C), the output bits under another grid or batch position (D), and the refusals (G).  The emulator runs the waves of a workgroup one after the
other: what it holds to account is the addressing, the borders, the tails and the tile schedule; tests/test_gpu_front.py runs the full tables where the
input prefetch, the counted waits and the wave-private rings really overlap."""
import pytest

from tests import front_ref as fr
from tests import train_glue_ref as tg


@pytest.fixture(scope="module")
def be():
    return tg.EmuBackend()


@pytest.mark.parametrize("case", fr.STEM_CASES_EMU, ids=str)
def test_emu_stem_raw_is_exact(be, case):
    fr.run_stem_exact(be, case)


@pytest.mark.parametrize("case", fr.STEM_CASES_EMU, ids=str)
def test_emu_stem_within_bound(be, case):
    fr.run_stem_parity(be, case)


def test_emu_stem_image_like_data(be):
    fr.run_stem_parity(be, fr.STEM_CASES_EMU[1], "image")


@pytest.mark.parametrize("case", fr.FRONT_CASES_EMU, ids=str)
def test_emu_front_matches_float64_chain(be, case):
    fr.run_front_parity(be, case)


@pytest.mark.parametrize("raw", [False, True], ids=["act", "raw"])
def test_emu_stem_bits_do_not_depend_on_the_grid(be, raw):
    fr.run_stem_schedule(be, fr.STEM_SCHED_EMU, raw, fr.MBS_EMU)


def test_emu_front_bits_do_not_depend_on_the_grid(be):
    fr.run_front_schedule(be, fr.FRONT_SCHED_EMU, fr.MBS_EMU)


@pytest.mark.parametrize("raw", [False, True], ids=["act", "raw"])
def test_emu_stem_bits_do_not_depend_on_the_batch_position(be, raw):
    fr.run_stem_batch(be, (5, 4, 64, 32), raw)


def test_emu_front_bits_do_not_depend_on_the_batch_position(be):
    fr.run_front_batch(be, fr.fc(5, 64, 64, mb=2))


def test_emu_front_refusals(be):
    fr.run_front_refusals(be)


def test_emu_stem_refusals(be):
    fr.run_stem_refusals(be)
