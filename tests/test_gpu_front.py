"""GPU: the fused front (y5_conv_front_fwd) and the NCHW stem kernels (y5_conv_stem_fwd, y5_conv_stem_fwd_raw) called directly through the C-ABI on the
full tables of tests/front_ref.py.  The raw stem on integers bit for bit (A), the stem within its derived bound (B), the front against the float64 chain
(C); the output bits under every grid and batch position (D) and over 40 runs beside a bandwidth-heavy copy (E) -- the next tile's input patch lands by
LDS-DMA while phases 2 and 3 run, the wait at the top of a tile counts the previous tile's stores, the stem's rings are wave-private: none of which the
host build can show; the refusals and one probe on either side of each size guard (G)."""
import pytest
import torch

from tests import front_ref as fr
from tests import train_glue_ref as tg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    assert torch.cuda.is_available()
    return tg.GpuBackend(torch.device("cuda:0"))


# ---- A / B. the stem ----
@pytest.mark.parametrize("case", fr.STEM_CASES + [fr.STEM_BENCH], ids=str)
def test_gpu_stem_raw_is_exact(be, case):
    fr.run_stem_exact(be, case)


@pytest.mark.parametrize("case", fr.STEM_CASES, ids=str)
def test_gpu_stem_within_bound(be, case):
    fr.run_stem_parity(be, case)


def test_gpu_stem_image_like_data(be):
    fr.run_stem_parity(be, fr.STEM_CASES[1], "image")


def test_gpu_stem_within_bound_at_the_benchmark_geometry(be):
    fr.run_stem_parity(be, fr.STEM_BENCH)


def test_gpu_stem_is_repeatable_under_load(be):
    """E (shares the reference of the test above)."""
    fr.run_stem_repeat(be)


# ---- C. the front ----
@pytest.mark.parametrize("case", fr.FRONT_CASES, ids=str)
def test_gpu_front_matches_float64_chain(be, case):
    fr.run_front_parity(be, case)


def test_gpu_front_matches_float64_chain_at_the_benchmark_shape(be):
    fr.run_front_parity(be, fr.FRONT_BENCH)


def test_gpu_front_is_repeatable_under_load(be):
    """E (shares the reference of the test above)."""
    fr.run_front_repeat(be)


# ---- D. schedule and batch invariance ----
@pytest.mark.parametrize("raw", [False, True], ids=["act", "raw"])
def test_gpu_stem_bits_do_not_depend_on_the_grid(be, raw):
    fr.run_stem_schedule(be, fr.STEM_SCHED, raw, fr.MBS_GPU)


def test_gpu_front_bits_do_not_depend_on_the_grid(be):
    fr.run_front_schedule(be, fr.FRONT_SCHED, fr.MBS_GPU)


@pytest.mark.parametrize("raw", [False, True], ids=["act", "raw"])
def test_gpu_stem_bits_do_not_depend_on_the_batch_position(be, raw):
    fr.run_stem_batch(be, (5, 34, 192, 32), raw)


def test_gpu_front_bits_do_not_depend_on_the_batch_position(be):
    fr.run_front_batch(be, fr.fc(5, 128, 128))


# ---- G. refusals and the size guards ----
def test_gpu_front_refusals(be):
    fr.run_front_refusals(be)


def test_gpu_stem_refusals(be):
    fr.run_stem_refusals(be)


@pytest.mark.parametrize("over", [False, True], ids=["under", "over"])
def test_gpu_stem_input_around_2_30_elements(be, over):
    try:
        fr.run_stem_size_guard(be, over)
    finally:
        torch.cuda.empty_cache()


@pytest.mark.parametrize("over", [False, True], ids=["under", "over"])
def test_gpu_front_input_around_2_31_bytes(be, over):
    try:
        fr.run_front_size_guard(be, over)
    finally:
        torch.cuda.empty_cache()
