"""GPU: the fused Bottlenecks at 32 and 64 channels (y5_bottleneck_fwd, y5_bottleneck_cv3_fwd at C = 32; csrc/conv_bneck.h) called directly through the
C-ABI on the full tables of tests/bneck_ref.py.  Every case against the float64 chain (C); the output bits under every grid, ring depth, wave count and
batch position (D) and over 40 runs beside a bandwidth-heavy copy (E) -- the receptive fields land by LDS-DMA in wave-private rings behind counted
waits, the eight-wave C = 64 form writes t over the stage it was read from: none of which the host build can show; the library's own grid under a CU
budget below eight slots, the refusals and one launch on either side of the size guard (G)."""
import pytest
import torch

from tests import bneck_ref as br
from tests import train_glue_ref as tg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    assert torch.cuda.is_available()
    return tg.GpuBackend(torch.device("cuda:0"))


# ---- C. the float64 chain ----
@pytest.mark.parametrize("case", br.BN_CASES, ids=str)
def test_gpu_bneck_matches_float64_chain(be, case):
    br.run_bn_parity(be, case)


@pytest.mark.parametrize("case", br.CV3_CASES, ids=str)
def test_gpu_bneck_cv3_matches_float64_chain(be, case):
    br.run_cv3_parity(be, case)


# ---- C / E. the benchmark's geometry (a case's E test shares the reference of the test above it) ----
def test_gpu_bneck32_matches_float64_chain_at_the_benchmark_geometry(be):
    br.run_bn_parity(be, br.BN_BENCH[0])


def test_gpu_bneck32_is_repeatable_under_load(be):
    br.run_repeat(be, br.bn_key(br.BN_BENCH[0]), f"bneck repeat {br.BN_BENCH[0]}")


def test_gpu_bneck64_matches_float64_chain_at_the_benchmark_geometry(be):
    br.run_bn_parity(be, br.BN_BENCH[1])


def test_gpu_bneck64_is_repeatable_under_load(be):
    br.run_repeat(be, br.bn_key(br.BN_BENCH[1]), f"bneck repeat {br.BN_BENCH[1]}")


def test_gpu_bneck64_four_waves_matches_float64_chain_at_the_benchmark_geometry(be):
    br.run_bn_parity(be, br.BN_BENCH[2])


def test_gpu_bneck_cv3_matches_float64_chain_at_the_benchmark_geometry(be):
    br.run_cv3_parity(be, br.CV3_BENCH)


def test_gpu_bneck_cv3_is_repeatable_under_load(be):
    br.run_repeat(be, br.cv3_key(br.CV3_BENCH), f"bneck+cv3 repeat {br.CV3_BENCH}")


# ---- D. schedule and batch invariance ----
@pytest.mark.parametrize("kind", [32, 64, "cv3"], ids=str)
def test_gpu_bneck_bits_do_not_depend_on_the_grid(be, kind):
    br.run_schedule(be, kind, br.MBS_GPU)


@pytest.mark.parametrize("kind", [32, 64, "cv3"], ids=str)
def test_gpu_bneck_bits_do_not_depend_on_the_batch_position(be, kind):
    br.run_batch(be, kind)


@pytest.mark.parametrize("case,budget", [(br.FIX_CASE, 4), ((32, 3, 12, 40, 1), 2)], ids=str)   # one workgroup per CU at C = 64, three at C = 32
def test_gpu_bneck_own_grid_under_a_cu_budget_is_never_refused(be, case, budget):
    br.run_own_grid(be, budget, case)


# ---- G. refusals and the size guard ----
def test_gpu_bneck_refusals(be):
    br.run_bn_refusals(be)


def test_gpu_bneck_cv3_refusals(be):
    br.run_cv3_refusals(be)


@pytest.mark.parametrize("over", [False, True], ids=["under", "over"])
def test_gpu_bneck_input_around_2_31_bytes(be, over):
    try:
        br.run_size_guard(be, over)
    finally:
        torch.cuda.empty_cache()
