"""CPU (emulator): the fused Bottlenecks at 32 and 64 channels (y5_bottleneck_fwd, y5_bottleneck_cv3_fwd at C = 32) through the C-ABI on the rows of
tests/bneck_ref.py marked for the host build: against the float64 chain (C), the output bits under another grid, ring depth, wave count or batch
position (D), the library's own grid where an explicit cap of the same size is refused, and the refusals (G); then all of it again in a child process
under the worst-case LDS-DMA landing model.  The emulator runs the waves of a workgroup one after the other: what it holds to account is the addressing,
the borders, the swizzles, the tile schedule, the host rules and the COUNT of each wait; tests/test_gpu_bneck.py runs the full tables where the
wave-private rings and the counted waits really overlap in time."""
import os
import subprocess
import sys

import pytest

from tests import bneck_ref as br
from tests import train_glue_ref as tg


@pytest.fixture(scope="module")
def be():
    return tg.EmuBackend()


@pytest.mark.parametrize("case", br.BN_CASES_EMU, ids=str)
def test_emu_bneck_matches_float64_chain(be, case):
    br.run_bn_parity(be, case)


@pytest.mark.parametrize("case", br.CV3_CASES_EMU, ids=str)
def test_emu_bneck_cv3_matches_float64_chain(be, case):
    br.run_cv3_parity(be, case)


@pytest.mark.parametrize("kind", [32, 64, "cv3"], ids=str)
def test_emu_bneck_bits_do_not_depend_on_the_grid(be, kind):
    br.run_schedule(be, kind, br.MBS_EMU)


@pytest.mark.parametrize("kind", [32, 64, "cv3"], ids=str)
def test_emu_bneck_bits_do_not_depend_on_the_batch_position(be, kind):
    br.run_batch(be, kind)


def test_emu_bneck_own_grid_is_never_refused(be):
    br.run_own_grid(be)


def test_emu_bneck_refusals(be):
    br.run_bn_refusals(be)


def test_emu_bneck_cv3_refusals(be):
    br.run_cv3_refusals(be)


def test_emu_bneck_parity_under_worst_case_dma_landing():
    """This file again with Y5_EMU_ASYNC=1: an LDS-DMA load lands only when a vmcnt wait of its wave covers it, so a counted wait of any (S, LP, SP) form
    that is one operation too lenient reads a stale stage.  The switch is latched per process, hence the child (as tests/test_emu_async_files.py)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", os.path.basename(__file__)), "-q", "-x", "-o", "addopts=", "-p", "no:cacheprovider",
                        "-k", "not worst_case"], env=dict(os.environ, Y5_EMU_ASYNC="1"), capture_output=True, text=True, cwd=root)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
