"""GPU: every op kind of the C-side execution plan against the direct entry point it launches, bit for bit, with rebinding, the setters and ranges
checked on the same plans (tests/plan_ops_ref.py; the host twin is tests/test_emu_plan_ops.py), and what only the device shows: a two-op range with a
side branch captured as a graph and replayed, and y5_plan_set_conv_cfg refused once a graph exists."""
import pytest
import torch

from tests import plan_ops_ref as po
from tests import train_glue_ref as tg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    assert torch.cuda.is_available()
    return tg.GpuBackend(torch.device("cuda:0"))


@pytest.mark.parametrize("kind", po.KINDS)
def test_gpu_plan_op_equals_direct_call(be, kind):
    po.run_parity(be, kind)


@pytest.mark.parametrize("kind", po.INPUT_KINDS)
def test_gpu_plan_set_input(be, kind):
    po.run_set_input(be, kind)


@pytest.mark.parametrize("kind", po.ANCHOR_KINDS)
def test_gpu_plan_set_anchors_and_obj_hint(be, kind):
    po.run_anchors_and_hint(be, kind)


def test_gpu_plan_nop_ranges_and_side_branch(be):
    po.run_nop_and_ranges(be)


def test_gpu_plan_captured_range(be):
    po.run_capture(be)
