"""CPU (emulator): every op kind of the C-side execution plan against the direct entry point it launches, bit for bit, with rebinding, the setters and
ranges checked on the same plans (tests/plan_ops_ref.py).  The plan code is host code: the host build runs the very same y5_plan_add_* / run / rebind /
set paths as the device library; tests/test_gpu_plan_ops.py adds the captured range."""
import pytest

from tests import plan_ops_ref as po
from tests import train_glue_ref as tg


@pytest.fixture(scope="module")
def be():
    return tg.EmuBackend()


@pytest.mark.parametrize("kind", po.KINDS)
def test_emu_plan_op_equals_direct_call(be, kind):
    po.run_parity(be, kind)


@pytest.mark.parametrize("kind", po.INPUT_KINDS)
def test_emu_plan_set_input(be, kind):
    po.run_set_input(be, kind)


@pytest.mark.parametrize("kind", po.ANCHOR_KINDS)
def test_emu_plan_set_anchors_and_obj_hint(be, kind):
    po.run_anchors_and_hint(be, kind)


def test_emu_plan_nop_ranges_and_side_branch(be):
    po.run_nop_and_ranges(be)
