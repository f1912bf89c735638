"""CPU: the filter repack kernels (train_misc.hip) and the data-gradient launches (device-packed sub-filter -> placed y5_conv2d_fwd per parity class -> dx)
compiled for the host on the HIP emulator, on the small tables of tests/conv_grad_ref.py (tests/test_gpu_conv_grad.py runs the full tables on the device)."""
import pytest

from tests import conv_grad_ref as cg
from tests import train_glue_ref as tg
from tests.conv_grad_ref import F16, F32


@pytest.fixture(scope="module")
def be():
    return tg.EmuBackend()


# ---- A. filter repack ----
@pytest.mark.parametrize("sp", cg.single_specs(cg.model_specs("yolov5n", distinct=True) + list(cg.EXTRA_SPECS)), ids=str)
def test_emu_repack_single_filter(be, sp):
    """yolov5n's geometries here (the same code paths as yolov5s's, a quarter of the elements); the device file reads yolov5s."""
    cg.run_single(be, sp)


@pytest.mark.parametrize("slack", [0, 5 * cg.MT_CH + 1])
def test_emu_filter_jobs_table(be, slack):
    """The reduced table still holds more than 2048 chunks: the emulator runs the capped grid of 2048 workgroups, each of which wraps."""
    cg.run_jobs(be, cg.jobs_table(full=False), slack)


def test_emu_filter_jobs_one_workgroup_crosses_jobs(be):
    """Ten chunks over five jobs; with max_total = 1 the launcher's grid is five workgroups: workgroup 0 takes chunks 0 and 5 and so advances
    across three jobs in one step, workgroup 1 across four.  (max_total only sizes the grid.)"""
    specs = cg.WALKER_SPECS
    assert [-(-cg.total_of(s) // cg.MT_CH) for s in specs] == [1, 1, 5, 1, 2]
    jobs = [cg.RepackJob(be, sp, ("walk", i)) for i, sp in enumerate(specs)]
    tg.ok(be, cg.launch_jobs(be, jobs, 1))
    for i, jb in enumerate(jobs):
        jb.check(f"walker job {i}")


@pytest.mark.parametrize("sp", [s for s in cg.EXTRA_SPECS if s[0] == 3 or s[10]], ids=str)
def test_emu_filter_job_alone(be, sp):
    """Kind 3 and the fp32 destination have no single-filter entry point: a table of one."""
    cg.run_jobs(be, [sp])


def test_emu_repack_refusals(be):
    cg.run_repack_refusals(be)


# ---- B. data-gradient launches ----
@pytest.mark.parametrize("cfg", range(cg.NUM_CFGS))
def test_emu_placed_launch_by_id(be, cfg):
    """Every id on the small odd-sized stride-2 case, without and with the residual: accepted exactly by the committed lists, refused with the family's
    message; an accepted id is verified once, accumulation alternating with the id."""
    cg.run_placed_id(be, cg.DG_SMALL, cfg, F16, check_acc=(cfg % 2,))


@pytest.mark.parametrize("cfg", range(cg.NUM_CFGS))
def test_emu_placed_launch_by_id_fp32(be, cfg):
    cg.run_placed_id(be, cg.DG_SMALL, cfg, F32, accs=(cfg % 2,))


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("case", cg.DG_EDGES, ids=lambda c: c[0])
def test_emu_dgrad_edges(be, case, acc):
    cg.run_dgrad(be, case, -1, acc)


@pytest.mark.parametrize("case", [cg.DG_SMALL, cg.DG_VIEW, cg.DG_DENSE[2]], ids=lambda c: c[0])
def test_emu_dgrad_fp32(be, case):
    for cfg, acc in ((0, 0), (1, 1), (2, 1), (3, 0)):
        cg.run_dgrad(be, case, cfg, acc, F32)


@pytest.mark.parametrize("cfg", [95, 96])
def test_emu_dgrad_dense_8phase(be, cfg):
    cg.run_dgrad(be, ("g8small", 1, 9, 8, 64, 64, 3, 1, 1, 0), cfg, 1)
