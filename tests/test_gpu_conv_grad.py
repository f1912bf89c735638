"""GPU: the filter repack kernels and the data-gradient launches, called directly through the C-ABI on the full tables of tests/conv_grad_ref.py:
every filter geometry of yolov5s bit for bit, one y5_filter_jobs table of a whole step's size and more, every configuration id that takes a placed
launch x {accumulate, not} against float64, and the probe of a placed destination image around 2^31 bytes."""
import pytest
import torch

from tests import conv_grad_ref as cg
from tests import train_glue_ref as tg
from tests.conv_grad_ref import F16, F32

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    assert torch.cuda.is_available()
    return tg.GpuBackend(torch.device("cuda:0"))


# ---- A. filter repack ----
def test_gpu_repack_single_filter(be):
    """Every distinct geometry of yolov5s, the extra cases and yolov5x's 3 x 3 through the three single-filter entry points."""
    specs = cg.single_specs(cg.model_specs("yolov5s", distinct=True) + list(cg.EXTRA_SPECS) + cg.BIG_SPECS)
    assert len(specs) > 100
    for sp in specs:
        cg.run_single(be, sp)


@pytest.mark.parametrize("slack", [0, 1 << 22])
def test_gpu_filter_jobs_table(be, slack):
    cg.run_jobs(be, cg.jobs_table(full=True), slack)


def test_gpu_filter_jobs_one_workgroup_crosses_jobs(be):
    jobs = [cg.RepackJob(be, sp, ("walk", i)) for i, sp in enumerate(cg.WALKER_SPECS)]
    tg.ok(be, cg.launch_jobs(be, jobs, 1))
    for i, jb in enumerate(jobs):
        jb.check(f"walker job {i}")


def test_gpu_repack_refusals(be):
    cg.run_repack_refusals(be)


# ---- B. data-gradient launches ----
@pytest.mark.parametrize("dtype", [F16, F32], ids=["f16", "f32"])
def test_gpu_placed_ids_are_the_committed_lists(be, dtype):
    for cfg in range(cg.NUM_CFGS):
        cg.run_placed_id(be, cg.DG_SMALL, cfg, dtype)


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("case", cg.DG_MATRIX, ids=lambda c: c[0])
def test_gpu_placed_matrix(be, case, acc):
    """Every accepting id; the worst ratio over the ids is the figure of DESIGN.md 4.1b."""
    worst = max(cg.run_dgrad(be, case, cfg, acc) for cfg in (cg.PLACED_IDS_RES if acc else cg.PLACED_IDS))
    print(f"\n[placed matrix] {case[0]} acc {acc}: worst kernel / torch over {len(cg.PLACED_IDS)} ids = {worst:.2f}")


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("case", [cg.DG_TAILS, cg.DG_ODD, cg.DG_VIEW], ids=lambda c: c[0])
def test_gpu_placed_matrix_fp32(be, case, acc):
    for cfg in cg.PLACED_IDS_F32:
        cg.run_dgrad(be, case, cfg, acc, F32)


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("case", cg.DG_EDGES + [cg.DG_TAILS, cg.DG_TRAIN, cg.DG_TRAIN2], ids=lambda c: c[0])
def test_gpu_dgrad_default_tile(be, case, acc):
    cg.run_dgrad(be, case, -1, acc)


@pytest.mark.parametrize("cfg", [95, 96])
@pytest.mark.parametrize("case", cg.DG_G8, ids=lambda c: c[0])
def test_gpu_dgrad_dense_8phase(be, case, cfg):
    cg.run_dgrad(be, case, cfg, 1)


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("over", [False, True], ids=["under", "over"])
def test_gpu_placed_image_around_2_31_bytes(be, over, acc):
    """Under the limit the launch must be right up to the far end of the buffer; over it, right or refused with a message."""
    free, _ = torch.cuda.mem_get_info(be.dev)
    try:
        res = cg.run_big_placed(be, over, acc)
    except torch.OutOfMemoryError as e:
        print(f"\n[big placed] skipped: the destination could not be allocated ({free >> 20} MiB free): {e}")
        pytest.skip("2 GiB destination could not be allocated")
    finally:
        torch.cuda.empty_cache()
    print(f"\n[big placed over={int(over)} acc={acc}] {res}")
    assert res == "ok" or (over and res.startswith("refused"))
