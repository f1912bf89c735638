"""GPU: the memory-bound kernels between the convolutions of the training path, each called directly through the C-ABI on the full tables of
tests/train_glue_ref.py: bit-exact data movement and small sums at every dispatch path, every y5_sppf_pool instantiation the launcher can select,
and the BatchNorm family against float64 up to the benchmark's pixel counts, with the conditioning sweep of the single-pass variance."""
import pytest
import torch

from tests import train_glue_ref as tg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    assert torch.cuda.is_available()
    return tg.GpuBackend(torch.device("cuda:0"))


@pytest.fixture
def sppf_gv(monkeypatch):
    return lambda v: monkeypatch.delenv("Y5_SPPF_GV", raising=False) if v is None else monkeypatch.setenv("Y5_SPPF_GV", str(v))


# ---- 1. pure data movement ----
@pytest.mark.parametrize("case", tg.MOVE_CASES)
def test_gpu_upsample2x(be, case):
    tg.run_upsample2x(be, case)


@pytest.mark.parametrize("case", tg.MOVE_CASES)
def test_gpu_copy_slice(be, case):
    tg.run_copy_slice(be, case)


@pytest.mark.parametrize("case", tg.NCHW_CASES)
def test_gpu_nchw_to_nhwc(be, case):
    tg.run_nchw_to_nhwc(be, case)


@pytest.mark.parametrize("case", tg.NHWC_NCHW_CASES)
def test_gpu_nhwc_to_nchw(be, case):
    tg.run_nhwc_to_nchw(be, case)


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("case", tg.RAW_CASES)
def test_gpu_head_layout(be, case, f32):
    tg.run_raw(be, case, f32)


def test_gpu_memset_zero(be):
    tg.run_memset_zero(be)


# ---- 2. exactly specified arithmetic ----
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("case", tg.SUM_CASES)
def test_gpu_upsample2x_bwd(be, case, acc):
    tg.run_upsample2x_bwd(be, case, acc)


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("case", tg.SUM_CASES)
def test_gpu_add_slice(be, case, acc):
    tg.run_add_slice(be, case, acc)


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("case", tg.SUM_CASES_F32)
def test_gpu_glue_f32_upsample2x_bwd_and_add_slice(be, case, acc):
    tg.run_upsample2x_bwd(be, case, acc, f32=True)
    tg.run_add_slice(be, case, acc, f32=True)


@pytest.mark.parametrize("case", tg.SPPF_BWD_F32_CASES)
def test_gpu_glue_f32_sppf_pool_bwd(be, case):
    tg.run_sppf_bwd_f32(be, case)


# ---- 3. SPPF pooling chain ----
@pytest.mark.parametrize("case", tg.SPPF_CASES)
def test_gpu_sppf_pool(be, case, sppf_gv):
    tg.run_sppf_pool(be, case, sppf_gv)


def test_gpu_sppf_pool_refuses_a_plane_beyond_lds(be, sppf_gv):
    tg.run_sppf_pool(be, tg.SPPF_UNSUPPORTED, sppf_gv, unsupported=True)


# ---- 4. BatchNorm family ----
@pytest.mark.parametrize("case", tg.bn_cases(full=True))
def test_gpu_bn_family(be, case):
    tg.run_bn(be, case)


# ---- 5. conditioning ----
@pytest.mark.parametrize("ratio", tg.COND_RATIOS)
@pytest.mark.parametrize("case", tg.cond_cases((1600, 102400)))
def test_gpu_bn_conditioning(be, case, ratio):
    tg.run_bn_conditioning(be, case, ratio)
