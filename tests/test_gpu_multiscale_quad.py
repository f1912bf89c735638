"""GPU (-m gpu): training at varying shapes on the MI355X -- the twins of tests/test_emu_multiscale_quad.py through the library on cuda:0
(quad against the reference's own collate_fn4, `y5_collate4` against the restatement, the multi-scale draws and pixels, the quad loss factor),
the loader's own canvas for the quad kernel (64 x 3 x 640^2 is 16 of these: row pitch 1280), and the plan-cache and end-to-end checks on
yolov5n / yolov5n-seg, batch 2, shapes 64^2 / 96^2 / 128^2, as three small plans."""
import copy

import numpy as np
import pytest
import torch

from oracle import yolo_oracle as yo
from tests import quad_ref as qr
from tests import test_emu_multiscale_quad as twin

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _seam(monkeypatch):
    """(replaces the twin's emulator seam: the product library, CUDA tensors)"""
    monkeypatch.setenv("Y5_DETERMINISTIC", "1")
    monkeypatch.delenv("Y5_TRAIN_PLAN_CACHE", raising=False)
    yield


_SD = {}


def _state(name):
    if name not in _SD:
        _SD[name] = yo.det_state_dict(yo.model_cfg(name), 0, fused=False)
    return copy.deepcopy(_SD[name])


def yolov5n(device):
    from yolov5_amd.yolo import DetectionModel

    m = DetectionModel("yolov5n.yaml")
    m.load_state_dict(_state("yolov5n"))
    return m.to(device).train()


def yolov5n_seg(device):
    from yolov5_amd.yolo import SegmentationModel

    m = SegmentationModel("yolov5n-seg.yaml")
    m.load_state_dict(_state("yolov5n-seg"))
    return m.to(device).train()


def test_quad_matches_reference_golden(dev):
    twin.check_quad_golden(dev)


@pytest.mark.parametrize("H,W", twin.KERNEL_CASES)
def test_collate4_kernel_matches_restatement(H, W, dev):
    twin.check_quad_kernel(H, W, dev)


def test_collate4_kernel_on_the_loader_canvas(dev):
    """640 x 640, n = 2 (B = 8): one group upsampled, one tiled, the 16-byte path at the loader's row pitch of 1280."""
    from yolov5_amd.dataloaders import collate_fn4

    imgs = qr.byte_patterns(8, 3, 640, 640, seed=11)
    got = collate_fn4(torch.from_numpy(imgs).to(dev), torch.zeros((0, 6)), None, None, twin.Coins([0.25, 0.5]))[0]
    assert tuple(got.shape) == (2, 3, 1280, 1280)
    assert np.array_equal(got.cpu().numpy(), qr.collate4_images(imgs, [True, False]))


def test_quad_guards(dev):
    twin.check_quad_guards(dev)


def test_quad_loader_drops_last_and_draws_after_the_samples(dev):
    twin.check_quad_loader(dev)


def test_multi_scale_draws(dev):
    twin.check_multi_scale_draws(dev, wide_calls=60)


def test_multi_scale_pixels_within_derived_bound(dev):
    twin.check_multi_scale_pixels(dev)


def test_plan_cache_sequence_shares_arena_and_tracks_weights(dev):
    twin.check_plan_cache_sequence(yolov5n, dev)


def test_plan_cache_byte_budget_evicts_and_releases(dev):
    twin.check_plan_cache_budget(yolov5n, dev)


def test_plan_cache_default_is_single_plan(dev):
    twin.check_plan_cache_default(yolov5n, dev)


def test_plan_cache_accumulates_across_shapes(dev):
    twin.check_plan_cache_accumulate(yolov5n, dev)


def test_plan_cache_stale_forward_still_raises(dev):
    twin.check_plan_cache_stale(yolov5n, dev)


def test_train_multi_scale_end_to_end(dev):
    twin.check_train_multi_scale(yolov5n, dev)


def test_train_multi_scale_end_to_end_segmentation(dev):
    twin.check_train_multi_scale(yolov5n_seg, dev, seg=True)


def test_quad_loss_factor_equals_scaled_gains(dev):
    twin.check_quad_factor(yolov5n, dev)
