"""GPU: yolov5_amd.segment_loss.ComputeLoss (HIP kernels behind y5_seg_loss_forward / _backward) against the reference-generated
fixture tests/golden/seg_loss.npz, through autograd, plus bit-repeatability."""
import os
import types

import numpy as np
import pytest
import torch

from tests import seg_loss_ref as sr

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "seg_loss.npz"))


class _Model(torch.nn.Module):
    def __init__(self, nc, dev):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1, device=dev))
        self.hyp = dict(sr.HYP)
        self.model = [types.SimpleNamespace(nl=3, na=3, nc=nc, nm=sr.NM, anchors=sr.ANCHORS.to(dev),
                                            stride=torch.tensor([float(s) for s in sr.STRIDES]))]


def _run(name, u8=False):
    from yolov5_amd.segment_loss import ComputeLoss

    dev = torch.device("cuda:0")
    c = sr.seg_case(name)
    cl = ComputeLoss(_Model(c["nc"], dev), overlap=c["overlap"])
    p = [torch.from_numpy(a).to(dev).requires_grad_(True) for a in c["p"]]
    proto = torch.from_numpy(c["proto"]).to(dev).requires_grad_(True)
    m = torch.from_numpy(c["masks"])
    if u8:
        m = m.to(torch.uint8)
    loss, items = cl((p, proto), torch.from_numpy(c["targets"]), m.to(dev))
    loss.backward()
    torch.cuda.synchronize()
    return (loss.detach().cpu().numpy(), items.cpu().numpy(), [pi.grad.cpu().numpy() for pi in p], proto.grad.cpu().numpy())


def _grad_close(got, ref, rtol=2e-4, atol_frac=1e-6):
    np.testing.assert_allclose(got.astype(np.float64), ref.astype(np.float64), rtol=rtol, atol=atol_frac * max(np.abs(ref).max(), 1e-30))


def _rel_l2(got, ref):
    got, ref = got.astype(np.float64).ravel(), ref.astype(np.float64).ravel()
    return np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-30)


@pytest.mark.parametrize("name", [c for c in sr.CASES if c != "fp16"])
def test_gpu_seg_loss_vs_reference_golden_fp32(name):
    loss, items, dp, dproto = _run(name)
    np.testing.assert_allclose(loss, G[f"{name}_loss"], rtol=1e-5)
    np.testing.assert_allclose(items, G[f"{name}_items"], rtol=1e-5, atol=1e-7)
    for i in range(3):
        _grad_close(dp[i], G[f"{name}_dp{i}"])
    _grad_close(dproto, G[f"{name}_dproto"])


def test_gpu_seg_loss_vs_reference_golden_fp16():
    loss, items, dp, dproto = _run("fp16")
    assert _rel_l2(loss, G["fp16_loss"]) <= 2e-3
    assert _rel_l2(items, G["fp16_items"]) <= 2e-3
    for i in range(3):
        assert dp[i].dtype == np.float16 and _rel_l2(dp[i], G[f"fp16_dp{i}"]) <= 2e-3, i
    assert dproto.dtype == np.float16 and _rel_l2(dproto, G["fp16_dproto"]) <= 2e-3


def test_gpu_seg_loss_u8_masks():
    loss, items, dp, dproto = _run("overlap", u8=True)
    np.testing.assert_allclose(loss, G["overlap_loss"], rtol=1e-5)
    _grad_close(dproto, G["overlap_dproto"])


def test_gpu_seg_loss_bit_repeatable():
    a, b = _run("unsorted"), _run("unsorted")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3])
    for x, y in zip(a[2], b[2]):
        assert np.array_equal(x, y)


def test_gpu_seg_loss_no_targets_without_overlap():
    """overlap=False, empty batch: masks (0, mh, mw) at another resolution -> the detection terms only, like the reference."""
    from yolov5_amd.segment_loss import ComputeLoss

    dev = torch.device("cuda:0")
    c = sr.seg_case("no_overlap")
    cl = ComputeLoss(_Model(c["nc"], dev), overlap=False)
    p = [torch.from_numpy(a).to(dev).requires_grad_(True) for a in c["p"]]
    proto = torch.from_numpy(c["proto"]).to(dev).requires_grad_(True)
    loss, items = cl((p, proto), torch.zeros((0, 6)), torch.zeros((0, 2 * proto.shape[2], 2 * proto.shape[3]), device=dev))
    loss.backward()
    it = items.cpu().numpy()
    assert np.isfinite(loss.item()) and it[0] == 0 and it[1] == 0 and it[2] > 0
    assert not proto.grad.any()


def test_gpu_seg_loss_autobalance_matches_detection_loss():
    """autobalance=True reads obji through y5_seg_loss_obji_offset: the balance after each call equals the detection loss's on the same
    objectness logits (the objectness term does not depend on the mask columns)."""
    from yolov5_amd.loss import ComputeLoss as DetLoss
    from yolov5_amd.segment_loss import ComputeLoss

    dev = torch.device("cuda:0")
    c = sr.seg_case("overlap")
    m = _Model(c["nc"], dev)
    seg, det = ComputeLoss(m, autobalance=True, overlap=True), DetLoss(m, autobalance=True)
    p = [torch.from_numpy(a).to(dev) for a in c["p"]]
    proto = torch.from_numpy(c["proto"]).to(dev)
    t = torch.from_numpy(c["targets"])
    for _ in range(2):
        seg((p, proto), t, torch.from_numpy(c["masks"]).to(dev))
        det([pi[..., :5 + c["nc"]].contiguous() for pi in p], t)
        assert seg.last_obji == det.last_obji
        assert seg.balance == det.balance and seg.balance != [4.0, 1.0, 0.4]
