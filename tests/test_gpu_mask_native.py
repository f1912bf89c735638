"""GPU (-m gpu): yolov5_amd.segment.process_mask_native / process_mask_native_batch (y5_process_mask_native_batch, csrc/mask_native.h)
on the MI355X: the cases of tests/mask_native_ref.py against the reference-generated golden, one predict-size call against the fp32
restatement run on the CPU, the output dtypes against each other, and the CPU refusal.  Acceptance rule: tests/mask_native_ref.py."""
import numpy as np
import pytest
import torch

from tests import mask_native_ref as mr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _rows(coef, boxes, dev, extra=4):
    """NMS-style padded rows [x1, y1, x2, y2, conf, cls, coefficients] with `extra` unused rows behind: the view of the first n is what
    non_max_suppression(padded=True) hands out."""
    n, c = coef.shape
    det = torch.full((n + extra, 6 + c), 9.0)
    det[:n, :4] = torch.from_numpy(boxes)
    det[:n, 6:] = torch.from_numpy(coef)
    return det.to(dev)[:n]


@pytest.mark.parametrize("pd", mr.PROTO_DTYPES)
@pytest.mark.parametrize("name", list(mr.CASES))
def test_process_mask_native_cases_vs_reference_golden(name, pd, dev):
    from yolov5_amd.segment import process_mask_native

    protos, coef, boxes, shape = mr.inputs(name, pd)
    P = torch.from_numpy(protos).to(dev)
    det = _rows(coef, boxes, dev)
    f = process_mask_native(P, det[:, 6:], det[:, :4], shape)
    assert f.dtype == torch.float32 and tuple(f.shape) == (mr.N,) + shape and f.device.type == "cuda"
    mr.accept_case(f.cpu().numpy(), name, pd, f"gpu {name}/{pd}/f32")
    u = process_mask_native(P, det[:, 6:], det[:, :4], shape, out_dtype=torch.uint8)
    b = process_mask_native(P, torch.from_numpy(coef).to(dev), torch.from_numpy(boxes).to(dev), shape, out_dtype=torch.bool)
    assert u.dtype == torch.uint8 and b.dtype == torch.bool
    assert torch.equal(u, f.to(torch.uint8)) and torch.equal(b, f.bool())


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.uint8])
@pytest.mark.parametrize("pd", mr.PROTO_DTYPES)
@pytest.mark.parametrize("proto_shape", [(8, 24, 40), (32, 40, 40)])
def test_process_mask_native_batch_vs_golden_and_single_calls(proto_shape, pd, out_dtype, dev):
    """All cases with the same prototype shape plus an image without detections in ONE call: every image is accepted against the golden and
    equals its single-image call bit for bit; the results are views of one allocation, 16-byte aligned per image."""
    from yolov5_amd.segment import process_mask_native, process_mask_native_batch

    names = [n for n, v in mr.CASES.items() if v[:3] == proto_shape]
    ins = [mr.inputs(n, pd) for n in names]
    names.insert(1, None)
    protos = torch.from_numpy(np.stack([ins[0][0], ins[0][0]] + [i[0] for i in ins[1:]])).to(dev)
    dets = [_rows(i[1], i[2], dev) for i in ins]
    shapes = [i[3] for i in ins]
    dets.insert(1, torch.zeros((0, 6 + proto_shape[0]), device=dev))
    shapes.insert(1, (45, 51))
    got = process_mask_native_batch(protos, dets, shapes, out_dtype=out_dtype)
    assert len(got) == len(names) and tuple(got[1].shape) == (0, 45, 51)
    base = got[0].untyped_storage().data_ptr()
    for k, (name, g, d, s) in enumerate(zip(names, got, dets, shapes)):
        assert g.dtype == out_dtype and tuple(g.shape) == (d.shape[0],) + tuple(s)
        assert g.untyped_storage().data_ptr() == base and g.data_ptr() % 16 == 0
        if name:
            mr.accept_case(g.cpu().numpy(), name, pd, f"gpu batch {name}/{pd}")
            assert torch.equal(g, process_mask_native(protos[k], d[:, 6:], d[:, :4], s, out_dtype=out_dtype)), (k, s)


def test_process_mask_native_predict_size(dev):
    """segment/predict.py at 640 with retina_masks: prototypes (32, 160, 160) fp16, a 1080 x 810 and a 720 x 1280 image, 20 instances each,
    coefficients and boxes read in place from NMS-style rows; against the fp32 restatement on the CPU."""
    from yolov5_amd.segment import process_mask_native_batch

    shapes = [(1080, 810), (720, 1280)]
    ins = [mr.make_inputs(f"predict{k}", 32, 160, 160, h0, w0, n=20, proto_dtype="f16") for k, (h0, w0) in enumerate(shapes)]
    protos = torch.from_numpy(np.stack([i[0] for i in ins])).to(dev)
    dets = [_rows(i[1], i[2], dev, extra=10) for i in ins]
    f = process_mask_native_batch(protos, dets, shapes)
    u = process_mask_native_batch(protos, dets, shapes, out_dtype=torch.uint8)
    b = process_mask_native_batch(protos, dets, shapes, out_dtype=torch.bool)
    for k, (i, s) in enumerate(zip(ins, shapes)):
        assert f[k].dtype == torch.float32 and u[k].dtype == torch.uint8 and b[k].dtype == torch.bool
        assert tuple(f[k].shape) == (20,) + s
        assert torch.equal(u[k], f[k].to(torch.uint8)) and torch.equal(b[k], f[k].bool())
        bits, v64, band = mr.reference_of(i[0], i[1], i[2], s)
        mr.accept(u[k].cpu().numpy(), bits, v64, band, f"gpu predict-size {s}")


def test_process_mask_native_refuses_cpu_tensors_and_bad_arguments(dev):
    from yolov5_amd.segment import process_mask_native, process_mask_native_batch

    protos, coef, boxes, shape = mr.inputs("up")
    P, Cf, Bx = torch.from_numpy(protos), torch.from_numpy(coef), torch.from_numpy(boxes)
    with pytest.raises(RuntimeError, match="no CPU path"):
        process_mask_native(P, Cf, Bx, shape)
    with pytest.raises(RuntimeError, match="no CPU path"):
        process_mask_native_batch(P[None], [torch.cat((Bx, Bx[:, :2], Cf), 1)], [shape])
    with pytest.raises(RuntimeError, match="no CPU path"):
        process_mask_native(P.to(dev), Cf, Bx.to(dev), shape)
    with pytest.raises(TypeError):
        process_mask_native(P.to(dev), Cf.to(dev), Bx.to(dev), shape, out_dtype=torch.float16)
    with pytest.raises(ValueError, match="empty window"):
        process_mask_native(torch.zeros((8, 25, 40), device=dev), Cf.to(dev), Bx.to(dev), (1, 300))
    with pytest.raises(ValueError):
        process_mask_native_batch(P[None].to(dev), [], [shape])
