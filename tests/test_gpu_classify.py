"""GPU: the classification kernels, the ClassificationModel plan and the predict / val loops on the MI355X, against tests/golden/classify.npz
(written from the unmodified reference) under the rules of tests/classify_ref.py -- the same cases as tests/test_emu_classify.py plus the sizes
only a GPU run is quick at."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import classify_ref as cr

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda"


def _lib():
    from yolov5_amd import _lib as L

    return L


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _frames(names):
    """Device copies of the sources whose rows are `stride` > 3 * w0 bytes apart, as on the host."""
    out = []
    for n in names:
        im, stride = cr.source(n)
        h0, w0 = im.shape[:2]
        wide = torch.zeros((h0, stride), dtype=torch.uint8)
        wide[:, :3 * w0] = torch.from_numpy(np.ascontiguousarray(im)).reshape(h0, 3 * w0)
        out.append(wide.to(DEV)[:, :3 * w0].unflatten(1, (w0, 3)))
    return out


def _transform(frames, size, half=False):
    from yolov5_amd.augmentations import classify_transform_batch

    # (classify_transform_batch makes strided views contiguous: the strided sources go through the C entry directly, then both are compared)
    L = _lib()
    jobs = (L.ClassifyJob * len(frames))()
    for j, f in zip(jobs, frames):
        j.src, j.h0, j.w0, j.stride = f.data_ptr(), f.shape[0], f.shape[1], f.stride(0)
    table = torch.frombuffer(bytearray(jobs), dtype=torch.uint8).to(DEV)
    lut = cr.lut().to(DEV)
    n = len(frames) * 3 * size * size
    dt = torch.float16 if half else torch.float32
    buf = torch.full((64 + n + 64,), -77.5, dtype=dt, device=DEV)
    out = buf[64:64 + n]
    rc = L.lib().y5_classify_transform_batch(_p(table), len(frames), size, _p(lut), _p(out), L.Y5_F16 if half else L.Y5_F32, L.stream(DEV))
    assert rc == 0, L.lib().y5_last_error()
    assert (buf[:64] == -77.5).all() and (buf[64 + n:] == -77.5).all() and (out != -77.5).all()
    via_api = classify_transform_batch([f.contiguous() for f in frames], size, half=half)
    got = out.reshape(len(frames), 3, size, size)
    assert torch.equal(got, via_api)
    return got.cpu().numpy()


def test_gpu_transform_cases_bit_equal_to_reference_golden():
    g = cr.golden()
    names = list(cr.TRANSFORM_CASES)
    frames = _frames(names)
    assert all(f.shape[0] == 1 or f.stride(0) > 3 * f.shape[1] for f in frames)
    batch = _transform(frames, cr.S)
    half = _transform(frames, cr.S, half=True)
    for i, n in enumerate(names):
        assert np.array_equal(batch[i], g[f"tf_{n}"]), n
        assert np.array_equal(half[i], batch[i].astype(np.float16)), n
        assert np.array_equal(_transform(frames[i:i + 1], cr.S)[0], batch[i]), n   # the ragged batch equals the single calls


def test_gpu_transform_full_hd_frame():
    im, _ = cr.source("hd", shape=(1080, 1920), pad=0)
    got = _transform([torch.from_numpy(np.ascontiguousarray(im)).to(DEV)], 224)[0]
    assert np.array_equal(got, cr.transform_restated(im, 224))


def _head(x, w, bias, C_, nc, form):
    L = _lib()
    B, HW, ld = x.shape
    X, Wt, Bi = (torch.from_numpy(a).to(DEV) for a in (x, w, bias))
    out = torch.full((B, nc + 3), -9.5, dtype=X.dtype, device=DEV)
    nbytes = L.lib().y5_classify_head_workspace_bytes(B, C_)
    ws = L.workspace(nbytes, DEV)
    rc = L.lib().y5_classify_head(_p(X), L.Y5_F16 if x.dtype == np.float16 else L.Y5_F32, B, HW, C_, ld, _p(Wt), _p(Bi), nc, _p(out), nc + 3, form, _p(ws),
                                  nbytes, L.stream(DEV))
    assert rc == 0, L.lib().y5_last_error()
    assert (out[:, nc:] == -9.5).all()
    return out[:, :nc].cpu().numpy()


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("dtype", [np.float16, np.float32])
def test_gpu_head_within_fp32_summation_bound_and_batch_independent(dtype, form):
    for shape in cr.HEAD_SHAPES + [(2, 6, 1280, 10, 1288), (130, 49, 1280, 1000)]:
        B, HW, C_, nc = shape[:4]
        x, w, bias = cr.head_inputs(B, HW, C_, nc, dtype, shape[4] if len(shape) > 4 else None)
        got = _head(x, w, bias, C_, nc, form)
        ref, bound = cr.head_ref(x, w, bias, C_)
        err = np.abs(got.astype(np.float64) - ref)
        print(f"head {shape} {np.dtype(dtype).name} form {form}: max err / bound = {(err / bound).max():.3f}")
        assert (err <= bound).all(), (shape, (err / bound).max())
        if B in (5, 130):   # rows on their own, and in another position of the batch: the same bits
            pick = [0, B // 2, B - 1]
            for b in pick:
                assert np.array_equal(_head(x[b:b + 1], w, bias, C_, nc, form), got[b:b + 1]), (shape, b)
            assert np.array_equal(_head(np.ascontiguousarray(x[::-1]), w, bias, C_, nc, form), got[::-1]), shape


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
def test_gpu_post_top5_exact_probs_and_loss_within_bound(dtype):
    from yolov5_amd.torch_utils import classify_post

    for nc in cr.POST_NC:
        for B in cr.POST_B:
            z, labels = cr.post_inputs(B, nc, dtype)
            zt = torch.full((B, nc + 3), 99.0, dtype=torch.from_numpy(z).dtype, device=DEV)
            zt[:, :nc] = torch.from_numpy(z).to(DEV)
            for eps in (0.0, 0.1):
                want5, p64, pb, l64, lb = cr.post_ref(z, labels, eps)
                top5, probs, loss = classify_post(zt[:, :nc], torch.from_numpy(labels).to(DEV), eps)
                assert np.array_equal(top5.cpu().numpy(), want5), (nc, B)
                ep, el = np.abs(probs.cpu().numpy() - p64), np.abs(loss.cpu().numpy() - l64)
                print(f"post nc {nc} B {B} {np.dtype(dtype).name} eps {eps}: probs err / bound {(ep / pb).max():.3f}, loss err / bound {(el / lb).max():.3f}")
                assert (ep <= pb).all() and (el <= lb).all(), (nc, B, eps)
            top5, probs, loss = classify_post(zt[:, :nc], want_probs=False)
            assert probs is None and loss is None and np.array_equal(top5.cpu().numpy(), want5)


def cls_model(name="yolov5n", fused=True):
    from yolov5_amd.yolo import ClassificationModel, DetectionModel

    m = ClassificationModel(model=DetectionModel(name + ".yaml"), nc=cr.MODEL_NC, cutoff=10)
    m.load_state_dict(cr.cls_state_dict(name))
    m.eval()
    return (m.fuse() if fused else m).to(DEV)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("key", list(cr.MODEL_INPUTS))
def test_gpu_yolov5n_cls_fp32_matches_reference_fp64(key, fused):
    ref = cr.golden()[f"logits64_{key}"]
    got = cls_model(fused=fused)(cr.model_input(key).to(DEV)).cpu().numpy()
    print(f"fp32 plan {key} fused={fused}: max error {np.abs(got - ref).max():.3e}")
    np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-4)
    cr.assert_top5_matches(got, ref, 1e-4 + 1e-4 * np.abs(ref).max(), f"top-5 {key}")


@pytest.mark.parametrize("key", list(cr.MODEL_INPUTS))
def test_gpu_yolov5n_cls_fp16_within_twice_the_reference_half_forward(key):
    g = cr.golden()
    ref = g[f"logits64_{key}"]
    noise = np.abs(g[f"logits16_{key}"].astype(np.float64) - ref).max()
    m = cls_model().half()
    got = m(cr.model_input(key).to(DEV).half()).float().cpu().numpy().astype(np.float64)
    err = np.abs(got - ref).max()
    print(f"fp16 plan {key}: max error {err:.3e}, reference half forward {noise:.3e}")
    assert err <= 2 * noise, (err, noise)
    cr.assert_top5_matches(got, ref, 2 * noise, f"top-5 {key} fp16")


def test_gpu_yolov5s_cls_224_fp32_matches_reference_fp64():
    from oracle import detgen

    ref = cr.golden()["s_logits64"]
    x = torch.from_numpy(detgen.uniform((2, 3, 224, 224), 0.0, 1.0, name="img", seed=5)).to(DEV)
    got = cls_model("yolov5s")(x).cpu().numpy()
    print(f"yolov5s-cls 224 fp32: max error {np.abs(got - ref).max():.3e}")
    np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-4)


def test_gpu_graph_replay_fresh_tensors_and_refresh_weights():
    m = cls_model().half()
    x = cr.model_input("sq").to(DEV).half()
    outs = [m(x) for _ in range(3)]
    eng = next(iter(m._engines.values()))
    assert eng._graph, "the forward did not replay a captured graph"
    assert len({o.data_ptr() for o in outs}) == 3 and all(torch.equal(o, outs[0]) for o in outs)
    with torch.no_grad():
        m.model[-1].linear.weight.mul_(0.5)
        m.model[-1].linear.bias.zero_()
    after = m(x)
    assert next(iter(m._engines.values())) is eng and not torch.equal(after, outs[0])
    fresh = cls_model().half()
    with torch.no_grad():
        fresh.model[-1].linear.weight.mul_(0.5)
        fresh.model[-1].linear.bias.zero_()
    assert torch.equal(after, fresh(x))


def test_gpu_predict_loop_equals_the_composition_of_its_seams():
    from yolov5_amd import classify_loop
    from yolov5_amd.augmentations import classify_transforms
    from yolov5_amd.common import DetectMultiBackend
    from yolov5_amd.detect_loop import load_image
    from yolov5_amd.torch_utils import classify_post

    ims = [load_image(os.path.join(G, n)) for n in ("bus.jpg", "zidane.jpg")]
    assert ims[0].shape != ims[1].shape   # one ragged batch
    m = DetectMultiBackend(cls_model(), device=torch.device(DEV), fuse=False)
    res, probs = classify_loop.predict(m, ims, imgsz=224, topk=5)
    x = classify_transforms(224)(ims, device=DEV)
    for i, im in enumerate(ims):
        assert np.array_equal(x[i].cpu().numpy(), cr.transform_restated(np.asarray(im), 224))
    top5, p, _ = classify_post(m(x))
    assert torch.equal(probs, p) and torch.allclose(p.sum(1), torch.ones(2, device=DEV), atol=1e-5)
    for i, (idx, pr) in enumerate(res):
        assert torch.equal(idx, top5[i].long().cpu()) and torch.equal(pr, p[i, idx.to(DEV)].cpu())


@pytest.mark.parametrize("k", [0, 1])
def test_gpu_val_run_over_three_batches_matches_the_reference(k):
    from yolov5_amd import classify_val
    from yolov5_amd.torch_utils import smartCrossEntropyLoss

    g = cr.golden()
    labels = torch.from_numpy(g["val_labels"]).to(DEV)
    loader = [(b.to(DEV), labels[2 * i:2 * i + len(b)]) for i, b in enumerate(cr.val_inputs())]
    top1, top5, loss = classify_val.run(cls_model(), loader, criterion=smartCrossEntropyLoss((0.0, 0.1)[k]), verbose=True)
    want = g[f"val_triple_{k}"]
    assert (top1, top5) == pytest.approx(tuple(want[:2]), abs=1e-6) and loss == pytest.approx(want[2], rel=1e-4, abs=1e-4)
    rows = np.array([[r[1], r[2], r[3]] for r in classify_val.run.rows], np.float64)
    np.testing.assert_allclose(rows, g[f"val_rows_{k}"], rtol=5e-3, equal_nan=True)


def test_gpu_classification_loader_one_launch_per_batch():
    from yolov5_amd.dataloaders import ClassificationLoader

    names = list(cr.TRANSFORM_CASES)[:5]
    frames = [np.ascontiguousarray(cr.source(n)[0]) for n in names]
    dl = ClassificationLoader(frames, [3, 1, 4, 1, 5], imgsz=cr.S, batch_size=2, device=DEV)
    got = list(dl)
    assert len(dl) == 3 and [tuple(x.shape) for x, _ in got] == [(2, 3, 32, 32), (2, 3, 32, 32), (1, 3, 32, 32)]
    assert torch.cat([y for _, y in got]).tolist() == [3, 1, 4, 1, 5] and got[0][1].dtype == torch.int64
    g = cr.golden()
    for i, n in enumerate(names):
        assert np.array_equal(got[i // 2][0][i % 2].cpu().numpy(), g[f"tf_{n}"])
