"""CPU: classification training on the HIP emulator -- the kernels of yolov5_amd/csrc/classify_train.h through their C entries, the
cross-entropy autograd Function, the TrainEngine plan of a ClassificationModel and yolov5_amd/classify_train.train -- against the float64
restatements of tests/classify_train_ref.py and tests/golden/classify_train.npz (written from the unmodified reference by
scripts/make_golden_classify_train.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import classify_ref as cr
from tests import classify_train_ref as ct
from tests.hipemu import backend as emu_backend
from tests.hipemu.emu import aligned, emu, ptr
from yolov5_amd import _lib

BAD, UNSUP, WS = -1, -2, -4


@pytest.fixture()
def emu_seam():
    emu_backend.install()
    yield
    emu_backend.uninstall()


# ---- head backward ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float16, np.float32])
@pytest.mark.parametrize("shape", ct.BWD_SHAPES)
def test_emu_head_bwd_within_bounds_and_deterministic(shape, dtype):
    ct.check_head_bwd(ct.EmuMem(), shape, dtype)


def test_emu_head_bwd_bad_arguments():
    lib = emu()
    B, HW, C_, nc = 2, 6, 64, 10
    dl, pooled, w = ct.bwd_inputs(B, HW, C_, nc, np.float32)
    DL = aligned(dl.shape, np.float32); DL[...] = dl
    P = aligned(pooled.shape, np.float32); P[...] = pooled
    Wt = aligned(w.shape, np.float32); Wt[...] = w
    db, dw, dx, ws = aligned((nc,), np.float32), aligned((nc, C_), np.float32), aligned((B, HW, C_), np.float32), aligned((B * C_,), np.float32)

    def call(**kw):
        a = dict(dl=ptr(DL), dt=_lib.Y5_F32, B=B, nc=nc, ldd=nc, P=ptr(P), w=ptr(Wt), HW=HW, C=C_, p=0.0, seed=0, db=ptr(db), dw=ptr(dw), dx=ptr(dx), ld=C_,
                 ws=ptr(ws), nb=B * C_ * 4)
        a.update(kw)
        return lib.y5_classify_head_bwd(a["dl"], a["dt"], a["B"], a["nc"], a["ldd"], a["P"], a["w"], a["HW"], a["C"], a["p"], a["seed"], a["db"], a["dw"],
                                        a["dx"], a["ld"], a["ws"], a["nb"], None)

    assert call() == 0
    for kw in (dict(dl=None), dict(P=None), dict(w=None), dict(db=None), dict(dw=None), dict(dx=None), dict(dt=_lib.Y5_U8), dict(B=0), dict(HW=0), dict(C=0),
               dict(nc=0), dict(ld=C_ - 8), dict(ldd=nc - 1), dict(p=-0.1), dict(p=1.5), dict(p=float("nan")), dict(dx=C.c_void_p(dx.ctypes.data + 4)),
               dict(w=C.c_void_p(Wt.ctypes.data + 8)), dict(P=C.c_void_p(P.ctypes.data + 4)), dict(dl=C.c_void_p(DL.ctypes.data + 2))):
        assert call(**kw) == BAD, kw
        assert b"classify_head_bwd" in lib.y5_last_error()
    for kw in (dict(C=60, ld=60), dict(ld=C_ + 2), dict(C=8200, ld=8200), dict(B=65536)):
        assert call(**kw) == UNSUP, kw
    for kw in (dict(ws=None), dict(nb=B * C_ * 4 - 1), dict(ws=C.c_void_p(ws.ctypes.data + 4))):
        assert call(**kw) == WS, kw


def test_emu_head_train_and_ce_bwd_bad_arguments():
    lib = emu()
    B, HW, C_, nc = 2, 6, 64, 10
    x, w, bias = cr.head_inputs(B, HW, C_, nc, np.float32)
    X = aligned(x.shape, np.float32); X[...] = x
    Wt = aligned(w.shape, np.float32); Wt[...] = w
    Bi = aligned(bias.shape, np.float32); Bi[...] = bias
    out, pooled = aligned((B, nc), np.float32), aligned((B * C_,), np.float32)

    def call(**kw):
        a = dict(x=ptr(X), dt=_lib.Y5_F32, B=B, HW=HW, C=C_, ld=C_, w=ptr(Wt), bias=ptr(Bi), nc=nc, out=ptr(out), ldo=nc, pl=ptr(pooled), nb=B * C_ * 4, p=0.5, seed=7)
        a.update(kw)
        return lib.y5_classify_head_train(a["x"], a["dt"], a["B"], a["HW"], a["C"], a["ld"], a["w"], a["bias"], a["nc"], a["out"], a["ldo"], a["pl"], a["nb"],
                                          a["p"], a["seed"], None)

    assert call() == 0
    for kw in (dict(x=None), dict(w=None), dict(bias=None), dict(out=None), dict(dt=_lib.Y5_U8), dict(B=0), dict(HW=0), dict(C=0), dict(nc=0), dict(ld=C_ - 8),
               dict(ldo=nc - 1), dict(p=-0.5), dict(p=1.01), dict(p=float("nan")), dict(x=C.c_void_p(X.ctypes.data + 4))):
        assert call(**kw) == BAD, kw
        assert b"classify_head_train" in lib.y5_last_error()
    for kw in (dict(C=60, ld=60), dict(ld=C_ + 2), dict(C=8200, ld=8200), dict(B=65536)):
        assert call(**kw) == UNSUP, kw
    for kw in (dict(pl=None), dict(nb=B * C_ * 4 - 1), dict(pl=C.c_void_p(pooled.ctypes.data + 4))):
        assert call(**kw) == WS, kw

    z, labels = cr.post_inputs(7, 10, np.float32)
    Z = aligned(z.shape, np.float32); Z[...] = z
    lab = aligned((7,), np.int32); lab[...] = labels
    G, D = aligned((7,), np.float32, 1.0), aligned((7, 10), np.float32)

    def ce(**kw):
        a = dict(z=ptr(Z), dt=_lib.Y5_F32, B=7, nc=10, ld=10, lab=ptr(lab), eps=0.1, g=ptr(G), d=ptr(D), ldd=10)
        a.update(kw)
        return lib.y5_classify_ce_bwd(a["z"], a["dt"], a["B"], a["nc"], a["ld"], a["lab"], a["eps"], a["g"], a["d"], a["ldd"], None)

    assert ce() == 0
    for kw in (dict(z=None), dict(lab=None), dict(g=None), dict(d=None), dict(dt=_lib.Y5_I32), dict(B=0), dict(nc=0), dict(ld=9), dict(ldd=9), dict(eps=-0.1),
               dict(eps=1.5), dict(eps=float("nan")), dict(z=C.c_void_p(Z.ctypes.data + 2)), dict(g=C.c_void_p(G.ctypes.data + 2))):
        assert ce(**kw) == BAD, kw
        assert b"classify_ce_bwd" in lib.y5_last_error()
    assert ce(nc=40000, ld=40000, ldd=40000) == UNSUP


# ---- Dropout ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float16, np.float32])
@pytest.mark.parametrize("p", [0.25, 0.5, 1.0])
def test_emu_dropout_matches_the_philox_restatement_forward_and_backward(p, dtype):
    ct.check_dropout(ct.EmuMem(), dtype, p)
    if p == 0.5:
        ct.check_dropout(ct.EmuMem(), dtype, p, shape=(33, 4, 1280, 33))   # more than one workgroup of the mask kernel, B past the tile


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
@pytest.mark.parametrize("shape", [(5, 6, 72, 10), (2, 9, 1280, 1003)])
def test_emu_dropout_zero_is_bit_equal_to_the_inference_head(shape, dtype):
    B, HW, C_, nc = shape
    mem = ct.EmuMem()
    x, w, bias = cr.head_inputs(B, HW, C_, nc, dtype)
    logits, _ = ct.run_head_train(mem, x, w, bias, C_, nc, 0.0, 99)
    assert np.array_equal(logits, ct.run_head_fwd(mem, x, w, bias, C_, nc, form=2))


def test_philox_restatement_known_answers():
    """Random123's known-answer vectors for philox4x32-10 (counter, key all zero / all ones): the restatement is the published algorithm."""
    assert int(ct.philox_word(0, [0])[0]) == 0x6627E8D5
    r = ct.philox_word(0xFFFFFFFFFFFFFFFF, np.array([0xFFFFFFFFFFFFFFFF], np.uint64))
    assert r.dtype == np.uint32   # (counter words 2, 3 are zero in this layout: no published vector; the all-zero one pins the rounds and constants)


# ---- cross-entropy gradient ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float16, np.float32])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("nc", cr.POST_NC)
def test_emu_ce_bwd_within_bound(nc, B, eps, dtype):
    ct.check_ce_bwd(ct.EmuMem(), nc, B, eps, dtype)


@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_emu_ce_function_agrees_with_torch_autograd(emu_seam, eps):
    from yolov5_amd.torch_utils import smartCrossEntropyLoss

    z, labels = cr.post_inputs(5, 10, np.float32)
    labels = torch.from_numpy(labels).long()
    a = torch.from_numpy(z).requires_grad_(True)
    b = torch.from_numpy(z).double().requires_grad_(True)
    la = smartCrossEntropyLoss(eps)(a, labels)
    lb = torch.nn.CrossEntropyLoss(label_smoothing=eps)(b, labels)
    (la * 3.0).backward()
    (lb * 3.0).backward()
    assert abs(float(la.detach()) - float(lb.detach())) < 1e-6 * abs(float(lb.detach()))
    ref, bound = ct.ce_bwd_ref(z, labels.numpy(), eps, np.full(5, 3.0 / 5, np.float32))
    np.testing.assert_allclose(b.grad.numpy(), ref, rtol=1e-7, atol=1e-12)   # the restatement is torch's gradient (3 / 5 is rounded to fp32 in it)
    assert (np.abs(a.grad.double().numpy() - b.grad.numpy()) <= bound).all()
    # logits that need no gradient: the plain forward, no graph
    plain = smartCrossEntropyLoss(eps)(a.detach(), labels)
    assert not plain.requires_grad and float(plain) == float(la.detach())


# ---- whole model -----------------------------------------------------------------------------------------------------------------------------
def test_emu_model_step_fp32_plan_matches_reference_fp64(emu_seam):
    ct.check_model_step("cpu", fp16=False)


def test_emu_model_step_fp16_plan_within_the_fp16_envelope(emu_seam):
    ct.check_model_step("cpu", fp16=True)


def test_emu_eval_after_a_train_step_sees_the_running_statistics(emu_seam):
    ct.check_eval_sees_the_step("cpu")


def test_emu_backward_of_a_stale_forward_raises(emu_seam):
    ct.check_stale_backward("cpu")


def test_emu_dropout_seed_comes_from_torchs_generator_only_when_p_is_positive(emu_seam):
    m = ct.cls_model("cpu")
    x = cr.model_input("sq")
    state = torch.get_rng_state()
    m(x)
    assert torch.equal(torch.get_rng_state(), state)
    m.model[-1].drop.p = 0.5   # read at every forward (classify/train.py:157-158 sets it after construction)
    torch.manual_seed(3)
    state = torch.get_rng_state()
    a = m(x).detach().clone()
    assert not torch.equal(torch.get_rng_state(), state)
    b = m(x).detach().clone()
    torch.manual_seed(3)
    c = m(x).detach().clone()
    assert torch.equal(a, c) and not torch.equal(a, b)


def test_train_mode_forward_of_a_cpu_tensor_without_a_backend_still_refuses():
    m = ct.cls_model("cpu")
    with pytest.raises(NotImplementedError, match="training"):
        m(cr.model_input("sq"))


@pytest.mark.parametrize("name", ["SGD", "Adam"])
def test_emu_train_loop_follows_the_reference_trajectory(emu_seam, name):
    out = ct.check_trajectory("cpu", name)
    assert len(out["tloss"]) == ct.TRAJ_EPOCHS and out["scaler"].skipped == 0 and out["best_fitness"] == 0.0


def test_classification_loader_shuffle_is_seeded_and_off_by_default(emu_seam):
    from yolov5_amd.dataloaders import ClassificationLoader

    frames = [torch.from_numpy(np.ascontiguousarray(cr.source("rect", (40, 40), pad=0)[0])) for _ in range(7)]
    labels = list(range(7))
    plain = [l.tolist() for _, l in ClassificationLoader(frames, labels, imgsz=32, batch_size=3)]
    assert plain == [[0, 1, 2], [3, 4, 5], [6]]
    ld = ClassificationLoader(frames, labels, imgsz=32, batch_size=3, shuffle=True, seed=5)
    e1, e2 = [l.tolist() for _, l in ld], [l.tolist() for _, l in ld]
    assert sorted(sum(e1, [])) == labels and sorted(sum(e2, [])) == labels and e1 != e2 and [len(b) for b in e1] == [3, 3, 1]
    again = ClassificationLoader(frames, labels, imgsz=32, batch_size=3, shuffle=True, seed=5)
    assert [l.tolist() for _, l in again] == e1
