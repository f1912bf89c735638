"""GPU: classification training on the MI355X -- the kernels of yolov5_amd/csrc/classify_train.h at the shapes of the emulator tests, the two
whole-model gradient checks on tests/golden/classify_train.npz, and yolov5_amd/classify_train.train end to end (fp16 plan, SGD through
HipSGD.step_fused and Adam through host_amp_step, checkpoints, validation between epochs).  Rules: tests/classify_train_ref.py."""
import copy

import numpy as np
import pytest
import torch

from tests import classify_ref as cr
from tests import classify_train_ref as ct

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
@pytest.mark.parametrize("shape", ct.BWD_SHAPES)
def test_gpu_head_bwd_within_bounds_and_deterministic(shape, dtype):
    ct.check_head_bwd(ct.GpuMem(), shape, dtype)


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
@pytest.mark.parametrize("p", [0.25, 0.5, 1.0])
def test_gpu_dropout_matches_the_philox_restatement_forward_and_backward(p, dtype):
    ct.check_dropout(ct.GpuMem(), dtype, p)
    if p == 0.5:
        ct.check_dropout(ct.GpuMem(), dtype, p, shape=(33, 4, 1280, 33))


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
@pytest.mark.parametrize("shape", [(5, 6, 72, 10), (2, 9, 1280, 1003)])
def test_gpu_dropout_zero_is_bit_equal_to_the_inference_head(shape, dtype):
    B, HW, C_, nc = shape
    mem = ct.GpuMem()
    x, w, bias = cr.head_inputs(B, HW, C_, nc, dtype)
    logits, _ = ct.run_head_train(mem, x, w, bias, C_, nc, 0.0, 99)
    assert np.array_equal(logits, ct.run_head_fwd(mem, x, w, bias, C_, nc, form=2))


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
@pytest.mark.parametrize("nc", cr.POST_NC)
def test_gpu_ce_bwd_within_bound(nc, dtype):
    for B in (1, 5):
        for eps in (0.0, 0.1):
            ct.check_ce_bwd(ct.GpuMem(), nc, B, eps, dtype)


def test_gpu_model_step_fp32_plan_matches_reference_fp64():
    ct.check_model_step("cuda", fp16=False)


def test_gpu_model_step_fp16_plan_within_the_fp16_envelope():
    ct.check_model_step("cuda", fp16=True)


def test_gpu_eval_after_a_train_step_and_stale_backward():
    ct.check_eval_sees_the_step("cuda")
    ct.check_stale_backward("cuda")


@pytest.mark.parametrize("name", ["SGD", "Adam"])
def test_gpu_train_loop_fp16_two_epochs(name, tmp_path):
    from yolov5_amd import classify_train
    from yolov5_amd.experimental import attempt_load

    m = ct.cls_model("cuda")
    m.model[-1].drop.p = 0.1   # Dropout on: the mask kernel and its backward ride along
    torch.manual_seed(0)
    start = copy.deepcopy(m.state_dict())
    loader = ct.traj_loader("cuda")
    seen = []
    out = classify_train.train(m, loader, loader, epochs=2, optimizer_name=name, amp=True, ema=True, save_dir=tmp_path, **ct.TRAJ_ARGS,
                               on_batch_end=lambda ni, loss, opt: seen.append(m.model[9].linear.bias.detach().clone()))
    assert hasattr(out["optimizer"], "step_fused") == (name == "SGD")
    losses = out["losses"]
    assert losses.shape == (4,) and torch.isfinite(losses).all(), losses
    assert len(out["tloss"]) == len(out["vloss"]) == len(out["top1"]) == len(out["lr"]) == 2 and all(np.isfinite(out["vloss"]))
    # every step either moved the parameters or is counted as skipped by the loss scaler
    prev, moved = start["model.9.linear.bias"], 0
    for b in seen:
        moved += int(not torch.equal(b, prev))
        prev = b
    print(f"train loop {name}: losses {losses.tolist()}, scale {out['scaler'].scale}, skipped {out['scaler'].skipped}, top1 {out['top1']}")
    assert moved == 4 - out["scaler"].skipped and moved >= 1
    ema = out["ema"]
    assert ema.updates == 4 and not torch.equal(ema.ema.state_dict()["model.9.linear.bias"], start["model.9.linear.bias"])
    # best.pt: the fp16 copy of the EMA, reloaded, gives the logits of the EMA taken through the same fp16 round trip -- bit for bit
    assert (tmp_path / "last.pt").is_file() and (tmp_path / "best.pt").is_file()
    loaded = attempt_load(tmp_path / "best.pt", device="cuda")
    ref = copy.deepcopy(ema.ema).cpu().half().float().fuse().eval().cuda()
    x = loader[0][0]
    with torch.no_grad():
        za, zb = loaded(x), ref(x)
    assert za.shape == (2, cr.MODEL_NC) and torch.equal(za, zb)


def test_gpu_train_validate_train_again_sees_the_refreshed_weights():
    """Without an EMA the loop validates the live model between epochs: its cached eval plan must pick up the Linear weights (and every other
    parameter) the fused step wrote through raw pointers -- the validation loss equals that of a fresh copy of the model, whose plan is new."""
    from yolov5_amd import classify_train, classify_val
    from yolov5_amd.torch_utils import smartCrossEntropyLoss

    m = ct.cls_model("cuda")
    loader = ct.traj_loader("cuda")
    out = classify_train.train(m, loader, loader, epochs=2, optimizer_name="SGD", lr0=0.05, amp=True, ema=False)
    assert out["vloss"][0] != out["vloss"][1] and all(np.isfinite(out["vloss"]))
    fresh = classify_val.run(copy.deepcopy(m), loader, criterion=smartCrossEntropyLoss(0.1))
    assert fresh[2] == out["vloss"][1], (fresh, out["vloss"])
    assert m.training is False   # (validation left it in eval mode, as classify/val.py does; the loop's next epoch would call train())
