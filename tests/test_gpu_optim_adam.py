"""GPU: the fused Adam / AdamW / RMSProp steps on the MI355X (csrc/optim.hip: y5_mt_adam_step, y5_mt_rmsprop_step) -- the step sequence, the
placement and the overflow rules of tests/optim_adam_ref.py, and both training loops with fused_optimizer=True: the reference's own Adam
trajectory (tests/golden/classify_train.npz), the fp16 classification loop and one detection epoch."""
import copy

import numpy as np
import pytest
import torch

from tests import classify_ref as cr
from tests import classify_train_ref as ct
from tests import optim_adam_ref as oa

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", oa.MODES)
@pytest.mark.parametrize("kind", list(oa.KINDS))
def test_gpu_fused_step_matches_torch_sequence(kind, mode):
    """Against torch.optim.* on the same GPU with its default implementation.  torch's GPU kernels may contract to FMA, so the fp64
    restatement of the sequence is the yardstick for both: per tensor the kernel is allowed the larger of the project tolerance and twice
    torch's own largest deviation from the fp64 sequence (figures: DESIGN.md, optimizer section)."""
    oa.check_sequence(kind, mode, "cuda", None, vs_fp64=True)


@pytest.mark.parametrize("kind", list(oa.KINDS))
def test_gpu_aligned_and_offset_placements_give_the_same_bits(kind):
    oa.check_alignment(kind, "cuda", None)


@pytest.mark.parametrize("kind", list(oa.KINDS))
def test_gpu_non_finite_gradient_skips_update_and_step_count_but_not_the_ema(kind):
    oa.check_non_finite(kind, "cuda", None)


def test_gpu_classification_trajectory_with_fused_adam_follows_the_reference():
    """The rule of tests/classify_train_ref.py:check_trajectory on the reference's own Adam run (fixture c_Adam_*): lr exact; losses and the
    final linear.bias of model and EMA within 4 x the largest deviation of the reference's fp32 run from its fp64 run."""
    from yolov5_amd import classify_train
    from yolov5_amd.torch_utils import HipAdam

    g = ct.golden()
    m = ct.cls_model("cuda")
    out = classify_train.train(m, ct.traj_loader("cuda"), None, epochs=ct.TRAJ_EPOCHS, optimizer_name="Adam", fused_optimizer=True, amp=False,
                               ema=True, **ct.TRAJ_ARGS)
    assert type(out["optimizer"]) is HipAdam and float(out["optimizer"]._step) == 2 * ct.TRAJ_EPOCHS
    pre = "c_Adam_64_"
    np.testing.assert_allclose(np.array(out["lr"]), g[pre + "lr"], rtol=1e-15, atol=0)
    got = dict(losses=out["losses"].double().numpy(), bias=m.model[9].linear.bias.detach().double().cpu().numpy(),
               ema_bias=out["ema"].ema.model[9].linear.bias.detach().double().cpu().numpy())
    ratios = {}
    for k, v in got.items():
        noise = float(np.abs(g[f"c_Adam_32_{k}"] - g[pre + k]).max())
        allowed = 4 * noise if noise > 0 else 1e-4 * float(np.abs(g[pre + k]).max())
        ratios[k] = float(np.abs(v - g[pre + k]).max()) / allowed
    print(f"trajectory fused Adam: deviation from the fp64 reference / allowed = {ratios}; losses {got['losses']}")
    assert all(r <= 1.0 for r in ratios.values()), ratios


@pytest.mark.parametrize("name", ["Adam", "RMSProp"])
def test_gpu_train_loop_fp16_two_epochs_fused(name, tmp_path):
    """tests/test_gpu_classify_train.py:test_gpu_train_loop_fp16_two_epochs with fused_optimizer=True."""
    from yolov5_amd import classify_train
    from yolov5_amd.experimental import attempt_load

    m = ct.cls_model("cuda")
    m.model[-1].drop.p = 0.1
    torch.manual_seed(0)
    start = copy.deepcopy(m.state_dict())
    loader = ct.traj_loader("cuda")
    seen = []
    out = classify_train.train(m, loader, loader, epochs=2, optimizer_name=name, fused_optimizer=True, amp=True, ema=True, save_dir=tmp_path,
                               **ct.TRAJ_ARGS, on_batch_end=lambda ni, loss, opt: seen.append(m.model[9].linear.bias.detach().clone()))
    assert hasattr(out["optimizer"], "step_fused")
    losses = out["losses"]
    assert losses.shape == (4,) and torch.isfinite(losses).all(), losses
    prev, moved = start["model.9.linear.bias"], 0
    for b in seen:
        moved += int(not torch.equal(b, prev))
        prev = b
    print(f"train loop fused {name}: losses {losses.tolist()}, scale {out['scaler'].scale}, skipped {out['scaler'].skipped}, top1 {out['top1']}")
    assert moved == 4 - out["scaler"].skipped and moved >= 1
    assert float(out["optimizer"]._step) == moved   # the device count advanced with the steps taken, and only with them
    ema = out["ema"]
    assert ema.updates == 4 and not torch.equal(ema.ema.state_dict()["model.9.linear.bias"], start["model.9.linear.bias"])
    assert (tmp_path / "last.pt").is_file() and (tmp_path / "best.pt").is_file()
    loaded = attempt_load(tmp_path / "best.pt", device="cuda")
    ref = copy.deepcopy(ema.ema).cpu().half().float().fuse().eval().cuda()
    x = loader[0][0]
    with torch.no_grad():
        za, zb = loaded(x), ref(x)
    assert za.shape == (2, cr.MODEL_NC) and torch.equal(za, zb)


def test_gpu_detection_epoch_with_fused_adamw_and_the_eval_plan_sees_it():
    """train_loop.train(optimizer_name="AdamW", fused_optimizer=True), one epoch of two batches: finite losses, moved parameters, and the
    model's cached eval plan picks up the weights the kernel wrote through raw pointers (bump_weights_epoch): its output equals that of a
    deep copy, whose plan is new."""
    from oracle import train_oracle as to, yolo_oracle as yo
    from yolov5_amd.torch_utils import HipAdamW
    from yolov5_amd.train_loop import TensorLoader, train
    from yolov5_amd.yolo import DetectionModel

    dev = torch.device("cuda:0")
    m = DetectionModel("yolov5n.yaml")
    m.load_state_dict(yo.det_state_dict(yo.model_cfg("yolov5n"), 0, fused=False))
    m = m.to(dev)
    imgs, tpi = to.synthetic_set(4, 64, per_img=2, seed=1)
    x = imgs[:2].to(dev).float() / 255
    with torch.no_grad():
        z0 = m.eval()(x)[0].clone()          # the eval plan exists before the step
    before = [p.detach().clone() for p in m.parameters()]
    res = train(m, TensorLoader(imgs.to(dev), [t.to(dev) for t in tpi], 2), hyp=dict(to.HYP), epochs=1, device=dev, amp=True, nbs=2,
                optimizer_name="AdamW", fused_optimizer=True)
    opt = res["optimizer"]
    assert type(opt) is HipAdamW and res["losses"].shape == (2, 3) and torch.isfinite(res["losses"]).all()
    taken = 2 - res["scaler"].skipped
    assert taken >= 1 and float(opt._step) == taken and res["ema"].updates == 2
    # (the warm-up starts the two weight groups at lr 0, train.py:383-385: after two iterations it is the bias group that has certainly moved)
    assert sum(int(not torch.equal(a, p)) for a, p in zip(before, m.parameters())) >= 1
    with torch.no_grad():
        z1 = m.eval()(x)[0].clone()
        fresh = copy.deepcopy(m).eval()(x)[0]
    assert torch.isfinite(z1).all() and not torch.equal(z1, z0) and torch.equal(z1, fresh)
