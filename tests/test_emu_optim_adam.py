"""CPU: the fused Adam / AdamW / RMSProp steps (csrc/optim.hip: y5_mt_adam_step, y5_mt_rmsprop_step, host-compiled on the HIP emulator;
torch_utils.HipAdam / HipAdamW / HipRMSprop) against the reference's own step sequence with the torch optimizers smart_optimizer offers
(train.py:413-421, utils/torch_utils.py:257-290, 343-369).  Rules and tolerance: tests/optim_adam_ref.py."""
import copy

import pytest
import torch

from tests import optim_adam_ref as oa
from tests.hipemu import backend as emu_backend
from tests.hipemu.emu import emu
from yolov5_amd.torch_utils import HipAdam, HipAdamW, HipRMSprop, HipSGD, ModelEMA, smart_optimizer


@pytest.mark.parametrize("mode", oa.MODES)
@pytest.mark.parametrize("kind", list(oa.KINDS))
def test_fused_step_matches_torch_sequence(kind, mode):
    oa.check_sequence(kind, mode, "cpu", emu())


@pytest.mark.parametrize("kind", list(oa.KINDS))
def test_aligned_and_offset_placements_give_the_same_bits(kind):
    oa.check_alignment(kind, "cpu", emu())


@pytest.mark.parametrize("kind", list(oa.KINDS))
def test_non_finite_gradient_skips_update_and_step_count_but_not_the_ema(kind):
    oa.check_non_finite(kind, "cpu", emu())


def test_fused_ema_matches_model_ema_update():
    """step_fused(ema=, model=) against torch.optim.Adam.step() + ModelEMA.update, BatchNorm running statistics moving in between."""
    m_ref = oa.make_net(2)
    x = torch.randn(4, 7, 3, 3, generator=torch.Generator().manual_seed(2))
    m_hip = copy.deepcopy(m_ref)
    ema_ref, ema_hip = ModelEMA(m_ref, tau=3), ModelEMA(m_hip, tau=3)
    opt_ref = oa.ref_optimizer(m_ref, "Adam", foreach=False)
    opt_hip = oa.hip_optimizer(m_hip, "Adam", emu())
    for step in range(3):
        for mm in (m_ref, m_hip):   # float buffers are part of the EMA
            mm.train()
            mm.b1(x * (step + 1))
        for p, q, g in zip(m_ref.parameters(), m_hip.parameters(), oa.grads(m_ref, 20 + step)):
            p.grad, q.grad = g.clone(), g.clone()
        opt_ref.step()
        ema_ref.update(m_ref)
        opt_hip.step_fused(ema=ema_hip, model=m_hip)
        assert ema_hip.updates == ema_ref.updates
        for (k, a), b in zip(ema_ref.ema.state_dict().items(), ema_hip.ema.state_dict().values()):
            if a.dtype.is_floating_point:
                torch.testing.assert_close(b, a, rtol=oa.RTOL, atol=oa.ATOL, msg=lambda s: f"step {step} {k}: {s}")
            else:
                assert torch.equal(a, b)
    assert not torch.equal(ema_hip.ema.b1.running_mean, torch.zeros(7))


def _load(model, seed):
    for p, g in zip(model.parameters(), oa.grads(model, seed)):
        p.grad = g.clone()


def _close(ma, mb, tag):
    for (n, p), q in zip(ma.named_parameters(), mb.parameters()):
        torch.testing.assert_close(p, q, rtol=oa.RTOL, atol=oa.ATOL, msg=lambda s: f"{tag} {n}: {s}")


@pytest.mark.parametrize("kind", ["Adam", "AdamW", "RMSProp"])
def test_state_dicts_travel_both_ways(kind):
    # ours -> torch: two steps here, two more in both
    m_a = oa.make_net(4)
    ours = oa.hip_optimizer(m_a, kind, emu())
    for s in range(2):
        oa.set_lrs(ours, s)
        _load(m_a, 30 + s)
        ours.step()
    sd = ours.state_dict()
    assert all(st["step"].device.type == "cpu" and float(st["step"]) == 2.0 for st in sd["state"].values())
    assert len({id(st["step"]) for st in sd["state"].values()}) == len(sd["state"])   # torch's layout: a tensor per parameter
    assert set(sd["state"][0]) == set(oa.state_names(kind)) | {"step"}
    m_b = copy.deepcopy(m_a)
    theirs = oa.ref_optimizer(m_b, kind, foreach=False)
    theirs.load_state_dict(copy.deepcopy(sd))
    for s in range(2, 4):
        for o, m in ((ours, m_a), (theirs, m_b)):
            oa.set_lrs(o, s)
            _load(m, 30 + s)
            o.step()
    assert all(float(theirs.state[p]["step"]) == 4.0 for p in m_b.parameters()) and float(ours._step) == 4.0
    _close(m_a, m_b, f"{kind} ours -> torch")
    # torch -> ours: host `step` tensors are adopted into the one device count
    m_c = copy.deepcopy(m_b)
    again = oa.hip_optimizer(m_c, kind, emu())
    again.load_state_dict(copy.deepcopy(theirs.state_dict()))
    assert float(again._step) == 4.0 and all(again.state[p]["step"] is again._step for p in m_c.parameters())
    for s in range(4, 6):
        for o, m in ((theirs, m_b), (again, m_c)):
            oa.set_lrs(o, s)
            _load(m, 30 + s)
            o.step()
    assert float(again._step) == 6.0
    _close(m_b, m_c, f"{kind} torch -> ours")
    for k in oa.state_names(kind):
        for p, q in zip(m_b.parameters(), m_c.parameters()):
            torch.testing.assert_close(again.state[q][k], theirs.state[p][k], rtol=oa.RTOL, atol=oa.ATOL)
    # unequal counts cannot become one count
    bad = copy.deepcopy(theirs.state_dict())
    bad["state"][1]["step"] = torch.tensor(9.0)
    with pytest.raises(ValueError, match="step"):
        oa.hip_optimizer(copy.deepcopy(m_b), kind, emu()).load_state_dict(bad)


def test_checkpoint_round_trip_with_hip_adam(tmp_path):
    from oracle import yolo_oracle as yo
    from oracle.make_golden import TINY_CFG
    from yolov5_amd.checkpoint import load_checkpoint, save_checkpoint, smart_resume
    from yolov5_amd.yolo import DetectionModel

    def model():
        torch.manual_seed(3)
        m = DetectionModel(dict(TINY_CFG))
        m.hyp = dict(yo.HYP_SCRATCH_LOW)
        m.names = {i: str(i) for i in range(80)}
        return m

    emu_backend.install()
    try:
        m = model()
        opt = smart_optimizer(m, "Adam", lr=1e-3, momentum=0.9, decay=5e-4, fused=True)
        assert isinstance(opt, HipAdam)
        ema = ModelEMA(m)
        g = torch.Generator().manual_seed(8)
        for _ in range(2):
            for p in m.parameters():
                p.grad = torch.randn(p.shape, generator=g) * 0.02
            opt.step_fused(max_norm=10.0, ema=ema, model=m)
        path = tmp_path / "last.pt"
        save_checkpoint(path, m, ema=ema, optimizer=opt, epoch=1, best_fitness=0.25)
        ck = load_checkpoint(path)
        m2 = model()
        opt2 = smart_optimizer(m2, "Adam", lr=1e-3, momentum=0.9, decay=5e-4, fused=True)
        ema2 = ModelEMA(m2)
        best, start, epochs = smart_resume(ck, opt2, ema2, weights=str(path), epochs=10, resume=True)
        assert (best, start, epochs) == (0.25, 2, 10) and ema2.updates == 2
        assert float(opt2._step) == 2.0
        for p, q in zip(m.parameters(), m2.parameters()):
            assert opt2.state[q]["step"] is opt2._step
            for k in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(opt.state[p][k], opt2.state[q][k])
    finally:
        emu_backend.uninstall()


def test_unsupported_settings_raise_at_construction():
    p = [torch.nn.Parameter(torch.zeros(3))]
    for cls in (HipAdam, HipAdamW):
        for flag in ("amsgrad", "maximize", "foreach", "capturable", "differentiable"):
            with pytest.raises(ValueError, match=flag):
                cls(p, **{flag: True})
    for flag in ("centered", "maximize", "foreach", "capturable", "differentiable"):
        with pytest.raises(ValueError, match=flag):
            HipRMSprop(p, **{flag: True})
    q = [torch.nn.Parameter(torch.zeros(2))]
    with pytest.raises(ValueError, match="betas"):
        HipAdam([{"params": p}, {"params": q, "betas": (0.8, 0.999)}])
    with pytest.raises(ValueError, match="eps"):
        HipAdamW([{"params": p}, {"params": q, "eps": 1e-6}])
    with pytest.raises(ValueError, match="alpha"):
        HipRMSprop([{"params": p}, {"params": q, "alpha": 0.9}])
    with pytest.raises(ValueError, match="momentum"):
        HipRMSprop([{"params": p}, {"params": q, "momentum": 0.5}])
    ok = HipAdam([{"params": p}, {"params": q, "lr": 0.5, "weight_decay": 0.1}])   # lr and weight_decay are per group
    with pytest.raises(ValueError, match="betas"):
        ok.add_param_group({"params": [torch.nn.Parameter(torch.zeros(1))], "betas": (0.5, 0.5)})
    with pytest.raises(ValueError, match="4 parameter groups"):
        five = HipAdam([{"params": [torch.nn.Parameter(torch.zeros(2))]} for _ in range(5)], lib=emu())
        for g in five.param_groups:
            g["params"][0].grad = torch.zeros(2)
        five.step()


def test_smart_optimizer_returns_the_fused_classes_only_when_asked():
    m = oa.make_net(0)
    assert type(smart_optimizer(m, "Adam")) is torch.optim.Adam
    assert type(smart_optimizer(m, "AdamW")) is torch.optim.AdamW
    assert type(smart_optimizer(m, "RMSProp")) is torch.optim.RMSprop
    assert type(smart_optimizer(m, "SGD", fused=True)) is HipSGD
    sizes = [len(g) for g in (oa.groups_of(m)[2], oa.groups_of(m)[0], oa.groups_of(m)[1])]
    for name, cls in (("Adam", HipAdam), ("AdamW", HipAdamW), ("RMSProp", HipRMSprop)):
        opt = smart_optimizer(m, name, lr=0.002, momentum=0.8, decay=3e-4, fused=True)
        ref = smart_optimizer(m, name, lr=0.002, momentum=0.8, decay=3e-4)
        assert type(opt) is cls and hasattr(opt, "step_fused")
        assert [len(g["params"]) for g in opt.param_groups] == sizes == [len(g["params"]) for g in ref.param_groups]
        assert [g["weight_decay"] for g in opt.param_groups] == [0.0, 3e-4, 0.0]
        for go, gr in zip(opt.param_groups, ref.param_groups):   # the reference's hyper-parameters, key by key as torch holds them
            assert {k: v for k, v in go.items() if k != "params"} == {k: v for k, v in gr.items() if k != "params"}
        if name != "RMSProp":
            assert opt.param_groups[0]["betas"] == (0.8, 0.999)
        else:
            assert opt.param_groups[0]["momentum"] == 0.8


def test_detection_loop_passes_the_flag_on():
    """train_loop.train(fused_optimizer=True): the optimizer is the fused class, its device count advanced with the step and the parameters
    moved (emulator backend, the small model of tests/test_loops.py)."""
    from oracle import train_oracle as to, yolo_oracle as yo
    from oracle.make_golden import TINY_CFG
    from yolov5_amd import train_loop
    from yolov5_amd.yolo import DetectionModel

    emu_backend.install()
    try:
        m = DetectionModel(copy.deepcopy(TINY_CFG))
        m.load_state_dict(yo.det_state_dict(copy.deepcopy(TINY_CFG), 2, fused=False))
        before = [p.detach().clone() for p in m.parameters()]
        imgs, tpi = to.synthetic_set(2, 64, per_img=2, seed=4)
        res = train_loop.train(m, train_loop.TensorLoader(imgs, tpi, 2), hyp=dict(to.HYP), epochs=1, device="cpu", amp=True, nbs=2,
                               optimizer_name="AdamW", fused_optimizer=True)
        assert type(res["optimizer"]) is HipAdamW and float(res["optimizer"]._step) == 1.0 and res["ema"].updates == 1
        assert any(not torch.equal(a, p) for a, p in zip(before, m.parameters()))
    finally:
        emu_backend.uninstall()


def test_classification_loop_passes_the_flag_on():
    """classify_train.train(fused_optimizer=True), one batch on the emulator backend with the model of tests/classify_train_ref.py."""
    from tests import classify_train_ref as ct
    from yolov5_amd import classify_train

    emu_backend.install()
    try:
        c = ct.cls_model("cpu")
        bias = c.model[9].linear.bias.detach().clone()
        out = classify_train.train(c, ct.traj_loader("cpu")[:1], None, epochs=1, optimizer_name="RMSProp", amp=False, ema=True, fused_optimizer=True,
                                   **ct.TRAJ_ARGS)
        assert type(out["optimizer"]) is HipRMSprop and float(out["optimizer"]._step) == 1.0 and out["ema"].updates == 1
        assert not torch.equal(bias, c.model[9].linear.bias)
    finally:
        emu_backend.uninstall()
