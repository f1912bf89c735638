"""Shared rules of tests/test_emu_optim_adam.py (kernel sources on the emulator, CPU tensors) and tests/test_gpu_optim_adam.py (MI355X):
HipAdam / HipAdamW / HipRMSprop (yolov5_amd/torch_utils.py on y5_mt_adam_step / y5_mt_rmsprop_step, csrc/optim.hip) against the
reference's step sequence train.py:413-421 with the torch optimizers of utils/torch_utils.py:257-290:
GradScaler.unscale_ -> clip_grad_norm_(10.0) -> torch.optim.{Adam, AdamW, RMSprop}.step() -> ModelEMA.update.

Tolerance: the project's rtol 2e-6 / atol 1e-7 (tests/test_emu_optim.py).  A separately rounded fp32 restatement of the three rules stays
within 4.5e-8 absolute of torch 2.10's CPU step over six steps at these magnitudes (|w| <= 0.5, gradients 0.02 N(0,1), lr 1e-3); it is not
bit-equal (torch's lerp and addcdiv round differently), so nothing here asserts equality with torch."""
import copy

import numpy as np
import torch
from torch import nn

from yolov5_amd.torch_utils import HipAdam, HipAdamW, HipRMSprop, ModelEMA, smart_optimizer

RTOL, ATOL = 2e-6, 1e-7
MODES = ("plain", "scaled_clipped", "scaled_not_clipped")
# kind -> (smart_optimizer name, torch class, momentum argument of smart_optimizer, our class)
KINDS = {
    "Adam": ("Adam", torch.optim.Adam, 0.9, HipAdam),
    "AdamW": ("AdamW", torch.optim.AdamW, 0.9, HipAdamW),
    "RMSProp": ("RMSProp", torch.optim.RMSprop, 0.9, HipRMSprop),
    "RMSProp0": ("RMSProp", torch.optim.RMSprop, 0.0, HipRMSprop),
}
LR, DECAY = 1e-3, 5e-4


class Net(nn.Module):
    """Parameter sizes 1, 7, 16384, 16385 and 24000 among others: a single element, a tail shorter than a vector, exactly one 16384-element
    chunk, a chunk plus one, two chunks.  Biases, BatchNorm weights and other weights: the three smart_optimizer groups."""

    def __init__(self):
        super().__init__()
        self.c2 = nn.Conv2d(24, 40, 5)            # 24000 + 40
        self.b1 = nn.BatchNorm2d(7)               # 7 + 7
        self.l1 = nn.Linear(128, 128)             # 16384 + 128
        self.l2 = nn.Linear(16385, 1)             # 16385 + 1


def signs(model):
    sg = torch.Generator().manual_seed(777)
    return [torch.where(torch.rand(p.shape, generator=sg) < 0.5, -1.0, 1.0) for p in model.parameters()]


def make_net(seed, device="cpu"):
    """0.05 <= |w| <= 0.5, with the sign of the element's gradients (see grads): weight decay then never turns the sign of grad + wd * w."""
    m = Net()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p, sign in zip(m.parameters(), signs(m)):
            p.copy_((0.05 + 0.45 * torch.rand(p.shape, generator=g)) * sign)
    assert sorted(p.numel() for p in m.parameters()) == [1, 7, 7, 40, 128, 16384, 16385, 24000]
    return m.to(device)


def grads(model, seed, scale=1.0, big=False):
    """0.02 |N(0,1)| (30 |N(0,1)| for the clipped mode) times a sign that is random per element and the SAME at every step.
    Why the sign is kept: RMSProp's momentum_buffer adds d / avg, about +-10 per step here (avg = sqrt(0.01 d^2) after the first step), where one
    ulp is 1e-6.  torch's CPU kernels round those addends their own way (addcmul is one FMA, sqrt is the vector library's: 1191 and 160 of
    24000 elements differ by an ulp from the separately rounded form csrc/optim.hip is asked to compute), so a buffer element whose addends
    cancel would carry an absolute difference of 1e-6 against a result near zero -- ten times the atol, which is sized for values up to 0.5.
    With a steady sign the buffer is a sum of like-signed terms and the comparison stays relative, as it is for every other tensor."""
    g = torch.Generator().manual_seed(seed)
    dev = next(model.parameters()).device
    return [(torch.randn(p.shape, generator=g).abs() * sign * (30.0 if big else 0.02) * scale).to(dev) for p, sign in zip(model.parameters(), signs(model))]


def groups_of(model):
    g = [], [], []
    for v in model.modules():
        for n, p in v.named_parameters(recurse=0):
            (g[2] if n == "bias" else g[1] if isinstance(v, nn.BatchNorm2d) else g[0]).append(p)
    return g


def ref_optimizer(model, kind, **kw):
    """utils/torch_utils.py:257-290 with torch's own optimizers (kw: foreach=False on the CPU -- torch's single-tensor order)."""
    name, cls, momentum, _ = KINDS[kind]
    g = groups_of(model)
    if name == "Adam":
        opt = cls(g[2], lr=LR, betas=(momentum, 0.999), **kw)
    elif name == "AdamW":
        opt = cls(g[2], lr=LR, betas=(momentum, 0.999), weight_decay=0.0, **kw)
    else:
        opt = cls(g[2], lr=LR, momentum=momentum, **kw)
    opt.add_param_group({"params": g[0], "weight_decay": DECAY})
    opt.add_param_group({"params": g[1], "weight_decay": 0.0})
    return opt


def hip_optimizer(model, kind, lib=None):
    name, _, momentum, cls = KINDS[kind]
    opt = smart_optimizer(model, name, lr=LR, momentum=momentum, decay=DECAY, fused=True)
    assert type(opt) is cls
    opt._lib = lib
    return opt


def set_lrs(opt, step):
    for i, g in enumerate(opt.param_groups):  # every group on its own schedule, another value at every step
        g["lr"] = LR * (1.0 + 0.3 * i) / (1 + step)


def state_names(kind):
    return ("exp_avg", "exp_avg_sq") if kind.startswith("Adam") else ("square_avg", "momentum_buffer") if kind == "RMSProp" else ("square_avg",)


class Ref64:
    """The same sequence in fp64 (the yardstick for torch's own GPU kernels, which may contract to FMA): unscale, clip, the rule of
    include/yolov5_hip.h for y5_mt_adam_step / y5_mt_rmsprop_step."""

    def __init__(self, model, kind):
        self.kind = kind
        self.p = [p.detach().double().cpu().clone() for p in model.parameters()]
        self.s = {k: [torch.zeros_like(p) for p in self.p] for k in state_names(kind)}
        gid = {id(p): i for i, grp in enumerate((groups_of(model)[2], groups_of(model)[0], groups_of(model)[1])) for p in grp}
        self.group = [gid[id(p)] for p in model.parameters()]
        self.wd = [0.0, DECAY, 0.0]
        self.t = 0

    def step(self, gs, inv_scale, max_norm, lrs):
        d = [g.detach().double().cpu() * inv_scale for g in gs]
        if max_norm > 0:
            total = float(torch.sqrt(sum((x * x).sum() for x in d)))
            coef = min(1.0, max_norm / (total + 1e-6))
            d = [x * coef for x in d]
        self.t += 1
        t, mu = self.t, KINDS[self.kind][2]
        for i, (w, g) in enumerate(zip(self.p, d)):
            lr, wd = lrs[self.group[i]], self.wd[self.group[i]]
            if self.kind == "AdamW":
                w *= 1 - lr * wd
            else:
                g = g + wd * w
            if self.kind.startswith("Adam"):
                b1, b2, eps = mu, 0.999, 1e-8
                m, v = self.s["exp_avg"][i], self.s["exp_avg_sq"][i]
                m += (g - m) * (1 - b1)
                v.mul_(b2).add_((1 - b2) * g * g)
                w += -(lr / (1 - b1 ** t)) * (m / (v.sqrt() / (1 - b2 ** t) ** 0.5 + eps))
            else:
                v = self.s["square_avg"][i]
                v.mul_(0.99).add_(0.01 * g * g)
                avg = v.sqrt() + 1e-8
                if mu > 0:
                    buf = self.s["momentum_buffer"][i]
                    buf.mul_(mu).add_(g / avg)
                    w -= lr * buf
                else:
                    w += -lr * (g / avg)


def check_sequence(kind, mode, device="cpu", lib=None, vs_fp64=False):
    """Four steps of ours against torch on deep copies of one model; parameters, both state tensors, `step` and stats[0] after every step.
    vs_fp64 (GPU: torch's default implementation): per tensor the allowance is the larger of the project tolerance and twice torch's own
    largest deviation from the fp64 sequence.  Returns (largest deviation of ours, of torch) from fp64 when vs_fp64."""
    m_ref = make_net(0, device)
    m_hip = copy.deepcopy(m_ref)
    opt_ref = ref_optimizer(m_ref, kind, **({} if vs_fp64 else {"foreach": False}))
    opt_hip = hip_optimizer(m_hip, kind, lib)
    assert [len(g["params"]) for g in opt_hip.param_groups] == [len(g["params"]) for g in opt_ref.param_groups]
    assert [g["weight_decay"] for g in opt_hip.param_groups] == [g["weight_decay"] for g in opt_ref.param_groups] == [0.0, DECAY, 0.0]
    r64 = Ref64(m_ref, kind) if vs_fp64 else None
    S = 1.0 if mode == "plain" else 1024.0
    big = mode == "scaled_clipped"
    worst = [0.0, 0.0]
    for step in range(4):
        set_lrs(opt_ref, step)
        set_lrs(opt_hip, step)
        gs = grads(m_ref, 10 + step, S, big)
        for p, q, g in zip(m_ref.parameters(), m_hip.parameters(), gs):
            p.grad, q.grad = g.clone(), g.clone()
        if r64 is not None:
            r64.step(gs, 1.0 / S, 0.0 if mode == "plain" else 10.0, [g["lr"] for g in opt_ref.param_groups])
        if mode != "plain":
            for p in m_ref.parameters():
                p.grad.mul_(1.0 / S)
            norm_ref = torch.nn.utils.clip_grad_norm_(m_ref.parameters(), max_norm=10.0)
        opt_ref.step()
        stats = opt_hip.step_fused(inv_scale=1.0 / S, max_norm=10.0) if mode != "plain" else opt_hip.step()
        if mode != "plain":
            np.testing.assert_allclose(float(stats[0]), float(norm_ref), rtol=2e-6)
            assert float(stats[2]) == 0.0
            assert (float(stats[1]) < 1.0) == big
        else:
            assert stats is None
        for i, ((n, p), q) in enumerate(zip(m_ref.named_parameters(), m_hip.parameters())):
            sr, sh = opt_ref.state[p], opt_hip.state[q]
            assert set(sh) == set(sr) == set(state_names(kind)) | {"step"}, (set(sh), set(sr))
            assert sh["step"] is opt_hip._step and sh["step"].dim() == 0 and sh["step"].device == q.device
            assert float(sh["step"]) == float(sr["step"]) == step + 1
            pairs = [("param", q.detach(), p.detach(), r64.p[i] if r64 else None)]
            pairs += [(k, sh[k], sr[k], r64.s[k][i] if r64 else None) for k in state_names(kind)]
            for tag, ours, theirs, exact in pairs:
                allowed = ATOL + RTOL * theirs.abs()
                if exact is not None:
                    dev_t = float((theirs.double().cpu() - exact).abs().max())
                    dev_o = float((ours.double().cpu() - exact).abs().max())
                    worst = [max(worst[0], dev_o), max(worst[1], dev_t)]
                    allowed = torch.clamp(allowed, min=2 * dev_t)
                bad = (ours - theirs).abs() > allowed
                assert not bool(bad.any()), (f"{kind} {mode} step {step} {n} {tag}: {int(bad.sum())} of {bad.numel()} beyond the allowance, "
                                             f"largest difference {float((ours - theirs).abs().max()):.3e}")
    if vs_fp64:
        print(f"{kind} {mode}: largest deviation from the fp64 sequence -- kernel {worst[0]:.3e}, torch {worst[1]:.3e}")
    return worst


class PlainEma:
    """The four members of ModelEMA that step_fused uses, over explicitly placed tensors (the alignment test chooses every address)."""

    def __init__(self, pairs, d=0.9):
        self.pairs, self.d, self.updates = pairs, d, 0

    def decay(self, x):
        return self.d

    def param_pairs(self, model):
        return self.pairs

    def lerp_rest(self, model, d, lib, stream, skip=()):
        pass


def check_alignment(kind, device="cpu", lib=None):
    """Same values once in tensors of their own (16-byte aligned: the 16-byte path) and once as views at element offsets 1, 2 and 3 of
    larger buffers (the 4-byte path), parameter / gradient / states / EMA offset independently: bit-identical results, and nothing
    outside the views is written."""
    _, _, momentum, cls = KINDS[kind]
    sizes = (1, 7, 16384, 16385, 24000)
    names = state_names(kind)
    gen = torch.Generator().manual_seed(5)
    w0 = [torch.rand(n, generator=gen) - 0.5 for n in sizes]
    g0 = [[torch.randn(n, generator=gen) * 0.02 * 256.0 for n in sizes] for _ in range(2)]
    SENT, PAD = 7.25, 8
    # role -> element offset inside its buffer in the second placement
    offs = {"param": 1, "grad": 2, names[0]: 3, "ema": 2}
    if len(names) > 1:
        offs[names[1]] = 1
    results = []
    for placed in (False, True):
        bufs = []

        def place(t, role):
            if not placed:
                a = t.clone().to(device)
                assert a.data_ptr() % 16 == 0
                return a
            buf = torch.full((t.numel() + PAD,), SENT, device=device)
            bufs.append((buf, offs[role], t.numel()))
            v = buf[offs[role]:offs[role] + t.numel()]
            v.copy_(t)
            assert v.data_ptr() % 16 == 4 * offs[role]
            return v

        params = [nn.Parameter(place(w, "param")) for w in w0]
        emas = [place(w, "ema") for w in w0]
        kw = dict(betas=(momentum, 0.999)) if kind.startswith("Adam") else dict(momentum=momentum)
        opt = cls([{"params": params[:2], "weight_decay": 0.0}, {"params": params[2:], "weight_decay": DECAY}], lr=LR, lib=lib, **kw)
        for p in params:
            for k in names:
                opt.state[p][k] = place(torch.zeros(p.numel()), k)
        ema = PlainEma({id(p): e for p, e in zip(params, emas)})
        for gs in g0:
            for p, g in zip(params, gs):
                p.grad = place(g, "grad")
            stats = opt.step_fused(inv_scale=1 / 256.0, max_norm=10.0, ema=ema, model=object())
            assert float(stats[2]) == 0.0
        assert float(opt._step) == 2.0
        for buf, o, n in bufs:
            assert bool((buf[:o] == SENT).all()) and bool((buf[o + n:] == SENT).all()), "an element outside a view was written"
        results.append([[p.detach().clone() for p in params], emas] + [[opt.state[p][k].clone() for p in params] for k in names])
    for a, b in zip(*results):
        for i, (x, y) in enumerate(zip(a, b)):
            assert torch.equal(x, y), f"{kind}: size {sizes[i]}: the 16-byte and the 4-byte path differ"
    assert not torch.equal(results[0][0][4], w0[4].to(device)) and not torch.equal(results[0][1][4], w0[4].to(device))


def check_non_finite(kind, device="cpu", lib=None):
    """tests/test_emu_optim.py:test_non_finite_gradient_skips_the_update_but_not_the_ema carried over: an inf, then a NaN, in one gradient:
    stats[2] == 1, parameters / both states / step bit-unchanged, the EMA still moves by d; the next clean step continues with step + 1."""
    m = make_net(1, device)
    opt = hip_optimizer(m, kind, lib)
    ema = ModelEMA(m, tau=5)
    names = state_names(kind)

    def load(seed):
        for p, g in zip(m.parameters(), grads(m, seed, 256.0)):
            p.grad = g

    load(3)
    opt.step_fused(inv_scale=1 / 256.0, max_norm=10.0, ema=ema, model=m)
    assert float(opt._step) == 1.0
    for n_bad, bad in enumerate((float("inf"), float("nan"))):
        before = [p.detach().clone() for p in m.parameters()]
        states = [[opt.state[p][k].clone() for k in names] for p in m.parameters()]
        ema_before = [p.detach().clone() for p in ema.ema.parameters()]
        load(4 + n_bad)
        m.c2.weight.grad[1, 2, 0, 0] = bad
        stats = opt.step_fused(inv_scale=1 / 256.0, max_norm=10.0, ema=ema, model=m)
        assert float(stats[2]) == 1.0
        assert float(opt._step) == 1.0
        for p, b, sb in zip(m.parameters(), before, states):
            assert torch.equal(p, b) and all(torch.equal(opt.state[p][k], s) for k, s in zip(names, sb))
            assert opt.state[p]["step"] is opt._step
        d = ema.decay(2 + n_bad)
        for e, eb, p in zip(ema.ema.parameters(), ema_before, m.parameters()):  # train.py:417-421: ema.update runs even on a skipped step
            torch.testing.assert_close(e, eb * d + (1 - d) * p.detach(), rtol=1e-6, atol=1e-7)
    # the next clean step is step 2 of the optimizer -- as for a torch optimizer that GradScaler.step did not call twice
    m2 = make_net(1, "cpu")   # (torch's single-tensor CPU step: separately rounded, see the module docstring)
    ref = ref_optimizer(m2, kind, foreach=False)
    for seed in (3, 6):
        for p, g in zip(m2.parameters(), grads(m2, seed, 256.0)):
            p.grad = g / 256.0
        torch.nn.utils.clip_grad_norm_(m2.parameters(), max_norm=10.0)
        ref.step()
    load(6)
    stats = opt.step_fused(inv_scale=1 / 256.0, max_norm=10.0, ema=ema, model=m)
    assert float(stats[2]) == 0.0 and float(opt._step) == 2.0
    for (n, p), q in zip(m2.named_parameters(), m.parameters()):
        torch.testing.assert_close(q.detach().cpu(), p.detach(), rtol=RTOL, atol=ATOL, msg=lambda s: f"{kind} {n}: {s}")
