"""Measures the optimizer block of a training step on one MI355X: the fused device path against the host path, for every optimizer of
smart_optimizer.

    python scripts/optim_bench.py [--out profiles/optim/optim_bench.json] [--models yolov5s,yolov5s-cls] [--min-seconds 0.5]

Models: yolov5s in train mode (three parameter groups) and the yolov5s-cls shape of scripts/classify_train_bench.py, each with a ModelEMA.
Gradients are synthetic: every .grad is a view of one flat fp32 arena (as the training engine lays them out), re-filled from a master copy
before every step on BOTH paths (the host path unscales in place); the refill is also timed alone.  inv_scale = 1 / 65536, max_norm = 10.
For Adam, AdamW, RMSProp and SGD, alternated in one process after a warm-up, three rounds:
  * fused: optimizer.step_fused(inv_scale, max_norm, ema, model) + LossScaler.record / update (HipAdam / HipAdamW / HipRMSprop / HipSGD);
  * host : train_loop.host_amp_step + ModelEMA.update + LossScaler.update with the torch optimizer on a copy of the model;
  * update only: step_fused without the norm pass (the update kernel + the EMA of the buffers), for the distance from the HBM rate.
Per variant: device-event time per step over windows of at least --min-seconds, wall time per step over such a window ending in a
synchronise (the host path's cost is its blocking read and its launch count), the bytes the fused kernels must move and that over the device
time as a fraction of the 8 TB/s HBM peak.  That fraction is a LOWER bound of what the kernels reach: when the host side of step_fused
paces the step (wall time = device time), the events time the enqueue; the kernels' own times come from a run under
`rocprofv3 --kernel-trace --stats -- python scripts/optim_bench.py --rounds 1 --min-seconds 0.05 --out ""`.
No test gates on these figures."""
import argparse
import copy
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from yolov5_amd.torch_utils import ModelEMA, smart_optimizer  # noqa: E402
from yolov5_amd.train_loop import LossScaler, host_amp_step  # noqa: E402
from yolov5_amd.yolo import ClassificationModel, DetectionModel  # noqa: E402

HBM_PEAK = 8e12
SCALE, MAX_NORM = 65536.0, 10.0
# fp32 words per parameter: the norm pass reads the gradient; the update reads w, g, state(s), EMA and writes w, state(s), EMA
WORDS = {"Adam": (1, 9), "AdamW": (1, 9), "RMSProp": (1, 9), "SGD": (1, 7)}


def build(name, dev):
    if name == "yolov5s":
        return DetectionModel("yolov5s.yaml").to(dev).train()
    if name == "yolov5s-cls":
        return ClassificationModel(model=DetectionModel("yolov5s.yaml"), nc=1000, cutoff=10).to(dev).train()
    raise ValueError(name)


def arena(model, seed):
    """One flat gradient arena, every .grad a view of it (16-byte aligned starts), and the master copy it is re-filled from."""
    params = list(model.parameters())
    offs, total = [], 0
    for p in params:
        offs.append(total)
        total += (p.numel() + 3) // 4 * 4
    dev = params[0].device
    g = torch.Generator(device=dev).manual_seed(seed)
    master = torch.randn(total, device=dev, generator=g) * 0.02 * SCALE
    flat = master.clone()
    for p, o in zip(params, offs):
        p.grad = flat[o:o + p.numel()].view_as(p)
    return flat, master


def host_optimizer(model, name):
    if name != "SGD":
        return smart_optimizer(model, name, lr=0.001, momentum=0.9, decay=5e-5)
    groups = smart_optimizer(model, "SGD", lr=0.001, momentum=0.9, decay=5e-5).param_groups   # the three groups; torch's own SGD on them
    return torch.optim.SGD([{"params": g["params"], "weight_decay": g["weight_decay"]} for g in groups], lr=0.001, momentum=0.9, nesterov=True)


def window(fn, min_seconds):
    """(device ms per call, wall ms per call): calls between two device events, doubled until the window reaches min_seconds; the wall
    clock runs from the first call to the end of a synchronise."""
    iters = 8
    while True:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        dev_ms = e0.elapsed_time(e1)
        if dev_ms >= min_seconds * 1e3 or wall >= min_seconds * 1e3:
            return dev_ms / iters, wall / iters
        iters *= 2


def bench_model(model_name, dev, min_seconds, rounds):
    base = build(model_name, dev)
    nparam = sum(p.numel() for p in base.parameters())
    out = {"parameters": nparam, "tensors": len(list(base.parameters())), "optimizers": {}}
    for name in ("Adam", "AdamW", "RMSProp", "SGD"):
        m_f, m_h = copy.deepcopy(base), copy.deepcopy(base)
        flat_f, master_f = arena(m_f, 1)
        flat_h, master_h = arena(m_h, 1)
        opt_f = smart_optimizer(m_f, name, lr=0.001, momentum=0.9, decay=5e-5, fused=True)
        opt_h = host_optimizer(m_h, name)
        assert hasattr(opt_f, "step_fused") and not hasattr(opt_h, "step_fused")
        ema_f, ema_h = ModelEMA(m_f), ModelEMA(m_h)
        sc_f, sc_h = LossScaler(enabled=True, init_scale=SCALE, growth_interval=10 ** 9), LossScaler(enabled=True, init_scale=SCALE, growth_interval=10 ** 9)
        params_h = list(m_h.parameters())

        def fused():
            flat_f.copy_(master_f)
            sc_f.record(opt_f.step_fused(inv_scale=1.0 / sc_f.scale, max_norm=MAX_NORM, ema=ema_f, model=m_f))
            sc_f.update()

        def host():
            flat_h.copy_(master_h)
            host_amp_step(opt_h, params_h, sc_h, MAX_NORM)
            ema_h.update(m_h)
            sc_h.update()

        def update_only():
            opt_f.step_fused(ema=ema_f, model=m_f)

        def refill():
            flat_f.copy_(master_f)

        variants = {"fused": fused, "host": host, "update_only": update_only, "refill": refill}
        for fn in variants.values():   # warm-up: code objects, state tensors, tables, torch's own kernel choices
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        assert sc_f.skipped == 0 and sc_h.skipped == 0, "the synthetic gradients overflowed"
        runs = {k: [] for k in variants}
        for _ in range(rounds):        # alternated: a disturbance from the shared host hits every variant alike
            for k, fn in variants.items():
                runs[k].append(window(fn, min_seconds))
        r = {}
        for k, v in runs.items():
            r[k + "_device_ms"] = sorted(x[0] for x in v)[len(v) // 2]
            r[k + "_wall_ms"] = sorted(x[1] for x in v)[len(v) // 2]
            r[k + "_device_ms_all"] = [x[0] for x in v]
        nw, uw = WORDS[name]
        r["fused_bytes"] = 4 * nparam * (nw + uw)
        r["update_bytes"] = 4 * nparam * uw
        r["fused_hbm_fraction"] = r["fused_bytes"] / ((r["fused_device_ms"] - r["refill_device_ms"]) * 1e-3) / HBM_PEAK
        r["update_hbm_fraction"] = r["update_bytes"] / (r["update_only_device_ms"] * 1e-3) / HBM_PEAK
        r["host_over_fused_device"] = r["host_device_ms"] / r["fused_device_ms"]
        r["host_over_fused_wall"] = r["host_wall_ms"] / r["fused_wall_ms"]
        out["optimizers"][name] = r
        print(f"{model_name} {name}: fused {r['fused_device_ms']:.3f} ms device / {r['fused_wall_ms']:.3f} ms wall, host {r['host_device_ms']:.3f} / "
              f"{r['host_wall_ms']:.3f}, update only {r['update_only_device_ms']:.3f} ms = {100 * r['update_hbm_fraction']:.1f} % of HBM peak, "
              f"refill {r['refill_device_ms']:.3f} ms", flush=True)
        del m_f, m_h, opt_f, opt_h, ema_f, ema_h
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="yolov5s,yolov5s-cls")
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="profiles/optim/optim_bench.json")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_bench: no GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda")
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "inv_scale": 1.0 / SCALE, "max_norm": MAX_NORM,
           "hbm_peak_bytes_per_s": HBM_PEAK, "min_seconds": a.min_seconds, "rounds": a.rounds, "models": {}}
    for name in a.models.split(","):
        res["models"][name] = bench_model(name, dev, a.min_seconds, a.rounds)
    print(json.dumps({k: v for k, v in res.items() if k != "models"} | {"models": {m: {o: {k: r[k] for k in ("fused_device_ms", "host_device_ms", "fused_wall_ms", "host_wall_ms", "update_hbm_fraction")}
                                                                                      for o, r in v["optimizers"].items()} for m, v in res["models"].items()}}))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
