"""Training at varying shapes on one GPU: yolov5s, bs 64, fp16, imgsz 640 (train.py --multi-scale draws 21 sizes, 320 .. 960; --quad).
Everything in ONE process after warm-up, device events around windows of at least 0.5 s (the rebuild case (c): host clock around
synchronised steps -- a rebuild is host work).

    python scripts/multi_scale_bench.py [--out profiles/multi_scale/multi_scale_bench.json]

  (a) step time at 320^2, 640^2 and 960^2 with the three plans cached (forward + ComputeLoss + backward + fused SGD / EMA step);
  (b) a step that SWITCHES between two cached shapes (640^2 <-> 960^2 alternating) against staying on one: pair time minus the sum of (a);
  (c) the same alternation with the plan cache at its default of one plan (Y5_TRAIN_PLAN_CACHE=1: every switch drops the plan and builds a new
      one, gradient arena included) -- the behaviour before the cache, the BASELINE of (b), measured with the tuner's choices already cached;
  (d) `nbytes` of the three plans, a least-squares line through them over the pixel count, and from it how many of the 21 plans fit the default
      byte budget (half of the device's memory) together -- an estimate: the 21 plans are not built here;
  (e) the `y5_scale_img` launch of torch_utils.multi_scale for 64 x 3 x 640^2 uint8 -> 960^2 fp16, and its share of the 960^2 step;
  (f) `y5_collate4` for 64 x 3 x 640^2 against the torch composition of the reference's collate_fn4 on the same device tensors (outputs compared
      byte for byte first).
No target is set for any of them."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WINDOW_S, REPEATS, B = 0.5, 5, 64


def window(fn, n):
    """Device time per call of n back-to-back calls, in ms."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def windows(fn, warm=3):
    for _ in range(warm):
        fn()
    n = max(2, int(WINDOW_S * 1e3 / window(fn, 2)) + 1)
    v = [window(fn, n) for _ in range(REPEATS)]
    return {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v)), "calls_per_window": n,
            "windows_ms": [round(float(x), 4) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--model", default="yolov5s")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "multi_scale_bench needs a GPU"
    dev = torch.device("cuda:0")
    from yolov5_amd import _lib, train_engine as te
    from yolov5_amd.dataloaders import collate_fn4
    from yolov5_amd.loss import ComputeLoss
    from yolov5_amd.torch_utils import ModelEMA, multi_scale, smart_optimizer
    from yolov5_amd.yolo import DetectionModel

    torch.manual_seed(0)
    m = DetectionModel(a.model + ".yaml").to(dev).train()
    m.hyp = {"box": 0.05, "cls": 0.5, "cls_pw": 1.0, "obj": 1.0, "obj_pw": 1.0, "anchor_t": 4.0, "fl_gamma": 0.0, "label_smoothing": 0.0}
    compute_loss = ComputeLoss(m)
    opt = smart_optimizer(m, "SGD", lr=0.01, momentum=0.937, decay=5e-4)
    ema = ModelEMA(m)
    g = torch.Generator(device="cpu").manual_seed(0)
    u8 = torch.randint(0, 256, (B, 3, 640, 640), generator=g, dtype=torch.uint8).to(dev)
    nt = B * 8
    t = torch.cat((torch.randint(0, B, (nt, 1), generator=g).float(), torch.randint(0, 80, (nt, 1), generator=g).float(),
                   torch.rand((nt, 2), generator=g) * 0.8 + 0.1, torch.rand((nt, 2), generator=g) * 0.3 + 0.02), 1).to(dev)

    class Fixed:   # multi_scale's size draw, fixed
        def __init__(self, v):
            self.v = v

        def randrange(self, lo, hi):
            return self.v

    xs = {s: (u8 if s == 640 else multi_scale(u8, 640, 32, torch.float16, rng=Fixed(s))) for s in (320, 640, 960)}
    assert [tuple(x.shape[2:]) for x in xs.values()] == [(320, 320), (640, 640), (960, 960)]
    scale = 1024.0

    def step(s):
        pred = m(xs[s])
        loss, _ = compute_loss(pred, t)
        opt.zero_grad(set_to_none=True)
        (loss * scale).backward()
        opt.step_fused(inv_scale=1.0 / scale, max_norm=10.0, ema=ema, model=m)

    res = {"model": a.model, "bs": B, "imgsz": 640, "dtype": "fp16", "device": torch.cuda.get_device_name(0), "window_s": WINDOW_S, "repeats": REPEATS}
    te.set_plan_cache(m, max_plans=8)
    t0 = time.perf_counter()
    for s in xs:
        step(s)
    torch.cuda.synchronize()
    res["build_and_tune_three_plans_s"] = round(time.perf_counter() - t0, 2)

    # (a)
    res["a_step"] = {str(s): windows(lambda s=s: step(s)) for s in xs}
    stay = res["a_step"]["640"]["median_ms"] + res["a_step"]["960"]["median_ms"]

    # (b)
    def pair():
        step(640)
        step(960)

    res["b_switch_cached"] = windows(pair)
    res["b_switch_cached"]["stay_pair_ms"] = stay
    res["b_switch_cached"]["cost_per_switch_ms"] = (res["b_switch_cached"]["median_ms"] - stay) / 2
    engines = m.__dict__["_train_engines"]
    res["plans_live"] = len(engines)

    # (d)
    nb = {int(k[0][2]): int(e.nbytes) for k, e in engines.items()}
    px = np.array(sorted(nb), dtype=np.float64) ** 2
    slope, icpt = np.polyfit(px, np.array([nb[s] for s in sorted(nb)], dtype=np.float64), 1)
    budget = torch.cuda.mem_get_info(dev)[1] // 2
    est = [float(icpt + slope * s * s) for s in range(320, 961, 32)]
    fit, acc = 0, 0.0
    for v in sorted(est):
        if acc + v > budget:
            break
        acc, fit = acc + v, fit + 1
    res["d_nbytes"] = {"per_plan": {str(s): nb[s] for s in sorted(nb)}, "arena_owner": next(int(k[0][2]) for k, e in engines.items() if e._owns_arena),
                       "fit_bytes_per_pixel_of_side2": slope, "fit_intercept": icpt,
                       "fit_residual_bytes": [float(nb[s] - (icpt + slope * s * s)) for s in sorted(nb)],
                       "default_budget_bytes": int(budget), "estimated_21_plans_bytes": float(sum(est)), "estimated_plans_that_fit_of_21": fit,
                       "torch_memory_allocated_bytes": int(torch.cuda.memory_allocated(dev))}

    # (e)
    res["e_scale_img_640_to_960"] = windows(lambda: multi_scale(u8, 640, 32, torch.float16, rng=Fixed(960)))
    res["e_scale_img_640_to_960"]["share_of_960_step_pct"] = 100.0 * res["e_scale_img_640_to_960"]["median_ms"] / res["a_step"]["960"]["median_ms"]

    # (f)
    class Alt:
        def __init__(self):
            self.k = 0

        def random(self):
            self.k += 1
            return 0.25 if self.k % 2 else 0.75

    empty = torch.zeros((0, 6))
    lib, stream = _lib.lib(), _lib.stream(dev)
    flags = [k % 2 == 0 for k in range(B // 4)]
    fl = torch.tensor(flags, dtype=torch.uint8).to(dev)
    out = torch.empty((B // 4, 3, 1280, 1280), dtype=torch.uint8, device=dev)

    def kernel():
        _lib.check(lib.y5_collate4(C.c_void_p(u8.data_ptr()), B, 3, 640, 640, C.c_void_p(fl.data_ptr()), C.c_void_p(out.data_ptr()), stream), lib)

    def composed():
        im4 = []
        for i, up in enumerate(flags):
            i *= 4
            if up:
                im4.append(F.interpolate(u8[i].unsqueeze(0).float(), scale_factor=2.0, mode="bilinear", align_corners=False)[0].type(u8[i].type()))
            else:
                im4.append(torch.cat((torch.cat((u8[i], u8[i + 1]), 1), torch.cat((u8[i + 2], u8[i + 3]), 1)), 2))
        return torch.stack(im4, 0)

    kernel()
    same = bool(torch.equal(out, composed())) and bool(torch.equal(out, collate_fn4(u8, empty, None, None, Alt())[0]))
    res["f_collate4"] = {"identical_to_torch": same, "kernel": windows(kernel), "torch_composition": windows(composed),
                         "bytes_moved": int(u8.numel() * (1 + 0.25) / 2 + out.numel())}
    res["f_collate4"]["speedup"] = res["f_collate4"]["torch_composition"]["median_ms"] / res["f_collate4"]["kernel"]["median_ms"]
    res["f_collate4"]["kernel_gbps"] = res["f_collate4"]["bytes_moved"] / res["f_collate4"]["kernel"]["median_ms"] / 1e6

    # (c) last: it drops the cached plans
    te.set_plan_cache(m, max_plans=1)
    v = []
    for _ in range(3):
        for s in (640, 960):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step(s)
            torch.cuda.synchronize()
            v.append((time.perf_counter() - t0) * 1e3)
    res["c_switch_single_plan"] = {"step_ms": [round(x, 2) for x in v], "median_pair_ms": float(np.median(v[0::2]) + np.median(v[1::2])), "stay_pair_ms": stay,
                                   "note": "every step rebuilds its plan; tuner choices cached by the warm-up above"}
    res["c_switch_single_plan"]["cost_per_switch_ms"] = (res["c_switch_single_plan"]["median_pair_ms"] - stay) / 2
    te.set_plan_cache(m)
    try:
        import bench

        res["gpu_state"] = bench.gpu_state_probe(kernel, dev)
    except Exception as e:  # the probe must never break the benchmark
        res["gpu_state"] = {"error": f"{type(e).__name__}: {e}"}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
