"""Copy-paste augmentation timing on one GPU: a full-size training batch (64 x 640^2 fp16 / 255, frames alternating 1920 x 1080 and
1280 x 960, 8 polygons per frame), everything in ONE process after warm-up, device events around windows of at least 0.5 s.

    python scripts/copy_paste_bench.py [--parent-lib build_variants/parent/libyolov5_hip.so] [--out profiles/copy_paste/copy_paste_bench.json]

  (a) parent comparison   the render launch y5_mosaic_batch with copy_paste = 0 on this tree's library and on the PARENT commit's library
                          (built beside it; --parent-lib), same job table, windows alternated.  `not_slower`: the new median is above the
                          parent's by no more than the spread (max - min) of the parent's own windows.  The two outputs are compared byte
                          for byte first.
  (b) cost of the feature y5_paste_planes + y5_mosaic_batch_paste at copy_paste = 0.1 and 1.0 over the SAME mosaics (the paste samples come
                          from a generator of their own, so the job table does not change with p): planes_us, render_us, both_us, the
                          overhead over (a), the plane bytes written and their rate.
The GPU's sampled clocks (bench.gpu_state_probe) are recorded with the figures."""
import argparse
import ctypes as C
import json
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import augment_oracle as ao  # noqa: E402
from tests import seg_data_ref as sd  # noqa: E402
from yolov5_amd import _lib, dataloaders as D  # noqa: E402

S, N, B, WINDOW_S, REPEATS = 640, 16, 64, 0.5, 7


def dataset(dev):
    ims, _ = ao.synthetic_dataset(N, seed=7, sizes=((1080, 1920), (960, 1280)))
    _, classes, segments = sd.full_size_dataset(N, per=8, seed=7, size=(8, 8))     # normalised polygons: the frame size does not matter
    labels = [D.labels_from_segments(c, sg) for c, sg in zip(classes, segments)]
    return [torch.from_numpy(im).to(dev) for im in ims], labels, segments


def window(fn, n):
    """Device time per call of n back-to-back calls, in us."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def calls_per_window(fn):
    for _ in range(5):
        fn()
    return max(8, int(WINDOW_S * 1e6 / window(fn, 20)) + 1)


def stats(v):
    return {"median_us": float(np.median(v)), "min_us": float(min(v)), "max_us": float(max(v)), "windows_us": [round(float(x), 2) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "copy_paste_bench needs a GPU"
    dev = torch.device("cuda:0")
    ims_t, labels, segments = dataset(dev)
    counts = [len(sg) for sg in segments]
    hyp = dict(ao.HYP_AUG)
    random.seed(13); np.random.seed(13)
    draws = [D.draw_sample_seg(i % N, N, S, hyp) for i in range(B)]
    lib = _lib.lib()
    stream = _lib.stream(dev)
    out = torch.empty((B, 3, S, S), dtype=torch.float16, device=dev)
    tail = (B, S, 114, C.c_void_p(out.data_ptr()), _lib.Y5_F16, 1, stream)
    res = {"bs": B, "imgsz": S, "device": torch.cuda.get_device_name(0), "window_s": WINDOW_S, "repeats": REPEATS}

    # (a)
    jobs = D._seg_assemble(ims_t, labels, segments, draws, S, hyp)[0]
    table = _lib.device_table(jobs, dev)
    new = lambda: _lib.check(lib.y5_mosaic_batch(C.c_void_p(table.data_ptr()), *tail), lib)  # noqa: E731
    n_calls = calls_per_window(new)
    res["calls_per_window"] = n_calls
    if a.parent_lib:
        plib = C.CDLL(os.path.abspath(a.parent_lib))
        plib.y5_mosaic_batch.restype, plib.y5_mosaic_batch.argtypes = _lib.EXPORTS["y5_mosaic_batch"]
        old = lambda: _lib.check(plib.y5_mosaic_batch(C.c_void_p(table.data_ptr()), *tail), lib)  # noqa: E731
        old()
        torch.cuda.synchronize()
        ref = out.clone()
        out.zero_()
        new()
        torch.cuda.synchronize()
        res["parent_output_identical"] = bool(torch.equal(ref.view(torch.int16), out.view(torch.int16)))
        for _ in range(5):
            old()
        t_old, t_new = [], []
        for _ in range(REPEATS):
            t_old.append(window(old, n_calls))
            t_new.append(window(new, n_calls))
        spread = max(t_old) - min(t_old)
        res["a_parent"], res["a_new"] = stats(t_old), stats(t_new)
        res["a_parent_spread_us"] = spread
        res["a_new_minus_parent_us"] = float(np.median(t_new) - np.median(t_old))
        res["not_slower"] = bool(np.median(t_new) - np.median(t_old) <= spread)
    else:
        res["a_new"] = stats([window(new, n_calls) for _ in range(REPEATS)])
    base = res["a_new"]["median_us"]

    # (b)
    for p in (0.1, 1.0):
        g = random.Random(29)
        for d in draws:
            d.pop("paste", None)
            n = sum(counts[i] for i in d["indices"])
            d["paste"] = g.sample(range(n), k=round(p * n))
        jobs_p, _, _, _, pasted = D._seg_assemble(ims_t, labels, segments, draws, S, dict(hyp, copy_paste=p))
        assert bytes(jobs_p) == bytes(jobs) and pasted
        polys = [pg for pl in pasted.values() for pg in pl]
        plane = [k for k, pl in enumerate(pasted.values()) for _ in pl]
        off = np.zeros(len(polys) + 1, np.int32)
        np.cumsum([len(pg) for pg in polys], out=off[1:])
        meta = torch.from_numpy(np.concatenate((*[pg.reshape(-1) for pg in polys], off, np.asarray(plane, np.int32))).astype(np.int32)).to(dev)
        job_plane = np.full(len(jobs), -1, np.int32)
        job_plane[list(pasted)] = np.arange(len(pasted))
        job_plane = torch.from_numpy(job_plane).to(dev)
        S2 = 2 * S
        planes = torch.empty((len(pasted), S2, (S2 + 31) // 32), dtype=torch.int32, device=dev)
        p_off = meta.data_ptr() + 8 * int(off[-1])

        def raster():
            _lib.check(lib.y5_paste_planes(C.c_void_p(meta.data_ptr()), C.c_void_p(p_off), C.c_void_p(p_off + 4 * len(off)), len(polys), len(pasted),
                                           S2, C.c_void_p(planes.data_ptr()), stream), lib)

        def render():
            _lib.check(lib.y5_mosaic_batch_paste(C.c_void_p(table.data_ptr()), len(jobs), C.c_void_p(job_plane.data_ptr()),
                                                 C.c_void_p(planes.data_ptr()), *tail), lib)

        def both():
            raster()
            render()

        for _ in range(5):
            both()
        n_r = calls_per_window(raster)
        r = {"pasting_jobs": len(pasted), "polygons": len(polys), "points": int(off[-1]), "plane_bytes": planes.numel() * 4,
             "planes": stats([window(raster, n_r) for _ in range(REPEATS)]), "render": stats([window(render, n_calls) for _ in range(REPEATS)]),
             "both": stats([window(both, n_calls) for _ in range(REPEATS)])}
        r["overhead_us"] = r["both"]["median_us"] - base
        r["overhead_pct"] = 100.0 * r["overhead_us"] / base
        r["planes_write_gbps"] = r["plane_bytes"] / r["planes"]["median_us"] / 1e3
        res[f"b_copy_paste_{p}"] = r

    try:
        import bench

        res["gpu_state"] = bench.gpu_state_probe(new, dev)
    except Exception as e:  # the probe must never break the benchmark
        res["gpu_state"] = {"error": f"{type(e).__name__}: {e}"}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
