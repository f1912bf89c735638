"""AutoAnchor timing on an MI355X: kmean_anchors(n=9, gen=1000) on 1 000 003 synthetic label sizes, HIP events after one warm-up, stage by stage,
against the fp64 numpy restatement (tests/autoanchor_ref.py) of the same call on the host's CPUs.

    python scripts/autoanchor_bench.py [--labels 1000003] [--gen 1000] [--cpu-gen 20] [--cpu-restarts 2]

The restatement at this size takes minutes, so it is timed on `--cpu-gen` generations and `--cpu-restarts` k-means restarts and scaled to
1000 generations / 30 restarts (both are sequences of identical steps); the JSON line says so.  A record, not a pass / fail figure."""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import autoanchor_ref as ar  # noqa: E402
from yolov5_amd import autoanchor as aa  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return out, a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--labels", type=int, default=1000003)
    ap.add_argument("--gen", type=int, default=1000)
    ap.add_argument("--cpu-gen", type=int, default=20)
    ap.add_argument("--cpu-restarts", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    wh = ar.synthetic_wh(a.labels, seed=0)
    wh[:, 0] = np.maximum(wh[:, 0], 2.5)  # every row stays past the >= 2 px filter after the round trip through normalised labels
    ds = ar.Dataset(np.array([[640.0, 640.0]]), [np.concatenate([np.zeros((len(wh), 3), np.float32), wh / np.float32(640)], 1)])

    def seed():
        np.random.seed(0)
        random.seed(0)

    seed()
    aa.kmean_anchors(ds, n=9, img_size=640, thr=4.0, gen=a.gen, verbose=False, device=dev)  # warm-up
    seed()
    k, ms_total = timed(lambda: aa.kmean_anchors(ds, n=9, img_size=640, thr=4.0, gen=a.gen, verbose=False, device=dev))
    # the two stages on their own (device tensors resident, draws made outside the timed region)
    _, whf = ar.label_wh(ds, 640)
    s = whf.std(0)
    obs = whf / s
    seed()
    idx = aa.draw_kmeans_init(len(obs), 9)
    obs_d, wh_d = torch.from_numpy(obs).to(dev), torch.from_numpy(whf).to(dev)
    km, ms_km = timed(lambda: aa.anchor_kmeans(obs_d, obs[idx]))
    k0 = km["book"][km["winner"]].astype(np.float32) * s
    k0 = k0[np.argsort(k0.prod(1))]
    v = aa.draw_mutations(a.gen, k0.shape)
    _, ms_ev = timed(lambda: aa.anchor_evolve(wh_d, k0, v, 4.0))

    torch.set_num_threads(min(16, torch.get_num_threads()))
    t0 = time.perf_counter()
    ar.evolve(whf, k0, v[:a.cpu_gen], 4.0)
    cpu_gen_s = (time.perf_counter() - t0) / (a.cpu_gen + 1)
    t0 = time.perf_counter()
    ref = ar.kmeans(obs, idx[:a.cpu_restarts])
    cpu_km_s = time.perf_counter() - t0
    cpu_iter_s = cpu_km_s / int(ref["iters"].sum())
    cpu_total_s = cpu_gen_s * (a.gen + 1) + cpu_iter_s * int(km["iters"].sum())
    print(json.dumps(dict(
        labels=len(whf), gen=a.gen, restarts=30, hip_kmean_anchors_ms=round(ms_total, 2), hip_kmeans_ms=round(ms_km, 2),
        hip_kmeans_iterations_max=int(km["iters"].max()), hip_kmeans_chain_iterations=int(km["iters"].sum()), hip_evolve_ms=round(ms_ev, 2),
        hip_per_generation_us=round(1e3 * ms_ev / (a.gen + 1), 2), cpu_restatement_per_generation_ms=round(1e3 * cpu_gen_s, 2),
        cpu_restatement_per_chain_iteration_ms=round(1e3 * cpu_iter_s, 2), cpu_restatement_extrapolated_s=round(cpu_total_s, 1),
        cpu_measured_on=f"{a.cpu_gen} generations, {a.cpu_restarts} restarts", anchors=np.round(k, 1).tolist())))


if __name__ == "__main__":
    main()
