"""AutoAnchor (utils/autoanchor.py) with the reference's names: `check_anchor_order`, `check_anchors`, `kmean_anchors`.

The label sizes are uploaded once; everything that touches all of them runs in HIP kernels (csrc/autoanchor.h):
    anchor_metric(wh, k, thr)        check_anchors.metric (:36-43): bpr / aat as exact integer counts
    anchor_kmeans(obs, guess)        scipy.cluster.vq.kmeans(obs, n, iter=30) of :139, all restarts advancing together in fp64
    anchor_evolve(wh, k, v, thr)     the 1000-generation mutate-and-keep-if-fitter chain of :148-160, no host synchronisation
The host keeps what is random or tiny: the RNG draws (`draw_kmeans_init`, `draw_mutations`: the same np.random / random call order as the
reference, all drawn before the chain runs -- they never depend on which candidates were accepted), the numpy expressions of :124-131 that
build the label sizes, and the choice among the restarts.  One device-to-host read ends each stage.

Differences from the reference: `check_anchors` returns (bpr, aat, replaced) instead of only logging; `kmean_anchors` takes a loaded
dataset only (no *.yaml path), its summary line is shorter, and `verbose` prints no per-generation results; k-means runs in fp64
(scipy: the float32 of its input), so its book agrees with scipy's to float32 rounding, not bit for bit.
"""
from __future__ import annotations

import ctypes as C
import random

import numpy as np
import torch

from . import _lib
from .general import LOGGER
from .yolo import check_anchor_order  # noqa: F401  (re-export: utils/autoanchor.py:16-23)

PREFIX = "AutoAnchor: "
MAX_ANCHORS = 40    # anchors in total, the loss's own limit
KMEANS_POLL = 8     # k-means iterations queued between two reads of the all-done flag


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _need_gpu(t, what):
    if not _lib.accepts(t):
        raise RuntimeError(f"yolov5_amd.autoanchor.{what} needs GPU tensors (no CPU path)")


def _wh_tensor(wh, what):
    _need_gpu(wh, what)
    if wh.dim() != 2 or wh.shape[1] != 2 or wh.shape[0] < 1:
        raise ValueError(f"{what}: label sizes must be (n, 2) with n >= 1, got {tuple(wh.shape)}")
    return wh if wh.dtype == torch.float32 and wh.is_contiguous() else wh.float().contiguous()


def _thr_inv(thr):
    if not thr > 0:
        raise ValueError(f"thr must be positive, got {thr}")
    return float(np.float32(1 / thr))   # a float32 tensor compared with the Python scalar 1 / thr: torch rounds the scalar to fp32


# ---- RNG draws ------------------------------------------------------------------------------------------------------------------------------
def draw_mutations(gen, shape, mp=0.9, sigma=0.1, rng=random, np_rng=np.random):
    """All mutation factors of the evolution, (gen, *shape) fp64, consuming both streams exactly as :151-153 do (np_rng.random, rng.random,
    np_rng.randn per attempt; redrawn until some factor differs from 1)."""
    out = np.empty((gen,) + tuple(shape), np.float64)
    for g in range(gen):
        v = np.ones(shape)
        while (v == 1).all():  # mutate until a change occurs (prevent duplicates)
            v = ((np_rng.random(shape) < mp) * rng.random() * np_rng.randn(*shape) * sigma + 1).clip(0.3, 3.0)
        out[g] = v
    return out


def draw_kmeans_init(n_obs, k, iters=30, np_rng=np.random):
    """Observation indices every k-means restart starts from, (iters, k) int64: scipy draws np_rng.choice(n_obs, k, replace=False) once per
    restart and nothing else, so drawing them first leaves the stream where scipy leaves it."""
    return np.stack([np_rng.choice(n_obs, size=int(k), replace=False) for _ in range(iters)]).astype(np.int64)


# ---- kernels --------------------------------------------------------------------------------------------------------------------------------
def anchor_metric(wh, k, thr):
    """(labels whose best anchor ratio > 1/thr, (label, anchor) pairs with ratio > 1/thr) as Python ints: bpr * n and aat * n of :36-43.
    wh (n, 2) device tensor of label sizes, k (na, 2) anchors in the same unit."""
    wh = _wh_tensor(wh, "anchor_metric")
    k = torch.as_tensor(k).to(device=wh.device, dtype=torch.float32).reshape(-1, 2).contiguous()
    counts = torch.empty(2, dtype=torch.int64, device=wh.device)
    lib = _lib.lib()
    _lib.check(lib.y5_anchor_metric(_p(wh), wh.shape[0], _p(k), k.shape[0], _thr_inv(thr), _p(counts), _lib.stream(wh.device)), lib)
    c = counts.cpu()
    return int(c[0]), int(c[1])


def anchor_evolve(wh, k, v, thr):
    """The accept chain of :148-160 from anchors k (na, 2) with pre-drawn factors v (gen, na, 2).  Returns (k fp64 numpy, fitness, accepted
    uint8 numpy (gen)); the fitness is mean(best * (best > 1/thr)) with the sum in fp64."""
    wh = _wh_tensor(wh, "anchor_evolve")
    dev = wh.device
    k = np.ascontiguousarray(np.asarray(k, np.float64).reshape(-1, 2))
    na = k.shape[0]
    v = np.ascontiguousarray(np.asarray(v, np.float64)).reshape(-1, na, 2)
    gen = v.shape[0]
    # one fp64 buffer: anchors, fitness, factors (a single upload); the result comes back in a single read
    buf = torch.from_numpy(np.concatenate([k.ravel(), [0.0], v.ravel()])).to(dev)
    acc = torch.zeros(max(gen, 1), dtype=torch.uint8, device=dev)
    lib = _lib.lib()
    ws = _lib.workspace(lib.y5_anchor_evolve_ws_bytes(wh.shape[0]), dev)
    kd, fd, vd = buf[:2 * na], buf[2 * na:2 * na + 1], buf[2 * na + 1:]
    _lib.check(lib.y5_anchor_evolve(_p(wh), wh.shape[0], na, _p(kd), _p(fd), 1, _p(vd) if gen else None, gen, _thr_inv(thr), _p(acc), _p(ws),
                                    ws.numel(), _lib.stream(dev)), lib)
    out = torch.cat([buf[:2 * na + 1], acc[:gen].double()]).cpu().numpy()
    return out[:2 * na].reshape(na, 2).copy(), float(out[2 * na]), out[2 * na + 1:].astype(np.uint8)


def anchor_kmeans(obs, guess, max_iter=10000):
    """scipy.cluster.vq.kmeans over R restarts at once: obs (n, 2) device tensor, guess (R, k, 2) starting centroids.  Returns dict(book
    (R, k, 2) fp64, alive (R, k) bool, dist (R) last mean distance, iters (R), winner = first restart with the lowest distance)."""
    obs = _wh_tensor(obs, "anchor_kmeans")
    dev = obs.device
    g = torch.as_tensor(guess).to(device=dev, dtype=torch.float32).contiguous()
    if g.dim() != 3 or g.shape[2] != 2:
        raise ValueError(f"anchor_kmeans: guess must be (restarts, k, 2), got {tuple(g.shape)}")
    R, k = int(g.shape[0]), int(g.shape[1])
    lib = _lib.lib()
    nws = lib.y5_anchor_kmeans_ws_bytes(obs.shape[0], R, k)
    if nws == 0:
        raise ValueError(f"anchor_kmeans: {R} restarts of {k} centroids over {obs.shape[0]} observations are not supported")
    ws = _lib.workspace(nws, dev)
    f64 = torch.empty(R * k * 2 + R, dtype=torch.float64, device=dev)   # book, last distance
    book, dist = f64[:R * k * 2], f64[R * k * 2:]
    alive = torch.empty(R * k, dtype=torch.uint8, device=dev)
    i32 = torch.empty(R + 1, dtype=torch.int32, device=dev)             # iterations, all-done flag
    iters, done = i32[:R], i32[R:]
    init, ran = 1, 0
    while True:
        _lib.check(lib.y5_anchor_kmeans(_p(obs), obs.shape[0], _p(g), R, k, init, KMEANS_POLL, _p(book), _p(alive), _p(dist), _p(iters), _p(done),
                                        _p(ws), ws.numel(), _lib.stream(dev)), lib)
        init, ran = 0, ran + KMEANS_POLL
        if int(done.item()):   # the only synchronisation: once per KMEANS_POLL iterations
            break
        if ran >= max_iter:
            raise RuntimeError(f"anchor_kmeans: not converged after {ran} iterations")
    out = torch.cat([f64, alive.double(), iters.double()]).cpu().numpy()   # one read for the stage
    nb = R * k * 2
    d = out[nb:nb + R]
    return dict(book=out[:nb].reshape(R, k, 2).copy(), dist=d.copy(), alive=out[nb + R:nb + R + R * k].reshape(R, k) != 0,
                iters=out[nb + R + R * k:].astype(np.int32), winner=int(np.argmin(d)))


# ---- the reference's functions --------------------------------------------------------------------------------------------------------------
def _device(device):
    if device is not None:
        return torch.device(device)
    return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")


def kmean_anchors(dataset, n=9, img_size=640, thr=4.0, gen=1000, verbose=True, device=None):
    """utils/autoanchor.py:67-162: k-means anchors evolved by the genetic algorithm, float32 (n, 2) sorted by area.
    dataset: any object with .shapes ((n_images, 2) array of (w, h)) and .labels (list of (m, 5) [cls, x, y, w, h], normalised)."""
    if isinstance(dataset, str):
        raise NotImplementedError("kmean_anchors: pass a loaded dataset (.shapes, .labels); the *.yaml path form is not implemented")
    if not 1 <= n <= MAX_ANCHORS:
        raise ValueError(f"kmean_anchors: need 1 <= n <= {MAX_ANCHORS}, got {n}")
    npr = np.random
    dev = _device(device)
    # Get label wh (:124-131, the reference's numpy expressions)
    ds_shapes = np.asarray(dataset.shapes, np.float64)
    shapes = img_size * ds_shapes / ds_shapes.max(1, keepdims=True)
    wh0 = np.concatenate([np.asarray(label)[:, 3:5] * shape for shape, label in zip(shapes, dataset.labels)])
    i = (wh0 < 3.0).any(1).sum()
    if i:
        LOGGER.warning(f"{PREFIX}Extremely small objects found: {i} of {len(wh0)} labels are <3 pixels in size")
    wh = wh0[(wh0 >= 2.0).any(1)].astype(np.float32)
    if not len(wh):
        raise ValueError("kmean_anchors: the dataset has no label of 2 pixels or more")
    wh_dev = torch.from_numpy(wh).to(dev)   # uploaded once

    # Kmeans init (:135-143)
    k = None
    LOGGER.info(f"{PREFIX}Running kmeans for {n} anchors on {len(wh)} points...")
    if n <= len(wh):
        s = wh.std(0)  # sigmas for whitening
        obs = wh / s
        idx = draw_kmeans_init(len(wh), n, np_rng=npr)
        km = anchor_kmeans(torch.from_numpy(obs).to(dev), obs[idx])
        w = km["winner"]
        book = km["book"][w][km["alive"][w]]
        if len(book) == n:  # kmeans may return fewer points than requested if wh is insufficient or too similar
            k = book.astype(np.float32) * s
    if k is None:
        LOGGER.warning(f"{PREFIX}switching strategies from kmeans to random init")
        k = np.sort(npr.rand(n * 2)).reshape(n, 2) * img_size
    k = k[np.argsort(k.prod(1))]

    # Evolve (:148-160)
    v = draw_mutations(gen, k.shape, rng=random, np_rng=npr)
    k, f, accepted = anchor_evolve(wh_dev, k, v, thr)
    k = k[np.argsort(k.prod(1))]
    if verbose:
        nb, npair = anchor_metric(torch.from_numpy(wh0.astype(np.float32)).to(dev), k.astype(np.float32), thr)
        LOGGER.info(f"{PREFIX}thr={1 / thr:.2f}: {nb / len(wh0):.4f} best possible recall, {npair / len(wh0):.2f} anchors past thr\n"
                    f"{PREFIX}n={n}, img_size={img_size}, fitness={f:.4f} after {int(accepted.sum())} of {gen} mutations: "
                    + ", ".join(f"{round(x[0])},{round(x[1])}" for x in k))
    return k.astype(np.float32)


def check_anchors(dataset, model, thr=4.0, imgsz=640):
    """utils/autoanchor.py:27-64: measures the best possible recall of the model's anchors on the dataset's label sizes and, when it is
    <= 0.98, replaces them IN PLACE (the engine and the loss watch the tensor) by `kmean_anchors` if those recall more.
    Returns (bpr, aat, replaced): the recall and anchors-above-threshold of the anchors the model came with, and whether they were replaced."""
    m = model.module.model[-1] if hasattr(model, "module") else model.model[-1]  # Detect()
    dev = m.anchors.device
    _need_gpu(m.anchors, "check_anchors")
    ds_shapes = np.asarray(dataset.shapes, np.float64)
    shapes = imgsz * ds_shapes / ds_shapes.max(1, keepdims=True)
    scale = np.random.uniform(0.9, 1.1, size=(shapes.shape[0], 1))  # augment scale
    wh = np.concatenate([np.asarray(label)[:, 3:5] * shape for shape, label in zip(shapes * scale, dataset.labels)]).astype(np.float32)
    if not len(wh):
        raise ValueError("check_anchors: the dataset has no labels")
    wh_dev = torch.from_numpy(wh).to(dev)
    nlab = np.float32(len(wh))

    def metric(k):  # torch's fp32 mean of 0/1 values is count / n exactly (n < 2**24)
        nb, npair = anchor_metric(wh_dev, k, thr)
        return np.float32(nb) / nlab, np.float32(npair) / nlab

    stride = m.stride.to(dev).view(-1, 1, 1)  # model strides
    anchors = m.anchors.clone() * stride  # current anchors
    bpr, aat = metric(anchors.view(-1, 2))
    s = f"\n{PREFIX}{aat:.2f} anchors/target, {bpr:.3f} Best Possible Recall (BPR). "
    replaced = False
    if bpr > 0.98:  # threshold to recompute
        LOGGER.info(f"{s}Current anchors are a good fit to dataset")
    else:
        LOGGER.info(f"{s}Anchors are a poor fit to dataset, attempting to improve...")
        na = m.anchors.numel() // 2  # number of anchors
        new = kmean_anchors(dataset, n=na, img_size=imgsz, thr=thr, gen=1000, verbose=False, device=dev)
        new_bpr = metric(new)[0]
        if new_bpr > bpr:  # replace anchors
            new = torch.tensor(new, device=dev).type_as(m.anchors)
            m.anchors[:] = new.clone().view_as(m.anchors)
            check_anchor_order(m)  # must be in pixel-space (not grid-space)
            m.anchors /= stride
            replaced = True
            LOGGER.info(f"{PREFIX}Done (optional: update model *.yaml to use these anchors in the future)")
        else:
            LOGGER.info(f"{PREFIX}Done (original anchors better than new anchors, proceeding with original anchors)")
    return float(bpr), float(aat), replaced
