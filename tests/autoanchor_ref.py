"""TEST INFRASTRUCTURE ONLY: fp64 numpy restatement of the two stages of the reference's kmean_anchors (utils/autoanchor.py:67-162) and a
seeded label-size generator.  scripts/make_golden_autoanchor.py pins the restatement against the unmodified reference (final anchors bit
for bit) and against scipy's k-means (book within float32 noise); the tests compare the HIP kernels against it.

Evolution (:148-160).  The mutation factors depend on the RNG streams only, so all generations are drawn first (`draw_mutations`, same
np.random / random call order as :151-153 including the redraw loop); the accept chain then runs with the fitness mean taken in fp64.
k-means (:139, scipy.cluster.vq.kmeans(obs, n, iter=30)).  30 draws of np.random.choice(n_obs, n, replace=False) up front, one Lloyd chain
per draw in fp64: nearest centroid by squared distance (lowest index on ties), mean EUCLIDEAN distance, stop when it moved by <= 1e-5 with
the book updated once more after the last distance, empty clusters dropped; the chain with the lowest last mean distance wins, first on ties."""
import random

import numpy as np

CASES = {  # name: images, labels per image (lo, hi), seed (of the dataset and of both RNG streams), kmean_anchors arguments.  Seeds were chosen so
    # that every condition scripts/make_golden_autoanchor.py asserts holds (a fixture that fails one is replaced, not tolerated)
    "d34": dict(n_img=12, per=(1, 5), seed=3, n=9, img_size=640, thr=4.0),
    "d247": dict(n_img=40, per=(2, 11), seed=11, n=9, img_size=640, thr=4.0),
    "d2080": dict(n_img=260, per=(3, 14), seed=7, n=9, img_size=640, thr=4.0),
    "d247_thr35": dict(n_img=40, per=(2, 11), seed=17, n=9, img_size=512, thr=3.5),
    "d247_n6": dict(n_img=40, per=(2, 11), seed=21, n=6, img_size=640, thr=4.0),
}
GEN = 1000
PREFIX = 150  # generations of the emulator test


class Dataset:
    """What check_anchors / kmean_anchors read of a dataset: .shapes (n, 2) (w, h) and .labels, a list of (m, 5) [cls, x, y, w, h] normalised."""

    def __init__(self, shapes, labels):
        self.shapes, self.labels = shapes, labels


def make_dataset(n_img, per=(2, 11), seed=0, lo=0.004, hi=0.9):
    """Image sizes uniform in 320..1280, label w and h log-uniform in lo..hi (float32 label rows, float64 shapes as the reference's loader)."""
    g = np.random.default_rng(seed)
    shapes = g.integers(320, 1281, (n_img, 2)).astype(np.float64)
    labels = []
    for _ in range(n_img):
        m = int(g.integers(per[0], per[1] + 1))
        lb = np.zeros((m, 5), np.float32)
        lb[:, 0] = g.integers(0, 80, m)
        lb[:, 1:3] = g.uniform(0.1, 0.9, (m, 2))
        lb[:, 3:5] = np.exp(g.uniform(np.log(lo), np.log(hi), (m, 2)))
        labels.append(lb)
    return Dataset(shapes, labels)


def case_dataset(name):
    c = CASES[name]
    return make_dataset(c["n_img"], c["per"], c["seed"])


def label_wh(dataset, img_size):
    """:124-131 -> (wh0 float64, wh float32 filtered)."""
    shapes = img_size * dataset.shapes / dataset.shapes.max(1, keepdims=True)
    wh0 = np.concatenate([lb[:, 3:5] * s for s, lb in zip(shapes, dataset.labels)])
    return wh0, wh0[(wh0 >= 2.0).any(1)].astype(np.float32)


def synthetic_wh(n, seed=0, img_size=640):
    """n label sizes (float32, px) of the same distribution without building a dataset (large-n tests and timing)."""
    g = np.random.default_rng(seed)
    side = g.integers(320, 1281, (n, 2)).astype(np.float64)
    shapes = img_size * side / side.max(1, keepdims=True)
    wh = np.exp(g.uniform(np.log(0.004), np.log(0.9), (n, 2))).astype(np.float32) * shapes
    wh = np.maximum(wh, [[2.0, 0.0]])  # keep every row past the >= 2 px filter
    return wh.astype(np.float32)


# ---- metric ---------------------------------------------------------------------------------------------------------------------------------
def best_ratio(wh, k32):
    """(x (n, na), best (n)) in fp32, operation by operation as torch evaluates :91-93 (numpy's fp32 divide is IEEE, like torch's)."""
    wh = np.asarray(wh, np.float32)
    k32 = np.asarray(k32, np.float32)
    with np.errstate(divide="ignore"):
        r = wh[:, None] / k32[None]
        x = np.minimum(r, np.float32(1) / r).min(2)
    return x, x.max(1)


def metric_counts(wh, k32, thr):
    """check_anchors.metric (:36-43) as integers: (labels with best > 1/thr, pairs with x > 1/thr)."""
    x, best = best_ratio(wh, k32)
    t = np.float32(1 / thr)
    return int((best > t).sum()), int((x > t).sum())


def fitness(wh, k64, thr):
    """anchor_fitness (:95-98) with the mean in fp64: k rounded to fp32, best * (best > 1/thr) summed in fp64 / n.  (Anchor by anchor: the
    same fp32 operations as best_ratio without its (n, na, 2) temporaries.)"""
    wh = np.asarray(wh, np.float32)
    best = None
    with np.errstate(divide="ignore"):
        for ka in np.asarray(k64).astype(np.float32):
            r = wh / ka
            x = np.minimum(r, np.float32(1) / r).min(1)
            best = x if best is None else np.maximum(best, x)
    t = np.float32(1 / thr)
    return float(np.where(best > t, best, np.float32(0)).astype(np.float64).sum() / len(wh))


# ---- evolution ------------------------------------------------------------------------------------------------------------------------------
def draw_mutations(gen, shape, mp=0.9, sigma=0.1, rng=random, np_rng=np.random):
    """(gen, *shape) fp64 factors, consuming both streams exactly as :151-153."""
    out = np.empty((gen,) + tuple(shape), np.float64)
    for g in range(gen):
        v = np.ones(shape)
        while (v == 1).all():
            v = ((np_rng.random(shape) < mp) * rng.random() * np_rng.randn(*shape) * sigma + 1).clip(0.3, 3.0)
        out[g] = v
    return out


def evolve(wh, k0, v, thr, snapshots=()):
    """The accept chain: returns (k fp64, f, accepted uint8 (gen), gaps (gen) = |fg - f| / f, {g: k after g generations})."""
    k = np.asarray(k0, np.float64).copy()
    f = fitness(wh, k, thr)
    acc = np.zeros(len(v), np.uint8)
    gaps = np.zeros(len(v), np.float64)
    snaps = {}
    for g in range(len(v)):
        kg = (k.copy() * v[g]).clip(min=2.0)
        fg = fitness(wh, kg, thr)
        gaps[g] = abs(fg - f) / f if f else np.inf
        if fg > f:
            f, k = fg, kg.copy()
            acc[g] = 1
        if g + 1 in snapshots:
            snaps[g + 1] = k.copy()
    return k, f, acc, gaps, snaps


# ---- k-means --------------------------------------------------------------------------------------------------------------------------------
def draw_kmeans_init(n_obs, k, iters=30, np_rng=np.random):
    """(iters, k) int64 observation indices: scipy's `_kpoints` draw of every restart, in order."""
    return np.stack([np_rng.choice(n_obs, size=int(k), replace=False) for _ in range(iters)]).astype(np.int64)


def lloyd(obs, guess):
    """One chain.  Returns (book fp64 (k, 2) with dead rows kept, alive (k) bool, last mean distance, iterations, stop margins)."""
    obs = np.asarray(obs, np.float64)
    book = np.asarray(guess, np.float64).copy()
    k = len(book)
    alive = np.ones(k, bool)
    prev, it, margins = np.inf, 0, []
    while True:
        idx = np.flatnonzero(alive)
        dx = obs[:, None, 0] - book[None, idx, 0]
        dy = obs[:, None, 1] - book[None, idx, 1]
        d2 = dx * dx + dy * dy
        code = d2.argmin(1)  # first minimum = lowest index
        dist = float(np.sqrt(d2[np.arange(len(obs)), code]).sum() / len(obs))
        members = np.bincount(code, minlength=len(idx))
        sx = np.bincount(code, weights=obs[:, 0], minlength=len(idx))
        sy = np.bincount(code, weights=obs[:, 1], minlength=len(idx))
        for j, c in enumerate(idx):
            if members[j]:
                book[c] = sx[j] / members[j], sy[j] / members[j]
            else:
                alive[c] = False
        it += 1
        diff = abs(prev - dist)
        prev = dist
        if it > 1:
            margins.append(abs(diff - 1e-5))
        if diff <= 1e-5:
            return book, alive, dist, it, margins


def kmeans(obs, idx):
    """All restarts.  idx (R, k) from draw_kmeans_init.  Returns dict(book (R, k, 2), alive (R, k), dist (R), iters (R), winner, margins)."""
    obs32 = np.asarray(obs, np.float32)
    res = [lloyd(obs32, obs32[i]) for i in idx]
    dist = np.array([r[2] for r in res])
    return dict(book=np.stack([r[0] for r in res]), alive=np.stack([r[1] for r in res]), dist=dist, iters=np.array([r[3] for r in res], np.int32),
                winner=int(dist.argmin()), margins=np.concatenate([np.asarray(r[4], np.float64) for r in res]))


def case_draws(name, n_obs, gen=GEN):
    """(restart draws (30, n), mutation factors (gen, n, 2)) of a CASES entry: both streams seeded, then consumed in kmean_anchors' order."""
    c = CASES[name]
    np.random.seed(c["seed"])
    random.seed(c["seed"])
    return draw_kmeans_init(n_obs, c["n"]), draw_mutations(gen, (c["n"], 2))


# ---- the whole call ---------------------------------------------------------------------------------------------------------------------------
def kmean_anchors(dataset, n=9, img_size=640, thr=4.0, gen=1000, details=False, book=None):
    """The reference's kmean_anchors on the restated stages, consuming np.random / random as it does.  book: start the evolution from this
    k-means result instead of the restated one (scipy's float32 book differs from the fp64 chain in the last bits, and the evolution's
    output is a bit-exact function of its start)."""
    npr = np.random
    wh0, wh = label_wh(dataset, img_size)
    info = {}
    k = None
    if n <= len(wh):
        s = wh.std(0)
        km = kmeans(wh / s, draw_kmeans_init(len(wh), n))
        w = km["winner"]
        info["kmeans"] = km
        book = km["book"][w][km["alive"][w]] if book is None else np.asarray(book)
        if len(book) == n:
            k = book.astype(np.float32) * s
    if k is None:
        k = np.sort(npr.rand(n * 2)).reshape(n, 2) * img_size
    k = k[np.argsort(k.prod(1))]
    info["k0"] = k.copy()
    v = draw_mutations(gen, k.shape)
    kf, f, acc, gaps, snaps = evolve(wh, k, v, thr, snapshots=(PREFIX, gen))
    info.update(v=v, accepted=acc, gaps=gaps, snaps=snaps, f=f, wh=wh)
    out = kf[np.argsort(kf.prod(1))].astype(np.float32)
    return (out, info) if details else out
