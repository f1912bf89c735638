"""Writes tests/golden/autoanchor.npz from the UNMODIFIED reference's utils/autoanchor.py (kmean_anchors :67-162, check_anchors :27-64),
imported read-only through oracle.ref_shim on torch-CPU, with scipy's own k-means.  Needs the reference checkout; no test runs this.

    python scripts/make_golden_autoanchor.py

The shim's TQDM is a MagicMock (iterating one yields nothing: the evolve loop would silently run zero generations), so
utils.autoanchor.TQDM is replaced by a pass-through iterable with a `desc` attribute.

Per case of tests/autoanchor_ref.CASES (np.random and random seeded per case):
  {c}_wh          label sizes after the >= 2 px filter (float32): the kernels' input
  {c}_ref         the reference's returned anchors (n, 2) float32
  {c}_scipy_book  the book scipy's kmeans returned to the reference (whitened units)
  {c}_init        the restatement's 30 restart draws (30, n) -- the same stream positions scipy consumed
  {c}_k0          anchors entering the evolution (fp64, sorted by area)
  {c}_v_last      the mutation factors of the last generation (n, 2): tests re-draw all 1000 with tests/autoanchor_ref.case_draws (the
                  seeded legacy streams are stable) and check their position in the stream against this
  {c}_accepted    the restatement's accept flags; {c}_k150 / {c}_k1000: its anchors after 150 / 1000 generations (fp64)
  {c}_winner, {c}_km_iters, {c}_km_dist  the restatement's winning restart, iterations and last mean distance per restart
For d247 also check_anchors on a Detect stand-in holding yolov5n's anchors scaled by 0.25 (the replacement branch runs):
  check_anchors_in / check_anchors_out (3, 3, 2) grid units, check_counts = (labels, bpr count, aat count) of the restated metric, whose
  formatted values must equal the ones the reference logged.

Asserted here, on the CPU; a fixture that fails one is replaced, not tolerated:
  restatement's final anchors == reference's, bit for bit (evolution started from scipy's book); every decision gap |fg - f| / f >= 1e-9; every k-means stop decision
  ||diff| - 1e-5| >= 1e-9; best and second-best restart distances differ by >= 1e-6 relative; restated book within 1e-5 of scipy's."""
import logging
import os
import random
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402
from tests import autoanchor_ref as ar  # noqa: E402

YOLOV5N_ANCHORS = [[10, 13, 16, 30, 33, 23], [30, 61, 62, 45, 59, 119], [116, 90, 156, 198, 373, 326]]
STRIDES = [8.0, 16.0, 32.0]


class PassThrough:
    def __init__(self, it, *a, **k):
        self.it, self.desc = it, ""

    def __iter__(self):
        return iter(self.it)


def seed(s):
    np.random.seed(s)
    random.seed(s)


def main():
    ns = ref_shim.load()
    cwd = os.getcwd()
    os.chdir(ref_shim.REFERENCE_ROOT)
    try:
        import utils.autoanchor as aa
    finally:
        os.chdir(cwd)
    import scipy.cluster.vq as vq

    aa.TQDM = PassThrough
    books = []
    real_kmeans = vq.kmeans

    def recording_kmeans(*a, **k):
        r = real_kmeans(*a, **k)
        books.append(np.array(r[0]))
        return r

    vq.kmeans = recording_kmeans
    out = {}
    for name, c in ar.CASES.items():
        ds = ar.case_dataset(name)
        args = dict(n=c["n"], img_size=c["img_size"], thr=c["thr"], gen=ar.GEN)
        seed(c["seed"])
        books.clear()
        ref = aa.kmean_anchors(ds, verbose=False, **args)
        seed(c["seed"])
        got, info = ar.kmean_anchors(ds, details=True, book=books[0], **args)   # the evolution is pinned from scipy's own (float32) book ...
        seed(c["seed"])
        own = ar.kmean_anchors(ds, **args)                                        # ... and the all-restated call lands within its noise
        assert np.abs(own - ref).max() / ref.max() <= 1e-3, (name, own, ref)
        km = info["kmeans"]
        assert ref.dtype == np.float32 and np.array_equal(ref, got), (name, ref, got)
        assert info["gaps"].min() >= 1e-9, (name, info["gaps"].min())
        assert km["margins"].min() >= 1e-9, (name, km["margins"].min())
        d = np.sort(km["dist"])
        assert (d[1] - d[0]) / d[0] >= 1e-6, (name, d[:2])
        w = km["winner"]
        assert km["alive"][w].all() and len(books) == 1
        rel = np.abs(km["book"][w] - books[0]).max() / np.abs(books[0]).max()
        assert rel <= 1e-5, (name, rel)
        init, v = ar.case_draws(name, len(info["wh"]))
        assert np.array_equal(v, info["v"])
        out.update({f"{name}_wh": info["wh"], f"{name}_ref": ref, f"{name}_scipy_book": books[0], f"{name}_init": init, f"{name}_k0": info["k0"],
                    f"{name}_v_last": info["v"][-1], f"{name}_accepted": info["accepted"], f"{name}_k150": info["snaps"][ar.PREFIX],
                    f"{name}_k1000": info["snaps"][ar.GEN], f"{name}_winner": np.int64(w), f"{name}_km_iters": km["iters"],
                    f"{name}_km_dist": km["dist"]})
        print(name, len(info["wh"]), "labels,", int(info["accepted"].sum()), "accepted, min gap %.2e," % info["gaps"].min(),
              "min stop margin %.2e, winner %d (%d iterations), book vs scipy %.2e" % (km["margins"].min(), w, km["iters"][w], rel))

    # check_anchors on a Detect stand-in (it reads .anchors and .stride only) with yolov5n's anchors scaled by 0.25
    name, c = "d247", ar.CASES["d247"]
    ds = ar.case_dataset(name)
    a0 = (torch.tensor(YOLOV5N_ANCHORS, dtype=torch.float32).view(3, 3, 2) / torch.tensor(STRIDES).view(3, 1, 1)) * 0.25
    det = types.SimpleNamespace(anchors=a0.clone(), stride=torch.tensor(STRIDES))
    model = types.SimpleNamespace(model=[det])
    msgs = []
    h = logging.Handler()
    h.emit = lambda rec: msgs.append(rec.getMessage())
    aa.LOGGER.addHandler(h)
    aa.LOGGER.setLevel(logging.INFO)
    seed(c["seed"])
    aa.check_anchors(ds, model, thr=c["thr"], imgsz=c["img_size"])
    aa.LOGGER.removeHandler(h)
    assert not torch.equal(det.anchors, a0), "the replacement branch did not run"
    seed(c["seed"])
    shapes = c["img_size"] * ds.shapes / ds.shapes.max(1, keepdims=True)
    scale = np.random.uniform(0.9, 1.1, size=(shapes.shape[0], 1))
    wh = np.concatenate([lb[:, 3:5] * s for s, lb in zip(shapes * scale, ds.labels)]).astype(np.float32)
    nb, npair = ar.metric_counts(wh, (a0 * torch.tensor(STRIDES).view(3, 1, 1)).view(-1, 2).numpy(), c["thr"])
    bpr, aat = np.float32(nb) / np.float32(len(wh)), np.float32(npair) / np.float32(len(wh))
    line = next(m for m in msgs if "Best Possible Recall" in m)
    assert f"{aat:.2f} anchors/target, {bpr:.3f} Best Possible Recall" in line, (line, aat, bpr)
    out.update(check_anchors_in=a0.numpy(), check_anchors_out=det.anchors.numpy(), check_counts=np.array([len(wh), nb, npair], np.int64))
    print("check_anchors:", line.strip(), "->", det.anchors.view(-1).tolist())
    path = os.path.join(ROOT, "tests", "golden", "autoanchor.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
