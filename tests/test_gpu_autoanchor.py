"""GPU: AutoAnchor (yolov5_amd/autoanchor.py over csrc/autoanchor.h) on the MI355X.

  * the full 1000-generation evolution of every golden case: accept flags and final anchors bit-equal to what the REFERENCE's kmean_anchors
    returned (tests/golden/autoanchor.npz, scripts/make_golden_autoanchor.py), started from the book scipy handed it;
  * 70 001 label sizes (many workgroups, a tail, the partial reduction), 100 generations, against the fp64 restatement (tests/autoanchor_ref.py)
    after checking that the restatement's own decision gaps admit no flip (>= 1e-9; an fp64 sum of <= 2^20 terms in another order moves < 1e-10);
  * k-means on 2180 and 19 457 points against the restatement: same iteration counts and winner, book and distances within 1e-9 relative;
  * determinism, kmean_anchors = its two stages composed, check_anchors on a live yolov5n (engine and loss pick the new anchors up),
    train_loop.train(autoanchor=...)."""
import os
import random

import numpy as np
import pytest
import torch

from oracle import detgen, yolo_oracle as yo
from tests import autoanchor_ref as ar

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "autoanchor.npz"))
K0 = np.array([[10, 13], [16, 30], [33, 23], [30, 61], [62, 45], [59, 119], [116, 90], [156, 198], [373, 326]], np.float64)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _seed(s):
    np.random.seed(s)
    random.seed(s)


@pytest.fixture(scope="module")
def big():
    """70 001 synthetic label sizes, 100 pre-drawn generations and the restatement's chain over them (computed once, never modified)."""
    wh = ar.synthetic_wh(70001, seed=0)
    _seed(0)
    v = ar.draw_mutations(100, (9, 2))
    k, f, acc, gaps, _ = ar.evolve(wh, K0, v, 4.0)
    return dict(wh=wh, v=v, k=k, f=f, acc=acc, gaps=gaps)


@pytest.mark.parametrize("name", list(ar.CASES))
def test_evolve_1000_generations_bit_equal_to_the_reference(dev, name):
    from yolov5_amd import autoanchor as aa

    wh = G[f"{name}_wh"]
    _, v = ar.case_draws(name, len(wh))
    assert np.array_equal(v[-1], G[f"{name}_v_last"])
    k, f, acc = aa.anchor_evolve(torch.from_numpy(wh).to(dev), G[f"{name}_k0"], v, ar.CASES[name]["thr"])
    assert np.array_equal(acc, G[f"{name}_accepted"]), np.flatnonzero(acc != G[f"{name}_accepted"])[:5]
    assert np.array_equal(k, G[f"{name}_k1000"])
    assert np.array_equal(k[np.argsort(k.prod(1))].astype(np.float32), G[f"{name}_ref"])  # what the reference returned
    assert abs(f - ar.fitness(wh, k, ar.CASES[name]["thr"])) <= 1e-12 * f


def test_evolve_70001_labels_vs_restatement(dev, big):
    from yolov5_amd import autoanchor as aa

    assert big["gaps"].min() >= 1e-9 and big["acc"].sum() > 10  # the fixture admits no flipped decision
    k, f, acc = aa.anchor_evolve(torch.from_numpy(big["wh"]).to(dev), K0, big["v"], 4.0)
    assert np.array_equal(acc, big["acc"])
    assert np.array_equal(k, big["k"])
    assert abs(f - big["f"]) <= 1e-10 * f
    nb, npair = aa.anchor_metric(torch.from_numpy(big["wh"]).to(dev), k.astype(np.float32), 4.0)
    assert (nb, npair) == ar.metric_counts(big["wh"], k.astype(np.float32), 4.0)


def _kmeans_vs_restatement(dev, obs, idx):
    from yolov5_amd import autoanchor as aa

    ref = ar.kmeans(obs, idx)
    d = np.sort(ref["dist"])
    assert ref["margins"].min() >= 1e-9 and (d[1] - d[0]) / d[0] >= 1e-6  # no stop decision and no winner the device could flip
    got = aa.anchor_kmeans(torch.from_numpy(obs).to(dev), obs[idx])
    assert np.array_equal(got["iters"], ref["iters"]) and np.array_equal(got["alive"], ref["alive"])
    assert got["winner"] == ref["winner"]
    np.testing.assert_allclose(got["dist"], ref["dist"], rtol=1e-9, atol=0)
    np.testing.assert_allclose(got["book"][got["alive"]], ref["book"][ref["alive"]], rtol=1e-9, atol=0)
    return got, ref


def test_kmeans_2180_points_vs_restatement_and_scipy_book(dev):
    wh = G["d2080_wh"]
    got, ref = _kmeans_vs_restatement(dev, wh / wh.std(0), G["d2080_init"])
    assert ref["winner"] == int(G["d2080_winner"])
    sb = G["d2080_scipy_book"]
    assert np.abs(got["book"][got["winner"]] - sb).max() / np.abs(sb).max() <= 1e-5  # scipy's float32 noise, 5x the measured 2.1e-6


def test_kmeans_19457_points_vs_restatement(dev):
    wh = ar.synthetic_wh(19457, seed=1)
    obs = wh / wh.std(0)
    np.random.seed(1)
    _kmeans_vs_restatement(dev, obs, ar.draw_kmeans_init(len(obs), 9))


def test_two_runs_are_bit_identical(dev, big):
    from yolov5_amd import autoanchor as aa

    wh = torch.from_numpy(big["wh"]).to(dev)
    a, b = (aa.anchor_evolve(wh, K0, big["v"][:30], 4.0) for _ in range(2))
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2])
    obs = big["wh"] / big["wh"].std(0)
    guess = obs[np.random.default_rng(0).choice(len(obs), (12, 9))]
    p, q = (aa.anchor_kmeans(torch.from_numpy(obs).to(dev), guess) for _ in range(2))
    for key in ("book", "dist", "alive", "iters"):
        assert np.array_equal(p[key], q[key]), key


def test_kmean_anchors_equals_its_two_stages_composed(dev):
    from yolov5_amd import autoanchor as aa

    name, c = "d2080", ar.CASES["d2080"]
    ds = ar.case_dataset(name)
    _seed(c["seed"])
    got = aa.kmean_anchors(ds, n=c["n"], img_size=c["img_size"], thr=c["thr"], gen=200, verbose=True, device=dev)
    _seed(c["seed"])
    _, wh = ar.label_wh(ds, c["img_size"])
    assert np.array_equal(wh, G[f"{name}_wh"])
    s = wh.std(0)
    obs = wh / s
    km = aa.anchor_kmeans(torch.from_numpy(obs).to(dev), obs[aa.draw_kmeans_init(len(wh), c["n"])])
    k = km["book"][km["winner"]].astype(np.float32) * s
    k = k[np.argsort(k.prod(1))]
    k, _, _ = aa.anchor_evolve(torch.from_numpy(wh).to(dev), k, aa.draw_mutations(200, k.shape), c["thr"])
    assert got.dtype == np.float32 and np.array_equal(got, k[np.argsort(k.prod(1))].astype(np.float32))
    # and the whole call lands on the reference's anchors up to the float32 rounding of scipy's book it started from
    _seed(c["seed"])
    full = aa.kmean_anchors(ds, n=c["n"], img_size=c["img_size"], thr=c["thr"], gen=ar.GEN, verbose=False, device=dev)
    np.testing.assert_allclose(full, G[f"{name}_ref"], rtol=0, atol=1e-5 * float(G[f"{name}_ref"].max()))


def _yolov5n(dev, seed=0):
    from yolov5_amd.yolo import DetectionModel

    cfg = yo.model_cfg("yolov5n")
    m = DetectionModel("yolov5n.yaml")
    m.load_state_dict(yo.det_state_dict(cfg, seed, fused=False))
    return m.to(dev)


def test_check_anchors_replaces_shrunken_anchors_and_engine_and_loss_follow(dev):
    from yolov5_amd import autoanchor as aa
    from yolov5_amd.loss import ComputeLoss
    from yolov5_amd.train_loop import HYP_SCRATCH_LOW

    c = ar.CASES["d247"]
    ds = ar.case_dataset("d247")
    m = _yolov5n(dev)
    m.hyp = dict(HYP_SCRATCH_LOW)
    det = m.model[-1]
    with torch.no_grad():
        det.anchors.copy_(torch.from_numpy(G["check_anchors_in"]))  # yolov5n's anchors scaled by 0.25
    x = torch.from_numpy(detgen.uniform((2, 3, 64, 64), 0.0, 1.0, name="img", seed=0)).to(dev)
    t = torch.from_numpy(detgen.synth_targets(2, 4, seed=3)).to(dev)
    compute_loss = ComputeLoss(m)
    z_old = m.eval()(x)[0].clone()              # plans and the loss's host copy exist before the anchors change
    loss_old = compute_loss(m.train()(x), t)[0].detach().clone()
    tensor = det.anchors
    _seed(c["seed"])
    bpr, aat, replaced = aa.check_anchors(ds, m, thr=c["thr"], imgsz=c["img_size"])
    n, nb, npair = (int(v) for v in G["check_counts"])
    assert (bpr, aat) == (float(np.float32(nb) / np.float32(n)), float(np.float32(npair) / np.float32(n)))
    assert replaced and det.anchors is tensor
    ref = G["check_anchors_out"]  # the reference's result; ours starts the evolution from the fp64 book instead of scipy's float32 one
    np.testing.assert_allclose(tensor.cpu().numpy(), ref, rtol=0, atol=1e-5 * float(ref.max()))
    z_new = m.eval()(x)[0]
    loss_new = compute_loss(m.train()(x), t)[0].detach()
    # a model CONSTRUCTED with the new anchors and taken through the same calls (the train-mode forwards move the BatchNorm statistics)
    # computes the same as the one whose anchors were replaced under a live engine and a live loss
    m2 = _yolov5n(dev)
    m2.hyp = dict(HYP_SCRATCH_LOW)
    with torch.no_grad():
        m2.model[-1].anchors.copy_(tensor)
    loss2 = ComputeLoss(m2)
    m2.eval()(x)
    loss2(m2.train()(x), t)
    z_ref = m2.eval()(x)[0]
    loss_ref = loss2(m2.train()(x), t)[0].detach()
    assert torch.allclose(z_new, z_ref, rtol=1e-4, atol=1e-4) and not torch.allclose(z_new, z_old, rtol=1e-2, atol=1e-2)
    assert torch.allclose(loss_new, loss_ref, rtol=1e-5, atol=0) and not torch.allclose(loss_new, loss_old, rtol=1e-3, atol=0)


def test_check_anchors_leaves_well_fitting_anchors_untouched(dev):
    from yolov5_amd import autoanchor as aa

    ds = ar.case_dataset("d247")
    m = _yolov5n(dev)
    det = m.model[-1]
    with torch.no_grad():
        det.anchors.copy_(torch.from_numpy(G["check_anchors_out"]))
    ver, before = det.anchors._version, det.anchors.clone()
    _seed(11)
    state = random.getstate()
    bpr, aat, replaced = aa.check_anchors(ds, m, thr=4.0, imgsz=640)
    assert bpr > 0.98 and not replaced and det.anchors._version == ver and torch.equal(det.anchors, before)
    assert random.getstate() == state


def _mosaic_loader(dev, seed=4):
    """16 images of 96..160 px whose labels are small boxes (2..12 % of the image): yolov5n's COCO anchors recall few of them at 128 px."""
    from yolov5_amd.dataloaders import MosaicLoader

    g = np.random.default_rng(seed)
    imgs, labels = [], []
    for _ in range(16):
        h, w = (int(v) for v in g.integers(96, 161, 2))
        imgs.append(torch.from_numpy(g.integers(0, 256, (h, w, 3), dtype=np.uint8)).to(dev))
        m = int(g.integers(3, 7))
        lb = np.zeros((m, 5), np.float32)
        lb[:, 0] = g.integers(0, 80, m)
        lb[:, 1:3] = g.uniform(0.2, 0.8, (m, 2))
        lb[:, 3:5] = g.uniform(0.02, 0.12, (m, 2))
        labels.append(lb)
    return MosaicLoader(imgs, labels, img_size=128, batch_size=8, seed=seed)


def test_train_loop_with_autoanchor_trains_on_replaced_anchors(dev):
    from yolov5_amd import train_loop

    m = _yolov5n(dev)
    a0 = m.model[-1].anchors.clone()
    loader = _mosaic_loader(dev)
    assert loader.shapes.shape == (16, 2)
    _seed(6)
    res = train_loop.train(m, loader, epochs=1, device=dev, batch_size=8, autoanchor=loader)
    bpr, aat, replaced = res["autoanchor"]
    assert bpr <= 0.98 and replaced
    a1 = m.model[-1].anchors
    assert not torch.equal(a1, a0)
    # the EMA copy was made after the replacement (its buffers then follow d * ema + (1 - d) * model: equal up to fp32 rounding)
    assert torch.allclose(res["ema"].ema.model[-1].anchors, a1, rtol=1e-5, atol=0)
    px = (a1 * m.model[-1].stride.view(-1, 1, 1)).view(-1, 2)
    assert float(px.max()) < 40  # fitted to the small boxes (imgsz defaulted to the loader's 128), not COCO's 373 x 326
    assert res["losses"].shape == (2, 3) and bool(torch.isfinite(res["losses"]).all())


def test_train_loop_without_autoanchor_is_unchanged(dev):
    """autoanchor=None (the default) adds nothing: no RNG draw, anchors untouched, and the same losses as a call that does not name the
    argument -- the call every earlier test makes (tests/test_gpu_loops.py pins those against the oracle, unchanged)."""
    from oracle import train_oracle as to
    from yolov5_amd.train_loop import TensorLoader, train

    imgs, tpi = to.synthetic_set(8, 64, per_img=3, seed=2)
    out = []
    for kw in ({}, {"autoanchor": None, "imgsz": 64}):
        m = _yolov5n(dev, seed=1)
        ver = m.model[-1].anchors._version
        _seed(9)
        state = (random.getstate(), np.random.get_state()[1].copy())
        res = train(m, TensorLoader(imgs.to(dev), [t.to(dev) for t in tpi], 4), hyp=dict(to.HYP), epochs=2, device=dev, amp=False, **kw)
        assert random.getstate() == state[0] and np.array_equal(np.random.get_state()[1], state[1])
        assert m.model[-1].anchors._version == ver and res["autoanchor"] is None
        out.append(res["losses"].numpy())
    # fp32 plan; 1e-3 relative is the per-step bound tests/test_gpu_loops.py holds this loop to against the oracle
    np.testing.assert_allclose(out[1], out[0], rtol=1e-3, atol=0)
