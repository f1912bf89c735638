"""CPU: the AutoAnchor kernels (yolov5_amd/csrc/autoanchor.h) on the HIP emulator against tests/autoanchor_ref.py, the fp64 restatement that
scripts/make_golden_autoanchor.py pins to the REFERENCE's kmean_anchors (evolution bit for bit) and to scipy's k-means (tests/golden/autoanchor.npz);
plus the host side of yolov5_amd/autoanchor.py: RNG stream positions, the fall-back branch, argument checks, header / EXPORTS agreement."""
import os
import random
import re
import types

import numpy as np
import pytest
import torch

from tests import autoanchor_ref as ar
from tests.hipemu import backend
from tests.hipemu.emu import aligned, emu, ptr
from yolov5_amd import _lib
from yolov5_amd import autoanchor as aa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "autoanchor.npz"))


def _a(x, dtype):
    x = np.asarray(x).astype(dtype)
    a = aligned(x.shape, dtype)
    a[...] = x
    return a


@pytest.fixture()
def seam():
    """The Python layer on CPU tensors against the host-compiled kernels."""
    backend.install()
    yield
    backend.uninstall()


# ---- raw C-ABI ------------------------------------------------------------------------------------------------------------------------------
def metric(wh, k, thr):
    lib = emu()
    W, K = _a(wh, np.float32), _a(k, np.float32)
    out = aligned((2,), np.int64, -1)
    rc = lib.y5_anchor_metric(ptr(W), len(wh), ptr(K), len(k), float(np.float32(1 / thr)), ptr(out), None)
    assert rc == 0, lib.y5_last_error()
    return int(out[0]), int(out[1])


def evolve(wh, k0, v, thr):
    lib = emu()
    W, K, V = _a(wh, np.float32), _a(k0, np.float64), _a(v, np.float64)
    f = aligned((1,), np.float64, -1.0)
    acc = aligned((len(v),), np.uint8, 7)
    ws = aligned((lib.y5_anchor_evolve_ws_bytes(len(wh)),), np.uint8)
    rc = lib.y5_anchor_evolve(ptr(W), len(wh), len(k0), ptr(K), ptr(f), 1, ptr(V), len(v), float(np.float32(1 / thr)), ptr(acc), ptr(ws), ws.nbytes, None)
    assert rc == 0, lib.y5_last_error()
    return K, float(f[0]), acc


def kmeans(obs, guess, poll=8):
    lib = emu()
    R, k = guess.shape[:2]
    O, Gs = _a(obs, np.float32), _a(guess, np.float32)
    book, alive = aligned((R, k, 2), np.float64), aligned((R, k), np.uint8)
    dist, iters, done = aligned((R,), np.float64), aligned((R,), np.int32), aligned((1,), np.int32)
    ws = aligned((lib.y5_anchor_kmeans_ws_bytes(len(obs), R, k),), np.uint8)
    init, polls = 1, 0
    while not done[0]:
        rc = lib.y5_anchor_kmeans(ptr(O), len(obs), ptr(Gs), R, k, init, poll, ptr(book), ptr(alive), ptr(dist), ptr(iters), ptr(done), ptr(ws), ws.nbytes, None)
        assert rc == 0, lib.y5_last_error()
        init, polls = 0, polls + 1
        assert polls < 100
    return book, alive != 0, dist, iters


@pytest.mark.parametrize("name", ["d34", "d247_thr35", "d247_n6"])
def test_emu_anchor_metric_counts_equal_restatement(name):
    wh, thr = G[f"{name}_wh"], ar.CASES[name]["thr"]
    for k in (G[f"{name}_ref"], G[f"{name}_ref"] * 0.25, G[f"{name}_k0"].astype(np.float32)):
        assert metric(wh, k, thr) == ar.metric_counts(wh, k, thr)


def test_emu_anchor_evolve_first_150_generations_equal_golden_prefix():
    """The draws are sequential, so the prefix of the 1000-generation run pinned to the reference is a 150-generation run."""
    name = "d247"
    wh = G[f"{name}_wh"]
    _, v = ar.case_draws(name, len(wh))
    assert np.array_equal(v[-1], G[f"{name}_v_last"])  # the re-drawn factors are the ones the golden run used
    k, f, acc = evolve(wh, G[f"{name}_k0"], v[:ar.PREFIX], ar.CASES[name]["thr"])
    assert np.array_equal(acc, G[f"{name}_accepted"][:ar.PREFIX])
    assert acc.sum() > 20
    assert np.array_equal(k, G[f"{name}_k150"])  # bit for bit
    assert abs(f - ar.fitness(wh, k, ar.CASES[name]["thr"])) <= 1e-12 * f  # the same fp64 sum taken in another order


def test_emu_anchor_evolve_is_deterministic_and_gen0_gives_the_fitness():
    wh = G["d34_wh"]
    _, v = ar.case_draws("d34", len(wh), gen=20)
    a = evolve(wh, G["d34_k0"], v, 4.0)
    b = evolve(wh, G["d34_k0"], v, 4.0)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2])
    k, f, _ = evolve(wh, G["d34_k0"], v[:0].reshape(0, 9, 2), 4.0)
    assert np.array_equal(k, G["d34_k0"]) and abs(f - ar.fitness(wh, G["d34_k0"], 4.0)) <= 1e-12 * f


@pytest.mark.parametrize("name", ["d34", "d247"])
def test_emu_anchor_kmeans_equals_restatement(name):
    wh = G[f"{name}_wh"]
    obs = wh / wh.std(0)
    idx = G[f"{name}_init"]
    ref = ar.kmeans(obs, idx)
    assert ref["winner"] == int(G[f"{name}_winner"]) and np.array_equal(ref["iters"], G[f"{name}_km_iters"])
    book, alive, dist, iters = kmeans(obs, obs[idx])
    assert np.array_equal(iters, ref["iters"])
    assert np.array_equal(alive, ref["alive"])
    assert int(np.argmin(dist)) == ref["winner"]
    np.testing.assert_allclose(dist, ref["dist"], rtol=1e-9, atol=0)
    np.testing.assert_allclose(book[alive], ref["book"][ref["alive"]], rtol=1e-9, atol=0)
    # the restatement (and so the kernel) against scipy's own book: 5x the float32 noise measured between the two
    w = ref["winner"]
    sb = G[f"{name}_scipy_book"]
    assert np.abs(ref["book"][w] - sb).max() / np.abs(sb).max() <= 1e-5


def test_emu_anchor_kmeans_drops_centroids_without_members():
    """Two coincident starting centroids: the later one never wins a tie, loses all members and is dead for the rest of its chain."""
    g = np.random.default_rng(2)
    obs = np.concatenate([g.normal(0, 0.1, (20, 2)), g.normal(3, 0.1, (21, 2))]).astype(np.float32)
    guess = np.stack([obs[[0, 0, 25]], obs[[1, 30, 2]]])
    ref = [ar.lloyd(obs, gs) for gs in guess]
    book, alive, dist, iters = kmeans(obs, guess, poll=3)
    assert alive.tolist() == [[True, False, True], [True, True, True]]
    for r in range(2):
        assert np.array_equal(alive[r], ref[r][1]) and iters[r] == ref[r][3]
        np.testing.assert_allclose(book[r][alive[r]], ref[r][0][ref[r][1]], rtol=1e-9)
        np.testing.assert_allclose(dist[r], ref[r][2], rtol=1e-9)


# ---- host side --------------------------------------------------------------------------------------------------------------------------------
def _reference_order_draws(gen, shape):
    """utils/autoanchor.py:151-153 written out (what the reference's loop consumes)."""
    npr = np.random
    for _ in range(gen):
        v = np.ones(shape)
        while (v == 1).all():
            v = ((npr.random(shape) < 0.9) * random.random() * npr.randn(*shape) * 0.1 + 1).clip(0.3, 3.0)


def test_draw_mutations_leaves_both_streams_where_the_reference_leaves_them():
    np.random.seed(4)
    random.seed(4)
    v = aa.draw_mutations(50, (9, 2))
    nxt = (np.random.random(), random.random())
    np.random.seed(4)
    random.seed(4)
    _reference_order_draws(50, (9, 2))
    assert nxt == (np.random.random(), random.random())
    np.random.seed(4)
    random.seed(4)
    assert np.array_equal(v, ar.draw_mutations(50, (9, 2)))
    assert v.shape == (50, 9, 2) and v.min() >= 0.3 and v.max() <= 3.0 and not (v == 1).all(axis=(1, 2)).any()


def test_draw_kmeans_init_leaves_the_stream_where_scipy_leaves_it():
    scipy_kmeans = pytest.importorskip("scipy.cluster.vq").kmeans

    obs = G["d34_wh"] / G["d34_wh"].std(0)
    np.random.seed(3)
    idx = aa.draw_kmeans_init(len(obs), 9)
    nxt = np.random.random()
    np.random.seed(3)
    scipy_kmeans(obs, 9, iter=30)
    assert nxt == np.random.random()
    assert np.array_equal(idx, G["d34_init"]) and all(len(set(r)) == 9 for r in idx.tolist())


def test_kmean_anchors_equals_the_two_stages_and_lands_on_the_reference(seam):
    name, c = "d34", ar.CASES["d34"]
    ds = ar.case_dataset(name)
    np.random.seed(c["seed"])
    random.seed(c["seed"])
    got = aa.kmean_anchors(ds, n=c["n"], img_size=c["img_size"], thr=c["thr"], gen=60, verbose=True, device="cpu")
    np.random.seed(c["seed"])
    random.seed(c["seed"])
    exp = ar.kmean_anchors(ds, n=c["n"], img_size=c["img_size"], thr=c["thr"], gen=60)
    assert got.dtype == np.float32 and got.shape == (9, 2)
    np.testing.assert_allclose(got, exp, rtol=1e-6)  # fp64 books agree to 1e-9, the float32 start of the evolution to an ulp
    assert np.all(np.diff(got.prod(1)) >= 0)


def test_kmean_anchors_falls_back_to_random_init(seam):
    ds = ar.make_dataset(2, per=(2, 2), seed=1, lo=0.1)  # 4 labels < 9 anchors
    np.random.seed(8)
    random.seed(8)
    got = aa.kmean_anchors(ds, n=9, img_size=640, thr=4.0, gen=30, verbose=False, device="cpu")
    np.random.seed(8)
    random.seed(8)
    exp, info = ar.kmean_anchors(ds, n=9, img_size=640, thr=4.0, gen=30, details=True)
    assert "kmeans" not in info  # the restatement took the fall-back too: no restart draws were consumed
    assert np.array_equal(got, exp)  # same random start -> the evolution is bit-exact


def test_check_anchors_replaces_in_place_and_returns_the_golden_counts(seam, monkeypatch):
    ds = ar.case_dataset("d247")
    c = ar.CASES["d247"]
    a0 = torch.from_numpy(G["check_anchors_in"]).clone()
    det = types.SimpleNamespace(anchors=a0.clone(), stride=torch.tensor([8.0, 16.0, 32.0]))
    tensor = det.anchors
    orig = aa.kmean_anchors
    # 1000 generations on the emulator take too long for a CPU test: 40 here, the full run against the reference's anchors is the GPU test's
    monkeypatch.setattr(aa, "kmean_anchors", lambda *a, **k: orig(*a, **{**k, "gen": 40}))
    np.random.seed(c["seed"])
    random.seed(c["seed"])
    bpr, aat, replaced = aa.check_anchors(ds, types.SimpleNamespace(model=[det]), thr=c["thr"], imgsz=c["img_size"])
    n, nb, npair = (int(x) for x in G["check_counts"])
    assert (bpr, aat) == (float(np.float32(nb) / np.float32(n)), float(np.float32(npair) / np.float32(n)))
    assert replaced and det.anchors is tensor and tensor._version > 0 and not torch.equal(tensor, a0)
    px = (tensor * det.stride.view(-1, 1, 1)).view(-1, 2)
    assert torch.all(px.prod(1)[1:] >= px.prod(1)[:-1])  # ascending with the strides


def test_check_anchors_leaves_well_fitting_anchors_alone(seam):
    ds = ar.case_dataset("d247")
    good = torch.from_numpy(G["check_anchors_out"]).clone()
    det = types.SimpleNamespace(anchors=good.clone(), stride=torch.tensor([8.0, 16.0, 32.0]))
    np.random.seed(11)
    random.seed(11)
    before = random.getstate()
    bpr, aat, replaced = aa.check_anchors(ds, types.SimpleNamespace(model=[det]), thr=4.0, imgsz=640)
    assert bpr > 0.98 and not replaced and det.anchors._version == 0 and torch.equal(det.anchors, good)
    assert random.getstate() == before  # only the augment-scale draw of np.random was consumed


def test_argument_checks(seam):
    wh = torch.from_numpy(G["d34_wh"])
    with pytest.raises(ValueError, match=r"\(n, 2\)"):
        aa.anchor_metric(wh.view(-1), np.ones((9, 2)), 4.0)
    with pytest.raises(ValueError, match="positive"):
        aa.anchor_metric(wh, np.ones((9, 2)), 0.0)
    with pytest.raises(ValueError, match="need n >= 1"):
        aa.anchor_metric(wh, np.ones((41, 2)), 4.0)
    with pytest.raises(ValueError, match="restarts, k, 2"):
        aa.anchor_kmeans(wh, np.ones((3, 2)))
    with pytest.raises(ValueError, match="not supported"):
        aa.anchor_kmeans(wh, np.ones((300, 2, 2)))
    with pytest.raises(NotImplementedError, match="yaml"):
        aa.kmean_anchors("data/coco128.yaml")
    with pytest.raises(ValueError, match="1 <= n <= 40"):
        aa.kmean_anchors(ar.case_dataset("d34"), n=41, device="cpu")
    lib = emu()
    W = _a(G["d34_wh"], np.float32)
    K = _a(np.ones((9, 2)), np.float64)
    bad = _lib.Y5_ERR_BAD_ARG
    assert lib.y5_anchor_metric(None, 10, ptr(K), 9, 0.25, ptr(K), None) == bad
    assert lib.y5_anchor_evolve(ptr(W), 10, 9, ptr(K), ptr(K), 1, None, 5, 0.25, None, ptr(K), 4096, None) == bad
    assert lib.y5_anchor_evolve(ptr(W), 10, 9, ptr(K), ptr(K), 1, None, 0, 0.25, None, ptr(K), 8, None) == _lib.Y5_ERR_WORKSPACE
    assert lib.y5_anchor_evolve_ws_bytes(0) == 0 and lib.y5_anchor_kmeans_ws_bytes(10, 0, 9) == 0 and lib.y5_anchor_kmeans_ws_bytes(10, 30, 300) == 0
    i = _a(np.zeros(64), np.int32)
    assert lib.y5_anchor_kmeans(ptr(W), 5, ptr(W), 2, 9, 1, 1, ptr(K), ptr(K), ptr(K), ptr(i), ptr(i), ptr(K), 1 << 20, None) == bad  # k > n
    assert lib.y5_anchor_kmeans(ptr(W), 38, ptr(W), 200, 10, 1, 1, ptr(K), ptr(K), ptr(K), ptr(i), ptr(i), ptr(K), 1 << 20, None) == _lib.Y5_ERR_UNSUPPORTED


def test_without_the_seam_cpu_tensors_are_refused():
    with pytest.raises(RuntimeError, match="GPU"):
        aa.anchor_metric(torch.ones(4, 2), np.ones((3, 2)), 4.0)


def test_header_declares_the_autoanchor_entries_bound_in_exports():
    hdr = open(os.path.join(ROOT, "include", "yolov5_hip.h")).read()
    declared = {n for n in re.findall(r"\b(y5_anchor_[a-z0-9_]+)\s*\(", hdr)}
    assert declared == {n for n in _lib.EXPORTS if n.startswith("y5_anchor_")} == {
        "y5_anchor_metric", "y5_anchor_evolve", "y5_anchor_evolve_ws_bytes", "y5_anchor_kmeans", "y5_anchor_kmeans_ws_bytes"}
    assert "utils/autoanchor.py" in hdr


def test_mosaic_loaders_expose_shapes():
    from yolov5_amd.dataloaders import MosaicLoader

    imgs = [torch.zeros(48, 64, 3, dtype=torch.uint8), torch.zeros(80, 32, 3, dtype=torch.uint8)]
    ld = MosaicLoader(imgs, [np.zeros((0, 5), np.float32)] * 2, img_size=64, batch_size=2)
    assert ld.shapes.dtype == np.float64 and ld.shapes.tolist() == [[64.0, 48.0], [32.0, 80.0]]
