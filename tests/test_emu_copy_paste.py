"""CPU (emulator): the copy-paste augmentation of the mosaic loaders (yolov5_amd/dataloaders.py `_copy_paste`, csrc/copy_paste.h
`y5_paste_planes`, the paste redirect of csrc/augment.hip `y5_mosaic_batch_paste`) against the batches the REFERENCE's own loaders produced with
hyp['copy_paste'] > 0 (tests/golden/copy_paste_{seg,det}.npz, scripts/make_golden_copy_paste.py) with the draws reproduced from the same
seeds: images bit-identical, targets identical (values and row order), masks bit-identical, NO tolerance.  Then the rasteriser and the paste
launch directly against the NumPy restatement (tests/copy_paste_ref.py) on cases built to break the row-band scheme, the geometry check that
does not rest on the restatement, the draw order, and the pins that stay."""
import ctypes as C
import os
import random

import numpy as np
import pytest
import torch

from oracle import augment_oracle as ao
from tests import copy_paste_ref as cp, seg_data_ref as sd
from tests.hipemu import backend as emu_backend

GOLD = os.path.join(os.path.dirname(__file__), "golden")
HYP = dict(ao.HYP_AUG, degrees=5.0, shear=2.0, flipud=0.3)
DEV = torch.device("cpu")
IDX3 = lambda s: (s % 6, (s + 2) % 6, (s + 4) % 6)  # noqa: E731
CONFIGS = {  # name -> (hyp, seeds, indices of the batch): scripts/make_golden_copy_paste.py:CONFIGS
    "mosaic": (dict(HYP, copy_paste=0.5), (1,), lambda s: (s % 6, (s + 3) % 6)),
    "mixed": (dict(HYP, mosaic=0.5, copy_paste=1.0), (11, 13), IDX3),
    "mixup": (dict(HYP, mixup=0.5, copy_paste=0.5), (24,), IDX3),
}
CASES = [(kind, n, s) for kind in ("seg", "det") for n, (_, seeds, _) in CONFIGS.items() for s in seeds]
BAND = 32   # csrc/copy_paste.h


@pytest.fixture(autouse=True)
def _seam():
    emu_backend.install()
    yield
    emu_backend.uninstall()


def dataset(device=DEV):
    from yolov5_amd.dataloaders import labels_from_segments

    ims, classes, segments = sd.polygon_dataset(6, seed=3)
    labels = [labels_from_segments(c, sg) for c, sg in zip(classes, segments)]
    return [torch.from_numpy(im).to(device) for im in ims], labels, segments


def check_golden(kind, name, seed, device=DEV):
    from yolov5_amd.dataloaders import draw_sample, draw_sample_seg, mosaic_batch, seg_mosaic_batch

    hyp, _, idx = CONFIGS[name]
    g = np.load(os.path.join(GOLD, f"copy_paste_{kind}.npz"))
    s, (overlap, ratio) = int(g["s"]), g[f"{name}_cfg"]
    ims, labels, segments = dataset(device)
    counts = [len(sg) for sg in segments]
    draws = []
    for index in idx(seed):
        random.seed(seed * 10 + index)            # the generators the reference consumed (scripts/make_golden_copy_paste.py)
        np.random.seed(seed * 10 + index)
        draws.append((draw_sample_seg if kind == "seg" else draw_sample)(index, 6, s, hyp, counts=counts))
    assert [d["mosaic"] for d in draws] == list(g[f"{name}_mosaic{seed}"])
    if kind == "seg":
        imgs, targets, masks = seg_mosaic_batch(ims, labels, segments, draws, s, hyp, dtype=torch.uint8, overlap=bool(overlap), mask_ratio=int(ratio))
    else:
        imgs, targets = mosaic_batch(ims, labels, draws, s, hyp, dtype=torch.uint8, segments=segments)
    assert np.array_equal(imgs.cpu().numpy(), g[f"{name}_img{seed}"])
    assert targets.shape == g[f"{name}_lab{seed}"].shape
    np.testing.assert_array_equal(targets.numpy(), g[f"{name}_lab{seed}"])
    if kind == "seg":
        assert masks.dtype == torch.uint8 and tuple(masks.shape) == g[f"{name}_mask{seed}"].shape
        assert np.array_equal(masks.cpu().numpy(), g[f"{name}_mask{seed}"])
    return draws


# ---- y5_paste_planes against the restatement -----------------------------------------------------------------------------------------------
def raster_cases():
    """(name, S2, n_planes, [(int32 polygon, plane)]): cases built to break the band scheme of csrc/copy_paste.h (BAND rows per workgroup)."""
    sq = lambda x0, y0, x1, y1: np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], np.int32)  # noqa: E731
    S2 = 100    # four bands, the last one of 4 rows; not a multiple of 32: the last word of a row holds 4 valid bits
    spans = np.array([[10, BAND - 1], [60, BAND - 1], [80, 2 * BAND], [70, 3 * BAND - 1], [40, 3 * BAND - 1], [20, 3 * BAND], [5, 2 * BAND]], np.int32)
    # ^ horizontal edges exactly on the last row of band 0 and of band 2, vertices on the first row of bands 2 and 3: spans all four bands
    overlap = [(sq(10, 10, 60, 70), 0), (np.array([[30, 40], [90, 45], [50, 95]], np.int32), 0)]   # union, not xor, across a band border
    edges = [(np.array([[0, 0], [S2, 0], [S2, 40], [0, 20]], np.int32), 0), (np.array([[S2, S2], [50, S2], [S2, 60]], np.int32), 0),
             (np.array([[0, 50], [30, S2], [0, S2]], np.int32), 0)]                                   # points at 0 and at S2: clip_line
    degenerate = [(np.array([[5, 5], [40, 40], [70, 70]], np.int32), 0), (np.array([[20, 64], [20, 64], [20, 64]], np.int32), 0),
                  (np.array([[3, 31], [90, 31]], np.int32), 0), (np.array([[50, 33]], np.int32), 0)]   # collinear; one repeated point; 2 and 1 points
    star = np.array([(50 + 45 * np.cos(a) * (1 if k % 2 else 0.4), 50 + 45 * np.sin(a) * (1 if k % 2 else 0.4))
                     for k, a in enumerate(np.linspace(0, 2 * np.pi, 14, endpoint=False))]).astype(np.int32)
    gap = [(sq(2, 2, 30, 40), 0), (star, 2), (sq(60, 60, 99, 99), 2), (sq(0, 90, 10, 99), 4)]       # planes 1 and 3 own no polygon
    S3 = 3 * BAND   # a multiple of 32, exactly three bands
    # more polygons in one plane than the band's bit map of reached polygons covers (MAX_MARKED = 1024): the first 1024 stay in bands 0 and 1,
    # the 40 behind them, which are never skipped, fill the bands below
    tri = lambda x, y, k: np.array([[x, y], [x + 4 + k % 3, y + 1], [x + 2, y + 5 + k % 2]], np.int32)  # noqa: E731
    many = [(tri(7 * k % 90, 11 * k % 50, k), 0) for k in range(1024)] + [(tri(13 * k % 90, 64 + 9 * k % 30, k), 0) for k in range(40)]
    return [("many_polygons", S2, 1, many), ("spans_bands", S2, 1, [(spans, 0)]), ("overlap_union", S2, 1, overlap), ("canvas_edge", S2, 1, edges),
            ("degenerate", S2, 1, degenerate), ("plane_gap", S2, 5, gap),
            ("three_bands", S3, 2, [(np.array([[0, 0], [S3, 31], [S3 - 1, 64], [3, S3]], np.int32), 0), (star + 20, 1), (sq(31, 31, 32, 64), 1)])]


def kernel_planes(polys, plane, n_planes, S2, device=DEV):
    from yolov5_amd.dataloaders import paste_planes

    return paste_planes(polys, plane, n_planes, S2, device).cpu().numpy().view(np.uint32)


def check_raster(name, device=DEV):
    _, S2, n_planes, items = next(c for c in raster_cases() if c[0] == name)
    polys, plane = [p for p, _ in items], [k for _, k in items]
    ref = cp.reference_planes(polys, plane, n_planes, S2)
    assert ref.any()
    got = kernel_planes(polys, plane, n_planes, S2, device)
    assert got.shape == ref.shape and np.array_equal(got, ref), name
    if name == "plane_gap":
        assert not got[1].any() and not got[3].any() and got[4].any()
    if name == "overlap_union":   # the intersection of the two polygons is set (an xor of the two fills would clear it)
        both = cp.plane_mask(polys[:1], S2) & cp.plane_mask(polys[1:], S2)
        assert both.sum() > 100 and cp.unpack_bits(got, S2)[0][both != 0].all()


def kernel_fill(pts, size, device=DEV):
    return cp.unpack_bits(kernel_planes([np.asarray(pts, np.int32)], [0], 1, size, device), size)[0]


def check_geometry(device=DEV):
    """Does not rest on the restatement (tests/seg_data_ref.check_fill_geometry): an axis-aligned rectangle that crosses a band border fills
    exactly its inclusive pixel rectangle; convex integer polygons on a three-band plane."""
    m = kernel_fill([[3, 20], [50, 20], [50, 70], [3, 70]], 96, device)
    exp = np.zeros((96, 96), np.uint8)
    exp[20:71, 3:51] = 1
    assert np.array_equal(m, exp)
    for p in sd.convex_polygons(12, 96, seed=5):
        sd.check_fill_geometry(kernel_fill(p, 96, device), p)


# ---- y5_mosaic_batch_paste against the restatement -------------------------------------------------------------------------------------------
def render_batch(device=DEV):
    """A batch that mixes a pasting mosaic, a non-pasting mosaic, a letterbox job and a mixup pair whose partner (only) pastes.
    -> (images, jobs, draws, pasted {job: polygons}, s, hyp)."""
    from yolov5_amd import _lib
    from yolov5_amd.dataloaders import _fill_job, _finish_job

    s = 48
    ims, _, _ = dataset(device)
    rnd = random.Random(7)
    nrnd = np.random.RandomState(7)

    def draw(mosaic, index):
        d = {"mosaic": mosaic, "angle": rnd.uniform(-5, 5), "scale": rnd.uniform(0.6, 1.4), "shear": (rnd.uniform(-2, 2), rnd.uniform(-2, 2)),
             "translate": (rnd.uniform(0.4, 0.6), rnd.uniform(0.4, 0.6)), "hsv": nrnd.uniform(-1, 1, 3) * [0.015, 0.7, 0.4] + 1,
             "flipud": rnd.random() < 0.5, "fliplr": rnd.random() < 0.5, "indices": [index]}
        if mosaic:
            d["yc"], d["xc"] = (int(rnd.uniform(s // 2, 2 * s - s // 2)) for _ in range(2))
            d["indices"] = [index, *rnd.choices(range(6), k=3)]
        return d

    draws = [draw(True, 0), draw(True, 1), draw(False, 2), draw(True, 3)]
    draws[3]["partner"], draws[3]["mix_r"] = draw(True, 4), 0.41
    tri = lambda cx, cy, r: np.array([[cx - r, cy - r // 2], [cx + r, cy], [cx - r // 3, cy + r]], np.int32)  # noqa: E731
    pasted = {0: [tri(30, 40, 22), np.array([[50, 5], [96, 5], [96, 60], [70, 30]], np.int32)], 4: [tri(60, 50, 30)]}
    jobs = (_lib.MosaicJob * 5)()
    for b, d in enumerate(draws):
        _fill_job(jobs[b], ims, d, s)
        _finish_job(jobs[b], d, True)
    _fill_job(jobs[4], ims, draws[3]["partner"], s)
    jobs[3].mix_job, jobs[3].mix_r = 5, 0.41
    return ims, jobs, draws, pasted, s, HYP


def check_render(device=DEV):
    from yolov5_amd.dataloaders import _render

    ims, jobs, draws, pasted, s, hyp = render_batch(device)
    out = _render(jobs, 4, s, device, torch.uint8, False, pasted).cpu().numpy()
    host = [im.cpu().numpy() for im in ims]
    ref = np.stack([cp.render(host, d, s, hyp, pasted.get(b), pasted.get(4) if b == 3 else None) for b, d in enumerate(draws)])
    assert np.array_equal(out, ref)
    plain = _render(jobs, 4, s, device, torch.uint8, False).cpu().numpy()
    assert not np.array_equal(plain[0], out[0]) and not np.array_equal(plain[3], out[3])      # the paste and the partner's paste are visible
    assert np.array_equal(plain[1], out[1]) and np.array_equal(plain[2], out[2])
    return jobs, s, plain


def check_no_plane_identity(device=DEV):
    """y5_mosaic_batch_paste with every job_plane = -1 (and a plane full of ones nobody may read) is y5_mosaic_batch, byte for byte."""
    from yolov5_amd import _lib

    ims, jobs, _, _, s, _ = render_batch(device)      # ims: the job table points into them
    lib = _lib.lib()
    table = _lib.device_table(jobs, device)
    job_plane = torch.full((5,), -1, dtype=torch.int32, device=device)
    planes = torch.full((1, 2 * s, (2 * s + 31) // 32), -1, dtype=torch.int32, device=device)
    for dtype in (torch.uint8, torch.float16):
        a, b = (torch.empty((4, 3, s, s), dtype=dtype, device=device) for _ in range(2))
        args = (4, s, 114, None, _lib.dtype_code(dtype), int(dtype != torch.uint8), _lib.stream(device))
        _lib.check(lib.y5_mosaic_batch(C.c_void_p(table.data_ptr()), *args[:3], C.c_void_p(a.data_ptr()), *args[4:]), lib)
        _lib.check(lib.y5_mosaic_batch_paste(C.c_void_p(table.data_ptr()), 5, C.c_void_p(job_plane.data_ptr()), C.c_void_p(planes.data_ptr()),
                                             *args[:3], C.c_void_p(b.data_ptr()), *args[4:]), lib)
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    del ims


# ---- tests -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,name,seed", CASES)
def test_batches_match_reference_golden(kind, name, seed):
    draws = check_golden(kind, name, seed)
    pastes = [d for d in draws if d.get("paste")] + [d["partner"] for d in draws if d.get("partner") is not None and d["partner"].get("paste")]
    assert pastes, "the fixture must paste"
    if name == "mixup":
        assert any(d.get("partner") is not None and d["partner"].get("paste") for d in draws), "a mixup partner must paste"


@pytest.mark.parametrize("name", [c[0] for c in raster_cases()])
def test_paste_planes_match_restatement(name):
    check_raster(name)


def test_paste_render_matches_restatement():
    check_render()


def test_no_plane_launch_is_mosaic_batch():
    check_no_plane_identity()


def test_fill_geometry_independent_of_the_restatement():
    check_geometry()


def test_restatement_copy_paste_is_the_plane_redirect():
    """tests/copy_paste_ref.copy_paste (the reference's function on a materialised canvas) and the plane redirect the kernel implements
    (`warped`: canvas[y, x] = canvas_before[y, w - 1 - x] where the un-flipped raster covers (y, w - 1 - x)) are the same image."""
    rng = np.random.default_rng(0)
    w = 64
    im = rng.integers(0, 256, (w, w, 3), dtype=np.uint8)
    segs = [np.array([[5, 5], [30, 8], [12, 40]], np.float32), np.array([[40.7, 30.2], [63.9, 35.5], [50.1, 60.0]], np.float32)]
    labels = np.array([[1, 5, 5, 30, 40], [2, 40.7, 30.2, 63.9, 60]], np.float32)
    before = im.copy()
    out, lab, sg, acc = cp.copy_paste(im, labels, [x.copy() for x in segs], [1, 0])
    assert acc == [1, 0] and len(lab) == 4 and len(sg) == 4
    m = cp.plane_mask([segs[j].astype(np.int32) for j in acc], w)
    exp = before.copy()
    ys, xs = np.nonzero(m[:, ::-1])
    exp[ys, xs] = before[ys, w - 1 - xs]
    assert np.array_equal(out, exp) and not np.array_equal(out, before)


def test_draw_order_and_pins():
    from yolov5_amd.dataloaders import MosaicLoader, SegMosaicLoader, draw_sample, draw_sample_seg, mosaic_batch

    ims, labels, segments = dataset()
    counts = [len(sg) for sg in segments]
    s, hyp = 96, dict(HYP, copy_paste=0.5)
    for draw, shuffle in ((draw_sample_seg, False), (draw_sample, True)):
        # hand-run of the reference's consumption (mosaic = 1, mixup = 0): gate; yc, xc; choices; (shuffle); random.sample; the eight; mixup gate;
        # flipud, fliplr
        r = random.Random(31)
        r.random()
        _ = [r.uniform(-x, 2 * s + x) for x in (-s // 2, -s // 2)]
        idx = [2, *r.choices(range(6), k=3)]
        if shuffle:
            r.shuffle(idx)
        n = sum(counts[i] for i in idx)
        sample = r.sample(range(n), k=round(0.5 * n))
        _ = [r.uniform(0, 1) for _ in range(8)]
        _ = r.random(), r.random(), r.random()
        g, npg = random.Random(31), np.random.RandomState(31)
        d = draw(2, 6, s, hyp, g, npg, counts=counts)
        assert d["indices"] == idx and d["paste"] == sample and len(sample) == round(0.5 * n) > 0
        assert g.getstate() == r.getstate()
        # copy_paste = 0: today's draws, whether counts are given or not
        a = draw(2, 6, s, HYP, random.Random(31), np.random.RandomState(31))
        b = draw(2, 6, s, HYP, random.Random(31), np.random.RandomState(31), counts=counts)
        assert "paste" not in a and a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
        assert a["indices"] == idx and a["angle"] != d["angle"]
    with pytest.raises(NotImplementedError):
        draw_sample_seg(0, 6, 64, hyp)                                 # no counts
    with pytest.raises(NotImplementedError):
        draw_sample_seg(0, 6, 64, dict(hyp, perspective=0.001), counts=counts)
    assert "paste" not in draw_sample(0, 6, 64, hyp, random.Random(1), np.random.RandomState(1))   # a dataset without polygons: n = 0, no draw
    bad = [list(sg) for sg in segments]
    bad[1] = bad[1][:-1]
    with pytest.raises(ValueError):
        MosaicLoader(ims, labels, img_size=64, batch_size=2, segments=bad)
    with pytest.raises(ValueError):
        mosaic_batch(ims, labels, [draw_sample(1, 6, 64, HYP, random.Random(1), np.random.RandomState(1))], 64, HYP, segments=bad)
    # both loaders run a copy_paste hyp end to end; without segments MosaicLoader is today's loader
    random.seed(0); np.random.seed(0)
    for loader in (SegMosaicLoader(ims, labels, segments, img_size=64, batch_size=4, hyp=dict(HYP, copy_paste=1.0), dtype=torch.float16),
                   MosaicLoader(ims, labels, img_size=64, batch_size=4, hyp=dict(HYP, copy_paste=1.0), dtype=torch.float16, segments=segments)):
        batches = list(loader)
        assert [tuple(b[0].shape) for b in batches] == [(4, 3, 64, 64), (2, 3, 64, 64)] and all(b[1].shape[1] == 6 for b in batches)
    random.seed(3); np.random.seed(3)
    a = list(MosaicLoader(ims, labels, img_size=64, batch_size=3, hyp=HYP))
    random.seed(3); np.random.seed(3)
    b = list(MosaicLoader(ims, labels, img_size=64, batch_size=3, hyp=dict(HYP, copy_paste=0.3)))
    assert all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(a, b))
