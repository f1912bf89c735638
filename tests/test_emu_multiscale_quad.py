"""CPU (emulator): training at varying shapes -- train.py's `--quad` (dataloaders.collate_fn4, csrc/collate4.h `y5_collate4`, the loss factor),
`--multi-scale` (torch_utils.multi_scale on `y5_scale_img`, train_loop.train(multi_scale=True)) and the cache of training plans under them
(train_engine.set_plan_cache: an LRU of TrainEngines on ONE gradient arena).  The `check_*` functions run here on CPU tensors through the
host-compiled kernels and again on cuda:0 from tests/test_gpu_multiscale_quad.py.

  1. quad against the REFERENCE's own collate_fn4 (tests/golden/quad.npz, scripts/make_golden_quad.py): images and targets bit for bit;
  2. the kernel against the NumPy restatement (tests/quad_ref.py) on shapes that take the byte-wise path, a rectangle and the border clamps;
  3. the multi-scale draws against the restated `randrange` sequence;
  4. the multi-scale pixels against torch's CPU F.interpolate in fp32, within a DERIVED bound: values in [0, 1], each of the two evaluation
     orders of the four-tap blend rounds at most four times (<= 8 * 2^-24 between them); an fp16 store adds half an fp16 ulp of the value;
  5. the plan cache: constructions counted, .grad addresses fixed, idle plans compute with the current weights, the byte budget evicts and
     releases, the default is the single-plan behaviour, accumulation across shapes, the stale-forward guard;
  6. train(multi_scale=True) end to end against a run over batches resized beforehand;
  7. quad's loss factor against the three loss gains scaled by 4.
The plan-cache and loop checks build the models they are given: the 0.13 M-parameter model of oracle/make_golden.py:TINY_CFG here (the emulator
runs a yolov5n step in ~17 s), yolov5n / yolov5n-seg in the GPU file.  Runs compared bit for bit set Y5_DETERMINISTIC=1 (read at plan
construction: weight gradients reduced in a fixed order)."""
import contextlib
import copy
import os
import random
import weakref

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import train_oracle as to, yolo_oracle as yo
from tests import quad_ref as qr
from tests.hipemu import backend as emu_backend

GOLD = os.path.join(os.path.dirname(__file__), "golden", "quad.npz")
DEV = torch.device("cpu")
SEED_MS = 8      # random.seed(8), imgsz 128, gs 32: the 50 draws hold all five sizes; the first three are 96, 128 (sf == 1), 160 (asserted below)
A, B_, C_ = 64, 96, 128


@pytest.fixture(autouse=True)
def _seam(monkeypatch):
    monkeypatch.setenv("Y5_DETERMINISTIC", "1")
    monkeypatch.delenv("Y5_TRAIN_PLAN_CACHE", raising=False)
    emu_backend.install()
    yield
    emu_backend.uninstall()


class Coins:
    """A `random` stand-in that hands out prepared values: `random()` for collate_fn4's coins, `randrange` for multi_scale's size."""

    def __init__(self, values):
        self.values = list(values)

    def random(self):
        return self.values.pop(0)

    def randrange(self, lo, hi):
        v = self.values.pop(0)
        assert lo <= v < hi
        return v


# ---- models ----------------------------------------------------------------------------------------------------------------------------------
def tiny_det(device=DEV):
    from oracle.make_golden import TINY_CFG
    from yolov5_amd.yolo import DetectionModel

    m = DetectionModel(copy.deepcopy(TINY_CFG))
    m.load_state_dict(yo.det_state_dict(copy.deepcopy(TINY_CFG), 2, fused=False))
    return m.to(device).train()


def tiny_seg(device=DEV):
    from oracle.make_golden import TINY_CFG
    from yolov5_amd.yolo import SegmentationModel

    cfg = copy.deepcopy(TINY_CFG)
    f, n, _, args = cfg["head"][-1]
    cfg["head"][-1] = [f, n, "Segment", list(args[:2]) + [8, 16]]
    m = SegmentationModel(copy.deepcopy(cfg))
    m.load_state_dict(yo.det_state_dict(cfg, 4, fused=False))
    return m.to(device).train()


# ---- 1. quad against the reference ---------------------------------------------------------------------------------------------------------------
def check_quad_golden(device=DEV):
    from yolov5_amd.dataloaders import collate_fn4

    g = np.load(GOLD)
    imgs, targets = torch.from_numpy(g["imgs8"]).to(device), torch.from_numpy(g["targets8"])
    seen = set()
    for seed in g["seeds"]:
        random.seed(int(seed))
        im4, lab4, paths, shapes = collate_fn4(imgs, targets, [f"img{b}" for b in range(8)], [(b, b) for b in range(8)])
        seen.add(tuple(bool(v) for v in g[f"flags{seed}"]))
        assert im4.dtype == torch.uint8 and im4.device.type == device.type and tuple(im4.shape) == (2, 3, 64, 64)
        assert np.array_equal(im4.cpu().numpy(), g[f"img{seed}"]), seed
        assert lab4.dtype == torch.float32 and tuple(lab4.shape) == g[f"lab{seed}"].shape
        assert np.array_equal(lab4.numpy(), g[f"lab{seed}"]), seed          # values AND row order
        assert paths == ["img0", "img1"] and shapes == [(0, 0), (1, 1)]
    assert seen == {(True, False), (False, True), (True, True), (False, False)}
    assert not (g["targets8"][:, 0] >= 4).any()                            # the second group of four holds no label
    # B = 11: three samples dropped
    random.seed(int(g["seed11"]))
    im4, lab4, paths, shapes = collate_fn4(torch.from_numpy(g["imgs11"]).to(device), torch.from_numpy(g["targets11"]), [f"img{b}" for b in range(11)],
                                           [(b, b) for b in range(11)])
    assert np.array_equal(im4.cpu().numpy(), g["img11"]) and np.array_equal(lab4.numpy(), g["lab11"])
    assert paths == ["img0", "img1"] and shapes == [(0, 0), (1, 1)] and int(g["npaths11"]) == 2
    assert collate_fn4(torch.from_numpy(g["imgs8"]).to(device), targets, None, None, Coins([0.0, 0.9]))[2:] == (None, None)   # the loaders' shapes


# ---- 2. the kernel against the restatement -------------------------------------------------------------------------------------------------------
KERNEL_CASES = [(20, 24), (32, 48), (1, 1), (2, 16), (3, 17), (16, 32)]   # (H, W): byte-wise path; rectangle; the clamps at both borders; odd; 16-byte path


def check_quad_kernel(H, W, device=DEV, B=9):
    from yolov5_amd.dataloaders import collate_fn4

    imgs = qr.byte_patterns(B, 3, H, W, seed=H * 100 + W)
    t = np.zeros((0, 6), np.float32)
    for flags in ([True, False], [False, True]):
        got = collate_fn4(torch.from_numpy(imgs).to(device), torch.from_numpy(t), None, None, Coins([0.0 if f else 0.75 for f in flags]))[0]
        ref = qr.collate4_images(imgs, flags)
        assert tuple(got.shape) == ref.shape == (B // 4, 3, 2 * H, 2 * W)
        assert np.array_equal(got.cpu().numpy(), ref), (H, W, flags)
    if H >= 16:   # the restatement of the upsample IS torch's CPU kernel, byte for byte (the argument of csrc/collate4.h: exact arithmetic)
        up = F.interpolate(torch.from_numpy(imgs[:1]).float(), scale_factor=2.0, mode="bilinear", align_corners=False).to(torch.uint8)
        assert np.array_equal(up[0].numpy(), qr.upsample2x(imgs[0]))


def check_quad_guards(device=DEV):
    from yolov5_amd.dataloaders import MosaicLoader, SegMosaicLoader, collate_fn4

    t = torch.zeros((0, 6))
    with pytest.raises(ValueError):
        collate_fn4(torch.zeros((3, 3, 16, 16), dtype=torch.uint8, device=device), t, None, None)
    with pytest.raises(TypeError):
        collate_fn4(torch.zeros((4, 3, 16, 16), dtype=torch.float16, device=device), t, None, None)
    with pytest.raises(NotImplementedError):
        SegMosaicLoader([], [], [], quad=True)
    with pytest.raises(TypeError):
        MosaicLoader([], [], dtype=torch.float16, quad=True)


def check_quad_loader(device=DEV):
    """MosaicLoader(quad=True): batches of batch_size / 4 images of twice the side, the trailing incomplete batch dropped, the coins drawn from
    `random` behind the batch's sample draws."""
    from tests import seg_data_ref as sd
    from yolov5_amd.dataloaders import MosaicLoader, collate_fn4, labels_from_segments

    ims, classes, segments = sd.polygon_dataset(6, seed=3)
    labels = [labels_from_segments(c, sg) for c, sg in zip(classes, segments)]
    ims_t = [torch.from_numpy(im).to(device) for im in ims]
    s = 32
    random.seed(9); np.random.seed(9)
    plain = MosaicLoader(ims_t, labels, img_size=s, batch_size=4, seed=1)
    first = next(iter(plain))
    coins = random.getstate()
    random.seed(9); np.random.seed(9)
    quad = MosaicLoader(ims_t, labels, img_size=s, batch_size=4, seed=1, quad=True)
    assert len(plain) == 2 and len(quad) == 1
    batches = list(quad)
    assert len(batches) == 1
    im4, lab4, paths, shapes = batches[0]
    assert tuple(im4.shape) == (1, 3, 2 * s, 2 * s) and im4.dtype == torch.uint8 and len(paths) == 1 and shapes is None
    rng = random.Random()
    rng.setstate(coins)
    exp = collate_fn4(*first, rng=rng)
    assert torch.equal(im4, exp[0]) and torch.equal(lab4, exp[1]) and (lab4[:, 0] == 0).all()


# ---- 3. / 4. multi-scale ---------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def count_scale_launches():
    from yolov5_amd import _lib

    lib, calls = _lib.lib(), []
    real = lib.y5_scale_img

    def spy(*a):
        calls.append(a)
        return real(*a)

    lib.y5_scale_img = spy
    try:
        yield calls
    finally:
        lib.y5_scale_img = real


def check_multi_scale_draws(device=DEV, wide_calls=6):
    from yolov5_amd.torch_utils import multi_scale

    exp = qr.multi_scale_sizes(random.Random(SEED_MS), 128, 32, 50, (128, 128))
    assert {sz for sz, _, _ in exp} == {64, 96, 128, 160, 192} and [sz for sz, _, _ in exp[:3]] == [96, 128, 160]
    x = torch.from_numpy(qr.byte_patterns(1, 1, 128, 128, 5)).to(device)
    random.seed(SEED_MS)
    with count_scale_launches() as calls:
        for sz, sf, ns in exp:
            n0 = len(calls)
            y = multi_scale(x, 128, 32, torch.float16)
            if ns is None:
                assert sz == 128 and y is x and len(calls) == n0                  # sf == 1: the same object, nothing launched
            else:
                assert tuple(y.shape) == (1, 1, *ns) == (1, 1, sz, sz) and y.dtype == torch.float16 and len(calls) == n0 + 1
    # imgsz = 640: randrange(320, 992) floored to the grid -- 21 sizes, 320 .. 960 (a draw of 992 itself is excluded); restated draws reach both ends
    sizes = {sz for sz, _, _ in qr.multi_scale_sizes(random.Random(0), 640, 32, 4000, (640, 640))}
    assert sizes == set(range(320, 961, 32)) and len(sizes) == 21
    small = torch.zeros((1, 1, 32, 32), dtype=torch.uint8, device=device)
    random.seed(1)
    ref = qr.multi_scale_sizes(random.Random(1), 640, 32, wide_calls, (32, 32))
    for sz, _, ns in ref:
        y = multi_scale(small, 640, 32, torch.float16)
        assert tuple(y.shape[2:]) == ns == (sz, sz) and 320 <= sz <= 992 and sz % 32 == 0
    with pytest.raises(TypeError):
        multi_scale(small.long(), 640, 32, torch.float16)


def fp16_half_ulp(v):
    """Half an fp16 ulp of |v| (fp32 array): 2^(e - 11) for 2^e <= |v| < 2^(e + 1), the subnormal spacing 2^-24 / 2 below 2^-14."""
    _, e = np.frexp(np.maximum(np.abs(v.astype(np.float64)), 2.0 ** -14))     # |v| = m * 2^e, 0.5 <= m < 1
    return np.ldexp(1.0, e - 1 - 11)


def check_multi_scale_pixels(device=DEV):
    from yolov5_amd.torch_utils import multi_scale

    rng = np.random.default_rng(7)
    u8 = torch.from_numpy(qr.byte_patterns(2, 3, 64, 96, 7))
    f32 = torch.from_numpy(rng.uniform(0, 1, (2, 3, 64, 96)).astype(np.float32))
    f32[0, 0, :4, :4] = torch.tensor([0.0, 1.0, 0.0, 1.0])
    shapes = set()
    for draw in (64 + 5, 160 + 31):                                             # floored to sz = 64 and sz = 160
        (sz, sf, ns), = qr.multi_scale_sizes(Coins([draw]), 128, 32, 1, (64, 96))
        assert sz in (64, 160) and ns is not None
        shapes.add(ns)
        for x in (u8, f32):
            ref = F.interpolate(x.float() / 255 if x.dtype == torch.uint8 else x, size=ns, mode="bilinear", align_corners=False).numpy()
            for dtype in (torch.float32, torch.float16):
                y = multi_scale(x.to(device), 128, 32, dtype, rng=Coins([draw]))
                assert y.dtype == dtype and tuple(y.shape) == (2, 3, *ns)
                d = np.abs(y.float().cpu().numpy().astype(np.float64) - ref.astype(np.float64))
                bound = 8 * 2.0 ** -24 + (fp16_half_ulp(ref) if dtype == torch.float16 else 0.0)
                print(f"[multi-scale] {tuple(x.shape[2:])} -> {ns} {x.dtype} -> {dtype}: max |d| {d.max():.3e}, worst d / bound {(d / bound).max():.3f}")
                assert (d <= bound).all(), (ns, x.dtype, dtype, float(d.max()))
    assert len(shapes) == 2 and any(h < 64 or w < 96 for h, w in shapes) and any(h > 64 and w > 96 for h, w in shapes)   # shrink and grow
    assert any(h * 96 != w * 64 for h, w in shapes)                                                                      # and a stretch


# ---- 5. the plan cache -----------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def count_engines():
    from yolov5_amd import train_engine as te

    built, real = [], te.TrainEngine.__init__

    def init(self, *a, **k):
        built.append(self)
        return real(self, *a, **k)

    te.TrainEngine.__init__ = init
    try:
        yield built
    finally:
        te.TrainEngine.__init__ = real


def _x(S, device, seed=0):
    return torch.from_numpy(np.random.default_rng(100 + S + seed).uniform(0, 1, (2, 3, S, S)).astype(np.float16)).to(device)


def _loss(out):
    return sum((o.float() ** 2).mean() for o in out)


def _grads(m):
    return [None if p.grad is None else p.grad.detach().clone() for p in m.parameters()]


def check_plan_cache_sequence(make_model, device=DEV):
    """max_plans = 3, A B A C B with an SGD step behind every backward: three plans are built, .grad keeps its address, and the second A -- a plan
    that sat idle while the weights moved twice -- equals a fresh model on the default single-plan path, bit for bit."""
    from yolov5_amd.train_engine import set_plan_cache

    m = make_model(device)
    set_plan_cache(m, max_plans=3)
    opt = torch.optim.SGD(m.parameters(), lr=0.001, momentum=0.9)
    ptrs = None
    with count_engines() as built:
        for step, S in enumerate((A, B_, A, C_, B_)):
            x = _x(S, device)
            if step == 2:
                state = {k: v.detach().clone() for k, v in m.state_dict().items()}
            opt.zero_grad(set_to_none=True)
            out = m(x)
            _loss(out).backward()
            now = [p.grad.data_ptr() for p in m.parameters()]
            assert all(p.grad is not None for p in m.parameters())
            ptrs = ptrs or now
            assert now == ptrs, f"step {step}: .grad moved"
            if step == 2:
                fresh = make_model(device)
                fresh.load_state_dict(state)
                assert "_train_max_plans" not in fresh.__dict__
                fout = fresh(x)
                _loss(fout).backward()
                assert all(bool(torch.isfinite(a).all()) and torch.equal(a, b) for a, b in zip(out, fout))
                assert all(torch.equal(p.grad, q.grad) for p, q in zip(m.parameters(), fresh.parameters()))
                assert any(float(p.grad.abs().max()) > 0 for p in m.parameters())
                built.remove(next(iter(fresh.__dict__["_train_engines"].values())))
            opt.step()
        assert len(built) == 3 and len(m.__dict__["_train_engines"]) == 3
    engines = list(m.__dict__["_train_engines"].values())
    assert all(e.gflat is engines[0].gflat for e in engines) and sum(e._owns_arena for e in engines) == 1
    assert all(e.nbytes > 0 for e in engines)


def check_plan_cache_budget(make_model, device=DEV):
    """A byte budget that fits any two of the three plans evicts the least recently used one when the third is built; its buffers are released
    at once (no cycle collection: gc is off while the references are checked)."""
    import gc

    from yolov5_amd.train_engine import set_plan_cache

    m = make_model(device)
    set_plan_cache(m, max_plans=8, max_bytes=1 << 50)
    for S in (A, B_, C_):
        m(_x(S, device))
    sizes = [e.nbytes for e in m.__dict__["_train_engines"].values()]
    assert len(sizes) == 3 and min(sizes) > 0
    m = make_model(device)
    set_plan_cache(m, max_plans=8, max_bytes=sum(sizes) - 1)
    gc.collect()
    gc.disable()
    try:
        with count_engines() as built:
            m(_x(A, device))
            m(_x(B_, device))
            cache = m.__dict__["_train_engines"]
            first = built[0]
            assert [e.nbytes for e in cache.values()] == sizes[:2] and len(cache) == 2
            refs = [weakref.ref(t) for t in (first.bufs[0], first.gbufs[-1], first.dz, first.dwflat, first.convs[0]["z"], first.convs[-1]["wp"])]
            arena = first.gflat
            m(_x(C_, device))
            assert len(built) == 3 and list(cache.values()) == built[1:]               # the least recently used plan went
            assert first._closed and first.nbytes == 0 and all(r() is None for r in refs)
            assert built[1].gflat is arena                                             # the arena lives on with the plans that share it
            with pytest.raises(RuntimeError):
                first.forward(_x(A, device))
            # a budget below a single plan: that plan is still built and kept as the only one
            set_plan_cache(m, max_plans=8, max_bytes=1)
            assert list(cache.values()) == [built[2]] and built[1]._closed
            m(_x(A, device))
            assert len(built) == 4 and list(cache.values()) == [built[3]] and built[2]._closed
    finally:
        gc.enable()


def check_plan_cache_default(make_model, device=DEV):
    """Nothing set: one plan, A B A builds three engines, each with an arena of its own (the behaviour before the cache)."""
    m = make_model(device)
    with count_engines() as built:
        for S in (A, B_, A):
            m(_x(S, device))
            assert len(m.__dict__["_train_engines"]) == 1
    assert len(built) == 3 and len({id(e.gflat) for e in built}) == 3 and not any(e._closed for e in built)
    assert not any(k in m.__dict__ for k in ("_train_arena", "_train_max_plans", "_train_max_bytes"))
    c = copy.deepcopy(m)
    assert not any(k.startswith("_train") for k in c.__dict__)


def check_plan_cache_accumulate(make_model, device=DEV):
    """backward at A, then at B, without zero_grad between: the sum of the two separate backwards, to the rounding of one fp32 addition."""
    from yolov5_amd.train_engine import set_plan_cache

    m = make_model(device)
    set_plan_cache(m, max_plans=2)
    xa, xb = _x(A, device), _x(B_, device)
    sep = []
    for x in (xa, xb):
        m.zero_grad(set_to_none=True)
        _loss(m(x)).backward()
        sep.append(_grads(m))
    m.zero_grad(set_to_none=True)
    _loss(m(xa)).backward()
    _loss(m(xb)).backward()
    worst = 0.0
    for g, a, b in zip(_grads(m), *sep):
        s = a.double() + b.double()
        err = (g.double() - s).abs()
        assert bool((err <= 2.0 ** -23 * s.abs()).all())
        worst = max(worst, float((err / s.abs().clamp_min(1e-300)).max()))
    print(f"[plan cache] accumulation across shapes: worst relative error {worst:.3e} (bound {2.0 ** -23:.3e})")
    assert any(float(a.abs().max()) > 0 and float(b.abs().max()) > 0 for a, b in zip(*sep))


def check_plan_cache_stale(make_model, device=DEV):
    from yolov5_amd.train_engine import set_plan_cache

    m = make_model(device)
    set_plan_cache(m, max_plans=2)
    old = _loss(m(_x(A, device)))
    other = _loss(m(_x(B_, device)))
    new = _loss(m(_x(A, device, seed=1)))
    with pytest.raises(RuntimeError, match="no longer the model's latest"):
        old.backward()
    other.backward()      # B's latest forward: its plan was not touched by the forwards at A
    new.backward()
    assert all(p.grad is not None for p in m.parameters())


# ---- 6. end to end ------------------------------------------------------------------------------------------------------------------------------
class ListLoader:
    def __init__(self, batches):
        self.batches = batches

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        return iter(self.batches)


def _seg_batches(device, n=6, S=128, bs=2):
    """(imgs, targets, paths, None, masks): three batches of two 128^2 images with two boxes each; overlap-mode masks (one uint8 plane per image at
    a quarter of the side, pixel = 1-based index of the instance among the image's targets)."""
    imgs, tpi = to.synthetic_set(n, S, per_img=2, seed=6)
    out = []
    for b0 in range(0, n, bs):
        t, masks = [], torch.zeros((bs, S // 4, S // 4), dtype=torch.uint8)
        for k in range(bs):
            ti = tpi[b0 + k].clone()
            ti[:, 0] = k
            t.append(ti)
            for j, (_, _, xc, yc, w, h) in enumerate(ti.tolist()):
                x0, x1, y0, y1 = (int(max(v, 0) * S / 4) for v in (xc - w / 2, xc + w / 2, yc - h / 2, yc + h / 2))
                masks[k, y0:max(y1, y0 + 1), x0:max(x1, x0 + 1)] = j + 1
        out.append((imgs[b0:b0 + bs].to(device), torch.cat(t, 0), None, None, masks.to(device)))
    return out


def check_train_multi_scale(make_model, device=DEV, seg=False, seed=SEED_MS):
    from yolov5_amd.torch_utils import multi_scale
    from yolov5_amd.train_engine import set_plan_cache
    from yolov5_amd.train_loop import TensorLoader, train

    exp = qr.multi_scale_sizes(random.Random(seed), 128, 32, 3, (128, 128))
    assert len({sz for sz, _, _ in exp}) >= 2
    if seg:
        loader = ListLoader(_seg_batches(device))
    else:
        imgs, tpi = to.synthetic_set(6, 128, per_img=2, seed=6)
        loader = TensorLoader(imgs.to(device), tpi, 2)
    m = make_model(device)
    set_plan_cache(m, max_plans=2, max_bytes=1 << 48)
    shapes = []
    hook = m.register_forward_pre_hook(lambda mod, inp: shapes.append(tuple(inp[0].shape)))
    random.seed(seed)
    with count_engines() as built:
        res = train(m, loader, epochs=1, device=device, multi_scale=True, imgsz=128, amp=True)
    hook.remove()
    assert shapes == [(2, 3, sz, sz) for sz, _, _ in exp]
    assert len(built) == len({sz for sz, _, _ in exp})                           # one plan per size, none rebuilt
    assert m.__dict__["_train_max_plans"] == 2 and m.__dict__["_train_max_bytes"] == 1 << 48    # the limits from before the run
    assert len(m.__dict__["_train_engines"]) <= 2
    assert tuple(res["losses"].shape) == (3, 4 if seg else 3) and bool(torch.isfinite(res["losses"]).all())
    # the same batches resized beforehand, through a run without multi_scale (default cache: one plan, rebuilt at every new size)
    rng = random.Random(seed)
    pre = []
    for batch in loader:
        pre.append((multi_scale(batch[0].to(device), 128, 32, torch.float16, rng=rng), *batch[1:]))
        if seg:
            assert pre[-1][4] is batch[4]                                        # only the images are resized
    assert [tuple(b[0].shape[2:]) for b in pre] == [(sz, sz) for sz, _, _ in exp]
    m2 = make_model(device)
    state = random.getstate()
    res2 = train(m2, ListLoader(pre), epochs=1, device=device, amp=True)
    assert random.getstate() == state                                            # multi_scale=False: no draw is consumed
    assert torch.equal(res["losses"], res2["losses"]), (res["losses"], res2["losses"])
    assert all(torch.equal(p, q) for p, q in zip(m.parameters(), m2.parameters()))
    assert not any(k in m2.__dict__ for k in ("_train_max_plans", "_train_max_bytes"))
    # an exception inside the run restores the limits as well
    with pytest.raises(ZeroDivisionError):
        train(m2, loader, epochs=1, device=device, multi_scale=True, imgsz=128, on_batch_end=lambda *a: 1 / 0)
    assert not any(k in m2.__dict__ for k in ("_train_max_plans", "_train_max_bytes")) and len(m2.__dict__["_train_engines"]) == 1


# ---- 7. quad's factor ------------------------------------------------------------------------------------------------------------------------
def check_quad_factor(make_model, device=DEV):
    from yolov5_amd.dataloaders import collate_fn4
    from yolov5_amd.train_loop import HYP_SCRATCH_LOW, train

    imgs, tpi = to.synthetic_set(8, 32, per_img=2, seed=8)
    t = []
    for k, ti in enumerate(tpi):
        ti = ti.clone()
        ti[:, 0] = k
        t.append(ti)
    batch = collate_fn4(imgs.to(device), torch.cat(t, 0), None, None, Coins([0.1, 0.9]))
    assert tuple(batch[0].shape) == (2, 3, 64, 64) and len(batch[1]) == 2 + 8
    ma, mb = make_model(device), make_model(device)
    start = [p.detach().clone() for p in ma.parameters()]
    hyp4 = dict(HYP_SCRATCH_LOW, **{k: 4 * HYP_SCRATCH_LOW[k] for k in ("box", "obj", "cls")})
    # fp32 plan (loss scale 1: the step is taken whatever the factor).  Under AMP the factor of 4 on top of the initial scale of 65536 overflows the
    # fp16 gradients of the first iteration in BOTH runs alike, so the AMP pair below is compared as it comes: equal parameters, equal skips.
    # max_norm far away: a clipped gradient (g * max_norm / |g|) does not depend on the loss's factor at all, which would make the comparison vacuous.
    ra = train(ma, ListLoader([batch]), hyp=dict(HYP_SCRATCH_LOW), epochs=1, device=device, quad=True, amp=False, max_norm=1e9)
    rb = train(mb, ListLoader([batch]), hyp=hyp4, epochs=1, device=device, quad=False, amp=False, max_norm=1e9)
    assert ra["scaler"].skipped == rb["scaler"].skipped == 0 and ra["ema"].updates == 1
    assert torch.equal(ra["losses"] * 4, rb["losses"])                            # a power of two: the loss scales exactly
    assert all(torch.equal(p, q) for p, q in zip(ma.parameters(), mb.parameters()))
    assert any(not torch.equal(p, s) for p, s in zip(ma.parameters(), start))     # and a step was taken
    mc = make_model(device)
    train(mc, ListLoader([batch]), hyp=dict(HYP_SCRATCH_LOW), epochs=1, device=device, quad=False, amp=False, max_norm=1e9)
    assert any(not torch.equal(p, q) for p, q in zip(ma.parameters(), mc.parameters()))   # the factor is not a no-op
    ma, mb = make_model(device), make_model(device)
    ra = train(ma, ListLoader([batch]), hyp=dict(HYP_SCRATCH_LOW), epochs=1, device=device, quad=True)
    rb = train(mb, ListLoader([batch]), hyp=hyp4, epochs=1, device=device, quad=False)
    assert ra["scaler"].skipped == rb["scaler"].skipped and torch.equal(ra["losses"] * 4, rb["losses"])
    assert all(torch.equal(p, q) for p, q in zip(ma.parameters(), mb.parameters()))


# ---- tests -----------------------------------------------------------------------------------------------------------------------------------
def test_quad_matches_reference_golden():
    check_quad_golden()


@pytest.mark.parametrize("H,W", KERNEL_CASES)
def test_collate4_kernel_matches_restatement(H, W):
    check_quad_kernel(H, W)


def test_quad_guards():
    check_quad_guards()


def test_quad_loader_drops_last_and_draws_after_the_samples():
    check_quad_loader()


def test_multi_scale_draws():
    check_multi_scale_draws()


def test_multi_scale_pixels_within_derived_bound():
    check_multi_scale_pixels()


def test_plan_cache_sequence_shares_arena_and_tracks_weights():
    check_plan_cache_sequence(tiny_det)


def test_plan_cache_byte_budget_evicts_and_releases():
    check_plan_cache_budget(tiny_det)


def test_plan_cache_default_is_single_plan():
    check_plan_cache_default(tiny_det)


def test_plan_cache_accumulates_across_shapes():
    check_plan_cache_accumulate(tiny_det)


def test_plan_cache_stale_forward_still_raises():
    check_plan_cache_stale(tiny_det)


def test_train_multi_scale_end_to_end():
    check_train_multi_scale(tiny_det)


def test_train_multi_scale_end_to_end_segmentation():
    check_train_multi_scale(tiny_seg, seg=True)


def test_quad_loss_factor_equals_scaled_gains():
    check_quad_factor(tiny_det)
