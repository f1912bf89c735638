"""Shared restatements and acceptance rules of the classification-training tests (tests/test_emu_classify_train.py,
tests/test_gpu_classify_train.py) and of scripts/make_golden_classify_train.py, which writes tests/golden/classify_train.npz from the
unmodified reference.

  * head backward / cross-entropy gradient: float64 restatements with the forward error bound of fp32 summation in any order, per output,
    built like tests/classify_ref.head_ref's (terms x 2^-24 x sum of the absolute values of the terms; + 2^-22 of that sum where an fp32
    operand enters the fp16 MFMA as hi + lo halves; + half an fp16 ulp where the output is fp16).
  * the Dropout stream of csrc/classify_train.h restated in numpy (Philox4x32-10, key = seed, counter = element index).
  * the seeded projection vectors the fixture's per-parameter gradient summaries are taken on.
"""
import os
import zlib

import numpy as np

from tests import classify_ref as cr

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "classify_train.npz")
U24 = cr.U24

# (B, HW, C, nc, ld): B and nc on both sides of the 32-wide tile, C no multiple of 16 / 32, ld > C
BWD_SHAPES = [(1, 1, 8, 1, 8), (5, 6, 72, 10, 72), (33, 4, 1280, 33, 1288), (2, 49, 1280, 1000, 1280)]

# fixture (a) / (b): one train-mode step of yolov5n-cls (nc = 10, Dropout 0)
STEP_INPUT = (4, 3, 64, 64)
STEP_LABELS = (3, 0, 9, 3)
FULL_GRADS = ("model.9.linear.weight", "model.9.linear.bias", "model.9.conv.bn.weight", "model.9.conv.bn.bias", "model.0.conv.weight")
NPROJ = 4
# fixture (c): 3 epochs x 2 batches of classify_ref.val_inputs()[:2]
TRAJ_EPOCHS = 3
TRAJ_LABELS = ((3, 0), (9, 3))
TRAJ_ARGS = dict(lr0=0.001, decay=5e-5, label_smoothing=0.1)


def golden():
    return np.load(GOLDEN, allow_pickle=False)


def step_input():
    import torch

    from oracle import detgen
    return torch.from_numpy(detgen.uniform(STEP_INPUT, 0.0, 1.0, name="img", seed=11))


def projections(name, numel):
    """(NPROJ, numel) float64 standard-normal vectors of parameter `name`, seeded by the name."""
    rs = np.random.RandomState(zlib.crc32(name.encode()) & 0x7fffffff)
    return rs.standard_normal((NPROJ, numel))


def half_ulp16(v):
    return np.spacing(np.abs(v).astype(np.float16)).astype(np.float64) / 2


# ---- Dropout stream --------------------------------------------------------------------------------------------------------------------------
def philox_word(seed, idx):
    """First output word of Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter (i & 0xffffffff, i >> 32, 0, 0), for an array of
    element indices i."""
    M32 = np.uint64(0xFFFFFFFF)
    idx = np.asarray(idx, np.uint64)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    c0, c1, c2, c3 = idx & M32, idx >> np.uint64(32), np.zeros_like(idx), np.zeros_like(idx)
    for r in range(10):
        if r:
            k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
        m0, m1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (m1 >> np.uint64(32)) ^ c1 ^ k0, m1 & M32, (m0 >> np.uint64(32)) ^ c3 ^ k1, m0 & M32
    return c0.astype(np.uint32)


def keep_mask(seed, B, C, p):
    """(B, C) bool: element b * C + c is kept iff (r >> 8) * 2^-24 >= p in fp32 (p == 0 keeps everything)."""
    if p <= 0:
        return np.ones((B, C), bool)
    r = philox_word(seed, np.arange(B * C, dtype=np.uint64))
    u = (r >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return (u >= np.float32(p)).reshape(B, C)


def dropout_ref(pooled32, seed, p):
    """nn.Dropout(p) on fp32 rows with that mask: zero, or exactly fp32(pooled / (1 - p))."""
    keep = keep_mask(seed, pooled32.shape[0], pooled32.shape[1], p)
    with np.errstate(divide="ignore", invalid="ignore"):
        scaled = pooled32.astype(np.float32) / (np.float32(1.0) - np.float32(p))
    return np.where(keep, scaled, np.float32(0.0)).astype(np.float32), keep


# ---- head backward ---------------------------------------------------------------------------------------------------------------------------
def bwd_inputs(B, HW, C, nc, dtype, seed=0):
    """dlogits (B, nc) of order 1 / B like a mean loss's, pooled (B, C) fp32 (pre-Dropout), w (nc, C)."""
    rs = np.random.RandomState(3000 + seed + B * 7 + HW * 13 + C + nc * 3)
    dl = (rs.standard_normal((B, nc)) / B).astype(dtype)
    v = rs.standard_normal((B, C))
    pooled = (v / (1.0 + np.exp(-v))).astype(np.float32)
    w = (rs.standard_normal((nc, C)) / np.sqrt(C)).astype(dtype)
    return dl, pooled, w


def head_bwd_ref(dl, pooled_d, w, HW, keep, p):
    """float64 (dbias, dW, g) with g[b, c] the value dx holds at every pixel of image b, and their bounds.  dl, w: the plan's dtype; pooled_d:
    the post-Dropout fp32 rows."""
    f16 = dl.dtype == np.float16
    B, nc = dl.shape
    d64, p64, w64 = dl.astype(np.float64), pooled_d.astype(np.float64), w.astype(np.float64)
    dbias = d64.sum(0)
    db_b = (B + 8) * U24 * np.abs(d64).sum(0)
    dw = d64.T @ p64
    mag = np.abs(d64).T @ np.abs(p64)
    dw_b = (B + 8) * U24 * mag + (2.0 ** -22 * mag if f16 else 0.0)
    scale = 0.0 if p >= 1 else 1.0 / (1.0 - float(np.float32(p))) / HW
    g = np.where(keep, (d64 @ w64) * scale, 0.0)
    g_b = np.where(keep, (nc + 8 + 2) * U24 * (np.abs(d64) @ np.abs(w64)) * scale, 0.0)
    if f16:
        g_b = g_b + half_ulp16(np.abs(g) + g_b)
    return dbias, db_b, dw, dw_b, g, g_b


# ---- cross-entropy gradient ------------------------------------------------------------------------------------------------------------------
def ce_bwd_ref(z, labels, eps, grad_rows):
    """float64 dlogits of the fp32-widened logits and their bound: the softmax's (nc + 8) * 2^-24 bound of classify_ref.post_ref, four more
    roundings on the terms, and half an fp16 ulp for an fp16 output."""
    z64 = z.astype(np.float32).astype(np.float64)
    B, nc = z64.shape
    e = np.exp(z64 - z64.max(1, keepdims=True))
    probs = e / e.sum(1, keepdims=True)
    onehot = np.zeros((B, nc))
    onehot[np.arange(B), labels] = 1.0 - eps
    g = grad_rows.astype(np.float64)[:, None]
    ref = g * (probs - onehot - eps / nc)
    bound = np.abs(g) * ((nc + 8) * U24 * probs + 4 * U24 * (probs + onehot + eps / nc))
    if z.dtype == np.float16:
        bound = bound + half_ulp16(np.abs(ref) + bound)
    return ref, bound


# ---- drivers shared by the emulator and the GPU tests ----------------------------------------------------------------------------------------
class EmuMem:
    """Buffers in host memory for the host-compiled kernels (tests/hipemu)."""

    def __init__(self):
        from tests.hipemu.emu import emu
        self.lib = emu()

    def put(self, a):
        from tests.hipemu.emu import aligned
        h = aligned(a.shape, a.dtype)
        h[...] = a
        return h

    def ptr(self, h):
        return h.ctypes.data

    def get(self, h):
        return np.array(h)


class GpuMem:
    """Buffers on the GPU for the real library."""

    def __init__(self):
        from yolov5_amd import _lib
        self.lib = _lib.lib()

    def put(self, a):
        import torch
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def ptr(self, h):
        return h.data_ptr()

    def get(self, h):
        import torch
        torch.cuda.synchronize()
        return h.cpu().numpy()


def _dt(a):
    from yolov5_amd import _lib
    return _lib.Y5_F16 if a.dtype == np.float16 else _lib.Y5_F32


def _vp(mem, h):
    import ctypes
    return ctypes.c_void_p(mem.ptr(h))


GUARD = 64


def run_head_train(mem, x, w, bias, C, nc, p, seed):
    """(logits (B, nc), pooled (B, C) fp32 as the call left them); guard elements behind both are checked."""
    B, HW, ld = x.shape
    X, W, Bi = mem.put(x), mem.put(w), mem.put(bias)
    out = mem.put(np.full((B * nc + GUARD,), -9.5, x.dtype))
    pooled = mem.put(np.full((B * C + GUARD,), -7.5, np.float32))
    rc = mem.lib.y5_classify_head_train(_vp(mem, X), _dt(x), B, HW, C, ld, _vp(mem, W), _vp(mem, Bi), nc, _vp(mem, out), nc, _vp(mem, pooled), B * C * 4,
                                        p, seed, None)
    assert rc == 0, mem.lib.y5_last_error()
    o, pl = mem.get(out), mem.get(pooled)
    assert (o[B * nc:] == -9.5).all() and (pl[B * C:] == -7.5).all(), "a store behind an output"
    return o[:B * nc].reshape(B, nc), pl[:B * C].reshape(B, C)


def run_head_fwd(mem, x, w, bias, C, nc, form=2):
    B, HW, ld = x.shape
    X, W, Bi = mem.put(x), mem.put(w), mem.put(bias)
    out = mem.put(np.zeros((B, nc), x.dtype))
    ws = mem.put(np.zeros((B * C,), np.float32))
    rc = mem.lib.y5_classify_head(_vp(mem, X), _dt(x), B, HW, C, ld, _vp(mem, W), _vp(mem, Bi), nc, _vp(mem, out), nc, form, _vp(mem, ws), B * C * 4, None)
    assert rc == 0, mem.lib.y5_last_error()
    return mem.get(out)


def run_head_bwd(mem, dl, pooled_d, w, HW, C, ld, p=0.0, seed=0, ldd=None):
    """(dbias (nc), dW (nc, C), dx (B, HW, C)); checks the guard elements behind every output, behind each dlogits row's reach and between C and ld."""
    B, nc = dl.shape
    ldd = ldd or nc
    DL = np.full((B, ldd), 55.0, dl.dtype)
    DL[:, :nc] = dl
    DL, P, W = mem.put(DL), mem.put(pooled_d), mem.put(w)
    dbias = mem.put(np.full((nc + GUARD,), -3.5, np.float32))
    dw = mem.put(np.full((nc * C + GUARD,), -3.5, np.float32))
    dx = mem.put(np.full((B * HW * ld + GUARD,), -9.5, dl.dtype))
    ws = mem.put(np.full((B * C + GUARD,), -1.5, np.float32))
    rc = mem.lib.y5_classify_head_bwd(_vp(mem, DL), _dt(dl), B, nc, ldd, _vp(mem, P), _vp(mem, W), HW, C, p, seed, _vp(mem, dbias), _vp(mem, dw), _vp(mem, dx), ld,
                                      _vp(mem, ws), B * C * 4, None)
    assert rc == 0, mem.lib.y5_last_error()
    db, dwv, dxv, wsv = mem.get(dbias), mem.get(dw), mem.get(dx), mem.get(ws)
    assert (db[nc:] == -3.5).all() and (dwv[nc * C:] == -3.5).all() and (dxv[B * HW * ld:] == -9.5).all() and (wsv[B * C:] == -1.5).all(), "a store behind an output"
    dxv = dxv[:B * HW * ld].reshape(B, HW, ld)
    assert (dxv[:, :, C:] == -9.5).all(), "a store between C and ld"
    return db[:nc], dwv[:nc * C].reshape(nc, C), dxv[:, :, :C].copy()


def run_ce_bwd(mem, z, labels, eps, grad_rows, ld=None, ldd=None):
    B, nc = z.shape
    ld, ldd = ld or nc, ldd or nc
    Z = np.full((B, ld), 99.0, z.dtype)
    Z[:, :nc] = z
    Z, L, G = mem.put(Z), mem.put(np.asarray(labels, np.int32)), mem.put(np.asarray(grad_rows, np.float32))
    out = mem.put(np.full((B * ldd + GUARD,), -9.5, z.dtype))
    rc = mem.lib.y5_classify_ce_bwd(_vp(mem, Z), _dt(z), B, nc, ld, _vp(mem, L), eps, _vp(mem, G), _vp(mem, out), ldd, None)
    assert rc == 0, mem.lib.y5_last_error()
    o = mem.get(out)
    assert (o[B * ldd:] == -9.5).all()
    o = o[:B * ldd].reshape(B, ldd)
    assert (o[:, nc:] == -9.5).all(), "a store behind a dlogits row"
    return o[:, :nc].copy()


def check_head_bwd(mem, shape, dtype):
    """The head backward against the float64 restatement within its bounds, and its determinism properties."""
    B, HW, C, nc, ld = shape
    dl, pooled, w = bwd_inputs(B, HW, C, nc, dtype)
    keep = np.ones((B, C), bool)
    db, dw, dx = run_head_bwd(mem, dl, pooled, w, HW, C, ld, ldd=nc + 3)
    rdb, bdb, rdw, bdw, rg, bg = head_bwd_ref(dl, pooled, w, HW, keep, 0.0)
    e_db, e_dw, e_dx = np.abs(db - rdb), np.abs(dw - rdw), np.abs(dx.astype(np.float64) - rg[:, None, :])
    ratios = [float((e / np.maximum(b, 1e-300)).max()) for e, b in ((e_db, bdb), (e_dw, bdw), (e_dx, bg[:, None, :]))]
    print(f"head bwd {shape} {np.dtype(dtype).name}: max err / bound  dbias {ratios[0]:.3f}  dW {ratios[1]:.3f}  dx {ratios[2]:.3f}")
    assert (e_db <= bdb).all() and (e_dw <= bdw).all() and (e_dx <= bg[:, None, :]).all(), ratios
    assert (dx == dx[:, :1]).all(), "the pixels of one image differ"
    db2, dw2, dx2 = run_head_bwd(mem, dl, pooled, w, HW, C, ld, ldd=nc + 3)
    assert np.array_equal(db, db2) and np.array_equal(dw, dw2) and np.array_equal(dx, dx2), "a run is not bit-equal to itself"
    for b in sorted({0, B // 2, B - 1}):
        _, _, dxb = run_head_bwd(mem, dl[b:b + 1], pooled[b:b + 1], w, HW, C, ld)
        assert np.array_equal(dxb[0], dx[b]), f"dx of image {b} differs from its single-row call"


def check_dropout(mem, dtype, p, shape=(5, 6, 72, 10)):
    """Forward: the post-Dropout rows equal the numpy Philox restatement; backward: the same mask."""
    B, HW, C, nc = shape
    x, w, bias = cr.head_inputs(B, HW, C, nc, dtype)
    seed = 0x1234_5678_9ABC_DEF1
    _, pooled0 = run_head_train(mem, x, w, bias, C, nc, 0.0, 0)
    logits, pooled_d = run_head_train(mem, x, w, bias, C, nc, p, seed)
    want, keep = dropout_ref(pooled0, seed, p)
    assert np.array_equal(pooled_d, want), "post-Dropout rows differ from the Philox restatement"
    frac = keep.mean()
    print(f"dropout p {p} {np.dtype(dtype).name}: kept {frac:.3f} of {keep.size}")
    assert (not keep.any()) if p >= 1 else abs(frac - (1 - p)) < 4 * np.sqrt(p * (1 - p) / keep.size) + 1e-9
    # the Linear ran on those rows
    ref = bias.astype(np.float64)[None] + pooled_d.astype(np.float64) @ w.astype(np.float64).T
    bound = (C + 8) * U24 * (np.abs(bias)[None] + np.abs(pooled_d).astype(np.float64) @ np.abs(w).astype(np.float64).T)
    if dtype == np.float16:
        bound = bound + half_ulp16(np.abs(ref) + bound)
    assert (np.abs(logits.astype(np.float64) - ref) <= bound).all()
    logits2, pooled2 = run_head_train(mem, x, w, bias, C, nc, p, seed)
    assert np.array_equal(pooled2, pooled_d) and np.array_equal(logits2, logits), "the same seed gave another mask"
    if 0 < p < 1:
        _, pooled3 = run_head_train(mem, x, w, bias, C, nc, p, seed + 1)
        assert not np.array_equal(pooled3 == 0, pooled_d == 0), "another seed gave the same mask"
    # backward
    dl, _, _ = bwd_inputs(B, HW, C, nc, dtype)
    db, dw, dx = run_head_bwd(mem, dl, pooled_d, w, HW, C, C, p=p, seed=seed)
    rdb, bdb, rdw, bdw, rg, bg = head_bwd_ref(dl, pooled_d, w, HW, keep, p)
    assert (dx[~keep[:, None, :].repeat(HW, 1)] == 0).all(), "dx is not zero where the forward dropped"
    assert (np.abs(dx.astype(np.float64) - rg[:, None, :]) <= bg[:, None, :]).all() and (np.abs(dw - rdw) <= bdw).all() and (np.abs(db - rdb) <= bdb).all()
    if p < 1:
        assert (dx[keep[:, None, :].repeat(HW, 1)] != 0).mean() > 0.99


def check_ce_bwd(mem, nc, B, eps, dtype):
    z, labels = cr.post_inputs(B, nc, dtype)
    rs = np.random.RandomState(nc * 17 + B)
    grad_rows = (rs.uniform(0.5, 1.5, B) / B * np.where(np.arange(B) % 2, 1.0, 128.0)).astype(np.float32)   # (a scaled loss's rows beside plain ones)
    got = run_ce_bwd(mem, z, labels, eps, grad_rows, ld=nc + 3, ldd=nc + 5)
    ref, bound = ce_bwd_ref(z, labels, eps, grad_rows)
    err = np.abs(got.astype(np.float64) - ref)
    print(f"ce bwd nc {nc} B {B} eps {eps} {np.dtype(dtype).name}: max err / bound {(err / bound).max():.3f}")
    assert (err <= bound).all(), (err / bound).max()
    assert (np.abs(got.astype(np.float64).sum(1)) <= bound.sum(1)).all(), "a row does not sum to zero within the bound"
    bad = labels.copy()
    bad[0] = nc
    got2 = run_ce_bwd(mem, z, bad, eps, grad_rows, ld=nc + 3, ldd=nc + 5)
    assert np.isnan(got2[0]).all() and np.array_equal(got2[1:], got[1:])
    bad[0] = -1
    assert np.isnan(run_ce_bwd(mem, z, bad, eps, grad_rows)[0]).all()


# ---- whole model (the product path: model(x) -> criterion -> backward; CPU tensors under the test seam, or the GPU) ---------------------------
def cls_model(device="cpu"):
    from yolov5_amd.yolo import ClassificationModel, DetectionModel

    m = ClassificationModel(model=DetectionModel("yolov5n.yaml"), nc=cr.MODEL_NC, cutoff=10)
    m.load_state_dict(cr.cls_state_dict("yolov5n", cr.MODEL_NC))
    m.model[-1].drop.p = 0.0   # (the reference's Dropout streams cannot be reproduced: the fixture was written without Dropout)
    return m.to(device).train()


class RecordingSink:
    """Stand-in for HipDDP's gradient sink (torch_utils.py): records what the backward plan tells it."""

    def __init__(self):
        self.ready, self.begun, self.finished = [], 0, 0

    def begin(self, eng):
        self.begun += 1

    def bucket_of(self, i):
        return self

    def grad_ready(self, i):
        self.ready.append(i)

    def finish(self, grads):
        self.finished += 1

    def abort(self):
        raise AssertionError("the backward plan aborted")


def check_model_step(device, fp16):
    """One train-mode step on fixture (a): loss, stored gradients, per-parameter norms and projections, running statistics, the gradient sink."""
    import torch

    from yolov5_amd.torch_utils import smartCrossEntropyLoss

    g = golden()
    m = cls_model(device)
    sink = m.__dict__["_ddp_sink"] = RecordingSink()
    x = step_input().to(device)
    labels = torch.tensor(STEP_LABELS, dtype=torch.int64, device=device)
    state = torch.get_rng_state()
    logits = m(x.half() if fp16 else x)
    assert torch.equal(torch.get_rng_state(), state), "a forward with Dropout 0 drew from torch's generator"
    assert logits.dtype == (torch.float16 if fp16 else torch.float32) and tuple(logits.shape) == (STEP_INPUT[0], cr.MODEL_NC) and logits.requires_grad
    loss0 = float(smartCrossEntropyLoss(0.0)(logits.detach(), labels))
    loss1 = smartCrossEntropyLoss(0.1)(logits, labels)
    loss1.backward()
    names = str(g["names"]).split("\n")
    assert names == [n for n, _ in m.named_parameters()]
    assert sorted(sink.ready) == list(range(len(names))) and sink.begun == 1 and sink.finished == 1, "the sink did not get every parameter index exactly once"
    rtol = 2e-2 if fp16 else 1e-4
    print(f"model step {'fp16' if fp16 else 'fp32'}: loss {loss0:.6f} / {float(loss1.detach()):.6f}, fixture {float(g['a_loss0']):.6f} / {float(g['a_loss1']):.6f}")
    assert abs(loss0 - float(g["a_loss0"])) <= rtol * float(g["a_loss0"]) and abs(float(loss1.detach()) - float(g["a_loss1"])) <= rtol * float(g["a_loss1"])
    worst = dict(rel=0.0, cos=1.0, norm=0.0, proj=0.0)
    for k, (n, p) in enumerate(m.named_parameters()):
        assert p.grad is not None and p.grad.dtype == torch.float32, n
        gr = p.grad.detach().double().cpu().numpy().ravel()
        rn = float(g["a_norm"][k])
        dn = abs(np.linalg.norm(gr) - rn) / rn
        V = projections(n, gr.size)
        dp = float((np.abs(V @ gr - g["a_proj"][k]) / (rn * np.linalg.norm(V, axis=1))).max())
        worst["norm"], worst["proj"] = max(worst["norm"], dn), max(worst["proj"], dp)
        if fp16:
            assert dn <= 0.25, (n, dn)
        else:
            assert dn <= 2e-3 and dp <= 2e-3, (n, dn, dp)
        if n in FULL_GRADS:
            ref = g["a_grad_" + n].ravel()
            rel = float(np.linalg.norm(gr - ref) / np.linalg.norm(ref))
            cos = float(gr @ ref / (np.linalg.norm(gr) * np.linalg.norm(ref)))
            worst["rel"], worst["cos"] = max(worst["rel"], rel), min(worst["cos"], cos)
            assert (cos > 0.97 and rel < 0.25) if fp16 else rel < 2e-3, (n, rel, cos)
    print(f"  worst over {len(names)} parameters: norm deviation {worst['norm']:.3e}, projection deviation {worst['proj']:.3e}; stored gradients: "
          f"relative L2 {worst['rel']:.3e}, cosine {worst['cos']:.6f}")
    # the head BatchNorm's running statistics took the step, and the eval plan sees them
    bn = m.model[9].conv.bn
    tol = dict(rtol=2e-2, atol=2e-3) if fp16 else dict(rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(bn.running_mean.cpu().numpy(), g["a_rm"], **tol)
    np.testing.assert_allclose(bn.running_var.cpu().numpy(), g["a_rv"], **tol)
    return m


def check_eval_sees_the_step(device):
    """model.eval() before and after a train-mode forward: the logits move with the running statistics (momentum 0.03) -- and a second eval call
    without a step in between repeats the first bit for bit."""
    import torch

    m = cls_model(device)
    x = step_input().to(device)
    with torch.no_grad():
        before = m.eval()(x).clone()
        m.train()(x)
        after = m.eval()(x).clone()
        again = m.eval()(x)
    assert torch.isfinite(after).all() and not torch.equal(before, after) and torch.equal(after, again)
    # the statistics moved by 3 %: so do the logits, roughly -- not by more than a fifth of their spread
    assert float((after - before).abs().max()) < 0.2 * float(before.max() - before.min())


def check_stale_backward(device):
    import pytest
    import torch

    m = cls_model(device)
    x = step_input().to(device)
    l1 = m(x)
    l2 = m(x)
    with pytest.raises(RuntimeError, match="no longer the model's latest"):
        l1.sum().backward()
    l2.sum().backward()
    assert all(p.grad is not None for p in m.parameters())


def traj_loader(device, half=False):
    import torch

    xs = [b.to(device) for b in cr.val_inputs()[:2]]
    return [(x.half() if half else x, torch.tensor(l, dtype=torch.int64, device=device)) for x, l in zip(xs, TRAJ_LABELS)]


def check_trajectory(device, name):
    """classify_train.train (fp32 plan, EMA) on fixture (c): lr exact; losses and the final linear.bias of model and EMA within 4 x the largest
    deviation of the reference's own fp32 run from its fp64 run (were that zero, the project's rtol 1e-4)."""
    from yolov5_amd import classify_train

    g = golden()
    m = cls_model(device)
    out = classify_train.train(m, traj_loader(device), None, epochs=TRAJ_EPOCHS, optimizer_name=name, amp=False, ema=True, **TRAJ_ARGS)
    pre = f"c_{name}_64_"
    np.testing.assert_allclose(np.array(out["lr"]), g[pre + "lr"], rtol=1e-15, atol=0)
    got = dict(losses=out["losses"].double().numpy(), bias=m.model[9].linear.bias.detach().double().cpu().numpy(),
               ema_bias=out["ema"].ema.model[9].linear.bias.detach().double().cpu().numpy())
    ratios = {}
    for k, v in got.items():
        noise = float(np.abs(g[f"c_{name}_32_{k}"] - g[pre + k]).max())
        allowed = 4 * noise if noise > 0 else 1e-4 * float(np.abs(g[pre + k]).max())
        ratios[k] = float(np.abs(v - g[pre + k]).max()) / allowed
    print(f"trajectory {name}: deviation from the fp64 reference / allowed = {ratios}; losses {got['losses']}")
    assert all(r <= 1.0 for r in ratios.values()), ratios
    return out
