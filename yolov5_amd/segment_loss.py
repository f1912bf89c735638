"""Segmentation `ComputeLoss` with the reference's constructor / call signature (utils/segment/loss.py:15-199), executed by the HIP
kernels behind `y5_seg_loss_forward` / `y5_seg_loss_backward` (include/yolov5_hip.h, yolov5_amd/csrc/seg_loss.h).

    compute_loss = ComputeLoss(model, overlap=True)              # model.hyp, model.model[-1] (Segment) are read like the reference
    loss, items = compute_loss((p, proto), targets, masks)       # items = (lbox, lseg, lobj, lcls)
    loss.backward()                                              # d loss / d p[i] and d loss / d proto

The reference's per-level x per-image Python loop over the mask term (loss.py:88-103, one host sync per level for `b.unique()`) is
one set of kernels here, with no host synchronisation except with `autobalance=True` (one read of nl floats, as in yolov5_amd.loss).
Masks whose resolution differs from the proto's are resampled with F.interpolate(mode="nearest") as loss.py:89-90 does.
Unsupported options raise: `sort_obj_iou`, `gr != 1`.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn.functional as F

from . import _lib
from .loss import ComputeLoss as _DetLoss, _void_pp, de_parallel


def _ptr_or_none(t):
    return C.c_void_p(t.data_ptr()) if t.numel() else None  # (an empty mask stack, e.g. overlap=False without targets)


class _SegLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, owner, targets, masks, proto, *p):
        lib = _lib.lib()
        dev = p[0].device
        nt = int(targets.shape[0])
        d = owner._seg_desc(p, proto, masks, nt)
        nbytes = lib.y5_seg_loss_workspace_bytes(C.byref(d), nt)
        if nbytes == 0:
            _lib.check(-1, lib)
        ws = _lib.workspace(nbytes, dev)
        out = torch.empty(5, dtype=torch.float32, device=dev)
        st = _lib.stream(dev)
        p = [pi.contiguous() for pi in p]
        proto = proto.contiguous()
        rc = lib.y5_seg_loss_forward(C.byref(d), _void_pp(p), C.c_void_p(proto.data_ptr()),
                                     C.c_void_p(targets.data_ptr()) if nt else None, nt, _ptr_or_none(masks),
                                     C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), nbytes, st)
        _lib.check(rc, lib)
        ctx.d, ctx.nt, ctx.ws, ctx.nbytes, ctx.p, ctx.proto, ctx.masks = d, nt, ws, nbytes, p, proto, masks
        owner._last = (d, nt, ws)
        loss, items = out[0:1], out[1:5]
        ctx.mark_non_differentiable(items)
        return loss, items

    @staticmethod
    def backward(ctx, g_loss, _g_items):
        lib = _lib.lib()
        p, proto = ctx.p, ctx.proto
        gs = g_loss.detach().to(torch.float32).reshape(-1)[:1].contiguous()
        dp = [torch.empty_like(pi) for pi in p]
        dproto = torch.empty_like(proto)
        st = _lib.stream(proto.device)
        rc = lib.y5_seg_loss_backward(C.byref(ctx.d), _void_pp(p), C.c_void_p(proto.data_ptr()), ctx.nt, _ptr_or_none(ctx.masks),
                                      C.c_void_p(gs.data_ptr()), _void_pp(dp), C.c_void_p(dproto.data_ptr()),
                                      C.c_void_p(ctx.ws.data_ptr()), ctx.nbytes, st)
        _lib.check(rc, lib)
        return (None, None, None, dproto, *dp)


class ComputeLoss(_DetLoss):
    """utils/segment/loss.py:15-120."""

    def __init__(self, model, autobalance=False, overlap=False):
        super().__init__(model, autobalance=autobalance)
        self.overlap = overlap
        self.nm = int(getattr(de_parallel(model).model[-1], "nm", 0))
        if not 1 <= self.nm <= 32:
            raise ValueError(f"segmentation ComputeLoss: the last module must be a Segment head with 1..32 masks, got nm={self.nm}")

    def _seg_desc(self, p, proto, masks, nt):
        det = self._desc([pi[..., :5 + self.nc] for pi in p])  # validates every level except its last dimension
        for i, pi in enumerate(p):
            if pi.shape[4] != 5 + self.nc + self.nm:
                raise ValueError(f"ComputeLoss: level {i} has shape {tuple(pi.shape)}, expected (bs,{self.na},ny,nx,{5 + self.nc + self.nm})")
        bs = int(p[0].shape[0])
        if proto.dtype != p[0].dtype or not _lib.accepts(proto) or proto.dim() != 4 or tuple(proto.shape[:2]) != (bs, self.nm):
            raise ValueError(f"ComputeLoss: proto must be a GPU ({bs}, {self.nm}, mh, mw) tensor of the predictions' dtype, got "
                             f"{tuple(proto.shape)} {proto.dtype}")
        d = _lib.SegLossDesc()
        d.det = det
        d.nm, d.mh, d.mw = self.nm, int(proto.shape[2]), int(proto.shape[3])
        d.overlap = 1 if self.overlap else 0
        d.mask_dtype = _lib.Y5_U8 if masks.dtype == torch.uint8 else _lib.Y5_F32
        d.nmask = int(masks.shape[0])
        if self.overlap and d.nmask != bs:
            raise IndexError(f"ComputeLoss(overlap=True): masks must hold one plane per image ({bs}), got {d.nmask}")
        if not self.overlap and d.nmask < nt:
            raise IndexError(f"ComputeLoss(overlap=False): masks must hold one plane per target ({nt}), got {d.nmask}")
        return d

    def __call__(self, preds, targets, masks):
        p, proto = preds
        if len(p) != self.nl:
            raise ValueError(f"ComputeLoss: expected {self.nl} prediction levels, got {len(p)}")
        dev = p[0].device
        targets = targets.to(device=dev, dtype=torch.float32).contiguous()
        masks = masks.to(dev)
        mh, mw = int(proto.shape[2]), int(proto.shape[3])
        if masks.dtype not in (torch.uint8, torch.float32):
            masks = masks.float()
        if tuple(masks.shape[-2:]) != (mh, mw):  # loss.py:89-90 (only reached with matched rows there: an empty stack is just reshaped)
            masks = F.interpolate(masks[None].float(), (mh, mw), mode="nearest")[0] if masks.numel() else masks.new_zeros((0, mh, mw))
        masks = masks.contiguous()
        out = _SegLossFn.apply(self, targets, masks, proto, *p)
        if self.autobalance:
            self._autobalance(len(p))
        return out

    def _autobalance(self, nl):
        d, nt, ws = self._last
        off = _lib.lib().y5_seg_loss_obji_offset(C.byref(d), nt)
        if off < 0:
            _lib.check(-1, _lib.lib())
        obji = ws[off:off + 4 * nl].view(torch.float32).tolist()
        self.last_obji = obji
        for i in range(nl):
            self.balance[i] = self.balance[i] * 0.9999 + 0.0001 / obji[i]
        self.balance = [x / self.balance[self.ssi] for x in self.balance]

    def build_targets(self, p, targets):
        raise NotImplementedError("segmentation ComputeLoss.build_targets: use yolov5_amd.loss.ComputeLoss.build_targets for the indices")
