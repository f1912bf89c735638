// C-ABI launcher for ComputeLoss forward/backward (loss_kernels.h).  Built with -ffp-contract=off so that the target
// assignment arithmetic (fp32 multiply / divide / compare chains of utils/loss.py:205-243) is not re-associated.
#include <hip/hip_runtime.h>

#include "../../include/yolov5_hip.h"
#include "loss_kernels.h"
#include "seg_loss.h"
#include "y5_host.h"

namespace {

struct LevelOff { size_t rb, ra, rgj, rgi, rcls, next, rt, tbox, anch, iou, rl_box, rl_cls, G, head, obj_part; };
struct Layout { size_t n_rows, obji; LevelOff lv[Y5_LOSS_MAX_NL]; long long cap, cells[Y5_LOSS_MAX_NL]; size_t head_begin, head_end, total; };

size_t take(size_t& o, size_t bytes) { const size_t r = o; o += (bytes + 255) & ~(size_t)255; return r; }

int validate(const y5_loss_desc* d, int nt) {
  if (!d) return y5_fail(Y5_ERR_BAD_ARG, "loss: null descriptor");
  if (d->dtype != Y5_F16 && d->dtype != Y5_F32) return y5_fail(Y5_ERR_BAD_ARG, "loss: dtype must be Y5_F16 or Y5_F32");
  if (d->nl < 1 || d->nl > Y5_LOSS_MAX_NL || d->na < 1 || d->na > Y5_LOSS_MAX_NA || d->nc < 1 || d->bs < 1 || nt < 0)
    return y5_fail(Y5_ERR_BAD_ARG, "loss: nl/na/nc/bs/nt out of range");
  for (int i = 0; i < d->nl; ++i)
    if (d->ny[i] < 1 || d->nx[i] < 1 || (long long)d->bs * d->na * d->ny[i] * d->nx[i] >= 0x7fffffffLL)
      return y5_fail(Y5_ERR_BAD_ARG, "loss: bad grid size");
  if (5LL * d->na * nt >= 0x7fffffffLL) return y5_fail(Y5_ERR_UNSUPPORTED, "loss: too many targets");
  return Y5_OK;
}

// no: row stride of p (5 + nc, or 5 + nc + nm for the segmentation loss); seg adds each row's target index
Layout layout(const y5_loss_desc* d, int nt, int no, bool seg, size_t& o) {
  Layout L{};
  const long long cap = 5LL * d->na * nt;
  const size_t capz = (size_t)(cap > 0 ? cap : 1);
  L.cap = cap;
  o = 0;
  L.n_rows = take(o, sizeof(int) * Y5_LOSS_MAX_NL);
  L.obji = take(o, sizeof(float) * Y5_LOSS_MAX_NL);
  for (int i = 0; i < d->nl; ++i) {
    LevelOff& v = L.lv[i];
    v.rb = take(o, capz * 4); v.ra = take(o, capz * 4); v.rgj = take(o, capz * 4); v.rgi = take(o, capz * 4);
    v.rcls = take(o, capz * 4); v.next = take(o, capz * 4);
    v.rt = seg ? take(o, capz * 4) : 0;
    v.tbox = take(o, capz * 16); v.anch = take(o, capz * 8);
    v.iou = take(o, capz * 4); v.rl_box = take(o, capz * 4); v.rl_cls = take(o, capz * 4);
    v.G = take(o, capz * no * 4);
    L.cells[i] = (long long)d->bs * d->na * d->ny[i] * d->nx[i];
    v.obj_part = take(o, (size_t)((L.cells[i] + 255) / 256) * 4);
  }
  L.head_begin = o;  // all head arrays are contiguous: one memset(0xFF) per forward
  for (int i = 0; i < d->nl; ++i) L.lv[i].head = take(o, (size_t)L.cells[i] * 4);
  L.head_end = o;
  L.total = o;
  return L;
}

Layout layout(const y5_loss_desc* d, int nt) {
  size_t o;
  return layout(d, nt, 5 + d->nc, false, o);
}

void fill(Y5LossParams& P, const y5_loss_desc* d, const Layout& L, char* ws, int nt, int no = 0, bool seg = false) {
  P.nl = d->nl; P.na = d->na; P.nc = d->nc; P.no = no ? no : 5 + d->nc; P.bs = d->bs; P.nt = nt;
  P.hyp_box = d->hyp_box; P.hyp_obj = d->hyp_obj; P.hyp_cls = d->hyp_cls; P.cls_pw = d->cls_pw; P.obj_pw = d->obj_pw; P.fl_gamma = d->fl_gamma;
  P.anchor_t = d->anchor_t; P.cp = d->cp; P.cn = d->cn;
  P.n_rows = reinterpret_cast<int*>(ws + L.n_rows);
  P.obji = reinterpret_cast<float*>(ws + L.obji);
  for (int i = 0; i < d->nl; ++i) {
    Y5LossLevel& v = P.lv[i];
    const LevelOff& f = L.lv[i];
    v.ny = d->ny[i]; v.nx = d->nx[i]; v.cells = L.cells[i]; v.cap = L.cap;
    v.rb = (int*)(ws + f.rb); v.ra = (int*)(ws + f.ra); v.rgj = (int*)(ws + f.rgj); v.rgi = (int*)(ws + f.rgi);
    v.rcls = (int*)(ws + f.rcls); v.next = (int*)(ws + f.next);
    v.rt = seg ? (int*)(ws + f.rt) : nullptr;
    v.tbox = (float*)(ws + f.tbox); v.anch = (float*)(ws + f.anch); v.iou = (float*)(ws + f.iou);
    v.rl_box = (float*)(ws + f.rl_box); v.rl_cls = (float*)(ws + f.rl_cls); v.G = (float*)(ws + f.G);
    v.head = (int*)(ws + f.head); v.obj_part = (float*)(ws + f.obj_part);
    v.balance = d->balance[i];
    for (int a = 0; a < d->na * 2; ++a) v.anchors[a] = d->anchors[i * Y5_LOSS_MAX_NA * 2 + a];
  }
}

}  // namespace

extern "C" size_t y5_loss_workspace_bytes(const y5_loss_desc* d, int nt) {
  if (validate(d, nt)) return 0;
  return layout(d, nt).total;
}

extern "C" long long y5_loss_obji_offset(const y5_loss_desc* d, int nt) {
  if (validate(d, nt)) return -1;
  return (long long)layout(d, nt).obji;
}

extern "C" int y5_loss_targets_layout(const y5_loss_desc* d, int nt, int level, size_t offs[10], long long* cap) {
  if (int rc = validate(d, nt)) return rc;
  if (level < 0 || level >= d->nl || !offs) return y5_fail(Y5_ERR_BAD_ARG, "loss_targets_layout: bad level");
  const Layout L = layout(d, nt);
  const LevelOff& f = L.lv[level];
  const size_t o[10] = {L.n_rows + 4 * (size_t)level, f.rb, f.ra, f.rgj, f.rgi, f.rcls, f.tbox, f.anch, f.iou, f.G};
  for (int i = 0; i < 10; ++i) offs[i] = o[i];
  if (cap) *cap = L.cap;
  return Y5_OK;
}

extern "C" int y5_loss_forward(const y5_loss_desc* d, const void* const* p, const float* targets, int nt, float* out4,
                               void* ws_, size_t ws_bytes, void* stream_) {
  hipStream_t st = static_cast<hipStream_t>(stream_);
  if (int rc = validate(d, nt)) return rc;
  if (!p || !out4 || !ws_ || (nt > 0 && !targets)) return y5_fail(Y5_ERR_BAD_ARG, "loss: null pointer");
  const Layout L = layout(d, nt);
  if (ws_bytes < L.total || ((uintptr_t)ws_ & 255)) return y5_fail(Y5_ERR_WORKSPACE, "loss: workspace too small or misaligned");
  char* ws = static_cast<char*>(ws_);
  Y5LossParams P{};
  fill(P, d, L, ws, nt);
  P.targets = targets; P.out = out4;
  for (int i = 0; i < d->nl; ++i) {
    if (!p[i]) return y5_fail(Y5_ERR_BAD_ARG, "loss: null prediction level");
    P.lv[i].p = p[i];
  }
  if (hipMemsetAsync(ws + L.head_begin, 0xFF, L.head_end - L.head_begin, st) != hipSuccess ||
      hipMemsetAsync(ws + L.n_rows, 0, sizeof(int) * Y5_LOSS_MAX_NL, st) != hipSuccess)
    return y5_fail(Y5_ERR_RUNTIME, "loss: memset failed");
  if (nt > 0) {
    hipLaunchKernelGGL(y5_loss_build_targets_kernel, dim3((unsigned)d->nl), dim3(1024), 4096, st, P);
    const unsigned rb = (unsigned)((L.cap + 3) / 4);
    for (int i = 0; i < d->nl; ++i) {
      if (d->dtype == Y5_F16) hipLaunchKernelGGL((y5_loss_rows_kernel<half_t>), dim3(rb), dim3(256), 0, st, P, i);
      else hipLaunchKernelGGL((y5_loss_rows_kernel<float>), dim3(rb), dim3(256), 0, st, P, i);
    }
  }
  for (int i = 0; i < d->nl; ++i) {
    const unsigned nb = (unsigned)((L.cells[i] + 255) / 256);
    if (d->dtype == Y5_F16) hipLaunchKernelGGL((y5_loss_obj_fwd_kernel<half_t>), dim3(nb), dim3(256), 1024, st, P, i);
    else hipLaunchKernelGGL((y5_loss_obj_fwd_kernel<float>), dim3(nb), dim3(256), 1024, st, P, i);
  }
  hipLaunchKernelGGL(y5_loss_finish_kernel, dim3(1), dim3(256), 2048, st, P);
  return y5_check_launch("y5_loss_forward");
}

extern "C" int y5_loss_backward(const y5_loss_desc* d, const void* const* p, int nt, const float* grad_scale, void* const* dp,
                                void* ws_, size_t ws_bytes, void* stream_) {
  hipStream_t st = static_cast<hipStream_t>(stream_);
  if (int rc = validate(d, nt)) return rc;
  if (!p || !dp || !ws_) return y5_fail(Y5_ERR_BAD_ARG, "loss: null pointer");
  const Layout L = layout(d, nt);
  if (ws_bytes < L.total || ((uintptr_t)ws_ & 255)) return y5_fail(Y5_ERR_WORKSPACE, "loss: workspace too small or misaligned");
  Y5LossParams P{};
  fill(P, d, L, static_cast<char*>(ws_), nt);
  P.gscale = grad_scale;
  for (int i = 0; i < d->nl; ++i) {
    if (!p[i] || !dp[i]) return y5_fail(Y5_ERR_BAD_ARG, "loss: null level pointer");
    P.lv[i].p = p[i];
    P.lv[i].dp = dp[i];
  }
  for (int i = 0; i < d->nl; ++i) {
    const unsigned nb = (unsigned)((L.cells[i] + 255) / 256);
    if (d->dtype == Y5_F16) hipLaunchKernelGGL((y5_loss_bwd_kernel<half_t>), dim3(nb), dim3(256), 2048, st, P, i);
    else hipLaunchKernelGGL((y5_loss_bwd_kernel<float>), dim3(nb), dim3(256), 2048, st, P, i);
  }
  return y5_check_launch("y5_loss_backward");
}

// ---- segmentation loss (seg_loss.h) ---------------------------------------------------------------------------------------------
namespace {

struct SegLayout { Layout L; size_t out4, ti, img_cnt, img_off, img_n, e_lvl, e_row, e_b, e_gt, e_n, e_box, e_area, e_coef, e_loss, total; };

int seg_validate(const y5_seg_loss_desc* d, int nt) {
  if (!d) return y5_fail(Y5_ERR_BAD_ARG, "seg_loss: null descriptor");
  if (int rc = validate(&d->det, nt)) return rc;
  if (d->nm < 1 || d->nm > Y5_SEG_MAX_NM || d->mh < 1 || d->mw < 1 || (long long)d->mh * d->mw >= 0x7fffffffLL / Y5_SEG_MAX_NM)
    return y5_fail(Y5_ERR_BAD_ARG, "seg_loss: nm must be 1..32 and mh, mw >= 1");
  if (d->det.bs > Y5_SEG_MAX_BS) return y5_fail(Y5_ERR_UNSUPPORTED, "seg_loss: batch size above 4096");
  if (d->mask_dtype != Y5_F32 && d->mask_dtype != Y5_U8) return y5_fail(Y5_ERR_BAD_ARG, "seg_loss: mask_dtype must be Y5_F32 or Y5_U8");
  if (d->overlap ? d->nmask != d->det.bs : d->nmask < nt)
    return y5_fail(Y5_ERR_BAD_ARG, "seg_loss: masks must be (bs, mh, mw) with overlap, (>= nt, mh, mw) without");
  return Y5_OK;
}

SegLayout seg_layout(const y5_seg_loss_desc* d, int nt) {
  SegLayout S{};
  size_t o;
  S.L = layout(&d->det, nt, 5 + d->det.nc + d->nm, true, o);
  const size_t E = (size_t)(S.L.cap > 0 ? S.L.cap : 1) * d->det.nl, nz = (size_t)(nt > 0 ? nt : 1), bs = (size_t)d->det.bs;
  S.out4 = take(o, 16); S.ti = take(o, nz * 4);
  S.img_cnt = take(o, bs * 4); S.img_off = take(o, bs * 4); S.img_n = take(o, bs * 4);
  S.e_lvl = take(o, E * 4); S.e_row = take(o, E * 4); S.e_b = take(o, E * 4); S.e_gt = take(o, E * 4); S.e_n = take(o, E * 4);
  S.e_box = take(o, E * 16); S.e_area = take(o, E * 4); S.e_coef = take(o, E * 4 * d->nm); S.e_loss = take(o, E * 4);
  S.total = o;
  S.L.total = o;
  return S;
}

void seg_fill(Y5LossParams& P, Y5SegParams& Q, const y5_seg_loss_desc* d, const SegLayout& S, char* ws, int nt) {
  fill(P, &d->det, S.L, ws, nt, 5 + d->det.nc + d->nm, true);
  Q.nm = d->nm; Q.mh = d->mh; Q.mw = d->mw; Q.overlap = d->overlap ? 1 : 0; Q.nmask = d->nmask;
  Q.ti = (float*)(ws + S.ti); Q.img_cnt = (int*)(ws + S.img_cnt); Q.img_off = (int*)(ws + S.img_off); Q.img_n = (int*)(ws + S.img_n);
  Q.e_lvl = (int*)(ws + S.e_lvl); Q.e_row = (int*)(ws + S.e_row); Q.e_b = (int*)(ws + S.e_b); Q.e_gt = (int*)(ws + S.e_gt);
  Q.e_n = (int*)(ws + S.e_n); Q.e_box = (float*)(ws + S.e_box); Q.e_area = (float*)(ws + S.e_area); Q.e_coef = (float*)(ws + S.e_coef);
  Q.e_loss = (float*)(ws + S.e_loss); Q.out4 = (float*)(ws + S.out4);
}

template <typename T, typename MT>
void seg_launch_rows(const Y5LossParams& P, const Y5SegParams& Q, unsigned nblk, hipStream_t st) {
  hipLaunchKernelGGL((y5_seg_rows_kernel<T, MT>), dim3(nblk), dim3(256), Y5_SEG_ROWS_LDS, st, P, Q);
}

template <typename T, typename MT>
void seg_launch_dproto(const Y5LossParams& P, const Y5SegParams& Q, hipStream_t st) {
  const unsigned nt = (unsigned)(((Q.mw + Y5_SEG_TW - 1) / Y5_SEG_TW) * ((Q.mh + Y5_SEG_TH - 1) / Y5_SEG_TH));
  hipLaunchKernelGGL((y5_seg_dproto_kernel<T, MT>), dim3(nt, (unsigned)P.bs), dim3(256), 0, st, P, Q);
}

}  // namespace

extern "C" size_t y5_seg_loss_workspace_bytes(const y5_seg_loss_desc* d, int nt) {
  if (seg_validate(d, nt)) return 0;
  return seg_layout(d, nt).total;
}

extern "C" long long y5_seg_loss_obji_offset(const y5_seg_loss_desc* d, int nt) {
  if (seg_validate(d, nt)) return -1;
  return (long long)seg_layout(d, nt).L.obji;
}

extern "C" int y5_seg_loss_forward(const y5_seg_loss_desc* d, const void* const* p, const void* proto, const float* targets, int nt,
                                   const void* masks, float* out5, void* ws_, size_t ws_bytes, void* stream_) {
  hipStream_t st = static_cast<hipStream_t>(stream_);
  if (int rc = seg_validate(d, nt)) return rc;
  if (!p || !proto || !out5 || !ws_ || (nt > 0 && (!targets || !masks))) return y5_fail(Y5_ERR_BAD_ARG, "seg_loss: null pointer");  // masks are not read without targets
  const SegLayout S = seg_layout(d, nt);
  if (ws_bytes < S.total || ((uintptr_t)ws_ & 255)) return y5_fail(Y5_ERR_WORKSPACE, "seg_loss: workspace too small or misaligned");
  char* ws = static_cast<char*>(ws_);
  Y5LossParams P{};
  Y5SegParams Q{};
  seg_fill(P, Q, d, S, ws, nt);
  P.targets = targets; P.out = Q.out4;
  Q.proto = proto; Q.masks = masks; Q.out5 = out5;
  const bool f16 = d->det.dtype == Y5_F16, u8 = d->mask_dtype == Y5_U8;
  for (int i = 0; i < d->det.nl; ++i) {
    if (!p[i]) return y5_fail(Y5_ERR_BAD_ARG, "seg_loss: null prediction level");
    P.lv[i].p = p[i];
  }
  if (hipMemsetAsync(ws + S.L.head_begin, 0xFF, S.L.head_end - S.L.head_begin, st) != hipSuccess ||
      hipMemsetAsync(ws + S.L.n_rows, 0, sizeof(int) * Y5_LOSS_MAX_NL, st) != hipSuccess)
    return y5_fail(Y5_ERR_RUNTIME, "seg_loss: memset failed");
  if (nt > 0) {
    hipLaunchKernelGGL(y5_loss_build_targets_kernel, dim3((unsigned)d->det.nl), dim3(1024), 4096, st, P);
    const unsigned rb = (unsigned)((S.L.cap + 3) / 4);
    for (int i = 0; i < d->det.nl; ++i) {
      if (f16) hipLaunchKernelGGL((y5_loss_rows_kernel<half_t>), dim3(rb), dim3(256), 0, st, P, i);
      else hipLaunchKernelGGL((y5_loss_rows_kernel<float>), dim3(rb), dim3(256), 0, st, P, i);
    }
    hipLaunchKernelGGL(y5_seg_tidx_kernel, dim3(1), dim3(1024), 16, st, P, Q);
    if (f16) hipLaunchKernelGGL((y5_seg_group_kernel<half_t>), dim3((unsigned)d->det.bs), dim3(1024), Y5_SEG_GROUP_LDS(d->det.bs), st, P, Q);
    else hipLaunchKernelGGL((y5_seg_group_kernel<float>), dim3((unsigned)d->det.bs), dim3(1024), Y5_SEG_GROUP_LDS(d->det.bs), st, P, Q);
    const unsigned ne = (unsigned)(S.L.cap * d->det.nl);
    if (f16) { if (u8) seg_launch_rows<half_t, unsigned char>(P, Q, ne, st); else seg_launch_rows<half_t, float>(P, Q, ne, st); }
    else { if (u8) seg_launch_rows<float, unsigned char>(P, Q, ne, st); else seg_launch_rows<float, float>(P, Q, ne, st); }
  }
  for (int i = 0; i < d->det.nl; ++i) {
    const unsigned nb = (unsigned)((S.L.cells[i] + 255) / 256);
    if (f16) hipLaunchKernelGGL((y5_loss_obj_fwd_kernel<half_t>), dim3(nb), dim3(256), 1024, st, P, i);
    else hipLaunchKernelGGL((y5_loss_obj_fwd_kernel<float>), dim3(nb), dim3(256), 1024, st, P, i);
  }
  hipLaunchKernelGGL(y5_loss_finish_kernel, dim3(1), dim3(256), 2048, st, P);
  hipLaunchKernelGGL(y5_seg_finish_kernel, dim3(1), dim3(256), 2048, st, P, Q);
  return y5_check_launch("y5_seg_loss_forward");
}

extern "C" int y5_seg_loss_backward(const y5_seg_loss_desc* d, const void* const* p, const void* proto, int nt, const void* masks,
                                    const float* grad_scale, void* const* dp, void* dproto, void* ws_, size_t ws_bytes, void* stream_) {
  hipStream_t st = static_cast<hipStream_t>(stream_);
  if (int rc = seg_validate(d, nt)) return rc;
  if (!p || !dp || !proto || !dproto || !ws_ || (nt > 0 && !masks)) return y5_fail(Y5_ERR_BAD_ARG, "seg_loss: null pointer");
  const SegLayout S = seg_layout(d, nt);
  if (ws_bytes < S.total || ((uintptr_t)ws_ & 255)) return y5_fail(Y5_ERR_WORKSPACE, "seg_loss: workspace too small or misaligned");
  Y5LossParams P{};
  Y5SegParams Q{};
  seg_fill(P, Q, d, S, static_cast<char*>(ws_), nt);
  P.gscale = grad_scale;
  Q.proto = proto; Q.dproto = dproto; Q.masks = masks;
  const bool f16 = d->det.dtype == Y5_F16, u8 = d->mask_dtype == Y5_U8;
  for (int i = 0; i < d->det.nl; ++i) {
    if (!p[i] || !dp[i]) return y5_fail(Y5_ERR_BAD_ARG, "seg_loss: null level pointer");
    P.lv[i].p = p[i];
    P.lv[i].dp = dp[i];
  }
  if (nt == 0) hipMemsetAsync(Q.img_n, 0, sizeof(int) * d->det.bs, st);  // no list: S5 writes zeros
  for (int i = 0; i < d->det.nl; ++i) {
    const unsigned nb = (unsigned)((S.L.cells[i] + 255) / 256);
    if (f16) hipLaunchKernelGGL((y5_loss_bwd_kernel<half_t>), dim3(nb), dim3(256), 2048, st, P, i);
    else hipLaunchKernelGGL((y5_loss_bwd_kernel<float>), dim3(nb), dim3(256), 2048, st, P, i);
  }
  if (f16) { if (u8) seg_launch_dproto<half_t, unsigned char>(P, Q, st); else seg_launch_dproto<half_t, float>(P, Q, st); }
  else { if (u8) seg_launch_dproto<float, unsigned char>(P, Q, st); else seg_launch_dproto<float, float>(P, Q, st); }
  return y5_check_launch("y5_seg_loss_backward");
}
