// Library core: status/error reporting, the per-device zero page, and the execution plan
// (recorded op list replayed by one host call, optionally through a captured hipGraph).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <utility>
#include <variant>
#include <vector>

#include "../../include/yolov5_hip.h"
#include "y5_host.h"

namespace {
thread_local std::string g_err;
std::mutex g_zero_mu;
void* g_zero[64] = {nullptr};
}  // namespace

int y5_fail(int code, const char* msg) {
  g_err = msg ? msg : "unknown error";
  return code;
}

int y5_check_launch(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return Y5_OK;
  g_err = std::string(what) + ": " + hipGetErrorString(e);
  return Y5_ERR_RUNTIME;
}

const void* y5_zero_page() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
  std::lock_guard<std::mutex> lk(g_zero_mu);
  if (!g_zero[dev]) {
    void* p = nullptr;
    if (hipMalloc(&p, 4096) != hipSuccess) return nullptr;
    if (hipMemset(p, 0, 4096) != hipSuccess) return nullptr;
    g_zero[dev] = p;
  }
  return g_zero[dev];
}

extern "C" int y5_version(void) { return 10000 * 0 + 100 * 1 + 0; }
extern "C" const char* y5_last_error(void) { return g_err.c_str(); }

// ---- CU budget: persistent kernels size their grids as (CUs x occupancy).  Under data-parallel training the gradient all-reduce (RCCL's own kernels,
// on the process group's stream) runs BESIDE the backward plan; with every CU held by a persistent workgroup for the whole life of each launch the
// collective's workgroups only get in at kernel boundaries (measured through a one-rank group: 28.9 MB exposed for 0.73 ms, profiles/r04).  A budget
// of CUs - r leaves r CUs' worth of workgroup slots to the collective (utils/torch_utils.py:61-70 smart_DDP; yolov5_amd.torch_utils.HipDDP sets it).
namespace { int g_cu_budget = 0; }
extern "C" int y5_set_cu_budget(int n_cus) {
  if (n_cus < 0) return y5_fail(Y5_ERR_BAD_ARG, "set_cu_budget: negative");
  g_cu_budget = n_cus;   // 0 = every CU of the device
  return Y5_OK;
}
int y5_num_cu() {
  static int cu_of_dev[64] = {};   // per device (the count of the first device queried was served for all)
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  if (!cu_of_dev[dev]) {
    int n = 0;
    hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
    cu_of_dev[dev] = n > 0 ? n : 256;
  }
  const int n = cu_of_dev[dev];
  return g_cu_budget > 0 && g_cu_budget < n ? g_cu_budget : n;
}

// ---------------------------------------------------------------------------------------------------
// plan
// ---------------------------------------------------------------------------------------------------
// One argument record per op kind.  Its fields are the parameters of the entry point the op launches, under that entry point's names
// (include/yolov5_hip.h); run() hands them on.  outputs() names, once, the pointers y5_plan_rebind_output may re-point: the main output,
// the second output and the objectness plane -- an input never appears there.
struct ConvArgs {
  y5_conv_desc d; const void* x; const void* w_packed; const float* bias; const void* residual; void* y; void* y_up2;
  template <class F> void outputs(F&& f) { f(y); f(y_up2); }
};
struct ToNhwcArgs {
  const void* src; int src_dtype; void* dst; int dst_dtype, B, C, H, W, ld; float scale;
  template <class F> void outputs(F&& f) { f(dst); }
};
struct ToNchwArgs {
  const void* src; int dtype; void* dst; int B, C, H, W, ld;
  template <class F> void outputs(F&& f) { f(dst); }
};
struct SppfPoolArgs {
  void* buf; int dtype, B, H, W, C, ld, k;
  template <class F> void outputs(F&& f) { f(buf); }
};
struct UpsampleArgs {
  const void* src; int dtype; void* dst; int B, H, W, C, lds, ldd;
  template <class F> void outputs(F&& f) { f(dst); }
};
struct CopyArgs {
  const void* src; int dtype; void* dst; int npix, C, lds, ldd;
  template <class F> void outputs(F&& f) { f(dst); }
};
// what the Detect decode and the fused head share: the anchors by value (y5_plan_set_anchors) and the objectness plane (y5_plan_set_obj_hint)
struct DetectTail { float anchors_px[16]; void* obj_hint; };
struct DecodeArgs : DetectTail {
  const void* logits; int dtype, B, ny, nx, na, no, nm, ld; float stride; void* z; int z_dtype; long long nrows_total, row_off; void* raw;
  template <class F> void outputs(F&& f) { f(z); f(raw); f(obj_hint); }
};
struct HeadArgs : DetectTail {
  y5_conv_desc d; const void* x; const void* w_packed; const float* bias; int ny, nx; float stride; void* z; long long nrows_total, row_off;
  template <class F> void outputs(F&& f) { f(z); f(obj_hint); }
};
struct StemArgs {
  const void* x_nchw; int B, H, W; const void* w_stem; const float* bias; int C2, Npad; void* y; int ldy;
  template <class F> void outputs(F&& f) { f(y); }
};
struct NopArgs {
  template <class F> void outputs(F&&) {}
};
struct BneckArgs {
  const void* x; int ldx; const void* w1_packed; const float* bias1; int Kpad1; const void* w2_packed; const float* bias2; int Kpad2; void* y;
  int ldy, B, H, W, C, add;
  template <class F> void outputs(F&& f) { f(y); }
};
struct K3pwArgs {
  y5_conv_desc d; const void* x; const void* w1_packed; const float* bias1; const void* w2_packed; const float* bias2; int C3, Npad2, Kpad2, act2;
  void* y; int ldy; void* y2; int ld2, split_n;
  template <class F> void outputs(F&& f) { f(y); f(y2); }
};
struct BneckCv3Args {
  const void* x; int ldx; const void* w1_packed; const float* bias1; int Kpad1; const void* w2_packed; const float* bias2; int Kpad2; const void* y2;
  int ld2; const void* w3_packed; const float* bias3; int Kpad3, C3, act3; void* out; int ldo, B, H, W, C, add;
  template <class F> void outputs(F&& f) { f(out); }
};
struct FrontArgs {
  const void* x_nchw; int B, H, W; const void* w_stem; const float* bias0; int C0; const void* w1_packed; const float* bias1; int C1, Npad1, Kpad1, act1;
  const void* w2_packed; const float* bias2; int C3, Npad2, Kpad2, act2; void* y; int ldy; void* y2; int ld2, split_n;
  template <class F> void outputs(F&& f) { f(y); f(y2); }
};
struct SppfFrontArgs {
  const void* x; int ldx; const void* w_packed; const float* bias; int Kpad; void* buf; int ld, B, H, W, C1, c_, k, act;
  template <class F> void outputs(F&& f) { f(buf); }
};

struct ClassifyHeadArgs {
  const void* x; int dtype, B, HW, C, ld; const void* w; const float* bias; int nc; void* logits; int ldo, form; void* workspace; size_t workspace_bytes;
  template <class F> void outputs(F&& f) { f(logits); }
};

static int run(const ConvArgs& a, void* st) { return y5_conv2d_fwd(&a.d, a.x, a.w_packed, a.bias, a.residual, a.y, a.y_up2, st); }
static int run(const ToNhwcArgs& a, void* st) { return y5_nchw_to_nhwc(a.src, a.src_dtype, a.dst, a.dst_dtype, a.B, a.C, a.H, a.W, a.ld, a.scale, st); }
static int run(const ToNchwArgs& a, void* st) { return y5_nhwc_to_nchw(a.src, a.dtype, a.dst, a.B, a.C, a.H, a.W, a.ld, st); }
static int run(const SppfPoolArgs& a, void* st) { return y5_sppf_pool(a.buf, a.dtype, a.B, a.H, a.W, a.C, a.ld, a.k, st); }
static int run(const UpsampleArgs& a, void* st) { return y5_upsample2x(a.src, a.dtype, a.dst, a.B, a.H, a.W, a.C, a.lds, a.ldd, st); }
static int run(const CopyArgs& a, void* st) { return y5_copy_slice(a.src, a.dtype, a.dst, a.npix, a.C, a.lds, a.ldd, st); }
static int run(const DecodeArgs& a, void* st) {
  return y5_detect_decode_hint(a.logits, a.dtype, a.B, a.ny, a.nx, a.na, a.no, a.nm, a.ld, a.stride, a.anchors_px, a.z, a.z_dtype, a.nrows_total, a.row_off,
                               a.raw, a.obj_hint, st);
}
static int run(const HeadArgs& a, void* st) {
  return y5_detect_head_fwd_hint(&a.d, a.x, a.w_packed, a.bias, a.ny, a.nx, a.stride, a.anchors_px, a.z, a.nrows_total, a.row_off, a.obj_hint, st);
}
static int run(const StemArgs& a, void* st) { return y5_conv_stem_fwd(a.x_nchw, a.B, a.H, a.W, a.w_stem, a.bias, a.C2, a.Npad, a.y, a.ldy, 0, st); }
static int run(const NopArgs&, void*) { return Y5_OK; }
static int run(const BneckArgs& a, void* st) {
  return y5_bottleneck_fwd(a.x, a.ldx, a.w1_packed, a.bias1, a.Kpad1, a.w2_packed, a.bias2, a.Kpad2, a.y, a.ldy, a.B, a.H, a.W, a.C, a.add, 0, st);
}
static int run(const K3pwArgs& a, void* st) {
  return y5_conv_k3pw_fwd(&a.d, a.x, a.w1_packed, a.bias1, a.w2_packed, a.bias2, a.C3, a.Npad2, a.Kpad2, a.act2, a.y, a.ldy, a.y2, a.ld2, a.split_n, st);
}
static int run(const BneckCv3Args& a, void* st) {
  return y5_bottleneck_cv3_fwd(a.x, a.ldx, a.w1_packed, a.bias1, a.Kpad1, a.w2_packed, a.bias2, a.Kpad2, a.y2, a.ld2, a.w3_packed, a.bias3, a.Kpad3, a.C3,
                               a.act3, a.out, a.ldo, a.B, a.H, a.W, a.C, a.add, 0, st);
}
static int run(const FrontArgs& a, void* st) {
  return y5_conv_front_fwd(a.x_nchw, a.B, a.H, a.W, a.w_stem, a.bias0, a.C0, a.w1_packed, a.bias1, a.C1, a.Npad1, a.Kpad1, a.act1, a.w2_packed, a.bias2, a.C3,
                           a.Npad2, a.Kpad2, a.act2, a.y, a.ldy, a.y2, a.ld2, a.split_n, 0, st);
}
static int run(const SppfFrontArgs& a, void* st) {
  return y5_sppf_cv1_pool_fwd(a.x, a.ldx, a.w_packed, a.bias, a.Kpad, a.buf, a.ld, a.B, a.H, a.W, a.C1, a.c_, a.k, a.act, st);
}

static int run(const ClassifyHeadArgs& a, void* st) {
  return y5_classify_head(a.x, a.dtype, a.B, a.HW, a.C, a.ld, a.w, a.bias, a.nc, a.logits, a.ldo, a.form, a.workspace, a.workspace_bytes, st);
}

using OpArgs = std::variant<NopArgs, ConvArgs, ToNhwcArgs, ToNchwArgs, SppfPoolArgs, UpsampleArgs, CopyArgs, DecodeArgs, HeadArgs, StemArgs, BneckArgs, K3pwArgs,
                            BneckCv3Args, FrontArgs, SppfFrontArgs, ClassifyHeadArgs>;

struct Op {
  int branch;  // 0: the caller's stream; 1: the plan's side stream (forked after the preceding main op, joined at the end of the range)
  OpArgs args;
};

static int run_op(const Op& o, void* st) {
  return std::visit([st](const auto& a) { return run(a, st); }, o.args);
}

struct GraphEntry { unsigned long long key; hipGraph_t graph; hipGraphExec_t exec; unsigned long long used; };

struct y5_plan {
  std::vector<Op> ops;
  hipGraph_t graph = nullptr;        // the SELECTED graph (one entry of `cache`, or the only graph of a plan that never rebinds)
  hipGraphExec_t exec = nullptr;
  std::vector<GraphEntry> cache;     // captured graphs by binding key (y5_plan_select_graph): outputs re-pointed per call keep their graphs
  unsigned long long cur_key = 0, tick = 0;
  hipStream_t side = nullptr;        // side-branch stream (y5_plan_set_branch), created on first use
  std::vector<hipEvent_t> events;    // fork / join markers, one per fork point of a run + one join
  bool flat = false;                 // run every op on the caller's stream (per-op timing: no fork / join latency in the figure)
};

static int plan_push(y5_plan* pl, OpArgs args) {
  pl->ops.push_back(Op{0, std::move(args)});
  return Y5_OK;
}
static Op* plan_op(y5_plan* pl, int op) { return pl && op >= 0 && op < (int)pl->ops.size() ? &pl->ops[op] : nullptr; }
// the Detect decode / fused head part of op `op`, or null
static DetectTail* plan_detect_tail(y5_plan* pl, int op) {
  Op* o = plan_op(pl, op);
  if (!o) return nullptr;
  if (auto* a = std::get_if<DecodeArgs>(&o->args)) return a;
  if (auto* a = std::get_if<HeadArgs>(&o->args)) return a;
  return nullptr;
}

extern "C" y5_plan* y5_plan_create(void) { return new y5_plan(); }
extern "C" void y5_plan_destroy(y5_plan* p) {
  if (!p) return;
  for (GraphEntry& g : p->cache) {  // (p->graph / p->exec alias one entry)
    if (g.exec) hipGraphExecDestroy(g.exec);
    if (g.graph) hipGraphDestroy(g.graph);
  }
  for (hipEvent_t e : p->events) hipEventDestroy(e);
  if (p->side) hipStreamDestroy(p->side);
  delete p;
}
extern "C" int y5_plan_size(const y5_plan* p) { return p ? (int)p->ops.size() : 0; }

extern "C" int y5_plan_add_conv(y5_plan* pl, const y5_conv_desc* d, const void* x, const void* w, const float* bias,
                                const void* res, void* y, void* y2) {
  if (!pl || !d) return y5_fail(Y5_ERR_BAD_ARG, "plan_add_conv: null");
  ConvArgs a{};
  a.d = *d; a.x = x; a.w_packed = w; a.bias = bias; a.residual = res; a.y = y; a.y_up2 = y2;
  return plan_push(pl, a);
}
extern "C" int y5_plan_add_nchw_to_nhwc(y5_plan* pl, const void* src, int sdt, void* dst, int ddt, int B, int C, int H, int W,
                                        int ld, float scale) {
  if (!pl) return y5_fail(Y5_ERR_BAD_ARG, "plan: null");
  ToNhwcArgs a{};
  a.src = src; a.src_dtype = sdt; a.dst = dst; a.dst_dtype = ddt; a.B = B; a.C = C; a.H = H; a.W = W; a.ld = ld; a.scale = scale;
  return plan_push(pl, a);
}
extern "C" int y5_plan_add_nhwc_to_nchw(y5_plan* pl, const void* src, int dt, void* dst, int B, int C, int H, int W, int ld) {
  if (!pl) return y5_fail(Y5_ERR_BAD_ARG, "plan: null");
  ToNchwArgs a{};
  a.src = src; a.dtype = dt; a.dst = dst; a.B = B; a.C = C; a.H = H; a.W = W; a.ld = ld;
  return plan_push(pl, a);
}
extern "C" int y5_plan_add_sppf_cv1_pool(y5_plan* pl, const void* x, int ldx, const void* w, const float* bias, int Kpad, void* buf, int ld, int B, int H, int W,
                                         int C1, int c_, int k, int act) {
  if (!pl) return y5_fail(Y5_ERR_BAD_ARG, "plan: null");
  SppfFrontArgs a{};
  a.x = x; a.ldx = ldx; a.w_packed = w; a.bias = bias; a.Kpad = Kpad; a.buf = buf; a.ld = ld; a.B = B; a.H = H; a.W = W; a.C1 = C1; a.c_ = c_; a.k = k; a.act = act;
  return plan_push(pl, a);
}
extern "C" int y5_plan_add_sppf_pool(y5_plan* pl, void* buf, int dt, int B, int H, int W, int C, int ld, int k) {
  if (!pl) return y5_fail(Y5_ERR_BAD_ARG, "plan: null");
  SppfPoolArgs a{};
  a.buf = buf; a.dtype = dt; a.B = B; a.H = H; a.W = W; a.C = C; a.ld = ld; a.k = k;
  return plan_push(pl, a);
}
extern "C" int y5_plan_add_upsample2x(y5_plan* pl, const void* src, int dt, void* dst, int B, int H, int W, int C, int lds, int ldd) {
  if (!pl) return y5_fail(Y5_ERR_BAD_ARG, "plan: null");
  UpsampleArgs a{};
  a.src = src; a.dtype = dt; a.dst = dst; a.B = B; a.H = H; a.W = W; a.C = C; a.lds = lds; a.ldd = ldd;
  return plan_push(pl, a);
}
extern "C" int y5_plan_add_copy_slice(y5_plan* pl, const void* src, int dt, void* dst, int npix, int C, int lds, int ldd) {
  if (!pl) return y5_fail(Y5_ERR_BAD_ARG, "plan: null");
  CopyArgs a{};
  a.src = src; a.dtype = dt; a.dst = dst; a.npix = npix; a.C = C; a.lds = lds; a.ldd = ldd;
  return plan_push(pl, a);
}
extern "C" int y5_plan_add_detect_decode(y5_plan* pl, const void* logits, int dt, int B, int ny, int nx, int na, int no, int nm, int ld,
                                         float stride, const float* anchors_px, void* z, int zdt, long long nrows_total,
                                         long long row_off, void* raw) {
  if (!pl || !anchors_px || na > 8) return y5_fail(Y5_ERR_BAD_ARG, "plan: null / na");
  DecodeArgs a{};
  a.logits = logits; a.dtype = dt; a.B = B; a.ny = ny; a.nx = nx; a.na = na; a.no = no; a.nm = nm; a.ld = ld; a.stride = stride; a.z = z; a.z_dtype = zdt;
  a.nrows_total = nrows_total; a.row_off = row_off; a.raw = raw;
  for (int k = 0; k < na * 2; ++k) a.anchors_px[k] = anchors_px[k];
  return plan_push(pl, a);
}

// fused Detect head (head.hip): the convolution `d` + the decode of one level; y5_plan_add_nop keeps the op numbering of the
// two-op form (convolution, decode) so that a plan built either way has the same indices
extern "C" int y5_plan_add_detect_head(y5_plan* pl, const y5_conv_desc* d, const void* x, const void* w, const float* bias, int ny, int nx,
                                       float stride, const float* anchors_px, void* z, long long nrows_total, long long row_off) {
  if (!pl || !d || !anchors_px) return y5_fail(Y5_ERR_BAD_ARG, "plan_add_detect_head: null");
  HeadArgs a{};
  a.d = *d; a.x = x; a.w_packed = w; a.bias = bias; a.ny = ny; a.nx = nx; a.stride = stride; a.z = z; a.nrows_total = nrows_total; a.row_off = row_off;
  for (int k = 0; k < 6; ++k) a.anchors_px[k] = anchors_px[k];
  return plan_push(pl, a);
}
extern "C" int y5_plan_add_bottleneck(y5_plan* pl, const void* x, int ldx, const void* w1, const float* b1, int Kpad1, const void* w2, const float* b2,
                                      int Kpad2, void* y, int ldy, int B, int H, int W, int C, int add) {
  if (!pl) return y5_fail(Y5_ERR_BAD_ARG, "plan: null");
  BneckArgs a{};
  a.x = x; a.ldx = ldx; a.w1_packed = w1; a.bias1 = b1; a.Kpad1 = Kpad1; a.w2_packed = w2; a.bias2 = b2; a.Kpad2 = Kpad2; a.y = y; a.ldy = ldy;
  a.B = B; a.H = H; a.W = W; a.C = C; a.add = add;
  return plan_push(pl, a);
}
extern "C" int y5_plan_add_conv_k3pw(y5_plan* pl, const y5_conv_desc* d, const void* x, const void* w1, const float* b1, const void* w2, const float* b2,
                                     int C3, int Npad2, int Kpad2, int act2, void* y, int ldy, void* y2, int ld2, int split_n) {
  if (!pl || !d) return y5_fail(Y5_ERR_BAD_ARG, "plan: null");
  K3pwArgs a{};
  a.d = *d; a.x = x; a.w1_packed = w1; a.bias1 = b1; a.w2_packed = w2; a.bias2 = b2; a.C3 = C3; a.Npad2 = Npad2; a.Kpad2 = Kpad2; a.act2 = act2;
  a.y = y; a.ldy = ldy; a.y2 = y2; a.ld2 = ld2; a.split_n = split_n;
  return plan_push(pl, a);
}
// Detect decode / fused head op `op`: also write every row's objectness to `hint` ((B, nrows_total), z's dtype) -- the NMS filter's shortcut
extern "C" int y5_plan_set_obj_hint(y5_plan* pl, int op, void* hint) {
  DetectTail* t = plan_detect_tail(pl, op);
  if (!t) return y5_fail(Y5_ERR_BAD_ARG, "plan_set_obj_hint: not a Detect decode / fused head op");
  t->obj_hint = hint;
  return Y5_OK;
}
extern "C" int y5_plan_add_bottleneck_cv3(y5_plan* pl, const void* x, int ldx, const void* w1, const float* b1, int Kpad1, const void* w2, const float* b2,
                                          int Kpad2, const void* y2, int ld2, const void* w3, const float* b3, int Kpad3, int C3, int act3, void* out, int ldo,
                                          int B, int H, int W, int C, int add) {
  if (!pl) return y5_fail(Y5_ERR_BAD_ARG, "plan: null");
  BneckCv3Args a{};
  a.x = x; a.ldx = ldx; a.w1_packed = w1; a.bias1 = b1; a.Kpad1 = Kpad1; a.w2_packed = w2; a.bias2 = b2; a.Kpad2 = Kpad2; a.y2 = y2; a.ld2 = ld2;
  a.w3_packed = w3; a.bias3 = b3; a.Kpad3 = Kpad3; a.C3 = C3; a.act3 = act3; a.out = out; a.ldo = ldo; a.B = B; a.H = H; a.W = W; a.C = C; a.add = add;
  return plan_push(pl, a);
}
extern "C" int y5_plan_add_conv_front(y5_plan* pl, const void* x_nchw, int B, int H, int W, const void* w_stem, const float* bias0, int C0, const void* w1,
                                      const float* bias1, int C1, int Npad1, int Kpad1, int act1, const void* w2, const float* bias2, int C3, int Npad2,
                                      int Kpad2, int act2, void* y, int ldy, void* y2, int ld2, int split_n) {
  if (!pl) return y5_fail(Y5_ERR_BAD_ARG, "plan: null");
  FrontArgs a{};
  a.x_nchw = x_nchw; a.B = B; a.H = H; a.W = W; a.w_stem = w_stem; a.bias0 = bias0; a.C0 = C0; a.w1_packed = w1; a.bias1 = bias1; a.C1 = C1; a.Npad1 = Npad1;
  a.Kpad1 = Kpad1; a.act1 = act1; a.w2_packed = w2; a.bias2 = bias2; a.C3 = C3; a.Npad2 = Npad2; a.Kpad2 = Kpad2; a.act2 = act2; a.y = y; a.ldy = ldy;
  a.y2 = y2; a.ld2 = ld2; a.split_n = split_n;
  return plan_push(pl, a);
}
// classification head (head.hip, classify.h): average pool + Linear behind the Classify convolution; `logits` is re-pointed per call like z
extern "C" int y5_plan_add_classify_head(y5_plan* pl, const void* x, int dtype, int B, int HW, int C, int ld, const void* w, const float* bias, int nc,
                                         void* logits, int ldo, int form, void* workspace, size_t workspace_bytes) {
  if (!pl) return y5_fail(Y5_ERR_BAD_ARG, "plan_add_classify_head: null");
  ClassifyHeadArgs a{};
  a.x = x; a.dtype = dtype; a.B = B; a.HW = HW; a.C = C; a.ld = ld; a.w = w; a.bias = bias; a.nc = nc; a.logits = logits; a.ldo = ldo; a.form = form;
  a.workspace = workspace; a.workspace_bytes = workspace_bytes;
  return plan_push(pl, a);
}
extern "C" int y5_plan_add_nop(y5_plan* pl) {
  if (!pl) return y5_fail(Y5_ERR_BAD_ARG, "plan: null");
  return plan_push(pl, NopArgs{});
}

extern "C" int y5_plan_add_conv_stem(y5_plan* pl, const void* x_nchw, int B, int H, int W, const void* w_stem, const float* bias,
                                     int C2, int Npad, void* y, int ldy) {
  if (!pl) return y5_fail(Y5_ERR_BAD_ARG, "plan: null");
  StemArgs a{};
  a.x_nchw = x_nchw; a.B = B; a.H = H; a.W = W; a.w_stem = w_stem; a.bias = bias; a.C2 = C2; a.Npad = Npad; a.y = y; a.ldy = ldy;
  return plan_push(pl, a);
}
extern "C" int y5_plan_set_input(y5_plan* pl, int op, const void* src) {
  Op* o = plan_op(pl, op);
  if (!o) return y5_fail(Y5_ERR_BAD_ARG, "plan_set_input: bad op index");
  if (auto* a = std::get_if<StemArgs>(&o->args)) a->x_nchw = src;
  else if (auto* a = std::get_if<ToNhwcArgs>(&o->args)) a->src = src;
  else if (auto* a = std::get_if<FrontArgs>(&o->args)) a->x_nchw = src;
  else return y5_fail(Y5_ERR_BAD_ARG, "plan_set_input: op does not read the model input");
  return Y5_OK;
}

// Re-point every output pointer of ops [first, last) that equals `old_ptr` at `new_ptr` (the Detect decode / fused head / to_nchw
// destinations: the model returns a FRESH z / proto tensor per call like the reference, models/yolo.py:115, without a copy).
extern "C" int y5_plan_rebind_output(y5_plan* pl, int first, int last, const void* old_ptr, void* new_ptr) {
  if (!pl || first < 0 || last > (int)pl->ops.size() || first > last || !old_ptr || !new_ptr) return y5_fail(Y5_ERR_BAD_ARG, "plan_rebind_output: bad args");
  int n = 0;
  auto repoint = [&](void*& p) {
    if (p == old_ptr) { p = new_ptr; ++n; }
  };
  for (int k = first; k < last; ++k) std::visit([&](auto& a) { a.outputs(repoint); }, pl->ops[k].args);
  if (!n) return y5_fail(Y5_ERR_BAD_ARG, "plan_rebind_output: no op writes that pointer");
  return Y5_OK;
}

// Graph cache: select the captured graph recorded under `key` (the caller's hash of the current output bindings).  Returns 1 when
// such a graph exists (y5_plan_launch_graph replays it), 0 when not (capture again: it is stored under `key`), < 0 on error.
// At most Y5_GRAPH_CACHE graphs are kept per plan; the least recently selected one is dropped.
#define Y5_GRAPH_CACHE 8
extern "C" int y5_plan_select_graph(y5_plan* pl, unsigned long long key) {
  if (!pl) return y5_fail(Y5_ERR_BAD_ARG, "plan_select_graph: null");
  pl->cur_key = key;
  for (GraphEntry& g : pl->cache)
    if (g.key == key) {
      g.used = ++pl->tick;
      pl->graph = g.graph; pl->exec = g.exec;
      return 1;
    }
  pl->graph = nullptr; pl->exec = nullptr;
  return 0;
}

// New anchor sizes (pixels) for a Detect decode / fused head op: Detect.anchors is a buffer the EMA interpolates like any other
// (utils/torch_utils.py:361-365), so a refreshed plan must pick it up together with the filters.
extern "C" int y5_plan_set_anchors(y5_plan* pl, int op, const float* anchors_px, int n) {
  if (!plan_op(pl, op) || !anchors_px || n < 1 || n > 16) return y5_fail(Y5_ERR_BAD_ARG, "plan_set_anchors: bad args");
  DetectTail* t = plan_detect_tail(pl, op);
  if (!t) return y5_fail(Y5_ERR_BAD_ARG, "plan_set_anchors: op has no anchors");
  for (int k = 0; k < n; ++k) t->anchors_px[k] = anchors_px[k];
  return Y5_OK;
}

extern "C" int y5_plan_set_branch(y5_plan* pl, int op, int branch) {
  Op* o = plan_op(pl, op);
  if (!o || branch < 0 || branch > 1) return y5_fail(Y5_ERR_BAD_ARG, "plan_set_branch: bad op index / branch");
  o->branch = branch;
  return Y5_OK;
}

extern "C" int y5_plan_set_conv_cfg(y5_plan* pl, int op, int cfg) {
  Op* o = plan_op(pl, op);
  ConvArgs* a = o ? std::get_if<ConvArgs>(&o->args) : nullptr;
  if (!a) return y5_fail(Y5_ERR_BAD_ARG, "plan_set_conv_cfg: not a convolution op");
  if (pl->graph || !pl->cache.empty()) return y5_fail(Y5_ERR_BAD_ARG, "plan_set_conv_cfg: the plan has captured graphs");
  a->d.cfg = cfg;
  return Y5_OK;
}

static hipEvent_t plan_event(y5_plan* pl, size_t idx) {
  while (pl->events.size() <= idx) {
    hipEvent_t e = nullptr;
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
    pl->events.push_back(e);
  }
  return pl->events[idx];
}

// Ops run in list order on `st`; a run of consecutive branch-1 ops is forked onto the plan's side stream behind the main op that
// precedes it (event record / wait) and main continues with the ops after the run; the side stream is joined back into `st` at
// the end of the range.  The host (engine.py) marks only ops whose inputs are complete at the fork point and whose outputs no
// later op of the range reads.  Under stream capture the same calls become the fork / join edges of the graph.
extern "C" int y5_plan_run_range(y5_plan* pl, int first, int last, void* st_) {
  if (!pl || first < 0 || last > (int)pl->ops.size() || first > last) return y5_fail(Y5_ERR_BAD_ARG, "plan_run_range: bad range");
  hipStream_t st = static_cast<hipStream_t>(st_);
  size_t nev = 0;
  bool used_side = false;
  for (int k = first; k < last; ++k) {
    const Op& o = pl->ops[k];
    if (o.branch == 1 && !pl->flat) {
      if (!pl->side && hipStreamCreateWithFlags(&pl->side, hipStreamNonBlocking) != hipSuccess) return y5_fail(Y5_ERR_RUNTIME, "plan: side stream create failed");
      if (k == first || pl->ops[k - 1].branch == 0) {
        hipEvent_t e = plan_event(pl, nev++);
        if (!e || hipEventRecord(e, st) != hipSuccess || hipStreamWaitEvent(pl->side, e, 0) != hipSuccess) return y5_fail(Y5_ERR_RUNTIME, "plan: fork failed");
      }
      used_side = true;
      const int rc = run_op(o, pl->side);
      if (rc) return rc;
    } else {
      const int rc = run_op(o, st_);
      if (rc) return rc;
    }
  }
  if (used_side) {
    hipEvent_t e = plan_event(pl, nev++);
    if (!e || hipEventRecord(e, pl->side) != hipSuccess || hipStreamWaitEvent(st, e, 0) != hipSuccess) return y5_fail(Y5_ERR_RUNTIME, "plan: join failed");
  }
  return Y5_OK;
}
extern "C" int y5_plan_run(y5_plan* pl, void* st) { return y5_plan_run_range(pl, 0, pl ? (int)pl->ops.size() : 0, st); }

extern "C" int y5_plan_capture_range(y5_plan* pl, int first, int last, void* st_) {
  if (!pl || first < 0 || last > (int)pl->ops.size() || first >= last) return y5_fail(Y5_ERR_BAD_ARG, "plan_capture: bad range");
  hipStream_t st = static_cast<hipStream_t>(st_);
  if (!y5_zero_page()) return y5_fail(Y5_ERR_RUNTIME, "plan_capture: zero page");
  // one eager run first: performs the per-kernel one-time attribute setup outside of capture
  int rc = y5_plan_run_range(pl, first, last, st_);
  if (rc) return rc;
  if (hipStreamSynchronize(st) != hipSuccess) return y5_fail(Y5_ERR_RUNTIME, "plan_capture: sync failed");
  for (size_t k = 0; k < pl->cache.size(); ++k)
    if (pl->cache[k].key == pl->cur_key) {  // re-capture under the same key: drop the stale entry
      if (pl->cache[k].exec) hipGraphExecDestroy(pl->cache[k].exec);
      if (pl->cache[k].graph) hipGraphDestroy(pl->cache[k].graph);
      pl->cache.erase(pl->cache.begin() + k);
      break;
    }
  pl->exec = nullptr; pl->graph = nullptr;  // aliases of cache entries
  // capture on a private stream (the caller's may be the legacy default stream, which cannot be captured); the graph itself
  // is stream-agnostic and is launched on whatever stream y5_plan_launch_graph receives
  hipStream_t cs = nullptr;
  if (hipStreamCreateWithFlags(&cs, hipStreamNonBlocking) != hipSuccess) return y5_fail(Y5_ERR_RUNTIME, "plan_capture: stream create failed");
  if (hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal) != hipSuccess) {
    hipStreamDestroy(cs);
    return y5_fail(Y5_ERR_RUNTIME, "plan_capture: begin capture failed");
  }
  rc = y5_plan_run_range(pl, first, last, cs);
  const hipError_t e = hipStreamEndCapture(cs, &pl->graph);
  hipStreamDestroy(cs);
  if (rc) return rc;
  if (e != hipSuccess || !pl->graph) {
    pl->graph = nullptr;
    return y5_fail(Y5_ERR_RUNTIME, "plan_capture: end capture failed");
  }
  if (hipGraphInstantiate(&pl->exec, pl->graph, nullptr, nullptr, 0) != hipSuccess) {
    hipGraphDestroy(pl->graph);
    pl->graph = nullptr; pl->exec = nullptr;
    return y5_fail(Y5_ERR_RUNTIME, "plan_capture: instantiate failed");
  }
  if (pl->cache.size() >= Y5_GRAPH_CACHE) {
    size_t lru = 0;
    for (size_t k = 1; k < pl->cache.size(); ++k)
      if (pl->cache[k].used < pl->cache[lru].used) lru = k;
    if (pl->cache[lru].exec) hipGraphExecDestroy(pl->cache[lru].exec);
    if (pl->cache[lru].graph) hipGraphDestroy(pl->cache[lru].graph);
    pl->cache.erase(pl->cache.begin() + lru);
  }
  pl->cache.push_back({pl->cur_key, pl->graph, pl->exec, ++pl->tick});
  return Y5_OK;
}
extern "C" int y5_plan_capture(y5_plan* pl, void* st_) { return y5_plan_capture_range(pl, 0, pl ? (int)pl->ops.size() : 0, st_); }

extern "C" int y5_plan_launch_graph(y5_plan* pl, void* st_) {
  if (!pl || !pl->exec) return y5_fail(Y5_ERR_BAD_ARG, "plan_launch_graph: plan not captured");
  if (hipGraphLaunch(pl->exec, static_cast<hipStream_t>(st_)) != hipSuccess) return y5_fail(Y5_ERR_RUNTIME, "plan_launch_graph: launch failed");
  return Y5_OK;
}

extern "C" int y5_plan_time_range(y5_plan* pl, int first, int last, int iters, void* st_, float* ms) {
  if (!pl || !ms || iters < 1) return y5_fail(Y5_ERR_BAD_ARG, "plan_time_range: bad args");
  hipStream_t st = static_cast<hipStream_t>(st_);
  hipEvent_t e0, e1;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return y5_fail(Y5_ERR_RUNTIME, "event create failed");
  pl->flat = true;  // kernels timed on `st` itself
  int rc = y5_plan_run_range(pl, first, last, st_);  // warm-up
  if (!rc) {
    hipEventRecord(e0, st);
    for (int it = 0; it < iters && !rc; ++it) rc = y5_plan_run_range(pl, first, last, st_);
    hipEventRecord(e1, st);
    if (hipEventSynchronize(e1) != hipSuccess) rc = y5_fail(Y5_ERR_RUNTIME, "event sync failed");
    else hipEventElapsedTime(ms, e0, e1);
  }
  pl->flat = false;
  hipEventDestroy(e0);
  hipEventDestroy(e1);
  return rc;
}

// In-situ per-op timing: ONE eager pass over ops [first, last) on `st` with a HIP event between consecutive ops, repeated `iters`
// times; ms_out[k - first] = median over the passes of op k's event-to-event time.  Unlike y5_plan_time_range (back-to-back
// launches of one op on warm buffers) every op here runs in its real position: inputs produced by the previous op, caches in the
// state the previous layer left them.  Side-branch ops run on `st` too (serialised), so the figures add up to a single-stream
// forward.  The cost of the event record itself (an empty event-to-event interval, measured in the same passes) is subtracted.
// Synchronises the stream.
extern "C" int y5_plan_profile_range(y5_plan* pl, int first, int last, int iters, void* st_, float* ms_out) {
  if (!pl || !ms_out || iters < 1 || first < 0 || last > (int)pl->ops.size() || first >= last) return y5_fail(Y5_ERR_BAD_ARG, "plan_profile_range: bad args");
  hipStream_t st = static_cast<hipStream_t>(st_);
  const int n = last - first;
  std::vector<hipEvent_t> ev(n + 2, nullptr);  // ev[n] -> ev[n + 1]: nothing in between = the cost of the event pair itself
  for (int k = 0; k <= n + 1; ++k)
    if (hipEventCreate(&ev[k]) != hipSuccess) return y5_fail(Y5_ERR_RUNTIME, "plan_profile_range: event create failed");
  std::vector<std::vector<float>> samples(n);
  std::vector<float> empty;
  int rc = Y5_OK;
  pl->flat = true;
  rc = y5_plan_run_range(pl, first, last, st_);  // warm-up pass
  for (int it = 0; it < iters && !rc; ++it) {
    hipEventRecord(ev[0], st);
    for (int k = 0; k < n && !rc; ++k) {
      rc = run_op(pl->ops[first + k], st_);
      hipEventRecord(ev[k + 1], st);
    }
    hipEventRecord(ev[n + 1], st);
    if (!rc && hipEventSynchronize(ev[n + 1]) != hipSuccess) rc = y5_fail(Y5_ERR_RUNTIME, "plan_profile_range: sync failed");
    for (int k = 0; k < n && !rc; ++k) {
      float ms = 0.f;
      hipEventElapsedTime(&ms, ev[k], ev[k + 1]);
      samples[k].push_back(ms);
    }
    if (!rc) {
      float ms = 0.f;
      hipEventElapsedTime(&ms, ev[n], ev[n + 1]);
      empty.push_back(ms);
    }
  }
  pl->flat = false;
  auto median = [](std::vector<float>& v) {
    for (size_t a = 1; a < v.size(); ++a)  // insertion sort (iters is small)
      for (size_t b = a; b > 0 && v[b] < v[b - 1]; --b) { const float t = v[b]; v[b] = v[b - 1]; v[b - 1] = t; }
    return v.empty() ? 0.f : v[v.size() / 2];
  };
  // an interval = [dispatch + run of the op] + [one event record]; the record's own cost (measured on the empty interval, ~5 us:
  // the completion signal + timestamp write-back of the marker packet) is taken off every op
  const float ev_cost = median(empty);
  for (int k = 0; k < n && !rc; ++k) {
    const float m = median(samples[k]) - ev_cost;
    ms_out[k] = m > 0.f ? m : 0.f;
  }
  for (hipEvent_t e : ev) hipEventDestroy(e);
  return rc;
}
