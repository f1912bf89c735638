// Fused optimizer step over all parameter tensors of the model (train.py:413-421):
//     scaler.unscale_(optimizer)                               g *= inv_scale, found_inf = any non-finite g
//     torch.nn.utils.clip_grad_norm_(model.parameters(), 10.0) g *= min(1, max_norm / (||g||_2 + 1e-6))
//     scaler.step(optimizer)                                   SGD(momentum, nesterov) over the 3 groups of
//                                                              utils/torch_utils.py:257-290 (skipped when found_inf)
//     ema.update(model)                                        e = d * e + (1 - d) * p   (utils/torch_utils.py:354-365)
// 177 tensors (yolov5s) would be ~1000 elementwise launches in stock torch; here: one deterministic sum-of-squares pass, one
// 1-block finish and one update pass, all driven by a device-resident tensor table.  Grid = (chunks of CH elements, tensors);
// workgroups past a tensor's end exit at once.  Built with -ffp-contract=off: every product / sum is rounded as torch's
// separate mul / add kernels round them.
#include <hip/hip_runtime.h>

#include "../../include/yolov5_hip.h"
#include "y5_common.h"
#include "y5_host.h"

namespace {
constexpr int CH = 16384;  // elements per workgroup: 256 threads x 16 float4
constexpr int CHV = 16384; // elements per workgroup of the Adam / RMSProp update: 256 threads x 16 x 16 bytes per stream (2048 ... 16384 measured: the same)

struct MtStats { float total_norm, clip_coef, found_inf, pad; };
}  // namespace

__global__ __launch_bounds__(256)
void y5_mt_sumsq_kernel(const y5_mt_tensor* __restrict__ tab, double* __restrict__ partial, int* __restrict__ nonfinite, int max_chunks) {
  const y5_mt_tensor t = tab[blockIdx.y];
  const long long base = (long long)blockIdx.x * CH;
  double* out = partial + (size_t)blockIdx.y * max_chunks + blockIdx.x;
  if (base >= t.n) {
    if (threadIdx.x == 0) *out = 0.0;
    return;
  }
  const float* g = static_cast<const float*>(t.grad);
  const long long end = base + CH < t.n ? base + CH : t.n;
  float acc = 0.f;
  bool bad = false;
  for (long long i = base + threadIdx.x; i < end; i += 256) {
    const float v = g[i];
    bad |= !(fabsf(v) <= 3.402823466e38f);  // inf or nan
    acc += v * v;
  }
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* s_red = reinterpret_cast<float*>(smem);
  int& s_bad = *reinterpret_cast<int*>(smem + 256 * sizeof(float));
  if (threadIdx.x == 0) s_bad = 0;
  s_red[threadIdx.x] = acc;
  __syncthreads();
  if (bad) s_bad = 1;
  for (int d = 128; d > 0; d >>= 1) {
    if ((int)threadIdx.x < d) s_red[threadIdx.x] += s_red[threadIdx.x + d];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    *out = (double)s_red[0];
    if (s_bad) atomicExch(nonfinite, 1);
  }
}

__global__ __launch_bounds__(256)
void y5_mt_norm_finish_kernel(const double* __restrict__ partial, int n, const int* __restrict__ nonfinite, float inv_scale, float max_norm,
                              MtStats* __restrict__ stats) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* s_red = reinterpret_cast<double*>(smem);
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += partial[i];
  s_red[threadIdx.x] = s;
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) {
    if ((int)threadIdx.x < d) s_red[threadIdx.x] += s_red[threadIdx.x + d];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float total = (float)(sqrt(s_red[0]) * (double)inv_scale);  // norm of the UNSCALED gradients
    float coef = 1.0f;
    if (max_norm > 0.f) {
      coef = max_norm / (total + 1e-6f);
      if (!(coef < 1.0f)) coef = 1.0f;  // torch.clamp(max=1.0); a NaN norm leaves the step to found_inf
    }
    stats->total_norm = total;
    stats->clip_coef = coef;
    stats->found_inf = (*nonfinite != 0 || !(total <= 3.402823466e38f)) ? 1.0f : 0.0f;
  }
}

// groups: lr[g], weight_decay[g] for g = tensor.group (0..3)
struct MtHyper { float lr[4]; float wd[4]; float momentum, inv_scale, ema_d; int nesterov, use_stats; };

__global__ __launch_bounds__(256)
void y5_mt_sgd_kernel(const y5_mt_tensor* __restrict__ tab, const MtStats* __restrict__ stats, const MtHyper h) {
  const y5_mt_tensor t = tab[blockIdx.y];
  const long long base = (long long)blockIdx.x * CH;
  if (base >= t.n) return;
  float coef = 1.0f;
  bool skip = false;  // GradScaler.step: a non-finite gradient skips the parameter update (the EMA still moves, train.py:417-421)
  if (h.use_stats) {
    skip = stats->found_inf != 0.f;
    coef = stats->clip_coef;
  }
  const long long end = base + CH < t.n ? base + CH : t.n;
  float* p = static_cast<float*>(t.param);
  const float* g = static_cast<const float*>(t.grad);
  float* m = static_cast<float*>(t.mom);
  float* e = static_cast<float*>(t.ema);
  const float lr = h.lr[t.group & 3], wd = h.wd[t.group & 3];
  const float one_minus_d = 1.0f - h.ema_d;
  if (skip && !e) return;
  for (long long i = base + threadIdx.x; i < end; i += 256) {
    float w = p[i];
    if (!skip) {
      float d_p = g[i];
      if (h.inv_scale != 1.0f) d_p = d_p * h.inv_scale;
      if (coef != 1.0f) d_p = d_p * coef;
      if (wd != 0.f) d_p = d_p + wd * w;
      if (m) {
        const float b = m[i] * h.momentum + d_p;  // zero-initialised buffer: the first step gives b = d_p exactly (torch clones d_p)
        m[i] = b;
        d_p = h.nesterov ? d_p + h.momentum * b : b;
      }
      w = w - lr * d_p;
      p[i] = w;
    }
    if (e) e[i] = e[i] * h.ema_d + one_minus_d * w;
  }
}

// ---- Adam / AdamW / RMSProp (torch/optim/adam.py _single_tensor_adam, rmsprop.py _single_tensor_rmsprop; the other choices of
// utils/torch_utils.py:257-290).  Same table, grid and stats contract as the SGD kernel; the second state tensor (exp_avg_sq /
// square_avg) comes as a parallel device array of pointers, one per table row.  The step count lives on the device: GradScaler.step skips
// optimizer.step() on overflow, so the count -- and the bias corrections that depend on it -- may only advance when the update is taken.
struct MtStepRec { float step_size[4]; float bc2_sqrt; float pad[3]; };  // lr[g] / (1 - b1^t) and sqrt(1 - b2^t), each rounded once from double
struct MtStepArgs { double lr[4]; double b1, b2; int bias, use_stats; };

// one thread in front of the update: advance the count (unless the step is skipped) and derive what depends on it
__global__ void y5_mt_step_prep_kernel(float* __restrict__ step, MtStepRec* __restrict__ rec, const MtStats* __restrict__ stats, const MtStepArgs a) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (a.use_stats && stats->found_inf != 0.f) return;
  const float t = *step + 1.0f;
  *step = t;
  if (!a.bias) return;
  const double bc1 = 1.0 - pow(a.b1, (double)t), bc2 = 1.0 - pow(a.b2, (double)t);  // torch: Python floats, i.e. doubles, on the host
  for (int g = 0; g < 4; ++g) rec->step_size[g] = (float)(a.lr[g] / bc1);
  rec->bc2_sqrt = (float)sqrt(bc2);
}

struct MtAdamHyper {
  float wd[4];     // Adam: grad += wd * w
  float decay[4];  // AdamW: w *= 1 - lr * wd
  float b2, one_minus_b1, one_minus_b2, eps, inv_scale, ema_d;
  int adamw, use_stats;
};
struct MtRmsHyper {
  float lr[4], wd[4];
  float alpha, one_minus_alpha, eps, mu, inv_scale, ema_d;
  int use_stats;
};

// One element of either path (16-byte or scalar accesses): the SAME code, so both give the same bits.
struct MtAdamOp {
  float coef, inv_scale, wd, decay, b2, omb1, omb2, eps, neg_step, bc2s;
  int adamw;
  __device__ __forceinline__ void operator()(float& w, float d, float& m, float& v) const {
    if (inv_scale != 1.0f) d = d * inv_scale;
    if (coef != 1.0f) d = d * coef;
    if (adamw) w = w * decay;
    else if (wd != 0.f) d = d + wd * w;
    m = m + (d - m) * omb1;                  // exp_avg.lerp_(grad, 1 - beta1)
    v = v * b2 + omb2 * d * d;               // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    const float denom = sqrtf(v) / bc2s + eps;
    w = w + neg_step * (m / denom);          // param.addcdiv_(exp_avg, denom, value=-step_size)
  }
};
struct MtRmsOp {
  float coef, inv_scale, wd, lr, alpha, oma, eps, mu;
  bool has_buf;
  __device__ __forceinline__ void operator()(float& w, float d, float& buf, float& v) const {
    if (inv_scale != 1.0f) d = d * inv_scale;
    if (coef != 1.0f) d = d * coef;
    if (wd != 0.f) d = d + wd * w;
    v = v * alpha + oma * d * d;             // square_avg.mul_(alpha).addcmul_(grad, grad, value=1 - alpha)
    const float avg = sqrtf(v) + eps;
    if (has_buf) {
      buf = buf * mu + d / avg;              // buf.mul_(momentum).addcdiv_(grad, avg)
      w = w - lr * buf;
    } else {
      w = w + (-lr) * (d / avg);             // param.addcdiv_(grad, avg, value=-lr)
    }
  }
};

// One CH-element chunk of one row: 16-byte accesses when every pointer of the row is 16-byte aligned (chunk starts are multiples of CH,
// so the row's alignment is the chunk's), scalar accesses otherwise and for the last n % 4 elements.  skip: only the EMA moves.
template <class Op>
__device__ __forceinline__ void mt_update_chunk(const y5_mt_tensor& t, float* __restrict__ v, long long base, bool skip, float ema_d, const Op& op) {
  const long long end = base + CHV < t.n ? base + CHV : t.n;
  float* p = static_cast<float*>(t.param);
  const float* g = static_cast<const float*>(t.grad);
  float* m = static_cast<float*>(t.mom);
  float* e = static_cast<float*>(t.ema);
  const float omd = 1.0f - ema_d;
  const uintptr_t bits = (uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)e;  // a null pointer adds nothing
  long long done = base;
  if ((bits & 15) == 0) {
    const long long nvec = (end - base) >> 2;
    for (long long k = threadIdx.x; k < nvec; k += 256) {
      const long long j = base + 4 * k;
      float4_t w4 = *reinterpret_cast<const float4_t*>(p + j);
      float4_t e4 = {0.f, 0.f, 0.f, 0.f};
      if (e) e4 = *reinterpret_cast<const float4_t*>(e + j);
      if (!skip) {
        const float4_t g4 = *reinterpret_cast<const float4_t*>(g + j);
        float4_t m4 = {0.f, 0.f, 0.f, 0.f};
        if (m) m4 = *reinterpret_cast<const float4_t*>(m + j);
        float4_t v4 = *reinterpret_cast<const float4_t*>(v + j);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          float w = w4[c], mm = m4[c], vv = v4[c];
          op(w, g4[c], mm, vv);
          w4[c] = w; m4[c] = mm; v4[c] = vv;
        }
        *reinterpret_cast<float4_t*>(p + j) = w4;
        if (m) *reinterpret_cast<float4_t*>(m + j) = m4;
        *reinterpret_cast<float4_t*>(v + j) = v4;
      }
      if (e) {
#pragma unroll
        for (int c = 0; c < 4; ++c) e4[c] = e4[c] * ema_d + omd * w4[c];
        *reinterpret_cast<float4_t*>(e + j) = e4;
      }
    }
    done = base + 4 * nvec;
  }
  for (long long i = done + threadIdx.x; i < end; i += 256) {
    float w = p[i];
    if (!skip) {
      float mm = m ? m[i] : 0.f, vv = v[i];
      op(w, g[i], mm, vv);
      p[i] = w;
      if (m) m[i] = mm;
      v[i] = vv;
    }
    if (e) e[i] = e[i] * ema_d + omd * w;
  }
}

__global__ __launch_bounds__(256)
void y5_mt_adam_kernel(const y5_mt_tensor* __restrict__ tab, float* const* __restrict__ second, const MtStats* __restrict__ stats,
                       const MtStepRec* __restrict__ rec, const MtAdamHyper h) {
  const y5_mt_tensor t = tab[blockIdx.y];
  const long long base = (long long)blockIdx.x * CHV;
  if (base >= t.n) return;
  float coef = 1.0f;
  bool skip = false;
  if (h.use_stats) {
    skip = stats->found_inf != 0.f;
    coef = stats->clip_coef;
  }
  if (skip && !t.ema) return;
  const int gi = t.group & 3;
  const MtAdamOp op{coef, h.inv_scale, h.wd[gi], h.decay[gi], h.b2, h.one_minus_b1, h.one_minus_b2, h.eps, -rec->step_size[gi], rec->bc2_sqrt, h.adamw};
  mt_update_chunk(t, second[blockIdx.y], base, skip, h.ema_d, op);
}

__global__ __launch_bounds__(256)
void y5_mt_rmsprop_kernel(const y5_mt_tensor* __restrict__ tab, float* const* __restrict__ second, const MtStats* __restrict__ stats, const MtRmsHyper h) {
  const y5_mt_tensor t = tab[blockIdx.y];
  const long long base = (long long)blockIdx.x * CHV;
  if (base >= t.n) return;
  float coef = 1.0f;
  bool skip = false;
  if (h.use_stats) {
    skip = stats->found_inf != 0.f;
    coef = stats->clip_coef;
  }
  if (skip && !t.ema) return;
  const int gi = t.group & 3;
  const MtRmsOp op{coef, h.inv_scale, h.wd[gi], h.lr[gi], h.alpha, h.one_minus_alpha, h.eps, h.mu, t.mom != nullptr};
  mt_update_chunk(t, second[blockIdx.y], base, skip, h.ema_d, op);
}

// dst = dst * d + (1 - d) * src  over a table whose entries use (param = src, ema = dst): ModelEMA over float BUFFERS
__global__ __launch_bounds__(256)
void y5_mt_lerp_kernel(const y5_mt_tensor* __restrict__ tab, float d) {
  const y5_mt_tensor t = tab[blockIdx.y];
  const long long base = (long long)blockIdx.x * CH;
  if (base >= t.n) return;
  const long long end = base + CH < t.n ? base + CH : t.n;
  const float* src = static_cast<const float*>(t.param);
  float* dst = static_cast<float*>(t.ema);
  const float omd = 1.0f - d;
  for (long long i = base + threadIdx.x; i < end; i += 256) dst[i] = dst[i] * d + omd * src[i];
}

static int mt_grid(int ntensors, long long max_numel, dim3* grid, int ch = CH) {
  if (ntensors < 1 || ntensors > 65535 || max_numel < 1) return y5_fail(Y5_ERR_BAD_ARG, "multi-tensor op: bad tensor count / size");
  const long long chunks = (max_numel + ch - 1) / ch;
  if (chunks > 0x7fffffffLL) return y5_fail(Y5_ERR_UNSUPPORTED, "multi-tensor op: tensor too large");
  *grid = dim3((unsigned)chunks, (unsigned)ntensors);
  return Y5_OK;
}

extern "C" size_t y5_mt_workspace_bytes(int ntensors, long long max_numel) {
  const long long chunks = (max_numel + CH - 1) / CH;
  return (size_t)ntensors * (size_t)chunks * sizeof(double) + 64;
}

extern "C" int y5_mt_grad_norm(const y5_mt_tensor* table_dev, int ntensors, long long max_numel, float inv_scale, float max_norm,
                               float* stats_dev, void* workspace, size_t workspace_bytes, void* stream_) {
  if (!table_dev || !stats_dev || !workspace) return y5_fail(Y5_ERR_BAD_ARG, "mt_grad_norm: null pointer");
  dim3 grid;
  if (int rc = mt_grid(ntensors, max_numel, &grid)) return rc;
  if (workspace_bytes < y5_mt_workspace_bytes(ntensors, max_numel)) return y5_fail(Y5_ERR_BAD_ARG, "mt_grad_norm: workspace too small");
  hipStream_t st = static_cast<hipStream_t>(stream_);
  int* flag = static_cast<int*>(workspace);
  double* partial = reinterpret_cast<double*>(static_cast<char*>(workspace) + 64);
  if (hipMemsetAsync(flag, 0, 64, st) != hipSuccess) return y5_fail(Y5_ERR_RUNTIME, "mt_grad_norm: memset failed");
  hipLaunchKernelGGL(y5_mt_sumsq_kernel, grid, dim3(256), 256 * sizeof(float) + 16, st, table_dev, partial, flag, (int)grid.x);
  hipLaunchKernelGGL(y5_mt_norm_finish_kernel, dim3(1), dim3(256), 256 * sizeof(double), st, partial, (int)(grid.x * grid.y), flag, inv_scale, max_norm,
                     reinterpret_cast<MtStats*>(stats_dev));
  return y5_check_launch("y5_mt_grad_norm");
}

extern "C" int y5_mt_sgd_step(const y5_mt_tensor* table_dev, int ntensors, long long max_numel, const float* lr4, const float* wd4, float momentum,
                              int nesterov, float inv_scale, const float* stats_dev, float ema_decay, void* stream_) {
  if (!table_dev || !lr4 || !wd4) return y5_fail(Y5_ERR_BAD_ARG, "mt_sgd_step: null pointer");
  dim3 grid;
  if (int rc = mt_grid(ntensors, max_numel, &grid)) return rc;
  MtHyper h{};
  for (int i = 0; i < 4; ++i) { h.lr[i] = lr4[i]; h.wd[i] = wd4[i]; }
  h.momentum = momentum; h.inv_scale = inv_scale; h.ema_d = ema_decay; h.nesterov = nesterov;
  h.use_stats = stats_dev != nullptr;
  hipLaunchKernelGGL(y5_mt_sgd_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream_), table_dev,
                     reinterpret_cast<const MtStats*>(stats_dev), h);
  return y5_check_launch("y5_mt_sgd_step");
}

extern "C" int y5_mt_adam_step(const y5_mt_tensor* table_dev, void* const* second_dev, int ntensors, long long max_numel, const double* lr4,
                               const double* wd4, double beta1, double beta2, double eps, int adamw, float inv_scale, const float* stats_dev,
                               float ema_decay, float* step_dev, float* rec_dev, void* stream_) {
  if (!table_dev || !second_dev || !lr4 || !wd4 || !step_dev || !rec_dev) return y5_fail(Y5_ERR_BAD_ARG, "mt_adam_step: null pointer");
  if (!(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0)) return y5_fail(Y5_ERR_BAD_ARG, "mt_adam_step: bad betas / eps");
  dim3 grid;
  if (int rc = mt_grid(ntensors, max_numel, &grid, CHV)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream_);
  const MtStats* stats = reinterpret_cast<const MtStats*>(stats_dev);
  MtStepArgs a{};
  MtAdamHyper h{};
  for (int i = 0; i < 4; ++i) {
    a.lr[i] = lr4[i];
    h.wd[i] = (float)wd4[i];
    h.decay[i] = (float)(1.0 - lr4[i] * wd4[i]);
  }
  a.b1 = beta1; a.b2 = beta2; a.bias = 1; a.use_stats = stats != nullptr;
  h.b2 = (float)beta2; h.one_minus_b1 = (float)(1.0 - beta1); h.one_minus_b2 = (float)(1.0 - beta2); h.eps = (float)eps;
  h.inv_scale = inv_scale; h.ema_d = ema_decay; h.adamw = adamw != 0; h.use_stats = stats != nullptr;
  hipLaunchKernelGGL(y5_mt_step_prep_kernel, dim3(1), dim3(1), 0, st, step_dev, reinterpret_cast<MtStepRec*>(rec_dev), stats, a);
  hipLaunchKernelGGL(y5_mt_adam_kernel, grid, dim3(256), 0, st, table_dev, reinterpret_cast<float* const*>(second_dev), stats,
                     reinterpret_cast<const MtStepRec*>(rec_dev), h);
  return y5_check_launch("y5_mt_adam_step");
}

extern "C" int y5_mt_rmsprop_step(const y5_mt_tensor* table_dev, void* const* second_dev, int ntensors, long long max_numel, const double* lr4,
                                  const double* wd4, double alpha, double eps, double momentum, float inv_scale, const float* stats_dev,
                                  float ema_decay, float* step_dev, void* stream_) {
  if (!table_dev || !second_dev || !lr4 || !wd4 || !step_dev) return y5_fail(Y5_ERR_BAD_ARG, "mt_rmsprop_step: null pointer");
  if (!(alpha >= 0.0 && eps >= 0.0 && momentum >= 0.0)) return y5_fail(Y5_ERR_BAD_ARG, "mt_rmsprop_step: bad alpha / eps / momentum");
  dim3 grid;
  if (int rc = mt_grid(ntensors, max_numel, &grid, CHV)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream_);
  const MtStats* stats = reinterpret_cast<const MtStats*>(stats_dev);
  MtStepArgs a{};
  MtRmsHyper h{};
  for (int i = 0; i < 4; ++i) { h.lr[i] = (float)lr4[i]; h.wd[i] = (float)wd4[i]; }
  a.bias = 0; a.use_stats = stats != nullptr;
  h.alpha = (float)alpha; h.one_minus_alpha = (float)(1.0 - alpha); h.eps = (float)eps; h.mu = (float)momentum;
  h.inv_scale = inv_scale; h.ema_d = ema_decay; h.use_stats = stats != nullptr;
  hipLaunchKernelGGL(y5_mt_step_prep_kernel, dim3(1), dim3(1), 0, st, step_dev, static_cast<MtStepRec*>(nullptr), stats, a);
  hipLaunchKernelGGL(y5_mt_rmsprop_kernel, grid, dim3(256), 0, st, table_dev, reinterpret_cast<float* const*>(second_dev), stats, h);
  return y5_check_launch("y5_mt_rmsprop_step");
}

extern "C" int y5_mt_lerp(const y5_mt_tensor* table_dev, int ntensors, long long max_numel, float decay, void* stream_) {
  if (!table_dev) return y5_fail(Y5_ERR_BAD_ARG, "mt_lerp: null pointer");
  dim3 grid;
  if (int rc = mt_grid(ntensors, max_numel, &grid)) return rc;
  hipLaunchKernelGGL(y5_mt_lerp_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream_), table_dev, decay);
  return y5_check_launch("y5_mt_lerp");
}
