// AutoAnchor on the device (utils/autoanchor.py): the anchor-fit metric of check_anchors (:36-43), the mutate-and-keep-if-fitter chain
// of kmean_anchors (:148-160) and the Lloyd iterations of its k-means start (:139, scipy.cluster.vq.kmeans).  Included from metrics.hip,
// which is built with -ffp-contract=off.
//
// Ratio metric, per label (w, h) and anchor (kw, kh), operation by operation in fp32 as torch evaluates :91-93:
//     r = wh / k;  x = min(min(rw, 1 / rw), min(rh, 1 / rh));  best = max over anchors of x
// Both divisions are the compiler's correctly rounded IEEE fp32 divide (no reciprocal shortcut, no k / wh rewrite): `best` must carry the
// same bits as torch's, because the chain below compares sums of it.
//
// Reductions are deterministic: every workgroup reduces its grid-stride share in a fixed LDS tree and writes ONE partial into a fixed slot
// of the workspace; a single-workgroup second launch adds the slots in index order.  No floating-point atomics anywhere.
//
// The evolution is a plain chain of 2 * gen tiny launches on one stream with no host synchronisation: generation g reads the anchors its
// predecessor's accept kernel left in `k`.  All mutation factors are drawn up front on the host (they depend on the RNG streams only,
// never on which candidates were accepted).  No batching of several generations per pass and no graph capture: one generation is a few
// microseconds of cache-resident reads.
#pragma once

namespace y5aa {
constexpr int T = 256;        // threads per workgroup
constexpr int MAX_NA = 40;    // anchors in total: the loss's own limit (y5_loss_desc.anchors holds 80 floats)
constexpr int MAX_BLOCKS = 256;

__device__ __forceinline__ float ratio_metric(float w, float h, float kw, float kh) {
  const float rw = w / kw, rh = h / kh;
  const float iw = 1.0f / rw, ih = 1.0f / rh;
  const float mw = iw < rw ? iw : rw, mh = ih < rh ? ih : rh;   // torch.min(r, 1 / r)
  return mh < mw ? mh : mw;                                     // .min(2)
}

// fixed-shape tree over T values in LDS; every thread of the workgroup must call it; the result is in s[0]
template <typename V>
__device__ __forceinline__ void block_tree(V* s, int tid) {
  __syncthreads();
  for (int m = T / 2; m > 0; m >>= 1) {
    if (tid < m) s[tid] += s[tid + m];
    __syncthreads();
  }
}
}  // namespace y5aa

// ---- check_anchors.metric (:36-43): exact integer counts ------------------------------------------------------------------------------
__global__ __launch_bounds__(256)
void y5_anchor_metric_kernel(const float* __restrict__ wh, long long n, const float* __restrict__ k, int na, float thr, unsigned long long* counts) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* s_k = reinterpret_cast<float*>(smem);                                            // [2 * MAX_NA]
  unsigned long long* s_c = reinterpret_cast<unsigned long long*>(s_k + 2 * y5aa::MAX_NA);  // [T]
  const int tid = threadIdx.x;
  if (tid < 2 * na) s_k[tid] = k[tid];
  __syncthreads();
  unsigned long long nbest = 0, npair = 0;
  for (long long i = (long long)blockIdx.x * y5aa::T + tid; i < n; i += (long long)gridDim.x * y5aa::T) {
    const float w = wh[2 * i], h = wh[2 * i + 1];
    float best = 0.f;
    for (int a = 0; a < na; ++a) {
      const float x = y5aa::ratio_metric(w, h, s_k[2 * a], s_k[2 * a + 1]);
      npair += x > thr ? 1u : 0u;
      best = (a == 0 || x > best) ? x : best;
    }
    nbest += best > thr ? 1u : 0u;
  }
  s_c[tid] = nbest;
  y5aa::block_tree(s_c, tid);
  const unsigned long long tb = s_c[0];
  __syncthreads();
  s_c[tid] = npair;
  y5aa::block_tree(s_c, tid);
  if (tid == 0) {   // integer sums: the order of the atomics cannot change them
    atomicAdd(counts, tb);
    atomicAdd(counts + 1, s_c[0]);
  }
}

// ---- kmean_anchors evolution (:148-160) -------------------------------------------------------------------------------------------------
// candidate of one generation: kg = max(k * v, 2.0) in fp64 (`(k.copy() * v).clip(min=2.0)`), or k itself for the initial fitness (v == nullptr)
__device__ __forceinline__ double y5_anchor_candidate(const double* k, const double* v, int i) {
  if (!v) return k[i];
  const double c = k[i] * v[i];
  return c < 2.0 ? 2.0 : c;
}

// partial[b] = this workgroup's share of sum(best * (best > thr)) in fp64, anchors rounded to fp32 as torch.tensor(kg, dtype=float32) does
__global__ __launch_bounds__(256)
void y5_anchor_fitness_kernel(const float* __restrict__ wh, long long n, const double* __restrict__ k, const double* __restrict__ v, int na, float thr,
                              double* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* s_sum = reinterpret_cast<double*>(smem);                    // [T]
  float* s_k = reinterpret_cast<float*>(s_sum + y5aa::T);             // [2 * MAX_NA]
  const int tid = threadIdx.x;
  if (tid < 2 * na) s_k[tid] = (float)y5_anchor_candidate(k, v, tid);
  __syncthreads();
  double acc = 0.0;
  for (long long i = (long long)blockIdx.x * y5aa::T + tid; i < n; i += (long long)gridDim.x * y5aa::T) {
    const float w = wh[2 * i], h = wh[2 * i + 1];
    float best = 0.f;
    for (int a = 0; a < na; ++a) {
      const float x = y5aa::ratio_metric(w, h, s_k[2 * a], s_k[2 * a + 1]);
      best = (a == 0 || x > best) ? x : best;
    }
    acc += (double)(best > thr ? best : 0.0f);
  }
  s_sum[tid] = acc;
  y5aa::block_tree(s_sum, tid);
  if (tid == 0) partial[blockIdx.x] = s_sum[0];
}

// one workgroup: fg = (partials added in index order) / n; `if fg > f: f, k = fg, kg`; accepted[g] = the decision.  accepted == nullptr: the
// initial fitness (f = fg unconditionally, k untouched)
__global__ __launch_bounds__(256)
void y5_anchor_accept_kernel(const double* __restrict__ partial, int nblk, long long n, double* k, const double* __restrict__ v, int na, double* f,
                             unsigned char* accepted) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* s_sum = reinterpret_cast<double*>(smem);   // [T]
  const int tid = threadIdx.x;
  s_sum[tid] = tid < nblk ? partial[tid] : 0.0;      // nblk <= MAX_BLOCKS == T
  y5aa::block_tree(s_sum, tid);
  const double fg = s_sum[0] / (double)n;
  if (!accepted) {
    if (tid == 0) *f = fg;
    return;
  }
  const bool take = fg > *f;
  const double kg = tid < 2 * na ? y5_anchor_candidate(k, v, tid) : 0.0;
  __syncthreads();   // every thread has read *f and k before either changes
  if (take && tid < 2 * na) k[tid] = kg;
  if (tid == 0) {
    if (take) *f = fg;
    *accepted = take ? 1 : 0;
  }
}

// ---- k-means (scipy.cluster.vq.kmeans as kmean_anchors calls it, :139): R restarts advance together -----------------------------------------
// Thread (chain r, sub-lane s) = tid = s * R + r walks the observations s, s + S, ... of its workgroup's grid-stride share and keeps the
// sums of ITS chain in LDS columns of its own (acc[a][tid], a = 3 c + {0: sum x, 1: sum y, 2: members} and a = 3 k: sum of distances), so one
// pass over `obs` serves every restart and nothing is shared between threads until the fixed-order fold over s at the end.
// Assignment: the centroid with the smallest squared fp64 distance, the lowest index winning ties (what scipy's vq does; the square root
// is monotone, so this is an argmin of the Euclidean distance); the distance that enters the mean is the square root of that minimum.
struct Y5KmeansState {
  double* book;          // (R, k, 2)
  unsigned char* alive;  // (R, k)
  double* last;          // (R) mean distance of the latest assignment
  int* iters;            // (R)
  int* frozen;           // (R) workspace
  int* done;             // workspace: 1 when every chain has converged
};

__global__ __launch_bounds__(256)
void y5_kmeans_assign_kernel(const float* __restrict__ obs, long long n, int R, int k, int S, Y5KmeansState st, double* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int NA = 3 * k + 1;
  const int AT = R * S;                                         // active threads
  double* s_acc = reinterpret_cast<double*>(smem);              // [NA][AT]
  double* s_book = s_acc + (size_t)NA * AT;                     // [R * k * 2]
  unsigned char* s_alive = reinterpret_cast<unsigned char*>(s_book + (size_t)R * k * 2);  // [R * k]
  const int tid = threadIdx.x;
  for (int i = tid; i < R * k * 2; i += y5aa::T) s_book[i] = st.book[i];
  for (int i = tid; i < R * k; i += y5aa::T) s_alive[i] = st.alive[i];
  if (tid < AT)
    for (int a = 0; a < NA; ++a) s_acc[a * AT + tid] = 0.0;
  __syncthreads();
  const int r = tid % R, s = tid / R;
  if (s < S && !st.frozen[r]) {
    const double* bk = s_book + (size_t)r * k * 2;
    const unsigned char* al = s_alive + (size_t)r * k;
    for (long long i = (long long)blockIdx.x * S + s; i < n; i += (long long)gridDim.x * S) {
      const double x = (double)obs[2 * i], y = (double)obs[2 * i + 1];
      double dmin = 0.0;
      int cmin = -1;
      for (int c = 0; c < k; ++c) {
        if (!al[c]) continue;
        const double dx = x - bk[2 * c], dy = y - bk[2 * c + 1];
        const double d2 = dx * dx + dy * dy;
        if (cmin < 0 || d2 < dmin) { dmin = d2; cmin = c; }
      }
      if (cmin >= 0) {   // (a chain always keeps at least one centroid: every observation has a nearest one)
        s_acc[(3 * cmin + 0) * AT + tid] += x;
        s_acc[(3 * cmin + 1) * AT + tid] += y;
        s_acc[(3 * cmin + 2) * AT + tid] += 1.0;
        s_acc[(3 * k) * AT + tid] += sqrt(dmin);
      }
    }
  }
  __syncthreads();
  for (int o = tid; o < R * NA; o += y5aa::T) {   // fold the sub-lanes in index order: partial[block][r][a]
    const int rr = o / NA, a = o - rr * NA;
    double t = 0.0;
    for (int ss = 0; ss < S; ++ss) t += s_acc[a * AT + ss * R + rr];
    partial[(size_t)blockIdx.x * R * NA + o] = t;
  }
}

// one workgroup: add the workgroups' partials in index order, then per chain what scipy's _kmeans loop does after vq(): record the mean
// distance, move every centroid to the mean of its members, drop the ones without members, and stop when the mean distance moved by <= 1e-5
// (the book has then been updated once more after the last distance was taken, exactly as in scipy's loop)
__global__ __launch_bounds__(256)
void y5_kmeans_update_kernel(const double* __restrict__ partial, int nblk, long long n, int R, int k, Y5KmeansState st) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int NA = 3 * k + 1;
  double* s_tot = reinterpret_cast<double*>(smem);   // [R * NA]
  const int tid = threadIdx.x;
  for (int o = tid; o < R * NA; o += y5aa::T) {
    double t = 0.0;
    for (int b = 0; b < nblk; ++b) t += partial[(size_t)b * R * NA + o];
    s_tot[o] = t;
  }
  __syncthreads();
  for (int r = tid; r < R; r += y5aa::T) {
    if (st.frozen[r]) continue;
    const double* tot = s_tot + (size_t)r * NA;
    for (int c = 0; c < k; ++c) {
      if (!st.alive[r * k + c]) continue;
      const double m = tot[3 * c + 2];
      if (m == 0.0) { st.alive[r * k + c] = 0; continue; }
      st.book[((size_t)r * k + c) * 2 + 0] = tot[3 * c + 0] / m;
      st.book[((size_t)r * k + c) * 2 + 1] = tot[3 * c + 1] / m;
    }
    const double dist = tot[3 * k] / (double)n;
    const bool first = st.iters[r] == 0;   // scipy starts from diff = inf
    const double diff = fabs(st.last[r] - dist);
    st.last[r] = dist;
    st.iters[r] += 1;
    if (!first && diff <= 1e-5) st.frozen[r] = 1;
  }
  __syncthreads();
  if (tid == 0) {
    int all = 1;
    for (int r = 0; r < R; ++r) all &= st.frozen[r] != 0;
    *st.done = all;
  }
}

__global__ __launch_bounds__(256)
void y5_kmeans_init_kernel(const float* __restrict__ guess, int R, int k, Y5KmeansState st) {
  const int i = blockIdx.x * y5aa::T + threadIdx.x;
  if (i < R * k * 2) st.book[i] = (double)guess[i];
  if (i < R * k) st.alive[i] = 1;
  if (i < R) { st.last[i] = 0.0; st.iters[i] = 0; st.frozen[i] = 0; }
  if (i == 0) *st.done = 0;
}

// ---- C-ABI ---------------------------------------------------------------------------------------------------------------------------------
namespace y5aa {
inline int blocks_for(long long n, int per_block) {
  const long long b = (n + per_block - 1) / per_block;
  return (int)(b < 1 ? 1 : (b > MAX_BLOCKS ? MAX_BLOCKS : b));
}
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
// sub-lanes per chain of the assign kernel: as many as 256 threads and 64 KiB of LDS allow (0: the problem does not fit)
inline int kmeans_sublanes(int R, int k, size_t* lds) {
  const size_t book = (size_t)R * k * 2 * 8 + (size_t)R * k, per_lane = (size_t)(3 * k + 1) * 8 * R, cap = 64 * 1024;
  if (R < 1 || R > T || k < 1 || book + per_lane > cap) return 0;
  size_t S = (cap - book) / per_lane;
  if (S > (size_t)(T / R)) S = T / R;
  if (lds) *lds = S * per_lane + book;
  return (int)S;
}
}  // namespace y5aa

extern "C" int y5_anchor_metric(const float* wh, long long n, const float* k, int na, float thr_inv, long long* counts, void* stream_) {
  if (!wh || !k || !counts) return y5_fail(Y5_ERR_BAD_ARG, "anchor_metric: null pointer");
  if (n < 1 || na < 1 || na > y5aa::MAX_NA) return y5_fail(Y5_ERR_BAD_ARG, "anchor_metric: need n >= 1 and 1 <= na <= 40");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (hipMemsetAsync(counts, 0, 2 * sizeof(long long), stream) != hipSuccess) return y5_fail(Y5_ERR_RUNTIME, "anchor_metric: memset failed");
  const size_t lds = 2 * y5aa::MAX_NA * sizeof(float) + y5aa::T * sizeof(unsigned long long);
  hipLaunchKernelGGL(y5_anchor_metric_kernel, dim3(y5aa::blocks_for(n, y5aa::T)), dim3(y5aa::T), lds, stream, wh, n, k, na, thr_inv,
                     reinterpret_cast<unsigned long long*>(counts));
  return y5_check_launch("y5_anchor_metric");
}

extern "C" size_t y5_anchor_evolve_ws_bytes(long long n) {
  if (n < 1) return 0;
  return (size_t)y5aa::MAX_BLOCKS * sizeof(double);
}

extern "C" int y5_anchor_evolve(const float* wh, long long n, int na, double* k, double* f, int init_f, const double* v, int gen, float thr_inv,
                                unsigned char* accepted, void* workspace, size_t workspace_bytes, void* stream_) {
  if (!wh || !k || !f || !workspace || (gen > 0 && (!v || !accepted))) return y5_fail(Y5_ERR_BAD_ARG, "anchor_evolve: null pointer");
  if (n < 1 || na < 1 || na > y5aa::MAX_NA || gen < 0) return y5_fail(Y5_ERR_BAD_ARG, "anchor_evolve: need n >= 1, 1 <= na <= 40, gen >= 0");
  if (workspace_bytes < y5_anchor_evolve_ws_bytes(n)) return y5_fail(Y5_ERR_WORKSPACE, "anchor_evolve: workspace too small");
  if (reinterpret_cast<uintptr_t>(workspace) & 7) return y5_fail(Y5_ERR_BAD_ARG, "anchor_evolve: workspace must be 8-byte aligned");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  double* partial = static_cast<double*>(workspace);
  const int nblk = y5aa::blocks_for(n, y5aa::T);
  const size_t lds_fit = y5aa::T * sizeof(double) + 2 * y5aa::MAX_NA * sizeof(float), lds_acc = y5aa::T * sizeof(double);
  for (int g = init_f ? -1 : 0; g < gen; ++g) {
    const double* vg = g < 0 ? nullptr : v + (size_t)g * na * 2;
    hipLaunchKernelGGL(y5_anchor_fitness_kernel, dim3(nblk), dim3(y5aa::T), lds_fit, stream, wh, n, k, vg, na, thr_inv, partial);
    hipLaunchKernelGGL(y5_anchor_accept_kernel, dim3(1), dim3(y5aa::T), lds_acc, stream, partial, nblk, n, k, vg, na, f,
                       g < 0 ? nullptr : accepted + g);
  }
  return y5_check_launch("y5_anchor_evolve");
}

extern "C" size_t y5_anchor_kmeans_ws_bytes(long long n, int R, int k) {
  if (n < 1 || R < 1 || k < 1 || R > y5aa::T || !y5aa::kmeans_sublanes(R, k, nullptr)) return 0;
  const int S = y5aa::kmeans_sublanes(R, k, nullptr);
  return y5aa::align256((size_t)(R + 1) * sizeof(int)) + (size_t)y5aa::blocks_for(n, S * 64) * R * (3 * k + 1) * sizeof(double);
}

extern "C" int y5_anchor_kmeans(const float* obs, long long n, const float* guess, int R, int k, int init, int steps, double* book,
                                unsigned char* alive, double* last_dist, int* iters, int* done, void* workspace, size_t workspace_bytes,
                                void* stream_) {
  if (!obs || !book || !alive || !last_dist || !iters || !done || !workspace || (init && !guess))
    return y5_fail(Y5_ERR_BAD_ARG, "anchor_kmeans: null pointer");
  if (n < 1 || R < 1 || R > y5aa::T || k < 1 || k > n || steps < 0) return y5_fail(Y5_ERR_BAD_ARG, "anchor_kmeans: need n >= k >= 1, 1 <= R <= 256, steps >= 0");
  size_t lds = 0;
  const int S = y5aa::kmeans_sublanes(R, k, &lds);
  if (!S) return y5_fail(Y5_ERR_UNSUPPORTED, "anchor_kmeans: R restarts of k centroids do not fit the 64 KiB of LDS sums");
  if (workspace_bytes < y5_anchor_kmeans_ws_bytes(n, R, k)) return y5_fail(Y5_ERR_WORKSPACE, "anchor_kmeans: workspace too small");
  if (reinterpret_cast<uintptr_t>(workspace) & 7) return y5_fail(Y5_ERR_BAD_ARG, "anchor_kmeans: workspace must be 8-byte aligned");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  Y5KmeansState st{book, alive, last_dist, iters, static_cast<int*>(workspace), done};
  double* partial = reinterpret_cast<double*>(static_cast<char*>(workspace) + y5aa::align256((size_t)(R + 1) * sizeof(int)));
  const int nblk = y5aa::blocks_for(n, S * 64);
  if (init) hipLaunchKernelGGL(y5_kmeans_init_kernel, dim3((R * k * 2 + y5aa::T - 1) / y5aa::T), dim3(y5aa::T), 0, stream, guess, R, k, st);
  for (int it = 0; it < steps; ++it) {
    hipLaunchKernelGGL(y5_kmeans_assign_kernel, dim3(nblk), dim3(y5aa::T), lds, stream, obs, n, R, k, S, st, partial);
    hipLaunchKernelGGL(y5_kmeans_update_kernel, dim3(1), dim3(y5aa::T), (size_t)R * (3 * k + 1) * sizeof(double), stream, partial, nblk, n, R, k, st);
  }
  return y5_check_launch("y5_anchor_kmeans");
}
