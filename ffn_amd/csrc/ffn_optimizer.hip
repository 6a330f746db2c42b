// libffn_hip.so, the parameter update of a training step
// (include/ffn_optimizer.h): gradient statistics and the clipped update of
// five rules over flat f32 arrays.
//
// apply_kernel<RULE> is one launch over all elements: a grid-stride loop over
// 16-byte vectors (global_load / global_store_dwordx4, lane i at base + 16 i)
// and the count % 4 tail elements by the first threads of the grid.  The rule
// is a template parameter, so an instantiation loads and stores only the
// arrays its rule names (8 to 28 bytes per element).  No LDS, no scratch.
// Contraction is off for the whole file: every product and sum of the
// definition is rounded on its own, so the result equals a restatement with
// one numpy f32 operation per written operation.
//
// aggregate_kernel has the same shape: one launch, a grid-stride loop over
// 16-byte vectors, the tail by the first threads.  A thread folds the n
// replica arrays of its vector in replica order (the loads of a vector's
// replicas are independent of the sum and are issued ahead of it, four at a
// time), divides once and stores once.  No LDS, no atomics.
//
// stats_kernel takes per-thread maxima and counts, an LDS tree per workgroup,
// and writes one partial per workgroup; stats_sum_kernel (one workgroup)
// combines them.  A maximum and integer sums are the same in any order.

#include "../../include/ffn_optimizer.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "ffn_unit.h"

#pragma clang fp contract(off)

namespace {

using ffn_unit::DevBuf;
using ffn_unit::PinnedBuf;

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

constexpr int kThreads = 256;
constexpr int kApplyBlocks = 512;  // at most: two workgroups a CU
constexpr int kStatBlocks = 256;   // at most: what stats_sum_kernel reads
constexpr int kRules = 5;
constexpr int kMaxReplicas = 256;  // arrays one aggregate folds

struct Coef {
  float lr, clip, c0, c1, eps;
};

// Which slots a rule names.
constexpr bool uses_slot0(int rule) { return rule != FFN_OPTIMIZER_SGD; }
constexpr bool uses_slot1(int rule) {
  return rule == FFN_OPTIMIZER_ADAM || rule == FFN_OPTIMIZER_RMSPROP;
}

// One element of the definition in ffn_optimizer.h, operation by operation.
template <int RULE>
__device__ __forceinline__ void update(float& p, float g, float& a, float& b,
                                       const Coef& k) {
  if (k.clip > 0.f) {
    g = g < -k.clip ? -k.clip : g;
    g = g > k.clip ? k.clip : g;
  }
  if (RULE == FFN_OPTIMIZER_SGD) {
    const float t = k.lr * g;
    p = p - t;
  } else if (RULE == FFN_OPTIMIZER_MOMENTUM) {
    const float t = a * k.c0;
    a = t + g;
    const float u = a * k.lr;
    p = p - u;
  } else if (RULE == FFN_OPTIMIZER_ADAGRAD) {
    const float gg = g * g;
    a = a + gg;
    const float t = k.lr * g;
    const float s = sqrtf(a);
    const float u = t / s;
    p = p - u;
  } else if (RULE == FFN_OPTIMIZER_ADAM) {
    const float d = g - a;
    const float dm = d * k.c0;
    a = a + dm;
    const float gg = g * g;
    const float e = gg - b;
    const float dv = e * k.c1;
    b = b + dv;
    const float t = a * k.lr;
    const float s = sqrtf(b);
    const float den = s + k.eps;
    const float u = t / den;
    p = p - u;
  } else {
    const float gg = g * g;
    const float e = gg - a;
    const float dms = e * k.c0;
    a = a + dms;
    const float bm = b * k.c1;
    const float t = g * k.lr;
    const float r = a + k.eps;
    const float s = sqrtf(r);
    const float u = t / s;
    b = bm + u;
    p = p - b;
  }
}

template <int RULE>
__global__ __launch_bounds__(kThreads) void apply_kernel(
    float* __restrict__ params, const float* __restrict__ grads,
    float* __restrict__ slot0, float* __restrict__ slot1, int count, Coef k) {
  const int nvec = count >> 2;
  const int tid = blockIdx.x * kThreads + threadIdx.x;
  const int stride = gridDim.x * kThreads;
  for (int i = tid; i < nvec; i += stride) {
    f32x4 p = reinterpret_cast<const f32x4*>(params)[i];
    const f32x4 g = reinterpret_cast<const f32x4*>(grads)[i];
    f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
    if (uses_slot0(RULE)) a = reinterpret_cast<const f32x4*>(slot0)[i];
    if (uses_slot1(RULE)) b = reinterpret_cast<const f32x4*>(slot1)[i];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float pc = p[c], ac = a[c], bc = b[c];
      update<RULE>(pc, g[c], ac, bc, k);
      p[c] = pc;
      a[c] = ac;
      b[c] = bc;
    }
    reinterpret_cast<f32x4*>(params)[i] = p;
    if (uses_slot0(RULE)) reinterpret_cast<f32x4*>(slot0)[i] = a;
    if (uses_slot1(RULE)) reinterpret_cast<f32x4*>(slot1)[i] = b;
  }
  // the count % 4 elements behind the last whole vector
  const int e = (nvec << 2) + tid;
  if (tid < 4 && e < count) {
    float p = params[e], a = 0.f, b = 0.f;
    if (uses_slot0(RULE)) a = slot0[e];
    if (uses_slot1(RULE)) b = slot1[e];
    update<RULE>(p, grads[e], a, b, k);
    params[e] = p;
    if (uses_slot0(RULE)) slot0[e] = a;
    if (uses_slot1(RULE)) slot1[e] = b;
  }
}

// One entry of a replica's gradient, clipped as `update` clips.
__device__ __forceinline__ float clipped(float g, float clip) {
  if (clip > 0.f) {
    g = g < -clip ? -clip : g;
    g = g > clip ? clip : g;
  }
  return g;
}

// dst[i] = (clip(src[0][i]) + clip(src[1][i]) + ... in this order) / n, the
// definition of aggregate in ffn_optimizer.h.  stride: floats between arrays.
__global__ __launch_bounds__(kThreads) void aggregate_kernel(
    const float* __restrict__ src, long long stride, int n, int count,
    float clip, float* __restrict__ dst) {
  const int nvec = count >> 2;
  const int tid = blockIdx.x * kThreads + threadIdx.x;
  const int step = gridDim.x * kThreads;
  const float fn = (float)n;
  for (int i = tid; i < nvec; i += step) {
    f32x4 t = reinterpret_cast<const f32x4*>(src)[i];
#pragma unroll
    for (int c = 0; c < 4; ++c) t[c] = clipped(t[c], clip);
#pragma unroll 4
    for (int r = 1; r < n; ++r) {
      const f32x4 g = reinterpret_cast<const f32x4*>(src + r * stride)[i];
#pragma unroll
      for (int c = 0; c < 4; ++c) t[c] = t[c] + clipped(g[c], clip);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) t[c] = t[c] / fn;
    reinterpret_cast<f32x4*>(dst)[i] = t;
  }
  // the count % 4 elements behind the last whole vector
  const int e = (nvec << 2) + tid;
  if (tid < 4 && e < count) {
    float t = clipped(src[e], clip);
    for (int r = 1; r < n; ++r) t = t + clipped(src[r * stride + e], clip);
    dst[e] = t / fn;
  }
}

struct Stats {
  float max_abs;
  u64 clipped, nonfinite;
};

// A thread's own counts fit 32 bits (count < 2^31).
__device__ __forceinline__ void stats_take(float g, float clip, float& max_abs,
                                           unsigned& clipped,
                                           unsigned& nonfinite) {
  const float m = fabsf(g);
  const bool finite = m < INFINITY;  // false for a NaN too
  max_abs = fmaxf(max_abs, finite ? m : 0.f);
  clipped += (finite && clip > 0.f && m > clip) ? 1u : 0u;
  nonfinite += finite ? 0u : 1u;
}

// The workgroup's combined value, in thread 0.
__device__ __forceinline__ Stats stats_block(Stats s) {
  __shared__ float s_max[kThreads];
  __shared__ u64 s_clip[kThreads], s_bad[kThreads];
  const int t = threadIdx.x;
  s_max[t] = s.max_abs;
  s_clip[t] = s.clipped;
  s_bad[t] = s.nonfinite;
  __syncthreads();
  for (int half = kThreads / 2; half > 0; half >>= 1) {
    if (t < half) {
      s_max[t] = fmaxf(s_max[t], s_max[t + half]);
      s_clip[t] += s_clip[t + half];
      s_bad[t] += s_bad[t + half];
    }
    __syncthreads();
  }
  return Stats{s_max[0], s_clip[0], s_bad[0]};
}

// partial_counts: [gridDim.x][2], partial_max: [gridDim.x].
__global__ __launch_bounds__(kThreads) void stats_kernel(
    const float* __restrict__ grads, int count, float clip,
    u64* __restrict__ partial_counts, float* __restrict__ partial_max) {
  const int nvec = count >> 2;
  const int tid = blockIdx.x * kThreads + threadIdx.x;
  const int stride = gridDim.x * kThreads;
  float max_abs = 0.f;
  unsigned clipped = 0, nonfinite = 0;
  for (int i = tid; i < nvec; i += stride) {
    const f32x4 g = reinterpret_cast<const f32x4*>(grads)[i];
#pragma unroll
    for (int c = 0; c < 4; ++c)
      stats_take(g[c], clip, max_abs, clipped, nonfinite);
  }
  const int e = (nvec << 2) + tid;
  if (tid < 4 && e < count)
    stats_take(grads[e], clip, max_abs, clipped, nonfinite);
  const Stats s = stats_block(Stats{max_abs, clipped, nonfinite});
  if (threadIdx.x == 0) {
    partial_counts[2 * blockIdx.x] = s.clipped;
    partial_counts[2 * blockIdx.x + 1] = s.nonfinite;
    partial_max[blockIdx.x] = s.max_abs;
  }
}

// out: clipped, nonfinite, and the bits of max_abs in the low half of out[2].
__global__ __launch_bounds__(kThreads) void stats_sum_kernel(
    const u64* __restrict__ partial_counts,
    const float* __restrict__ partial_max, int nblocks, u64* __restrict__ out) {
  const int t = threadIdx.x;
  Stats s = {0.f, 0, 0};
  if (t < nblocks) {
    s.max_abs = partial_max[t];
    s.clipped = partial_counts[2 * t];
    s.nonfinite = partial_counts[2 * t + 1];
  }
  s = stats_block(s);
  if (t == 0) {
    out[0] = s.clipped;
    out[1] = s.nonfinite;
    out[2] = (u64)__float_as_uint(s.max_abs);
  }
}

}  // namespace

struct ffn_optimizer : ffn_unit::Unit {
  DevBuf counts;  // kStatBlocks x 2 partial counts + the 3 results
  DevBuf maxima;  // kStatBlocks partial maxima
  PinnedBuf stage;
  double ms[3] = {0, 0, 0};  // grad_stats, apply, aggregate
};

namespace {

#define O_PTR(p)                                                \
  do {                                                          \
    if (!(p)) return ffn_set_error(FFN_ERR_ARG, #p " is NULL"); \
  } while (0)

int check_count(const ffn_optimizer* h, int64_t count) {
  if (!h) return ffn_set_error(FFN_ERR_ARG, "handle is NULL");
  if (count < 1 || count >= (1ll << 31))
    return ffn_set_error(FFN_ERR_ARG, "count = %lld, expected 1 .. 2^31 - 1",
                         (long long)count);
  return FFN_OK;
}

int check_aligned(const float* p, const char* name) {
  if (reinterpret_cast<uintptr_t>(p) % 16 != 0)
    return ffn_set_error(FFN_ERR_ARG, "%s is not 16-byte aligned", name);
  return FFN_OK;
}

bool overlap(const float* a, const float* b, size_t count) {
  return a < b + count && b < a + count;
}

int begin(ffn_optimizer* h) {
  U_TRY(hipSetDevice(h->device_id));
  return h->timer_start();
}

int end(ffn_optimizer* h, int which) {
  U_TRY(hipGetLastError());
  return h->timer_stop(&h->ms[which]);
}

template <int RULE>
void launch_apply(ffn_optimizer* h, int blocks, float* params,
                  const float* grads, float* slot0, float* slot1, int count,
                  Coef k) {
  hipLaunchKernelGGL(apply_kernel<RULE>, dim3(blocks), dim3(kThreads), 0,
                     h->stream, params, grads, slot0, slot1, count, k);
}

// Workgroups for `count` elements, four a thread: 1 .. cap.
int blocks_for(int64_t count, int cap) {
  const int64_t nvec = std::max<int64_t>(1, count / 4);
  return (int)std::min<int64_t>(cap, (nvec + kThreads - 1) / kThreads);
}

}  // namespace

extern "C" {

int ffn_optimizer_create(int device_id, ffn_optimizer** out) {
  U_OK(ffn_unit::unit_create(device_id, out));
  ffn_optimizer* h = *out;
  int rc = ffn_unit::ensure(h->counts, (2 * kStatBlocks + 3) * sizeof(u64));
  if (rc == FFN_OK) rc = ffn_unit::ensure(h->maxima, kStatBlocks * sizeof(float));
  if (rc == FFN_OK) rc = ffn_unit::ensure(h->stage, 3 * sizeof(u64));
  if (rc != FFN_OK) {
    ffn_unit::unit_destroy(h);
    *out = nullptr;
  }
  return rc;
}

void ffn_optimizer_destroy(ffn_optimizer* h) { ffn_unit::unit_destroy(h); }

int ffn_optimizer_grad_stats(ffn_optimizer* h, int64_t count,
                             const float* grads_dev, float clip,
                             float* max_abs, uint64_t* clipped,
                             uint64_t* nonfinite) {
  U_OK(check_count(h, count));
  O_PTR(grads_dev);
  O_PTR(max_abs);
  O_PTR(clipped);
  O_PTR(nonfinite);
  U_OK(check_aligned(grads_dev, "grads_dev"));
  if (std::isnan(clip)) return ffn_set_error(FFN_ERR_ARG, "clip is a NaN");
  U_OK(begin(h));
  u64* counts = static_cast<u64*>(h->counts.p);
  float* maxima = static_cast<float*>(h->maxima.p);
  u64* result = counts + 2 * kStatBlocks;
  const int blocks = blocks_for(count, kStatBlocks);
  hipLaunchKernelGGL(stats_kernel, dim3(blocks), dim3(kThreads), 0, h->stream,
                     grads_dev, (int)count, clip, counts, maxima);
  hipLaunchKernelGGL(stats_sum_kernel, dim3(1), dim3(kThreads), 0, h->stream,
                     static_cast<const u64*>(counts),
                     static_cast<const float*>(maxima), blocks, result);
  U_OK(end(h, 0));
  U_TRY(hipMemcpyAsync(h->stage.p, result, 3 * sizeof(u64),
                       hipMemcpyDeviceToHost, h->stream));
  U_TRY(hipStreamSynchronize(h->stream));
  const u64* got = static_cast<const u64*>(h->stage.p);
  const uint32_t bits = (uint32_t)got[2];
  *clipped = got[0];
  *nonfinite = got[1];
  memcpy(max_abs, &bits, sizeof(float));
  return FFN_OK;
}

int ffn_optimizer_apply(ffn_optimizer* h, int rule, int64_t count,
                        float* params_dev, const float* grads_dev,
                        float* slot0_dev, float* slot1_dev, float lr,
                        float clip, float c0, float c1, float eps) {
  U_OK(check_count(h, count));
  if (rule < 0 || rule >= kRules)
    return ffn_set_error(FFN_ERR_ARG, "rule = %d, expected 0 .. %d", rule,
                         kRules - 1);
  O_PTR(params_dev);
  O_PTR(grads_dev);
  if (uses_slot0(rule) != (slot0_dev != nullptr))
    return ffn_set_error(FFN_ERR_ARG, "rule %d %s slot0_dev", rule,
                         uses_slot0(rule) ? "needs" : "takes no");
  if (uses_slot1(rule) != (slot1_dev != nullptr))
    return ffn_set_error(FFN_ERR_ARG, "rule %d %s slot1_dev", rule,
                         uses_slot1(rule) ? "needs" : "takes no");
  const float* arrays[4] = {params_dev, grads_dev, slot0_dev, slot1_dev};
  const char* names[4] = {"params_dev", "grads_dev", "slot0_dev", "slot1_dev"};
  for (int i = 0; i < 4; ++i) {
    if (!arrays[i]) continue;
    U_OK(check_aligned(arrays[i], names[i]));
    for (int j = 0; j < i; ++j)
      if (arrays[j] && overlap(arrays[i], arrays[j], (size_t)count))
        return ffn_set_error(FFN_ERR_ARG, "%s overlaps %s", names[i], names[j]);
  }
  if (!std::isfinite(lr)) return ffn_set_error(FFN_ERR_ARG, "lr is not finite");
  if (std::isnan(clip)) return ffn_set_error(FFN_ERR_ARG, "clip is a NaN");
  U_OK(begin(h));
  const Coef k = {lr, clip, c0, c1, eps};
  const int blocks = blocks_for(count, kApplyBlocks);
  const int n = (int)count;
  switch (rule) {
    case FFN_OPTIMIZER_SGD:
      launch_apply<FFN_OPTIMIZER_SGD>(h, blocks, params_dev, grads_dev, nullptr,
                                      nullptr, n, k);
      break;
    case FFN_OPTIMIZER_MOMENTUM:
      launch_apply<FFN_OPTIMIZER_MOMENTUM>(h, blocks, params_dev, grads_dev,
                                           slot0_dev, nullptr, n, k);
      break;
    case FFN_OPTIMIZER_ADAGRAD:
      launch_apply<FFN_OPTIMIZER_ADAGRAD>(h, blocks, params_dev, grads_dev,
                                          slot0_dev, nullptr, n, k);
      break;
    case FFN_OPTIMIZER_ADAM:
      launch_apply<FFN_OPTIMIZER_ADAM>(h, blocks, params_dev, grads_dev,
                                       slot0_dev, slot1_dev, n, k);
      break;
    default:
      launch_apply<FFN_OPTIMIZER_RMSPROP>(h, blocks, params_dev, grads_dev,
                                          slot0_dev, slot1_dev, n, k);
      break;
  }
  return end(h, 1);
}

int ffn_optimizer_aggregate(ffn_optimizer* h, int64_t count, int n,
                            const float* src_dev, int64_t stride, float clip,
                            float* dst_dev) {
  U_OK(check_count(h, count));
  if (n < 1 || n > kMaxReplicas)
    return ffn_set_error(FFN_ERR_ARG, "n = %d, expected 1 .. %d", n,
                         kMaxReplicas);
  O_PTR(src_dev);
  O_PTR(dst_dev);
  if (stride < count || stride % 4 != 0)
    return ffn_set_error(FFN_ERR_ARG,
                         "stride = %lld, expected a multiple of 4 that is >= "
                         "count = %lld", (long long)stride, (long long)count);
  U_OK(check_aligned(src_dev, "src_dev"));
  U_OK(check_aligned(dst_dev, "dst_dev"));
  // (n - 1) * stride + count < 2^8 * 2^31: no overflow of size_t
  const size_t span = (size_t)(n - 1) * (size_t)stride + (size_t)count;
  if (src_dev < dst_dev + count && dst_dev < src_dev + span)
    return ffn_set_error(FFN_ERR_ARG, "dst_dev overlaps src_dev");
  if (std::isnan(clip)) return ffn_set_error(FFN_ERR_ARG, "clip is a NaN");
  U_OK(begin(h));
  hipLaunchKernelGGL(aggregate_kernel, dim3(blocks_for(count, kApplyBlocks)),
                     dim3(kThreads), 0, h->stream, src_dev, (long long)stride,
                     n, (int)count, clip, dst_dev);
  return end(h, 2);
}

int ffn_optimizer_last_timing(ffn_optimizer* h, double kernel_ms[2]) {
  if (!h || !kernel_ms) return ffn_set_error(FFN_ERR_ARG, "NULL argument");
  kernel_ms[0] = h->ms[0];
  kernel_ms[1] = h->ms[1];
  return FFN_OK;
}

int ffn_optimizer_last_timing_aggregate(ffn_optimizer* h, double* kernel_ms) {
  if (!h || !kernel_ms) return ffn_set_error(FFN_ERR_ARG, "NULL argument");
  *kernel_ms = h->ms[2];
  return FFN_OK;
}

}  // extern "C"
