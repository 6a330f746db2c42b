// libffn_hip.so -- host side of the C-ABI declared in include/ffn_hip.h.
//
// One engine = one GPU + one HIP stream + the conv-stack weights + staging and
// activation buffers for up to max_batch concurrent fields of view.  Canvases
// (image / seed / segmentation of a whole subvolume) are device resident.
// The reference interfaces each entry point replaces are cited in the header.
//
// This unit: the engine itself (create, destroy, weights, the pace tuner), the stateless
// predict calls, the FoV step (submit, wait) and the segment loop that drives it.  The conv
// stack they run is the launch layer behind ffn_stack.h (run_stack; no conv kernel is
// named here).  What a canvas does between steps is ffn_canvas.hip; options, profiler and
// debug readers are ffn_options.hip (ffn_engine.h).

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "ffn_engine.h"
#include "ffn_stack.h"
#include "ffn_kernels.h"
#include "ffn_step_kernels.h"

namespace {
thread_local std::string g_error;
}  // namespace

int ffn_set_error(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_error = buf;
  return code;
}

namespace {
constexpr int kFlowStrikes = 3;

// A step came back void, and its own record says why (ffn_step_result.range_error
// 3, written from word 1 of the step's range flag): the resident launch gave up on
// a producer (conv32ps: a poll reached its bound -- some workgroup was not on the
// chip, or far too late), not the fp16 range check.  Then the caller gets
// FFN_ERR_FLOW instead of FFN_ERR_RANGE: same contract (nothing was pasted,
// repeat the step), but the arithmetic stays -- the repeat runs the same convs as
// per-layer launches (same bits) -- and after kFlowStrikes such steps in a row
// the engine stops using the resident launch.  0: not a flow time-out.
int flow_voided(ffn_engine* e, bool timed_out) {
  if (!timed_out) return 0;
  EngineLock lock_(e);
  e->stat_flow_voids += 1;
  e->flow_strikes += 1;
  e->flow_skip = 1;
  if (e->flow_strikes >= kFlowStrikes && e->flow == 2) {
    e->flow = 0;
    e->flow_auto_off = 1;
    e->flow_skip = 0;
    return fail(FFN_ERR_FLOW,
                "the resident conv launch timed out waiting for one of its own "
                "workgroups %d steps in a row (is the GPU shared or partitioned?): "
                "the step changed nothing; this engine now runs one launch per conv "
                "(option flow = 0; set flow = 2 to try again) -- repeat the step",
                kFlowStrikes);
  }
  return fail(FFN_ERR_FLOW,
              "the resident conv launch timed out waiting for one of its own "
              "workgroups: the step changed nothing; repeat it (the repeat runs one "
              "launch per conv, same arithmetic)");
}

// x ~= hi + 2^-11 * res with hi, res fp16 (what the device does when staging)
inline void split_fp16x2(float x, uint16_t part[2]) {
  const float xh = std::fabs(x) < 6.103515625e-05f ? 0.0f : x;
  const _Float16 hi = (_Float16)xh;
  const _Float16 res = (_Float16)((x - (float)hi) * 2048.0f);
  std::memcpy(&part[0], &hi, 2);
  std::memcpy(&part[1], &res, 2);
}

// Step descriptors for the dense uploaded FoVs (predict / forward_resident):
// each FoV is its own FoV-sized "canvas" centred on its middle voxel.
int dense_items(ffn_engine* e, int n, StepItems* si) {
  const Geom& g = e->g;
  for (int k = 0; k < n; ++k) {
    StepItem& it = e->h_items[k];
    std::memset(&it, 0, sizeof(it));
    it.image = e->up_image + (size_t)k * g.V;
    it.seed = e->up_seed + (size_t)k * g.V;
    it.cz = g.fz;
    it.cy = g.fy;
    it.cx = g.fx;
    it.req.pos[0] = g.fz / 2;
    it.req.pos[1] = g.fy / 2;
    it.req.pos[2] = g.fx / 2;
  }
  si->items = e->d_items;
  si->use_inline = n == 1;
  si->inline_item = e->h_items[0];
  if (n > 1)
    HIP_TRY(hipMemcpyAsync(e->d_items, e->h_items, sizeof(StepItem) * n,
                           hipMemcpyHostToDevice, e->stream));
  return FFN_OK;
}


// what the stateless calls check before they touch the device
int check_batch(const ffn_engine* e, int n) {
  if (n < 1 || n > e->max_batch)
    return fail(FFN_ERR_ARG, "batch %d outside [1, %d]", n, e->max_batch);
  if (!e->weights_set) return fail(FFN_ERR_STATE, "weights not set");
  return FFN_OK;
}

// The stack on the n uploaded FoVs, until a run counts.  A void run is repeated: after a
// time-out of the resident launch with per-layer launches of the same kernels (same
// bits), after a range error -- also one that only shows in that repeat -- with the
// exact-f32 kernel.  At most two repeats.  after_run: queued behind every run (the copy
// of its logits, where they leave the engine run by run); who: the caller, for the error.
template <class AfterRun>
int predict_uploaded(ffn_engine* e, int n, const char* who, AfterRun after_run) {
  StepItems si;
  int rc = dense_items(e, n, &si);
  if (rc) return rc;
  for (int attempt = 0;; ++attempt) {
    // NaNs in a caller-provided seed stay NaN (the reference would feed them to TF).
    rc = run_stack(e, n, si, std::nanf(""), INFINITY);
    if (!rc) rc = after_run();
    if (rc) return rc;
    unsigned flag[2] = {0, 0};
    if (e->conv_variant >= 6)
      HIP_TRY(hipMemcpyAsync(flag, e->range_flag, sizeof(flag), hipMemcpyDeviceToHost,
                             e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    const bool is_void = e->conv_variant >= 6 && flag[0] == e->range_tag;
    if (!is_void) {
      if (e->last_stack_resident) e->flow_strikes = 0;
      return FFN_OK;
    }
    if (attempt == 2) return fail(FFN_ERR_HIP, "%s: the step stayed void", who);
    if (flow_voided(e, flag[1] == e->range_tag) == 0) {
      rc = switch_variant(e, e->caps.exact_variant);
      if (rc) return rc;
    }
  }
}
}  // namespace

extern "C" {

int ffn_abi_version(void) { return 10; }

const char* ffn_last_error(void) { return g_error.c_str(); }

size_t ffn_engine_weight_count(int depth, int features) {
  const size_t F = (size_t)features;
  return 27 * 2 * F + F + (size_t)(2 * depth - 1) * (27 * F * F + F) + F + 1;
}

int ffn_engine_create(int device_id, const int32_t fov_zyx[3],
                      const int32_t deltas_zyx[3], int depth, int features,
                      int max_batch, ffn_engine** out) {
  if (!out || !fov_zyx || !deltas_zyx) return fail(FFN_ERR_ARG, "null argument");
  *out = nullptr;
  if (features != kFeatures)
    return fail(FFN_ERR_ARG, "features must be %d (got %d)", kFeatures, features);
  if (depth < 1 || max_batch < 1)
    return fail(FFN_ERR_ARG, "depth and max_batch must be >= 1");
  for (int k = 0; k < 3; ++k) {
    if (fov_zyx[k] < 3 || fov_zyx[k] % 2 == 0)
      return fail(FFN_ERR_ARG, "fov must be odd and >= 3 per axis");
    if (deltas_zyx[k] < 0 || 2 * deltas_zyx[k] + 1 > fov_zyx[k])
      return fail(FFN_ERR_ARG, "deltas do not fit inside the fov");
  }
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device_id < 0 || device_id >= ndev)
    return fail(FFN_ERR_ARG, "device %d not present (%d visible)", device_id, ndev);
  HIP_TRY(hipSetDevice(device_id));

  ffn_engine* e = new ffn_engine();
  e->device = device_id;
  e->depth = depth;
  e->max_batch = max_batch;
  Geom& g = e->g;
  g = fov_geom(fov_zyx, deltas_zyx);
  // everything the geometry fixes for the conv kernels, before the first allocation
  e->caps = conv_caps(g, depth);
  const ConvCaps& caps = e->caps;
  g.act_stride = caps.act_stride;
  if (caps.lds_bytes > 160 * 1024) {
    const size_t bytes = caps.lds_bytes;
    delete e;
    return fail(FFN_ERR_ARG, "fov too wide for the LDS-staged conv (%zu B)", bytes);
  }
  e->conv_variant = caps.default_variant;

#define E_TRY(expr)                                                          \
  do {                                                                       \
    hipError_t _e = (expr);                                                  \
    if (_e != hipSuccess) {                                                  \
      int _rc = fail(FFN_ERR_HIP, "%s failed: %s (%s:%d)", #expr,            \
                     hipGetErrorString(_e), __FILE__, __LINE__);             \
      ffn_engine_destroy(e);                                                 \
      return _rc;                                                            \
    }                                                                        \
  } while (0)

  E_TRY(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
  {
    int lo = 0, hi = 0;  // (numerically lowest = highest priority)
    E_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
    E_TRY(hipStreamCreateWithPriority(&e->ustream, hipStreamNonBlocking, hi));
  }
  E_TRY(hipEventCreateWithFlags(&e->main_ev, hipEventDisableTiming));
  const size_t act_bytes = (size_t)3 * max_batch * g.act_stride * sizeof(float);
  E_TRY(hipMalloc(&e->act_base, act_bytes));
  E_TRY(hipMemset(e->act_base, 0, act_bytes));
  e->rawT = e->act_base;
  e->rawX = e->rawT + (size_t)max_batch * g.act_stride;
  e->rawS = e->rawX + (size_t)max_batch * g.act_stride;
  e->bufT = e->rawT + (size_t)g.guard * kFeatures;
  e->bufX = e->rawX + (size_t)g.guard * kFeatures;
  const size_t vbytes = (size_t)max_batch * g.V * sizeof(float);
  E_TRY(hipMalloc(&e->up_image, vbytes));
  E_TRY(hipMalloc(&e->up_seed, vbytes));
  E_TRY(hipMalloc(&e->seed_raw, vbytes));
  E_TRY(hipMalloc(&e->seed_raw_alt, vbytes));
  E_TRY(hipMalloc(&e->logits, vbytes));
  E_TRY(hipHostMalloc(&e->h_io, 3 * vbytes, hipHostMallocDefault));
  E_TRY(hipMemset(e->up_image, 0, vbytes));
  E_TRY(hipMemset(e->up_seed, 0, vbytes));
  E_TRY(hipMalloc(&e->count, sizeof(unsigned) * max_batch *
                                  std::max<size_t>(kHeadBlocks, (g.V + 31) / 32)));
  E_TRY(hipMalloc(&e->d_items, sizeof(StepItem) * 2 * max_batch));
  E_TRY(hipHostMalloc(&e->h_items, sizeof(StepItem) * 2 * max_batch,
                      hipHostMallocDefault));
  E_TRY(hipHostMalloc(&e->h_pub,
                      sizeof(unsigned long long) * kPubWords * 2 * max_batch,
                      hipHostMallocDefault));
  std::memset(e->h_pub, 0, sizeof(unsigned long long) * kPubWords * 2 * max_batch);

  // validity table of the padded-flat layout
  {
    std::vector<uint8_t> v((size_t)g.nchunks * kChunk, 0);
    for (int p = 0; p < g.npos; ++p) {
      const int rem = p % g.plane;
      v[p] = (rem / g.XS < g.fy && rem % g.XS < g.fx) ? 1 : 0;
    }
    E_TRY(hipMalloc(&e->valid, v.size()));
    E_TRY(hipMemcpy(e->valid, v.data(), v.size(), hipMemcpyHostToDevice));
    std::vector<uint32_t> bits((size_t)g.nchunks * 5, 0u);
    for (size_t p = 0; p < v.size(); ++p)
      if (v[p]) bits[(p / kChunk) * 5 + ((p % kChunk) >> 5)] |= 1u << (p & 31);
    static_assert(kChunk == 160, "validbits layout assumes 5 words per chunk");
    E_TRY(hipMalloc(&e->validbits, bits.size() * sizeof(uint32_t)));
    E_TRY(hipMemcpy(e->validbits, bits.data(), bits.size() * sizeof(uint32_t),
                    hipMemcpyHostToDevice));
  }

  // dense -> padded position table of the compact variant
  {
    std::vector<int32_t> pidx(std::max((size_t)caps.nchunks_c * kCChunk,
                                       (size_t)caps.nchunks_k * kDChunk));
    for (size_t v = 0; v < pidx.size(); ++v) {
      const int vv = (int)std::min<size_t>(v, (size_t)g.V - 1);
      const int x = vv % g.fx, y = (vv / g.fx) % g.fy, z = vv / (g.fx * g.fy);
      pidx[v] = z * g.plane + y * g.XS + x;
    }
    E_TRY(hipMalloc(&e->d_dbg, (24 + 4 * kDbgMaxWgs) * sizeof(long long)));
    E_TRY(hipMemset(e->d_dbg, 0, (24 + 4 * kDbgMaxWgs) * sizeof(long long)));
    E_TRY(hipMalloc(&e->pidx, pidx.size() * sizeof(int32_t)));
    E_TRY(hipMemcpy(e->pidx, pidx.data(), pidx.size() * sizeof(int32_t),
                    hipMemcpyHostToDevice));
  }
  // The residency halves of flow_fits and h_ok: what the geometry allows
  // (ffn_stack_plan.h) and THIS device can hold.
  E_TRY(hipDeviceGetAttribute(&e->cus, hipDeviceAttributeMultiprocessorCount, device_id));
  // (the attributes first: the occupancy a resident kernel is asked for is the one it has
  // with its LDS granted)
  int rc_stack = set_stack_lds_attrs(e);
  if (!rc_stack) rc_stack = stack_residency(e);
  if (rc_stack) {
    ffn_engine_destroy(e);
    return rc_stack;
  }
  e->flow = e->flow_fits ? 2 : 0;

  // weights: [w0a 27*2*32][b0a 32] ([wpack 27*32*32][bias 32]) x (2*depth-1)
  // [wl 32 + 1]
  {
    size_t off = 0;
    e->w0a_off = off;
    off += 27 * 2 * kFeatures;
    e->b0a_off = off;
    off += kFeatures;
    e->w0ap_off = off;
    off += 27 * 2 * kFeatures;
    for (int l = 0; l < 2 * depth - 1; ++l) {
      e->wpack_off.push_back(off);
      off += 27 * kFeatures * kFeatures;
      e->bias_off.push_back(off);
      off += kFeatures;
    }
    e->wl_off = off;
    off += kFeatures + 1;
    off = (off + 3) & ~(size_t)3;
    E_TRY(hipMalloc(&e->weights, off * sizeof(float)));
    e->wpackd_layer = (size_t)kDTaps * 2 * 2 * 64 * 8;  // + the all-zero tap
    E_TRY(hipMalloc(&e->wpackd, e->wpackd_layer * (2 * depth - 1) *
                                    sizeof(uint16_t)));
    E_TRY(hipMalloc(&e->wpackh, e->wpackd_layer * (2 * depth - 1) * sizeof(uint16_t)));
    // two words each: [0] the tag of the last void run, [1] ... of the last run that
    // was void because the resident launch timed out (the cause, per step)
    E_TRY(hipMalloc(&e->range_flag, 2 * sizeof(unsigned)));
    E_TRY(hipMemset(e->range_flag, 0, 2 * sizeof(unsigned)));
    E_TRY(hipMalloc(&e->range_flag_alt, 2 * sizeof(unsigned)));
    E_TRY(hipMemset(e->range_flag_alt, 0, 2 * sizeof(unsigned)));
    {
      const size_t words = ((size_t)(g.V + 31) / 32 + 64) * kFlowStride;
      E_TRY(hipMalloc(&e->flow_flags, words * sizeof(unsigned)));
      E_TRY(hipMemset(e->flow_flags, 0, words * sizeof(unsigned)));
      E_TRY(hipMalloc(&e->flow_err, sizeof(unsigned)));
      E_TRY(hipMemset(e->flow_err, 0, sizeof(unsigned)));
      if (caps.t_ok) {
        e->flow_trace_slots = std::max(caps.n_main + caps.n_tail, (g.V + kHChunk - 1) / kHChunk);
        const size_t bytes = (size_t)e->flow_trace_slots * kFlowTraceLayers * 8 * sizeof(long long);
        E_TRY(hipMalloc(&e->flow_trace, bytes));
        E_TRY(hipMemset(e->flow_trace, 0, bytes));
      }
    }
    E_TRY(hipMalloc(&e->d_stamps, (32 + 1024) * sizeof(long long)));
    E_TRY(hipMemset(e->d_stamps, 0, (32 + 1024) * sizeof(long long)));
    E_TRY(hipMalloc(&e->d_spec_choice, sizeof(int)));
    E_TRY(hipMemset(e->d_spec_choice, 0xff, sizeof(int)));
    E_TRY(hipMalloc(&e->d_spec_choice_alt, sizeof(int)));
    E_TRY(hipMemset(e->d_spec_choice_alt, 0xff, sizeof(int)));
  }

  e->events.resize(2 * 64);
  for (auto& ev : e->events) E_TRY(hipEventCreate(&ev));
  for (auto& ev : e->ahead_ev) E_TRY(hipEventCreate(&ev));

#undef E_TRY
  *out = e;
  return FFN_OK;
}

void ffn_engine_destroy(ffn_engine* e) {
  if (!e) return;
  (void)hipSetDevice(e->device);
  if (e->stream) (void)hipStreamSynchronize(e->stream);
  // Orphan the canvases still alive: their device memory goes with the engine;
  // ffn_canvas_destroy on an orphan only frees the host struct.
  for (ffn_canvas* c : e->canvases) {
    (void)hipFree(c->image);
    (void)hipFree(c->image_u8);
    (void)hipFree(c->image_lut);
    (void)hipFree(c->seed);
    (void)hipFree(c->seg);
    (void)hipFree(c->restrict_planes);
    c->restrict_planes = nullptr;
    if (c->ev_util) (void)hipEventDestroy(c->ev_util);
    c->ev_util = nullptr;
    c->image = c->seed = nullptr;
    c->image_u8 = nullptr;
    c->image_lut = nullptr;
    c->seg = nullptr;
    c->engine = nullptr;
  }
  e->canvases.clear();
  if (e->ustream) (void)hipStreamSynchronize(e->ustream);
  if (e->main_ev) (void)hipEventDestroy(e->main_ev);
  if (e->ustream) (void)hipStreamDestroy(e->ustream);
  for (auto& ev : e->events)
    if (ev) (void)hipEventDestroy(ev);
  for (auto& ev : e->ahead_ev)
    if (ev) (void)hipEventDestroy(ev);
  void* const device_mem[] = {
      e->act_base, e->up_image, e->up_seed, e->seed_raw, e->seed_raw_alt, e->range_flag_alt,
      e->d_spec_choice_alt, e->logits, e->count, e->wpackd, e->wpackh, e->range_flag,
      e->flow_flags, e->flow_err, e->flow_trace, e->d_spec_choice, e->d_stamps, e->valid,
      e->validbits, e->pidx, e->d_dbg, e->weights, e->d_items, e->d_scratch, e->d_turn};
  for (void* p : device_mem) (void)hipFree(p);
  void* const pinned[] = {e->h_turn, e->h_io, e->h_items, e->h_pub, e->h_scratch};
  for (void* p : pinned)
    if (p) (void)hipHostFree(p);
  if (e->stream) (void)hipStreamDestroy(e->stream);
  delete e;
}

// The beat of the paced resident stack is measured, not assumed: the chain a conv of the
// stack has to get through (words seen -> rows staged -> taps -> stores drained -> word
// published) is 6.2 - 7.0 us depending on the box and its clocks; a beat below it leaves
// the stack free-running (no loss), a beat above it costs 24 x the excess -- and on a box
// whose free-running stack already runs at its chain's length pacing gains nothing at all
// (profiles/r06_pacing.txt: -5 % on three boxes, 0 on a fourth).  So: bring the clocks up
// (~150 ms of stacks), time the free-running stack before AND after a ladder of beats on
// noise inputs, take the best beat + 0.1 us, and CONFIRM it against the free-running stack
// in two alternating rounds; it is kept only if it wins both by more than 1.5 %.  The
// answer is cached per (device, depth, FoV) for the process: ~0.3 s once.
struct PaceKey {
  int device, depth, V;
  bool operator<(const PaceKey& o) const {
    return device != o.device ? device < o.device : depth != o.depth ? depth < o.depth : V < o.V;
  }
};
struct PaceVal { int beat; float free_us, best_us; };
std::mutex g_pace_mu;
std::map<PaceKey, PaceVal> g_pace_cache;

int tune_pace(ffn_engine* e) {
  e->pace_auto = 0;
  e->pace_auto_us[0] = e->pace_auto_us[1] = 0.f;
  // (only where a single FoV's stack is conv32ps: conv_variant 9 with flow = 2, which the
  // option setters grant only where the geometry and the device admit them)
  if (!resident_mt(plan_for(e, 1, 0))) return FFN_OK;
  const PaceKey key{e->device, e->depth, e->g.V};
  {
    std::lock_guard<std::mutex> lk(g_pace_mu);
    auto it = g_pace_cache.find(key);
    if (it != g_pace_cache.end()) {
      e->pace_auto = it->second.beat;
      e->pace_auto_us[0] = it->second.free_us;
      e->pace_auto_us[1] = it->second.best_us;
      return FFN_OK;
    }
  }
  const size_t V = (size_t)e->g.V;
  {
    std::vector<float> noise(2 * V);
    unsigned x = 12345u;
    for (auto& v : noise) {
      x = x * 1664525u + 1013904223u;
      v = ((int)(x >> 8) % 2001 - 1000) * 1e-3f;
    }
    HIP_TRY(hipMemcpy(e->up_image, noise.data(), V * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->up_seed, noise.data() + V, V * sizeof(float), hipMemcpyHostToDevice));
  }
  unsigned errs0 = 0;
  HIP_TRY(hipMemcpy(&errs0, e->flow_err, sizeof(errs0), hipMemcpyDeviceToHost));
  StepItems si;
  int rc = dense_items(e, 1, &si);
  if (rc) return rc;
  hipEvent_t ev0, ev1;
  HIP_TRY(hipEventCreate(&ev0));
  HIP_TRY(hipEventCreate(&ev1));
  const int user_pace = e->flow_pace;
  auto stacks_us = [&](int pace, int reps, float* us) -> int {
    e->flow_pace = pace;
    int r = FFN_OK;
    for (int k = 0; k < 6 && !r; ++k) r = run_stack(e, 1, si, std::nanf(""), INFINITY);
    if (!r && hipEventRecord(ev0, e->stream) != hipSuccess) r = FFN_ERR_HIP;
    for (int k = 0; k < reps && !r; ++k) r = run_stack(e, 1, si, std::nanf(""), INFINITY);
    if (!r && (hipEventRecord(ev1, e->stream) != hipSuccess ||
               hipEventSynchronize(ev1) != hipSuccess))
      r = FFN_ERR_HIP;
    float ms = 0.f;
    if (!r && hipEventElapsedTime(&ms, ev0, ev1) != hipSuccess) r = FFN_ERR_HIP;
    *us = ms * 1e3f / (float)reps;
    return r;
  };
  float us = 0.f, free_us = 0.f, best_us = 0.f;
  int best = 0;
  {  // clocks up: the board needs ~100 ms under load to settle
    const long long t_end = steady_ns() + 150000000LL;
    while (!rc && steady_ns() < t_end) rc = stacks_us(0, 60, &us);
  }
  if (!rc) rc = stacks_us(0, 40, &free_us);
  best_us = 1e30f;
  for (int pace = 560; pace <= 800 && !rc; pace += 20) {
    rc = stacks_us(pace, 24, &us);
    if (!rc && us < best_us) {
      best_us = us;
      best = pace;
    }
  }
  if (!rc) {
    rc = stacks_us(0, 40, &us);
    free_us = std::min(free_us, us);
  }
  bool keep = !rc && best > 0 && best_us < 0.985f * free_us;
  float conf_free = free_us, conf_paced = best_us;
  for (int round = 0; round < 2 && keep && !rc; ++round) {  // confirm, alternating
    float f = 0.f, p = 0.f;
    rc = stacks_us(0, 40, &f);
    if (!rc) rc = stacks_us(best + 10, 40, &p);
    keep = !rc && p < 0.985f * f;
    conf_free = f;
    conf_paced = p;
  }
  e->flow_pace = user_pace;
  (void)hipEventDestroy(ev0);
  (void)hipEventDestroy(ev1);
  if (rc) return rc;
  unsigned errs = 0;
  HIP_TRY(hipMemcpy(&errs, e->flow_err, sizeof(errs), hipMemcpyDeviceToHost));
  const bool timed_out = errs != errs0;
  e->pace_auto_us[0] = conf_free;
  e->pace_auto_us[1] = keep ? conf_paced : best_us;
  if (!timed_out && keep) e->pace_auto = best + 10;
  if (!timed_out) {
    std::lock_guard<std::mutex> lk(g_pace_mu);
    g_pace_cache[key] = PaceVal{e->pace_auto, e->pace_auto_us[0], e->pace_auto_us[1]};
  }
  return FFN_OK;
}

int ffn_engine_set_weights(ffn_engine* e, const float* blob, size_t count) {
  EngineLock lock_(e);
  if (!e || !blob) return fail(FFN_ERR_ARG, "null argument");
  const size_t want = ffn_engine_weight_count(e->depth, kFeatures);
  if (count != want)
    return fail(FFN_ERR_ARG, "weight blob has %zu floats, expected %zu", count,
                want);
  drop_spec(e);
  HIP_TRY(hipSetDevice(e->device));
  const int F = kFeatures;
  std::vector<float> host(e->wl_off + F + 1 + 3, 0.0f);
  const float* src = blob;
  // conv0_a: [27][2][32] + bias, used as stored
  std::vector<uint16_t> hostd(e->wpackd_layer * (2 * e->depth - 1));  // zero tap 27
  std::vector<uint16_t> hosth(hostd.size());
  bool d_weights_ok = true;
  bool weights_in_fp16_range = true;
  // tap (kz', ky', kx') of the permuted layout = the original tap whose offset
  // along axis oa[a] is k'[a]
  int tap_of[27];
  for (int t = 0; t < 27; ++t) {
    const int kp[3] = {t / 9, (t / 3) % 3, t % 3};
    int ko[3];
    for (int a = 0; a < 3; ++a) ko[e->caps.gp.oa[a]] = kp[a];
    tap_of[t] = ko[0] * 9 + ko[1] * 3 + ko[2];
  }
  std::memcpy(&host[e->w0a_off], src, sizeof(float) * 27 * 2 * F);
  for (int t = 0; t < 27; ++t)
    std::memcpy(&host[e->w0ap_off + (size_t)t * 2 * F], src + (size_t)tap_of[t] * 2 * F,
                sizeof(float) * 2 * F);
  src += 27 * 2 * F;
  std::memcpy(&host[e->b0a_off], src, sizeof(float) * F);
  src += F;
  // 32->32 convs: repack W[tap][ci][co] for the MFMA B operand:
  //   wpack[tap][nhalf][h][lane = 16*g + j][s] = W[tap][16h + 4g + s][16*nhalf + j]
  for (int l = 0; l < 2 * e->depth - 1; ++l) {
    float* wp = &host[e->wpack_off[l]];
    for (int tap = 0; tap < 27; ++tap)
      for (int nh = 0; nh < 2; ++nh)
        for (int h = 0; h < 2; ++h)
          for (int lane = 0; lane < 64; ++lane)
            for (int s = 0; s < 4; ++s) {
              const int gq = lane >> 4, j = lane & 15;
              const int ci = 16 * h + 4 * gq + s, co = 16 * nh + j;
              wp[((((size_t)tap * 2 + nh) * 2 + h) * 64 + lane) * 4 + s] =
                  src[((size_t)tap * F + ci) * F + co];
            }
    // conv32d / conv32m: W ~= hi + 2^-11 res (both fp16) as the 32x32x16 A
    // operand (rows = cout), + an all-zero tap 27
    //   wpackd[tap][khalf][plane hi, res][lane][c] =
    //       part(W[tap][16 khalf + 8 (lane >> 5) + c][lane & 31])
    {
      uint16_t* wd = &hostd[(size_t)l * e->wpackd_layer];
      for (int tap = 0; tap < 27; ++tap)
        for (int kh = 0; kh < 2; ++kh)
          for (int lane = 0; lane < 64; ++lane)
            for (int c = 0; c < 8; ++c) {
              const int ci = 16 * kh + 8 * (lane >> 5) + c, co = lane & 31;
              const float w = src[((size_t)tap_of[tap] * F + ci) * F + co];
              if (!(std::fabs(w) <= 65504.0f)) weights_in_fp16_range = false;
              uint16_t part[2];
              split_fp16x2(w, part);
              const size_t base = ((((size_t)tap * 2 + kh) * 2) * 64 + lane) * 8 + c;
              wd[base] = part[0];
              wd[base + 64 * 8] = part[1];
            }
    }
    // conv32h: the 16x16x32 A operand (rows = cout of half h, K = all 32 cin)
    //   wpackh[tap][h][plane hi, res][lane][c] = part(W[tap][8 (lane >> 4) + c][16 h + (lane & 15)])
    {
      uint16_t* wd = &hosth[(size_t)l * e->wpackd_layer];
      for (int tap = 0; tap < 27; ++tap)
        for (int h = 0; h < 2; ++h)
          for (int lane = 0; lane < 64; ++lane)
            for (int c = 0; c < 8; ++c) {
              const int ci = 8 * (lane >> 4) + c, co = 16 * h + (lane & 15);
              uint16_t part[2];
              split_fp16x2(src[((size_t)tap_of[tap] * F + ci) * F + co], part);
              const size_t base = ((((size_t)tap * 2 + h) * 2) * 64 + lane) * 8 + c;
              wd[base] = part[0];
              wd[base + 64 * 8] = part[1];
            }
    }
    src += 27 * F * F;
    std::memcpy(&host[e->bias_off[l]], src, sizeof(float) * F);
    src += F;
  }
  HIP_TRY(hipMemcpy(e->wpackd, hostd.data(), hostd.size() * sizeof(uint16_t),
                    hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(e->wpackh, hosth.data(), hosth.size() * sizeof(uint16_t),
                    hipMemcpyHostToDevice));
  e->d_weights_ok = d_weights_ok;
  e->fp16_ok = weights_in_fp16_range;
  if ((!e->fp16_ok || !e->d_weights_ok) && e->conv_variant >= 6) {
    int rc = switch_variant(e, e->caps.exact_variant);
    if (rc) return rc;
  }
  std::memcpy(&host[e->wl_off], src, sizeof(float) * (F + 1));
  HIP_TRY(hipStreamSynchronize(e->stream));
  HIP_TRY(hipMemcpy(e->weights, host.data(),
                    sizeof(float) * (e->wl_off + F + 1), hipMemcpyHostToDevice));
  e->weights_set = true;
  if (e->flow_pace < 0) {
    int rc = tune_pace(e);
    if (rc) return rc;
  }
  return FFN_OK;
}

int ffn_predict(ffn_engine* e, int n, const float* seed, const float* image,
                float* logits_out) {
  EngineLock lock_(e);
  if (!e || !seed || !image || !logits_out) return fail(FFN_ERR_ARG, "null argument");
  if (int rc = check_batch(e, n)) return rc;
  HIP_TRY(hipSetDevice(e->device));
  const size_t bytes = (size_t)n * e->g.V * sizeof(float);
  // through engine-owned pinned buffers: a pageable hipMemcpy costs ~80 us each
  float* h_seed = e->h_io;
  float* h_image = e->h_io + (size_t)e->max_batch * e->g.V;
  float* h_logits = e->h_io + 2 * (size_t)e->max_batch * e->g.V;
  std::memcpy(h_seed, seed, bytes);
  std::memcpy(h_image, image, bytes);
  HIP_TRY(hipMemcpyAsync(e->up_seed, h_seed, bytes, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(e->up_image, h_image, bytes, hipMemcpyHostToDevice, e->stream));
  const int rc = predict_uploaded(e, n, "ffn_predict", [&]() -> int {
    HIP_TRY(hipMemcpyAsync(h_logits, e->logits, bytes, hipMemcpyDeviceToHost, e->stream));
    return FFN_OK;
  });
  if (rc) return rc;
  std::memcpy(logits_out, h_logits, bytes);
  return FFN_OK;
}

int ffn_predict_device(ffn_engine* e, int n, const float* seed_dev,
                       const float* image_dev, float* logits_dev) {
  EngineLock lock_(e);
  if (!e || !seed_dev || !image_dev || !logits_dev)
    return fail(FFN_ERR_ARG, "null argument");
  if (int rc = check_batch(e, n)) return rc;
  HIP_TRY(hipSetDevice(e->device));
  const size_t bytes = (size_t)n * e->g.V * sizeof(float);
  HIP_TRY(hipMemcpyAsync(e->up_seed, seed_dev, bytes, hipMemcpyDeviceToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(e->up_image, image_dev, bytes, hipMemcpyDeviceToDevice,
                         e->stream));
  // the logits leave the engine only once a run has counted, so logits_dev may be one
  // of the inputs
  if (int rc = predict_uploaded(e, n, "ffn_predict_device", [] { return (int)FFN_OK; }))
    return rc;
  HIP_TRY(hipMemcpyAsync(logits_dev, e->logits, bytes, hipMemcpyDeviceToDevice, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return FFN_OK;
}

int ffn_forward_resident(ffn_engine* e, int n, int repeats) {
  EngineLock lock_(e);
  if (!e) return fail(FFN_ERR_ARG, "null argument");
  if (int rc = check_batch(e, n)) return rc;
  HIP_TRY(hipSetDevice(e->device));
  StepItems si;
  int rc = dense_items(e, n, &si);
  if (rc) return rc;
  for (int r = 0; r < repeats; ++r) {
    rc = run_stack(e, n, si, std::nanf(""), INFINITY);
    if (rc) return rc;
  }
  return FFN_OK;
}

int ffn_engine_set_pred_size(ffn_engine* e, const int32_t pred_zyx[3]) {
  EngineLock lock_(e);
  if (!e || !pred_zyx) return fail(FFN_ERR_ARG, "null argument");
  Geom& g = e->g;
  const int f[3] = {g.fz, g.fy, g.fx}, d[3] = {g.dz, g.dy, g.dx};
  for (int a = 0; a < 3; ++a) {
    if (pred_zyx[a] < 1 || pred_zyx[a] > f[a])
      return fail(FFN_ERR_ARG, "pred size %d outside 1..%d (axis %d)", pred_zyx[a],
                  f[a], a);
    if (d[a] > pred_zyx[a] / 2)
      return fail(FFN_ERR_ARG, "delta %d beyond the prediction's half size %d (axis %d)",
                  d[a], pred_zyx[a] / 2, a);
    // the reference pastes into [start + delta, end - delta) with delta = (seed -
    // pred) // 2 (inference.py:218,410-411): an odd difference gives it a box of
    // pred + 1 voxels and a shape mismatch -- not a geometry it can run
    if ((f[a] - pred_zyx[a]) % 2 != 0)
      return fail(FFN_ERR_ARG, "seed size %d - pred size %d is odd (axis %d): the "
                  "prediction cannot be centred in the seed FoV", f[a], pred_zyx[a], a);
  }
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  drop_spec(e);
  g.Vp = 1;
  g.crop = 0;
  for (int a = 0; a < 3; ++a) {
    // update_seed's zero padding (model.py:168-183): (seed - pred) // 2 in front
    g.c0[a] = (f[a] - pred_zyx[a]) / 2;
    g.c1[a] = g.c0[a] + pred_zyx[a];
    g.Vp *= pred_zyx[a];
    g.crop |= pred_zyx[a] != f[a];
  }
  return FFN_OK;
}

int ffn_canvas_step_submit(ffn_engine* e, int n, ffn_canvas* const* canvases,
                           const ffn_step_request* requests,
                           const ffn_step_params* params, uint32_t* ticket) {
  EngineLock lock_(e);
  if (!e || !canvases || !requests || !params || !ticket)
    return fail(FFN_ERR_ARG, "null argument");
  if (int rc = check_batch(e, n)) return rc;
  // the slot after the last one used, else the other one (two host threads
  // need not alternate)
  const int slot = e->slot_n[e->next_slot] == 0 ? e->next_slot : e->next_slot ^ 1;
  if (e->slot_n[slot] != 0)
    return fail(FFN_ERR_STATE,
                "two steps already in flight: call ffn_canvas_step_wait first");
  HIP_TRY(hipSetDevice(e->device));
  const Geom& g = e->g;
  // the segment loop's hint belongs to THIS call (a single FoV) or to none
  int hint_n = 0;
  int hint_pos[kSpecMax][3];
  bool from_loop = false;
  for (int k = 0; k < n; ++k)
    if (canvases[k]) {
      if (n == 1) {
        hint_n = canvases[k]->hint_n;
        std::memcpy(hint_pos, canvases[k]->hint_pos, sizeof(hint_pos));
        from_loop = canvases[k]->hint_from_loop;
      }
      canvases[k]->hint_n = 0;
      canvases[k]->hint_from_loop = false;
    }
  StepItem* h_items = e->h_items + (size_t)slot * e->max_batch;
  StepItem* d_items = e->d_items + (size_t)slot * e->max_batch;
  unsigned long long* h_pub = e->h_pub + (size_t)slot * e->max_batch * kPubWords;
  const int other = slot ^ 1;
  for (int k = 0; k < n; ++k) {
    const ffn_canvas* c = canvases[k];
    if (!c || c->engine != e) return fail(FFN_ERR_ARG, "canvas %d not of this engine", k);
    const ffn_step_request& r = requests[k];
    const int half[3] = {g.fz / 2, g.fy / 2, g.fx / 2};
    const int dims[3] = {c->cz, c->cy, c->cx};
    for (int a = 0; a < 3; ++a)
      if (r.pos[a] - half[a] < 0 || r.pos[a] + half[a] >= dims[a])
        return fail(FFN_ERR_ARG, "FoV at (%d,%d,%d) leaves the canvas", r.pos[0],
                    r.pos[1], r.pos[2]);
    if (r.num_candidates < 0 || r.num_candidates > FFN_MAX_CANDIDATES)
      return fail(FFN_ERR_ARG, "num_candidates out of range");
    for (int k2 = 0; k2 < k; ++k2)
      if (canvases[k2] == c)
        return fail(FFN_ERR_ARG, "canvas appears twice in one batch");
    // a canvas steps sequentially: it cannot also be in the step in flight
    for (int k2 = 0; k2 < e->slot_n[other]; ++k2)
      if (e->slot_canvas[other][k2] == c)
        return fail(FFN_ERR_STATE, "canvas %d already has a step in flight", k);
    {
      const int lo[3] = {r.pos[0] - half[0], r.pos[1] - half[1], r.pos[2] - half[2]};
      const int hi[3] = {r.pos[0] + half[0] + 1, r.pos[1] + half[1] + 1,
                         r.pos[2] + half[2] + 1};
      const_cast<ffn_canvas*>(c)->mark_dirty(lo, hi);
    }
    if (c->util_pending) {  // its last commit / re-seed, on the utility stream
      HIP_TRY(hipStreamWaitEvent(e->stream, c->ev_util, 0));
      const_cast<ffn_canvas*>(c)->util_pending = false;
    }
    // a single-FoV step raises its flag before it pastes (below)
    const_cast<ffn_canvas*>(c)->paste_after_flag = n == 1;
    StepItem& it = h_items[k];
    it.image = c->image;
    it.image_u8 = c->image_u8;
    it.image_lut = c->image_lut;
    it.seed = c->seed;
    it.seg = c->seg;
    it.cz = c->cz;
    it.cy = c->cy;
    it.cx = c->cx;
    it.req = r;
  }
  HIP_TRY(hipSetDevice(e->device));
  StepItems si;
  si.items = d_items;
  si.use_inline = n == 1;
  si.inline_item = h_items[0];
  if (n > 1)
    HIP_TRY(hipMemcpyAsync(d_items, h_items, sizeof(StepItem) * n,
                           hipMemcpyHostToDevice, e->stream));
  // the speculative conv0_a queued behind the last step, if this is the step it
  // was made for (same canvas and parameters, a position on its list): the
  // device took the first valid position of that list, and so did the caller
  // (only the loop's own steps: it pops the FIRST valid position of its list; a
  // caller stepping the canvas itself may pick any)
  int spec_expected = -1;
  if (e->spec.valid && n == 1 && from_loop && e->spec.canvas == canvases[0] &&
      e->spec.variant == e->conv_variant &&
      std::memcmp(&e->spec.pad_value, &params->pad_value, sizeof(float)) == 0 &&
      std::memcmp(&e->spec.move_thr, &params->move_threshold, sizeof(float)) == 0)
    for (int j = 0; j < e->spec.n && spec_expected < 0; ++j)
      if (std::memcmp(e->spec.pos[j], requests[0].pos, sizeof(int) * 3) == 0)
        spec_expected = j;
  if (spec_expected >= 0) e->stat_spec_hits += 1;
  else if (e->spec.valid && n == 1 && from_loop && e->spec.canvas == canvases[0]) {
    // a launch made ahead that this step does not run on: was its hint list full (the
    // queue held more candidates than a launch looks at) or short (the step comes from the
    // moves the last step queued)?
    if (e->spec.n >= kSpecMax) e->stat_spec_miss_full += 1;
    else e->stat_spec_miss_short += 1;
  }
  if (spec_expected >= 0 && e->spec_force_mismatch > 0) {  // test hook
    e->spec_force_mismatch -= 1;
    spec_expected = kSpecMax;  // an index the device cannot have chosen
  }
  const bool traced = n == 1 && e->fused_trace_in > 0 && --e->fused_trace_in == 0;
  e->trace_now = traced;  // (the launches of this call stamp: a kernel argument)
  if (e->debug_submit_delay_ns > 0) {
    const long long t_d = steady_ns();
    while (steady_ns() - t_d < e->debug_submit_delay_ns) {}
  }
  int rc = FFN_OK;
  if (e->ahead_valid && spec_expected >= 0) {
    // this step's stack is in the stream already, behind the conv0_a made for it
    // (what run_stack would have done was done when it was queued)
    e->ahead_valid = false;
    e->spec.valid = false;
    e->stat_ahead_used += 1;
    if (e->ahead_ev_pending) {  // its event pair is a stack's: among the samples from now on
      e->ahead_ev_pending = false;
      rc = event_pair(e);
      if (rc) return rc;
      e->chain_launches_pending.push_back(2 * e->depth - 1);
      std::swap(e->events[e->events_used++], e->ahead_ev[0]);
      std::swap(e->events[e->events_used++], e->ahead_ev[1]);
    }
  } else {
    rc = run_stack(e, n, si, params->pad_value, params->move_threshold,
                   spec_expected >= 0);
  }
  if (rc) return rc;
  const bool this_stack_resident = e->last_stack_resident;
  const unsigned step_id = ++e->step_id ? e->step_id : ++e->step_id;  // never 0
  // One FoV: faces first -- the host's turn-around is on the critical path and
  // the paste runs under it.  Several: paste first, so that the completion flag
  // the host waits for also says "pasted" and a canvas whose segment has ended
  // can be committed on the utility stream at once (ffn_engine::ustream).
  auto paste = [&]() {
    hipLaunchKernelGGL(paste_kernel, dim3(71, n), dim3(512), 0, e->stream, si, g,
                       e->logits, e->seed_raw, e->count, e->count_blocks,
                       params->move_threshold, params->disco_seed_threshold,
                       e->range_flag, e->range_tag,
                       e->d_spec_choice, spec_expected);
  };
  // the next step's conv0_a, behind the paste and ahead of the host's turn-around
  // (SpecArgs): for the positions the segment loop expects to pop next
  SpecArgs sp;
  sp.n = 0;
  sp.move_thr = params->move_threshold;
  sp.choice = nullptr;  // (launch_conv0a / conv0a_split_args: the next step's word)
  if (n == 1) {
    const ffn_canvas* c = canvases[0];
    const int half[3] = {g.fz / 2, g.fy / 2, g.fx / 2};
    const int dims[3] = {c->cz, c->cy, c->cx};
    for (int j = 0; j < hint_n && e->speculate; ++j) {
      bool inside = true;
      for (int a = 0; a < 3; ++a)
        if (hint_pos[j][a] - half[a] < 0 || hint_pos[j][a] + half[a] >= dims[a])
          inside = false;
      if (!inside) continue;
      for (int a = 0; a < 3; ++a) sp.pos[sp.n][a] = hint_pos[j][a];
      ++sp.n;
    }
    for (int j = sp.n; j < kSpecMax && sp.n > 0; ++j)  // unused slots: readable positions
      for (int a = 0; a < 3; ++a) sp.pos[j][a] = sp.pos[0][a];
  }
  // ... in the SAME launch as this step's faces and paste where it can be
  // (faces_paste_conv0a_kernel: it gathers the canvas as the paste is leaving it)
  const bool fused_next = n == 1 && sp.n > 0 && e->fuse_paste && e->fuse_conv0a &&
                          e->conv_variant >= 6;
  if (n > 1) paste();
  if (fused_next) {
    Conv0Next nx;
    const int tiles = conv0a_split_args(e, params->pad_value, next_tag(e->range_tag), sp,
                                        true, nx);
    const int paste_blocks = e->paste_blocks > 0
        ? e->paste_blocks
        : std::max(kPasteBlocksMin, std::min(kPasteBlocks, e->cus - 1 - tiles));
    const auto fused = [&](int trace) {
#define FFN_FUSED(LABV)                                                                    \
  hipLaunchKernelGGL(faces_paste_conv0a_kernel<LABV>, dim3(1 + paste_blocks + tiles),      \
                     dim3(512), 0, e->stream, si, g, e->logits, e->seed_raw, e->count,     \
                     e->count_blocks, params->move_threshold,                              \
                     params->disco_seed_threshold, params->deleted_threshold,              \
                     e->range_flag, e->range_tag, h_pub, step_id, e->d_spec_choice,        \
                     spec_expected, nx, e->d_stamps, trace, paste_blocks)
      // (the production form does not stamp: a traced launch, or flow_lab, takes the other)
      if (trace != 0 || e->flow_lab != 0) FFN_FUSED(true);
      else FFN_FUSED(false);
#undef FFN_FUSED
    };
    // (experiment debug_fused_twice: the same launch made twice -- idempotent: same record,
    // same paste, same conv0_a -- so that the second, traced one starts on warm caches)
    if (e->debug_fused_twice) fused(0);
    fused(e->trace_now ? 1 : 0);
  } else if (n == 1 && e->fuse_paste) {
    hipLaunchKernelGGL(faces_paste_kernel, dim3(1 + 71), dim3(512), 0, e->stream, si,
                       g, e->logits, e->seed_raw, e->count, e->count_blocks,
                       params->move_threshold, params->disco_seed_threshold,
                       params->deleted_threshold, e->range_flag, e->range_tag,
                       h_pub, step_id, e->d_spec_choice, spec_expected);
  } else {
    hipLaunchKernelGGL(faces_kernel, dim3(n), dim3(512), 0, e->stream, si, g,
                       e->logits, e->seed_raw, e->count, e->count_blocks,
                       params->move_threshold, params->disco_seed_threshold,
                       params->deleted_threshold, e->range_flag, e->range_tag,
                       h_pub, step_id, e->d_spec_choice, spec_expected);
    if (n == 1) paste();
  }
  if (n == 1) {
    ffn_canvas* c = canvases[0];
    if (sp.n > 0) {
      if (!fused_next)
        launch_conv0a(e, 1, si, params->pad_value, next_tag(e->range_tag), sp, true);
      // ... and that step's stack behind it (stack_ahead): only where this step's own
      // stack was a resident launch that is still trusted, and the loop made the step
      bool ahead = false;
      if (fused_next && e->stack_ahead && from_loop && this_stack_resident &&
          resident_mt(plan_for(e, 1, e->flow_skip))) {
        rc = run_stack(e, 1, si, params->pad_value, params->move_threshold, true, true);
        if (rc) return rc;
        ahead = true;
      }
      e->ahead_valid = ahead;
      e->spec.valid = true;
      e->spec.canvas = c;
      e->spec.n = sp.n;
      std::memcpy(e->spec.pos, sp.pos, sizeof(sp.pos));
      e->spec.pad_value = params->pad_value;
      e->spec.move_thr = params->move_threshold;
      e->spec.variant = e->conv_variant;
      e->stat_spec_launched += 1;
    }
  }
  e->trace_now = false;
  HIP_TRY(hipGetLastError());
  e->stat_calls += 1;
  e->stat_items += n;
  e->stat_hist[n < 64 ? n : 64] += 1;
  e->slot_n[slot] = n;
  e->slot_resident[slot] = this_stack_resident;
  e->slot_ticket[slot] = step_id;
  e->slot_canvas[slot].assign(canvases, canvases + n);
  e->next_slot = other;
  *ticket = step_id;
  return FFN_OK;
}

namespace {
int step_wait_impl(ffn_engine* e, uint32_t ticket, ffn_step_result* results,
                   bool* spec_mismatch);
}

int ffn_canvas_step_wait(ffn_engine* e, uint32_t ticket,
                         ffn_step_result* results) {
  return step_wait_impl(e, ticket, results, nullptr);
}

namespace {
// spec_mismatch: where to report a step that ran on a speculative conv0_a made
// for another position (it pasted nothing; ffn_canvas_step repeats it) -- NULL:
// such a step is an error
int step_wait_impl(ffn_engine* e, uint32_t ticket, ffn_step_result* results,
                   bool* spec_mismatch) {
  if (spec_mismatch) *spec_mismatch = false;
  if (!e || !results) return fail(FFN_ERR_ARG, "null argument");
  int slot = -1;
  int n = 0;
  {
    EngineLock lock_(e);
    for (int s = 0; s < 2; ++s)
      if (e->slot_n[s] != 0 && e->slot_ticket[s] == ticket && !e->slot_waited[s])
        slot = s;
    if (slot < 0)
      return fail(FFN_ERR_STATE, "no step with ticket %u in flight", ticket);
    n = e->slot_n[slot];
    e->slot_waited[slot] = true;
  }
  const unsigned step_id = ticket;
  unsigned long long* h_pub = e->h_pub + (size_t)slot * e->max_batch * kPubWords;
  // The slot -- its descriptor, result and flag arrays -- stays taken until the
  // results have been copied out (another thread may submit meanwhile); it is
  // free again whatever happens below.  No lock while waiting: that wait is
  // what two host threads overlap.
  struct SlotRelease {
    ffn_engine* e;
    int slot;
    ~SlotRelease() {
      EngineLock lock_(e);
      e->slot_n[slot] = 0;
      e->slot_waited[slot] = false;
      e->slot_canvas[slot].clear();
    }
  } release_{e, slot};
  HIP_TRY(hipSetDevice(e->device));
  // every published word of the n records carries this step's number
  auto arrived = [&]() {
    for (int k = 0; k < n * kPubWords; ++k)
      if ((unsigned)(__atomic_load_n(&h_pub[k], __ATOMIC_ACQUIRE) >> 32) != step_id)
        return false;
    return true;
  };
  if (e->sync_mode == 1) {
    // Poll the records the faces blocks write into pinned memory: lower wake-up
    // latency than a blocking stream synchronise.  Bounded spin, then fall back
    // to the stream so that device faults still surface as errors.
    // (the stream is asked only after 2 ms without the record, then every 2 ms: a
    // hipStreamQuery on a busy stream puts a system-scope barrier packet into the queue --
    // one per step when it was asked every 4096 spins, sitting between the step's last
    // launch and the next step's first: a full cache release + acquire the next launch
    // waited behind, 3 us per step where launches are queued ahead; profiles/r06_turn_around.txt)
    bool done = false;
    long long t_first = 0, t_query = 0;
    for (long spin = 0; !done; ++spin) {
      done = arrived();
      if (!done && (spin & 0xfff) == 0xfff) {
        const long long now = steady_ns();
        if (t_first == 0) t_first = t_query = now;
        if (now - t_first > 10000000000LL) break;  // 10 s: let the stream say what happened
        if (now - t_query > 2000000) {
          t_query = now;
          if (hipStreamQuery(e->stream) == hipSuccess)
            done = true;  // stream drained: the records must be there (or the kernel died)
        }
      }
    }
    if (!done) HIP_TRY(hipStreamSynchronize(e->stream));
  } else {
    HIP_TRY(hipStreamSynchronize(e->stream));
  }
  if (!arrived()) {
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (!arrived()) return fail(FFN_ERR_HIP, "step %u did not complete", step_id);
  }
  if (n == 1) e->t_arrived_ns = steady_ns();
  {
    uint32_t* out = reinterpret_cast<uint32_t*>(results);
    for (int k = 0; k < n * kPubWords; ++k)
      out[k] = (uint32_t)__atomic_load_n(&h_pub[k], __ATOMIC_RELAXED);
  }
  for (int k = 0; k < n; ++k)
    if (results[k].range_error == 2) {
      if (spec_mismatch) {
        *spec_mismatch = true;
        return FFN_OK;
      }
      return fail(FFN_ERR_STATE,
                  "the speculative conv0_a launch of step %u chose another position "
                  "than the segment loop; the step changed nothing (speculate 0 "
                  "turns the launches off)", step_id);
    }
  bool any_void = false;
  for (int k = 0; k < n; ++k) any_void = any_void || results[k].range_error != 0;
  if (any_void) {
    bool timed_out = false;  // the cause is per step: two steps may be in flight
    for (int k = 0; k < n; ++k) timed_out = timed_out || results[k].range_error == 3;
    const int frc = flow_voided(e, timed_out);
    if (frc) return frc;
  } else {
    EngineLock lock_(e);
    if (e->slot_resident[slot]) e->flow_strikes = 0;
  }
  for (int k = 0; k < n; ++k)
    if (results[k].range_error)
      return fail(FFN_ERR_RANGE,
                  "an activation left the fp16 range (conv_variant >= 6): the "
                  "step changed nothing; set conv_variant -1 and repeat it");
  return FFN_OK;
}
}  // namespace

int ffn_canvas_step(ffn_engine* e, int n, ffn_canvas* const* canvases,
                    const ffn_step_request* requests,
                    const ffn_step_params* params, ffn_step_result* results) {
  if (!results) return fail(FFN_ERR_ARG, "null argument");
  uint32_t ticket = 0;
  int rc = ffn_canvas_step_submit(e, n, canvases, requests, params, &ticket);
  if (rc) return rc;
  bool mismatch = false;
  rc = step_wait_impl(e, ticket, results, &mismatch);
  if (rc || !mismatch) return rc;
  // The device's choice and the loop's differ (not expected: both apply
  // Canvas.is_valid_pos to the same values).  Nothing was pasted: the step is
  // made again, conv0_a included.
  {
    EngineLock lock_(e);
    e->stat_spec_mismatch += 1;
    drop_spec(e);
  }
  rc = ffn_canvas_step_submit(e, n, canvases, requests, params, &ticket);
  if (rc) return rc;
  return step_wait_impl(e, ticket, results, nullptr);
}

namespace {
// What the segment calls check per canvas; k: the canvas' index in a batched call, whose
// messages name it (-1: the call has one canvas).
int check_segment_params(const ffn_canvas* c, const ffn_segment_params& p, int resume, int k) {
  if (p.prefetch < 0 || p.prefetch > FFN_MAX_CANDIDATES)
    return fail(FFN_ERR_ARG, "prefetch must be 0..%d", FFN_MAX_CANDIDATES);
  if (p.shape_zyx[0] != c->cz || p.shape_zyx[1] != c->cy || p.shape_zyx[2] != c->cx)
    return k < 0 ? fail(FFN_ERR_ARG, "shape_zyx does not match the canvas")
                 : fail(FFN_ERR_ARG, "shape_zyx does not match canvas %d", k);
  for (int a = 0; a < 3; ++a)
    if (p.deltas_zyx[a] < 0 || p.margin_zyx[a] < 0)
      return fail(FFN_ERR_ARG, "negative deltas / margin");
  if (resume && !c->loop.active)
    return k < 0 ? fail(FFN_ERR_STATE, "no segment to resume")
                 : fail(FFN_ERR_STATE, "canvas %d: no segment to resume", k);
  return FFN_OK;
}

// the HIP canvas as the device of the host loop
struct HipLoopDevice {
  ffn_canvas* c;
  int step(const ffn_step_request& req, const ffn_step_params& params,
           ffn_step_result* res) {
    ffn_canvas* one = c;
    return ffn_canvas_step(c->engine, 1, &one, &req, &params, res);
  }
  int read_point(const int32_t pos[3], float* seed, int32_t* seg) {
    return ffn_canvas_read_points(c, 1, pos, seed, seg);
  }
  int turn(const ffn_turn_request& rq, const int32_t* cand, ffn_turn_result* out,
           int32_t max_overlaps, int32_t* ids, int64_t* counts, int32_t* flags,
           float* cand_seed, int32_t* cand_seg) {
    return ffn_canvas_segment_turn(c, &rq, cand, out, max_overlaps, ids, counts, flags,
                                   cand_seed, cand_seg);
  }
  // the positions the loop expects to pop after the step it is about to make
  void hint_next(int n, const int32_t (*pos)[3]) {
    EngineLock lock_(c->engine);
    c->hint_from_loop = true;
    c->hint_n = n < kSpecMax ? n : kSpecMax;
    for (int j = 0; j < c->hint_n; ++j)
      for (int a = 0; a < 3; ++a) c->hint_pos[j][a] = pos[j][a];
  }
};
}  // namespace

namespace {
// The step ffn_canvas_segment_many_carry left in flight: wait for it and hand its
// results to the loops of its canvases.  `only`: nothing to do unless that canvas
// is one of them.  Callers hold neither `mu` nor `many_mu`.
int resolve_many_carry_locked(ffn_engine* e) {
  if (!e->many_carry.active) return FFN_OK;
  HipLoopDevice dev{e->many_canvases.empty() ? nullptr : e->many_canvases[0]};
  auto wait = [&](ffn_step_result* res) {
    return step_wait_impl(e, e->many_ticket, res, nullptr);
  };
  const int rc = ffn_host::resolve_carry(&e->many_carry, dev, wait);
  e->many_canvases.clear();
  return rc;
}
}  // namespace

}  // extern "C"

// (declared in ffn_engine.h: the canvas calls of ffn_canvas.hip resolve it too)
int resolve_many_carry(ffn_engine* e, const ffn_canvas* only) {
  std::lock_guard<std::mutex> guard(e->many_mu);
  if (only && std::find(e->many_canvases.begin(), e->many_canvases.end(), only) ==
                  e->many_canvases.end())
    return FFN_OK;
  return resolve_many_carry_locked(e);
}

extern "C" {

int ffn_canvas_segment_at(ffn_canvas* c, const int32_t start[3],
                          const ffn_segment_params* p, int resume,
                          ffn_segment_result* out) {
  if (!c || !start || !p || !out) return fail(FFN_ERR_ARG, "null argument");
  if (!c->engine) return fail(FFN_ERR_STATE, "canvas outlived its engine");
  if (int rc = resolve_many_carry(c->engine, c)) return rc;
  if (int rc = check_segment_params(c, *p, resume, -1)) return rc;
  HipLoopDevice dev{c};
  ffn_host::SegmentLoop<HipLoopDevice> loop(dev, c->loop, *p);
  return loop.run(start, resume, out);
}

int ffn_canvas_segment_all(ffn_canvas* c, const ffn_seed_loop_args* a,
                           ffn_seed_loop_result* out) {
  if (!c || !a || !out) return fail(FFN_ERR_ARG, "null argument");
  if (!c->engine) return fail(FFN_ERR_STATE, "canvas outlived its engine");
  if (!ffn_host::seed_loop_args_ok(*a))
    return fail(FFN_ERR_ARG, "seed list, candidates, records or overlap arrays");
  if (int rc = resolve_many_carry(c->engine, c)) return rc;
  if (int rc = check_segment_params(c, a->segment, 0, -1)) return rc;
  if (a->resume && !(c->seed_loop.in_segment && c->loop.active))
    return fail(FFN_ERR_STATE, "no segment to resume");
  HipLoopDevice dev{c};
  ffn_host::SeedLoop<HipLoopDevice> loop(dev, c->loop, c->seed_loop, *a, out);
  return loop.run();
}

int ffn_canvas_segment_many(ffn_engine* e, int n, ffn_canvas* const* canvases,
                            const int32_t (*starts)[3],
                            const ffn_segment_params* params, const int32_t* resume,
                            ffn_segment_result* results, int32_t* finished) {
  return ffn_canvas_segment_many_carry(e, n, canvases, starts, params, resume, results,
                                       finished, 0);
}

int ffn_canvas_segment_many_carry(ffn_engine* e, int n, ffn_canvas* const* canvases,
                                  const int32_t (*starts)[3],
                                  const ffn_segment_params* params,
                                  const int32_t* resume, ffn_segment_result* results,
                                  int32_t* finished, int32_t carry) {
  if (!e || !canvases || !starts || !params || !resume || !results || !finished)
    return fail(FFN_ERR_ARG, "null argument");
  if (n < 1 || n > e->max_batch)
    return fail(FFN_ERR_ARG, "batch %d outside [1, %d]", n, e->max_batch);
  std::vector<HipLoopDevice> devs(n);
  std::vector<ffn_host::SegmentState*> states(n);
  for (int k = 0; k < n; ++k) {
    ffn_canvas* c = canvases[k];
    if (!c) return fail(FFN_ERR_ARG, "null canvas");
    if (c->engine != e) return fail(FFN_ERR_ARG, "canvas %d is not of this engine", k);
    for (int k2 = 0; k2 < k; ++k2)
      if (canvases[k2] == c) return fail(FFN_ERR_ARG, "canvas appears twice");
    const ffn_segment_params& p = params[k];
    if (int rc = check_segment_params(c, p, resume[k], k)) return rc;
    if (std::memcmp(&p.step, &params[0].step, sizeof(ffn_step_params)) != 0)
      return fail(FFN_ERR_ARG, "canvas %d: step parameters differ from canvas 0's", k);
    devs[k].c = c;
    states[k] = &c->loop;
  }
  std::vector<ffn_canvas*> batch(n);
  auto batch_step = [&](int nb, const int* idx, const ffn_step_request* reqs,
                        const ffn_step_params& sp, ffn_step_result* res) {
    for (int b = 0; b < nb; ++b) batch[b] = canvases[idx[b]];
    return ffn_canvas_step(e, nb, batch.data(), reqs, &sp, res);
  };
  // a step left in flight by the last call (of whichever kind) comes first; with
  // `carry` this call may leave one itself
  std::unique_lock<std::mutex> many_guard(e->many_mu);
  if (!carry) {
    const int rc = resolve_many_carry_locked(e);
    many_guard.unlock();
    if (rc) return rc;
    return ffn_host::segment_many(n, devs.data(), states.data(), starts, params,
                                  resume, results, finished, batch_step);
  }
  auto submit = [&](int nb, const int* idx, const ffn_step_request* reqs,
                    const ffn_step_params& sp) {
    for (int b = 0; b < nb; ++b) batch[b] = canvases[idx[b]];
    const int rc = ffn_canvas_step_submit(e, nb, batch.data(), reqs, &sp,
                                          &e->many_ticket);
    if (rc == FFN_OK) {
      e->many_canvases.assign(batch.begin(), batch.begin() + nb);
      e->stat_many_carried += 1;
    }
    return rc;
  };
  auto wait = [&](ffn_step_result* res) {
    const int rc = step_wait_impl(e, e->many_ticket, res, nullptr);
    e->many_canvases.clear();
    return rc;
  };
  return ffn_host::segment_many(n, devs.data(), states.data(), starts, params, resume,
                                results, finished, batch_step, &e->many_carry, submit,
                                wait);
}

}  // extern "C"
