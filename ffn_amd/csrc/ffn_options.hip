// libffn_hip.so -- the engine's options (one table), its profiler and its debug readers
// (ffn_engine.h).  Host code only: no kernel header is included and nothing is launched.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <map>

#include "ffn_engine.h"
#include "ffn_stack.h"

// Flush the per-launch event pairs recorded since the last flush.
int flush_events(ffn_engine* e) {
  if (e->events_used == 0) return FFN_OK;
  HIP_TRY(hipEventSynchronize(e->events[e->events_used - 1]));
  for (int k = 0; k + 1 < e->events_used; k += 2) {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e->events[k], e->events[k + 1]));
    e->conv_ms += ms;
    if (e->prof_samples.size() < (size_t)(1 << 16)) e->prof_samples.push_back(ms);
    if (e->prof_mode == 2 && !e->chain_launches_pending.empty()) {
      e->conv_launches += e->chain_launches_pending.front();
      e->chain_launches_pending.erase(e->chain_launches_pending.begin());
    } else {
      e->conv_launches += 1;
    }
  }
  e->events_used = 0;
  return FFN_OK;
}

namespace {

// ---- the options whose set is more than a field store ----

int set_conv_variant(ffn_engine* e, int value) {
  if (value == -1) value = e->caps.exact_variant;  // "the exact-f32 kernel of this FoV"
  if (value != 0 && value != 2 && !(value >= 6 && value <= 10))
    return fail(FFN_ERR_ARG, "conv_variant must be 0, 2, 6, 7, 8, 9 or 10 (1, 3, 4, 5 "
                             "were removed in ABI 7)");
  if (value == 10 && !e->h_ok)
    return fail(FFN_ERR_ARG, "conv_variant 10 unsupported for this fov / depth / device "
                             "(80-voxel workgroups, two per CU, all resident)");
  if (value >= 6 && e->weights_set && !e->fp16_ok)
    return fail(FFN_ERR_ARG, "conv_variant %d: a weight is outside the fp16 range",
                value);
  if (value == 6 && !e->caps.d_ok)
    return fail(FFN_ERR_ARG, "conv_variant 6 unsupported for this fov / depth");
  if (value == 7 && !e->caps.e_ok)
    return fail(FFN_ERR_ARG, "conv_variant 7 unsupported for this fov / depth");
  if (value == 8 && !e->caps.m_ok)
    return fail(FFN_ERR_ARG, "conv_variant 8 unsupported for this fov / depth");
  if (value == 9 && !e->caps.t_ok)
    return fail(FFN_ERR_ARG, "conv_variant 9 unsupported for this fov / depth "
                             "(257 .. 512 chunks of 128 voxels)");
  if (value >= 6 && e->weights_set && !e->d_weights_ok)
    return fail(FFN_ERR_ARG, "conv_variant 6: a weight x 2^11 is outside the fp16 range");
  if (value == 2 && !(e->caps.Rc == 256 || e->caps.Rc == 288))
    return fail(FFN_ERR_ARG, "conv_variant %d unsupported for this fov", value);
  return switch_variant(e, value);
}

// single-FoV steps of conv_variant 9: 0 one dependent launch per conv; 1 the same
// launches with the flagged hand-off compiled in; 2 the resident stack (conv32ps: one
// launch for all convs).  Same bits in every mode.
int set_flow(ffn_engine* e, int value) {
  if (value && !e->caps.t_ok)
    return fail(FFN_ERR_ARG, "flow needs conv32mt's geometry (conv_variant 9)");
  if (value && e->depth < 2) return fail(FFN_ERR_ARG, "flow needs depth >= 2");
  if (value == 2 && !e->flow_fits)
    return fail(FFN_ERR_ARG, "flow 2: this device cannot hold the resident launch's "
                "workgroups all at once (compute units x occupancy)");
  drop_spec(e);
  e->flow = value;
  e->flow_auto_off = 0;
  e->flow_strikes = 0;
  e->flow_skip = 0;
  return FFN_OK;
}

// MFMA products per fp16 operand pair in conv32m / conv32mt: 3 (the split product,
// f32-accurate) or 1 (hi x hi alone: fp16 inference).  Stored whatever the variant;
// plan_stack decides where it takes effect.
int set_mfma_products(ffn_engine* e, int value) {
  if (value != 1 && value != 3) return fail(FFN_ERR_ARG, "mfma_products must be 3 or 1");
  drop_spec(e);
  e->mfma_products = value;
  return FFN_OK;
}

int set_stat_reset(ffn_engine* e, int) {
  e->stat_spec_launched = e->stat_spec_hits = e->stat_spec_mismatch = 0;
  e->stat_ahead_used = e->stat_ahead_wasted = 0;
  e->stat_spec_miss_full = e->stat_spec_miss_short = 0;
  e->stat_segturn_queue_ns = e->stat_segturn_wait_ns = 0;
  e->stat_segturn_calls = 0;
  e->stat_calls = e->stat_items = 0;
  std::memset(e->stat_hist, 0, sizeof(e->stat_hist));
  e->stat_turn_host_ns = e->stat_launch_host_ns = 0;
  e->stat_turn_host_count = 0;
  e->stat_lab_launches = 0;
  e->t_arrived_ns = 0;
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  HIP_TRY(hipMemset(e->d_stamps, 0, 32 * sizeof(long long)));
  return FFN_OK;
}

// the N-th single-FoV step from now stamps when its launches' roles ran
// (ConvStackTab::stamps [4 .. 11]; read with debug_fused_stamp_K)
// (minima at +inf, maxima at 0 -- here, not in the stream of the traced step)
int set_debug_fused_trace(ffn_engine* e, int value) {
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  HIP_TRY(hipMemset(e->d_stamps + 4, 0x7f, 4 * sizeof(long long)));
  HIP_TRY(hipMemset(e->d_stamps + 8, 0, 4 * sizeof(long long)));
  HIP_TRY(hipMemset(e->d_stamps + 12, 0, 20 * sizeof(long long)));
  HIP_TRY(hipMemset(e->d_stamps + 32, 0, 1024 * sizeof(long long)));
  e->fused_trace_in = value;
  return FFN_OK;
}

// ---- the options whose get is more than a field read ----

int mean_ns(long long sum, long count) { return count ? (int)(sum / count) : 0; }

// device words as they are once everything queued on the engine's stream has run
int read_device_words(ffn_engine* e, void* dst, const void* src, size_t bytes) {
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
  return FFN_OK;
}

int get_stat_ahead_aborted(ffn_engine* e, const char*, int* value) {
  long long st[4] = {0, 0, 0, 0};
  if (int rc = read_device_words(e, st, e->d_stamps, sizeof(st))) return rc;
  *value = (int)st[3];
  return FFN_OK;
}

int get_stat_turn_gpu_ns(ffn_engine* e, const char*, int* value) {
  long long st[4] = {0, 0, 0, 0};
  if (int rc = read_device_words(e, st, e->d_stamps, sizeof(st))) return rc;
  *value = st[2] ? (int)(st[1] * 10 / st[2]) : 0;
  return FFN_OK;
}

int get_stat_flow_timeouts(ffn_engine* e, const char*, int* value) {
  unsigned v = 0;
  if (int rc = read_device_words(e, &v, e->flow_err, sizeof(v))) return rc;
  *value = (int)v;
  return FFN_OK;
}

// debug_fused_stamp_<k>: stamp k (4 .. 11) minus the stack's first entry [7], in 10-ns ticks
int get_debug_fused_stamp(ffn_engine* e, const char* rest, int* value) {
  const int k = std::atoi(rest);
  long long st[32 + 1024];
  if (int rc = read_device_words(e, st, e->d_stamps, sizeof(st))) return rc;
  for (int w = 0; w < 512; ++w) st[25] = std::max(st[25], st[32 + w]);  // (per-workgroup ends)
  {  // [27]: main workgroups that share their CU with another main workgroup
    std::map<unsigned, int> per_cu;
    for (int w = 0; w < 512; ++w) {
      const unsigned v = (unsigned)st[32 + 512 + w];
      if (st[32 + 512 + w] != 0 && ((v - 1) >> 31)) per_cu[(v - 1) & 0x7fffffffu] += 1;
    }
    long long shared = 0;
    for (const auto& kv : per_cu) if (kv.second > 1) shared += kv.second;
    st[27] = st[4] + shared;  // (the getter subtracts the origin)
    if (!e->stack_ahead) st[27] = st[7] + shared;
  }
  if (k < 4 || k > 27 || k == 15) return fail(FFN_ERR_ARG, "debug_fused_stamp_4 .. 27");
  // (stack_ahead: the stack inside the traced window is the NEXT step's; the fused
  // launch's first faces entry [4] is the origin then)
  *value = (int)(st[k] - (e->stack_ahead ? st[4] : st[7]));
  return FFN_OK;
}

// stat_hist_<k>: step calls with k FoVs (64: that many or more) since the last stat_reset
int get_stat_hist(ffn_engine* e, const char* rest, int* value) {
  const int k = std::atoi(rest);
  if (k < 0 || k > 64) return fail(FFN_ERR_ARG, "stat_hist_<0..64>");
  *value = (int)e->stat_hist[k];
  return FFN_OK;
}

// ---- the table: one row per option name ----
// A set checks [lo, hi] (lo < hi: a ranged row), calls drop_spec where the row says so,
// then calls `set` or stores into `field` (value != 0 for an on / off row); a get calls
// `get` or reads `field` / `counter`.  A row without that side is unknown to it, as a
// name without a row is.  What each option does: include/ffn_hip.h, ffn_hip_debug.h.
enum : unsigned { kOnOff = 1, kDrop = 2, kReadOnly = 4, kPrefix = 8 };
using E = ffn_engine;
struct Option {
  const char* name;
  int E::*field;  // a plain int field, or NULL
  int lo, hi;
  unsigned flags;
  int (*set)(E* e, int value);
  int (*get)(E* e, const char* rest, int* value);  // rest: what follows a kPrefix name
  long E::*counter;  // a counter: read only
};
constexpr Option counter(const char* name, long E::*c) {
  return {name, nullptr, 0, 0, 0, nullptr, nullptr, c};
}
constexpr Option derived(const char* name, int (*get)(E*, const char*, int*),
                         unsigned flags = 0) {
  return {name, nullptr, 0, 0, flags, nullptr, get, nullptr};
}
#define FFN_GET(EXPR) [](E* e, const char*, int* value) { *value = (EXPR); return (int)FFN_OK; }

const Option kOptions[] = {
    // what a user sets
    {"conv_variant", &E::conv_variant, 0, 0, 0, set_conv_variant},
    {"flow", &E::flow, 0, 2, 0, set_flow},
    {"batch_chunks", &E::batch_chunks, 0, 2},
    {"tail_batched", &E::tail_batched, 0, 0, kOnOff},
    {"mfma_products", &E::mfma_products, 0, 0, 0, set_mfma_products},
    {"speculate", &E::speculate, 0, 0, kOnOff | kDrop},
    {"stack_ahead", &E::stack_ahead, 0, 0, kOnOff | kDrop},
    {"sync_mode", &E::sync_mode, 0, 1},
    {"profile_every", &E::prof_every, 1, INT_MAX},
    {"store_policy", &E::store_policy, 0, 2},
    {"fuse_head", &E::fuse_head, 0, 0, kOnOff},
    {"fuse_paste", &E::fuse_paste, 0, 0, kOnOff},
    {"fuse_conv0a", &E::fuse_conv0a, 0, 0, kOnOff | kDrop},
    derived("exact_variant", FFN_GET(e->caps.exact_variant)),
    {"flow_auto_off", &E::flow_auto_off, 0, 0, kReadOnly},
    // the lab: pacing, ablation, tracing
    {"paste_blocks", &E::paste_blocks, 0, 1024},
    {"flow_pace", &E::flow_pace, -1, 5000},
    {"flow_pace_spread", &E::flow_pace_spread, -1, 5000},
    {"flow_pace_tail", &E::flow_pace_tail, 0, 5000},
    derived("flow_pace_now", FFN_GET(e->flow_pace < 0 ? e->pace_auto : e->flow_pace)),
    derived("flow_pace_free_ns", FFN_GET((int)(e->pace_auto_us[0] * 1e3f))),
    derived("flow_pace_best_ns", FFN_GET((int)(e->pace_auto_us[1] * 1e3f))),
    {"flow_lab", &E::flow_lab, 0, 1},
    {"flow_debug", &E::flow_debug},
    {"debug_clock", &E::dbg_clock},
    {"debug_layer", &E::dbg_layer},
    {"ablate", &E::ablate},
    {"spec_force_mismatch", &E::spec_force_mismatch},
    {"debug_fused_twice", &E::debug_fused_twice},
    {"debug_submit_delay_ns", &E::debug_submit_delay_ns},
    {"debug_fused_trace", nullptr, 0, 0, 0, set_debug_fused_trace},
    derived("debug_fused_stamp_", get_debug_fused_stamp, kPrefix),
    // counters since the last stat_reset
    {"stat_reset", nullptr, 0, 0, 0, set_stat_reset},
    counter("stat_step_calls", &E::stat_calls),
    counter("stat_step_items", &E::stat_items),
    derived("stat_hist_", get_stat_hist, kPrefix),
    counter("stat_spec_launched", &E::stat_spec_launched),
    counter("stat_spec_hits", &E::stat_spec_hits),
    counter("stat_spec_mismatch", &E::stat_spec_mismatch),
    counter("stat_spec_miss_full", &E::stat_spec_miss_full),
    counter("stat_spec_miss_short", &E::stat_spec_miss_short),
    counter("stat_ahead_used", &E::stat_ahead_used),
    counter("stat_ahead_wasted", &E::stat_ahead_wasted),
    derived("stat_ahead_aborted", get_stat_ahead_aborted),
    counter("stat_many_carried", &E::stat_many_carried),
    counter("stat_flow_voids", &E::stat_flow_voids),
    derived("stat_flow_timeouts", get_stat_flow_timeouts),
    counter("stat_lab_launches", &E::stat_lab_launches),
    counter("stat_segturn_calls", &E::stat_segturn_calls),
    derived("stat_segturn_queue_ns",
            FFN_GET(mean_ns(e->stat_segturn_queue_ns, e->stat_segturn_calls))),
    derived("stat_segturn_wait_ns",
            FFN_GET(mean_ns(e->stat_segturn_wait_ns, e->stat_segturn_calls))),
    counter("stat_turn_count", &E::stat_turn_host_count),
    derived("stat_turn_host_ns", FFN_GET(mean_ns(e->stat_turn_host_ns, e->stat_turn_host_count))),
    derived("stat_launch_host_ns",
            FFN_GET(mean_ns(e->stat_launch_host_ns, e->stat_turn_host_count))),
    derived("stat_turn_gpu_ns", get_stat_turn_gpu_ns),
};
#undef FFN_GET

// the row of `name`, and what follows the row's name in it
const Option* find_option(const char* name, const char** rest) {
  for (const Option& o : kOptions) {
    const size_t len = std::strlen(o.name);
    if (o.flags & kPrefix ? std::strncmp(name, o.name, len) == 0 : std::strcmp(name, o.name) == 0) {
      *rest = name + len;
      return &o;
    }
  }
  return nullptr;
}

}  // namespace

extern "C" {

int ffn_engine_set_option(ffn_engine* e, const char* name, int value) {
  EngineLock lock_(e);
  if (!e || !name) return fail(FFN_ERR_ARG, "null argument");
  const char* rest = nullptr;
  const Option* o = find_option(name, &rest);
  if (!o || !(o->set || (o->field && !(o->flags & kReadOnly))))
    return fail(FFN_ERR_ARG, "unknown option '%s'", name);
  if (o->lo < o->hi && (value < o->lo || value > o->hi))
    return fail(FFN_ERR_ARG, "%s: %d..%d", o->name, o->lo, o->hi);
  if (o->flags & kDrop) drop_spec(e);
  if (o->set) return o->set(e, value);
  e->*(o->field) = o->flags & kOnOff ? value != 0 : value;
  return FFN_OK;
}

int ffn_engine_get_option(ffn_engine* e, const char* name, int* value) {
  EngineLock lock_(e);
  if (!e || !name || !value) return fail(FFN_ERR_ARG, "null argument");
  const char* rest = nullptr;
  const Option* o = find_option(name, &rest);
  if (o && o->get) return o->get(e, rest, value);
  if (o && o->field) *value = e->*(o->field);
  else if (o && o->counter) *value = (int)(e->*(o->counter));
  else return fail(FFN_ERR_ARG, "unknown option '%s'", name);
  return FFN_OK;
}

int ffn_engine_debug_flow_trace(ffn_engine* e, long long* out, int max_slots) {
  EngineLock lock_(e);
  if (!e || !out) return fail(FFN_ERR_ARG, "null argument");
  if (!e->flow_trace) return fail(FFN_ERR_ARG, "no flow trace on this engine (conv_variant 9)");
  if (max_slots < 0 || max_slots > e->flow_trace_slots)
    return fail(FFN_ERR_ARG, "max_slots must be 0..%d", e->flow_trace_slots);
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  const size_t row = (size_t)kFlowTraceLayers * 8 * sizeof(long long);
  HIP_TRY(hipMemcpy(out, e->flow_trace, row * max_slots, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemset(e->flow_trace, 0, row * e->flow_trace_slots));
  return FFN_OK;
}

int ffn_engine_debug_workgroups(ffn_engine* e, long long* out, int max_wgs) {
  EngineLock lock_(e);
  if (!e || !out) return fail(FFN_ERR_ARG, "null argument");
  if (max_wgs < 0 || max_wgs > kDbgMaxWgs)
    return fail(FFN_ERR_ARG, "max_wgs must be 0..%d", kDbgMaxWgs);
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  HIP_TRY(hipMemcpy(out, e->d_dbg + 24, (size_t)4 * max_wgs * sizeof(long long),
                    hipMemcpyDeviceToHost));
  // the next run starts from zeros (a workgroup that did not run leaves them)
  HIP_TRY(hipMemset(e->d_dbg + 24, 0, (size_t)4 * kDbgMaxWgs * sizeof(long long)));
  return FFN_OK;
}

int ffn_engine_debug_clocks(ffn_engine* e, long long* out24) {
  EngineLock lock_(e);
  if (!e || !out24) return fail(FFN_ERR_ARG, "null argument");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  HIP_TRY(hipMemcpy(out24, e->d_dbg, 24 * sizeof(long long), hipMemcpyDeviceToHost));
  return FFN_OK;
}

int ffn_engine_synchronize(ffn_engine* e) {
  EngineLock lock_(e);
  if (!e) return fail(FFN_ERR_ARG, "null argument");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return FFN_OK;
}

int ffn_engine_set_profiling(ffn_engine* e, int mode) {
  EngineLock lock_(e);
  if (!e) return fail(FFN_ERR_ARG, "null argument");
  if (mode < 0 || mode > 2) return fail(FFN_ERR_ARG, "mode must be 0, 1 or 2");
  HIP_TRY(hipSetDevice(e->device));
  int rc = flush_events(e);
  if (rc) return rc;
  e->chain_launches_pending.clear();
  e->prof_mode = mode;
  return FFN_OK;
}

int ffn_engine_get_profile(ffn_engine* e, double* conv_ms_total,
                           int64_t* conv_launches, int reset) {
  EngineLock lock_(e);
  if (!e) return fail(FFN_ERR_ARG, "null argument");
  HIP_TRY(hipSetDevice(e->device));
  int rc = flush_events(e);
  if (rc) return rc;
  if (conv_ms_total) *conv_ms_total = e->conv_ms;
  if (conv_launches) *conv_launches = e->conv_launches;
  if (reset) {
    e->conv_ms = 0.0;
    e->conv_launches = 0;
    e->prof_samples.clear();
  }
  return FFN_OK;
}

int ffn_engine_get_profile_samples(ffn_engine* e, float* out_ms, int max_n, int* n) {
  EngineLock lock_(e);
  if (!e || !n || (max_n > 0 && !out_ms)) return fail(FFN_ERR_ARG, "null argument");
  HIP_TRY(hipSetDevice(e->device));
  int rc = flush_events(e);
  if (rc) return rc;
  const int k = (int)std::min<size_t>(e->prof_samples.size(), (size_t)std::max(max_n, 0));
  for (int i = 0; i < k; ++i) out_ms[i] = e->prof_samples[i];
  *n = (int)e->prof_samples.size();
  return FFN_OK;
}

}  // extern "C"
