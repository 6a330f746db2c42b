// The engine and the canvas as the engine's own translation units see them (not part
// of the C-ABI, no kernel in here):
//   ffn_hip.hip      the engine, the FoV step, the segment loop
//   ffn_stack*.hip   the conv launch layer (ffn_stack.h): run_stack and the kernel families
//   ffn_canvas.hip   everything a canvas does between steps
//   ffn_options.hip  options, profiler, debug readers (host code only)
// A helper that more than one of them calls is declared here and defined once.
// Which conv kernel family runs a stack, and the arithmetic on the FoV that decides it:
// ffn_stack_plan.h (host only, no HIP; ffn_engine::caps).
#ifndef FFN_ENGINE_H_
#define FFN_ENGINE_H_

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <mutex>
#include <vector>

#include "ffn_internal.h"
#include "ffn_types.h"
#include "ffn_stack_plan.h"
#include "ffn_host_loop.h"

using namespace ffn;

// ffn_set_error (ffn_internal.h) under the short name these units use
__attribute__((format(printf, 2, 3))) inline int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  return ffn_set_error(code, "%s", buf);
}

#define HIP_TRY(expr)                                                        \
  do {                                                                       \
    hipError_t _e = (expr);                                                  \
    if (_e != hipSuccess)                                                    \
      return fail(FFN_ERR_HIP, "%s failed: %s (%s:%d)", #expr,               \
                  hipGetErrorString(_e), __FILE__, __LINE__);                \
  } while (0)

constexpr int kDbgLayerDefault = 3;  // engine option debug_layer as an engine starts

struct ffn_engine {
  // Entry points may be called from several host threads (the two canvas groups
  // of MultiCanvasDriver, their between-segment work): each one holds this lock
  // while it touches engine state or queues work on the stream -- except the
  // wait for a step's completion flags, which is what the threads overlap.
  std::recursive_mutex mu;
  // The canvas utility calls (point / box reads and writes, commit counts) own
  // the scratch buffers and WAIT for their result; they hold `util_mu` for all
  // of it but `mu` only while they queue their work, and wait for their own
  // event, not for the stream -- so another thread's next FoV step is queued
  // (and runs) behind them instead of waiting for the host to wake up.
  std::mutex util_mu;
  // They run on their OWN stream: a canvas between two segments is in no step,
  // so what is committed / read / re-seeded on it must not queue behind the FoV
  // steps other canvases have in flight (2 ms each at batch 16).  Ordering
  // per canvas: the step side waits for the canvas' last utility event
  // (ffn_canvas::ev_util) before its next step; the utility side starts after
  // the canvas' last step has pasted -- batched steps paste BEFORE the faces
  // kernel raises the completion flag the host waits for, a single-FoV step
  // (faces first: the host's turn-around is on its critical path) makes the
  // utility stream wait for an event recorded behind it.
  hipStream_t ustream = nullptr;
  hipEvent_t main_ev = nullptr;  // "everything queued on `stream` so far"
  // ffn_canvas_segment_many_carry: the batched step it left in flight when it
  // returned (one per engine: the driver that runs ONE group of canvases and
  // does a canvas' between-segment work under the others' next step).  `many_mu`
  // is taken before `mu`, never the other way round.
  std::mutex many_mu;
  ffn_host::ManyCarry many_carry;
  uint32_t many_ticket = 0;
  std::vector<ffn_canvas*> many_canvases;  // the carried step's, in batch order
  int device = 0;
  hipStream_t stream = nullptr;
  Geom g{};   // the FoV as the caller sees it (zyx): gather / paste / faces, I/O
  // what the FoV's geometry fixes for the conv kernels (ffn_stack_plan.h): the layout
  // of the split-product family (caps.gp), chunk counts, LDS sizes, which families
  // the FoV admits, the tap schedules
  ConvCaps caps;
  int depth = 0;
  int max_batch = 0;
  bool weights_set = false;

  float* act_base = nullptr;  // 2 activation buffers (T, X) x max_batch
  float* bufT = nullptr;      // logical origins
  float* bufX = nullptr;
  uint32_t* validbits = nullptr;
  int32_t* pidx = nullptr;    // dense FoV index -> padded position (variant 2)
  int fuse_head = 1;      // 1x1x1 head fused into the last conv32c launch
  int count_blocks = kHeadBlocks;  // entries per item in `count` for the last step
  int store_policy = 1;  // conv32c epilogue stores: sc1 write-through (-1.4 % per stack)
  long long* d_dbg = nullptr;  // debug clocks of conv32c WG 0 (24 values)
  int dbg_clock = 0;
  int dbg_layer = kDbgLayerDefault;  // the launch whose clocks are recorded (3 = a conv_a)
  // rawT / rawX / rawS: the three activation allocations
  float* rawT = nullptr;
  float* rawX = nullptr;
  float* rawS = nullptr;
  int batch_chunks = 1;   // option: variant 6 uses the 96-voxel form for n >= 2
  int tail_batched = 0;   // option: steps with >= 2 FoVs take conv32mt's tail form too
  int mfma_products = 3;  // option: 1 = conv32m / conv32mt keep the hi x hi product alone
  // FLOW (ffn_conv_split.h "flagged launches"): 0 off; 1 conv32mt's launches with
  // the flagged hand-off compiled in (still one dependent launch per conv: the
  // words are always there already -- isolates the cost of the sc1 reads and
  // the poll); 2 the resident stack, conv32ps: ONE launch for the 2 depth - 1 convs
  // of a single-FoV step
  int flow = 0;
  unsigned* flow_flags = nullptr;  // one word per producer workgroup, kFlowStride apart
  unsigned* flow_err = nullptr;    // polls that gave up, ever
  unsigned flow_epoch = 0;         // sequence number of the last conv queued
  int flow_debug = 0;              // debug option: ConvDArgs::flow_dbg
  // The resident stack and the fused step launch exist twice: the production form, and the
  // LAB form that carries the lab's plumbing (debug_clock, debug_layer, flow_debug,
  // debug_fused_trace, the flow trace).  flow_lab 0: the LAB form where one of those is on
  // (lab_wanted, ffn_stack_resident.hip); 1: always.
  int flow_lab = 0;
  long stat_lab_launches = 0;      // resident stacks queued in the LAB form
  // The resident launch needs every one of its workgroups on the chip at once.
  // flow_fits: the device can hold them (CU count x occupancy, checked at create);
  // at run time a poll that gives up voids the step (FFN_ERR_FLOW): the repeat
  // runs per-layer launches (flow_skip, one stack), and kFlowStrikes voided
  // resident steps in a row turn the resident launch off for this engine
  // (flow_auto_off; option "flow" turns it on again).
  bool flow_fits = false;
  int flow_strikes = 0;            // voided resident steps since the last good one
  int flow_skip = 0;               // the next single-FoV stack runs per-layer launches
  int flow_auto_off = 0;
  long stat_flow_voids = 0;
  bool last_stack_resident = false;  // what run_stack queued last
  bool slot_resident[2] = {false, false};
  long long* flow_trace = nullptr; // debug_clock 4: ConvDArgs::flow_trace
  int flow_trace_slots = 0;
  bool d_weights_ok = true;      // every |weight| x 2^11 inside the fp16 range
  uint16_t* wpackd = nullptr;    // [28][khalf][plane hi, res][64][8] fp16 per layer
  size_t wpackd_layer = 0;       // halves per layer
  // conv32h / conv32hs (variant 10): 80-voxel workgroups on 16x16x32 tiles, two
  // hand-off chains per SIMD for a single FoV; several FoVs run conv32m as under 9
  uint16_t* wpackh = nullptr;    // [28][out half][plane hi, res][64][8] fp16 per layer
  bool h_ok = false;             // geometry (caps.h_geom_ok) + residency
  // Pacing of the resident stack (ConvStackTab::pace, 10-ns ticks between two convs of a
  // workgroup).  flow_pace: -1 = the beat measured by tune_pace() when the weights were
  // set (conv_variant 9; 0 if no beat beat the free-running stack), 0 = off, > 0 = that
  // beat.  flow_pace_spread: -1 = as wide as the beat (the FoV's last voxel one beat behind
  // its first), else ticks.
  int flow_pace = -1;
  int flow_pace_tail = 0;        // ConvStackTab::pace_tail
  int flow_pace_spread = -1;
  int pace_auto = 0;             // tune_pace()'s beat (0: none)
  float pace_auto_us[2] = {0.f, 0.f};  // us per stack it measured: free-running, at the beat
  int cus = 0;                   // compute units of the device
  unsigned* range_flag = nullptr;  // device word: tag of the last void run
  // Speculative conv0_a of a single-FoV step's successor (SpecArgs): the launch
  // queued behind the last step's paste, and what a step must match to run on it
  struct Spec {
    bool valid = false;
    const ffn_canvas* canvas = nullptr;
    int n = 0;
    int pos[kSpecMax][3] = {};
    float pad_value = 0.f, move_thr = 0.f;
    int variant = 0;
  } spec;
  int speculate = 1;        // option
  int spec_force_mismatch = 0;  // debug option: fail the next N matches
  long stat_spec_mismatch = 0;
  long stat_many_carried = 0;  // batched steps left in flight across a return
  int fuse_paste = 1;       // option: faces + paste of a single FoV as one launch
  int fuse_conv0a = 1;      // option: ... and the next step's conv0_a in it as well
  int* d_spec_choice = nullptr;
  long stat_spec_launched = 0, stat_spec_hits = 0;
  long stat_spec_miss_full = 0, stat_spec_miss_short = 0;
  // ffn_canvas_segment_turn on the host: queueing its sequence, waiting for its record
  long long stat_segturn_queue_ns = 0, stat_segturn_wait_ns = 0;
  long stat_segturn_calls = 0;
  // The NEXT step's resident stack queued right behind the launch that holds its
  // speculative conv0_a, before the host has seen this step's record (engine option
  // stack_ahead): the stack reads only what that conv0_a wrote (and gives up after its
  // first conv when the device found no valid position), so the host's turn-around and
  // the launch latency of the stack leave the step's critical path.
  int stack_ahead = 1;
  int paste_blocks = 0;  // fused step launch: paste blocks (0: one block per CU, see kPasteBlocks)
  int debug_submit_delay_ns = 0;
  int debug_fused_twice = 0;  // experiment: the host idles this long in front of a step's launches
  bool trace_now = false;     // debug_fused_trace: the launches being queued stamp
  bool ahead_valid = false;   // such a stack is in the stream, for the step e->spec describes
  long stat_ahead_used = 0, stat_ahead_wasted = 0;
  unsigned range_tag = 0;        // tag of the run being queued
  bool fp16_ok = true;           // every weight inside the fp16 range
  int conv_variant = 0;       // 0 conv32 (any FoV), 2 conv32c (exact f32), 6 conv32d, 7 = 6
                              // with 96-voxel chunks, 8 conv32m, 9 conv32mt (+ conv32m)
  float* h_io = nullptr;      // pinned staging of ffn_predict: seed, image, logits
  float* up_image = nullptr;  // dense FoVs uploaded by ffn_predict
  float* up_seed = nullptr;
  float* seed_raw = nullptr;  // raw (NaN-preserving) seed FoV of the current step
  // The conv0_a of the NEXT step may run in the same launch as this step's faces
  // and paste (faces_paste_conv0a_kernel): what it writes -- the raw seed copy,
  // a range flag, the position it chose -- goes to the OTHER of two sets, which
  // run_stack makes the current one when that step is queued.
  float* seed_raw_alt = nullptr;
  unsigned* range_flag_alt = nullptr;
  int* d_spec_choice_alt = nullptr;
  float* logits = nullptr;
  unsigned* count = nullptr;
  uint8_t* valid = nullptr;
  float* weights = nullptr;  // one allocation; layout below
  size_t w0a_off = 0, b0a_off = 0, wl_off = 0;
  size_t w0ap_off = 0;  // conv0_a weights with the taps in gp's axis order
  std::vector<size_t> wpack_off, bias_off;  // 2*depth-1 entries (conv0_b ..)

  StepItem* d_items = nullptr;
  StepItem* h_items = nullptr;
  // pinned, written by the faces block: kPubWords 8-byte words per item and slot,
  // (step number << 32) | one 32-bit word of the item's ffn_step_result
  unsigned long long* h_pub = nullptr;
  unsigned step_id = 0;
  // two result / descriptor slots: one step may be queued behind the running one
  int next_slot = 0;
  int slot_n[2] = {0, 0};
  bool slot_waited[2] = {false, false};  // a thread is in ffn_canvas_step_wait for it
  unsigned slot_ticket[2] = {0, 0};
  std::vector<ffn_canvas*> slot_canvas[2];
  int sync_mode = 1;  // 0 = hipStreamSynchronize, 1 = poll h_pub (then sync)
  // since the last set_option("stat_reset"): batched step calls, FoVs in them,
  // and a histogram of FoVs per call (index min(n, 64))
  long stat_calls = 0, stat_items = 0;
  long stat_hist[65] = {};
  // the turn-around between two single-FoV steps: the GPU's view (d_stamps, see
  // ConvStackTab::stamps) and the host's (steady-clock ns from "record arrived" to
  // "the next resident launch is queued", and inside that hipLaunchKernelGGL alone)
  long long* d_stamps = nullptr;
  long long t_arrived_ns = 0;
  int fused_trace_in = 0;        // debug_fused_trace: steps until the traced one
  long long stat_turn_host_ns = 0, stat_launch_host_ns = 0;
  long stat_turn_host_count = 0;

  void* d_scratch = nullptr;
  void* h_scratch = nullptr;
  size_t scratch_bytes = 0;

  // The segment turn's own scratch (ffn_canvas_segment_turn, ffn_canvas_commit_count;
  // under util_mu, on the utility stream).  d_turn: [TurnRecord][partials: kTurnBlocks
  // pairs][flags, seed, seg: 4 bytes, voxel index: 8 bytes, turn_ncap each][histogram:
  // turn_hcap words].  The histogram is zeroed when it is allocated and every turn's
  // last kernel leaves it zero again (turn_hist_clean: false while a turn is under way
  // or after one that failed -- the next one zeroes it first).  h_turn: pinned and
  // device-mapped, 8-byte words: [candidates, 3 turn_ncap int32][published: 8 +
  // 3 turn_ncap + 2 turn_ocap words, upper half = turn_seq of the turn that wrote it].
  void* d_turn = nullptr;
  unsigned long long* h_turn = nullptr;
  unsigned long long* h_turn_dev = nullptr;  // h_turn as the device addresses it
  size_t turn_ncap = 0, turn_hcap = 0, turn_ocap = 0;
  bool turn_hist_clean = false;
  unsigned turn_seq = 0;

  int prof_mode = 0;
  std::vector<hipEvent_t> events;
  int events_used = 0;
  // the event pair around a stack queued AHEAD (stack_ahead): it joins the samples when the
  // stack is used by its step -- one that found no position to run at ends after its first
  // conv, and its ~10 us would pass for a stack's duration
  hipEvent_t ahead_ev[2] = {nullptr, nullptr};
  bool ahead_ev_pending = false;
  double conv_ms = 0.0;
  int64_t conv_launches = 0;
  std::vector<ffn_canvas*> canvases;  // live canvases created from this engine
  int prof_every = 1;                 // profile 1 of every N run_stack calls
  long stack_calls = 0;
  bool prof_now = false;
  int ablate = 0;                     // debug: skip phases of the conv kernel
  std::vector<int> chain_launches_pending;  // mode 2: launches per event pair
  std::vector<float> prof_samples;  // ms of every event pair since the last reset
};

struct ffn_canvas {
  ffn_engine* engine = nullptr;
  float* image = nullptr;        // f32 image; NULL for a uint8 canvas
  uint8_t* image_u8 = nullptr;   // uint8 canvas: raw image (1 B / voxel) ...
  float* image_lut = nullptr;    // ... and (v - mean) / stddev for v = 0..255
  float* seed = nullptr;
  int32_t* seg = nullptr;
  int cz = 0, cy = 0, cx = 0;
  size_t nvox = 0;
  // Bounding box of every seed voxel that may differ from NaN since the last
  // clear: Canvas.init_seed (inference.py:443-450) clears the WHOLE volume per
  // seed (62.5 MB at 250^3, 4.3 GB at 1024^3); here only this box is re-filled.
  int dirty_lo[3] = {0, 0, 0};
  int dirty_hi[3] = {0, 0, 0};  // exclusive; lo >= hi: nothing dirty
  ffn_host::SegmentState loop;  // ffn_canvas_segment_at's queue / visited set
  ffn_host::SeedLoopState seed_loop;  // ffn_canvas_segment_all's interrupted segment
  hipEvent_t ev_util = nullptr;  // behind the last utility operation on this canvas
  bool util_pending = false;     // ... which the next step has to wait for
  bool paste_after_flag = false; // the last step pasted AFTER raising its flag
  // the segment loop's guess of the positions the step after the next one may
  // be made at (consumed by the next single-FoV ffn_canvas_step_submit)
  int hint_n = 0;
  int hint_pos[kSpecMax][3] = {};
  bool hint_from_loop = false;  // the next step is the segment loop's own
  // MovementRestrictor (ffn_canvas_set_restrictor): [pos plane][seed plane] of
  // restrict_plane_words 64-bit words each (ffn_restrict_kernels.h); NULL: none.
  // The host loop reads its copy of the pos plane (restrict_host).
  unsigned long long* restrict_planes = nullptr;
  size_t restrict_plane_words = 0;
  int restrict_row_words = 0;
  std::vector<uint64_t> restrict_host;

  void mark_dirty(const int lo[3], const int hi[3]) {
    const int dims[3] = {cz, cy, cx};
    const bool empty = dirty_lo[0] >= dirty_hi[0];
    for (int k = 0; k < 3; ++k) {
      const int l = std::max(lo[k], 0), h = std::min(hi[k], dims[k]);
      dirty_lo[k] = empty ? l : std::min(dirty_lo[k], l);
      dirty_hi[k] = empty ? h : std::max(dirty_hi[k], h);
    }
  }
};

inline long long steady_ns() {
  return std::chrono::duration_cast<std::chrono::nanoseconds>(
             std::chrono::steady_clock::now().time_since_epoch()).count();
}
inline unsigned next_tag(unsigned t) { return t + 1 ? t + 1 : 1; }  // never 0
// A speculative conv0_a launch that no step will use: its range tag is spent.
inline void drop_spec(ffn_engine* e) {
  if (e->spec.valid && !e->ahead_valid) e->range_tag = next_tag(e->range_tag);
  // (a stack queued ahead has taken the tag already: run_stack)
  if (e->ahead_valid) e->stat_ahead_wasted += 1;
  e->spec.valid = false;
  e->ahead_valid = false;
}
struct EngineLock {
  std::unique_lock<std::recursive_mutex> lk;
  explicit EngineLock(ffn_engine* e) {
    if (e) lk = std::unique_lock<std::recursive_mutex>(e->mu);
  }
};

// util_mu, then mu (the step path takes only mu: no lock-order inversion)
struct UtilLock {
  std::unique_lock<std::mutex> ul;
  std::unique_lock<std::recursive_mutex> lk;
  explicit UtilLock(ffn_engine* e) {
    if (e) {
      ul = std::unique_lock<std::mutex>(e->util_mu);
      lk = std::unique_lock<std::recursive_mutex>(e->mu);
    }
  }
  // Before the first utility operation of a call: the canvas' last step has
  // pasted (see ffn_engine::ustream).
  // reads_only: the call looks at the canvas and changes nothing -- a speculative conv0_a
  // (and the stack queued behind it) stays what it is; the segment loop's own point reads
  // between two steps used to cost it its launch (0.5 % of the steps: a whole stack run for
  // nothing + a step made the ordinary way)
  hipError_t begin(ffn_engine* e, ffn_canvas* c, bool reads_only = false) {
    if (!reads_only) drop_spec(e);  // the canvas may change under a speculative conv0_a
    if (!c->paste_after_flag) return hipSuccess;
    hipError_t err = hipEventRecord(e->main_ev, e->stream);
    if (err == hipSuccess) err = hipStreamWaitEvent(e->ustream, e->main_ev, 0);
    if (err == hipSuccess) c->paste_after_flag = false;
    return err;
  }
  // After the last one: mark the point the canvas' next step waits for ...
  hipError_t end(ffn_engine* e, ffn_canvas* c) {
    c->util_pending = true;
    return hipEventRecord(c->ev_util, e->ustream);
  }
  // ... and, for calls that return data, wait for it (`mu` released meanwhile)
  hipError_t wait(ffn_engine* e, ffn_canvas* c) {
    hipError_t err = end(e, c);
    if (err != hipSuccess) return err;
    lk.unlock();
    err = hipEventSynchronize(c->ev_util);
    lk.lock();
    if (err == hipSuccess) c->util_pending = false;  // done: nothing to wait for
    return err;
  }
  // ... or, where the call's last kernel publishes what the call returns into pinned
  // memory (turn_publish_kernel), poll for it instead of blocking on the stream (`mu`
  // released meanwhile).  arrived(): every published word carries this call's number.
  // Bounded, and as ffn_canvas_step_wait polls: no hipStreamQuery in the loop (on a busy
  // stream it puts a barrier packet into the queue), the stream is asked only after 2 ms
  // without the record, then every 2 ms, so that a device fault still surfaces as an error.
  // That last kernel runs behind everything the call queued, so the canvas is left as a
  // completed wait() leaves it: nothing pending, and ev_util -- not recorded again here --
  // complete, since whatever recorded it last ran earlier on the same stream.
  template <typename Arrived>
  hipError_t wait_published(ffn_engine* e, ffn_canvas* c, Arrived arrived) {
    if (e->sync_mode != 1) {
      const hipError_t err = wait(e, c);
      if (err != hipSuccess) return err;
      return arrived() ? hipSuccess : hipErrorUnknown;
    }
    lk.unlock();
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
          if (hipStreamQuery(e->ustream) != hipErrorNotReady) break;  // drained, or an error
        }
      }
    }
    hipError_t err = hipSuccess;
    if (!done) {
      err = hipStreamSynchronize(e->ustream);
      if (err == hipSuccess && !arrived()) err = hipErrorUnknown;  // the kernel died
    }
    lk.lock();
    if (err == hipSuccess) c->util_pending = false;
    return err;
  }
};

// ffn_engine::d_turn / h_turn for n candidates, a histogram of hist_n bins and
// up to novl published overlap pairs
struct TurnLayout {
  size_t o_part, o_flag, o_hist, d_bytes;  // d_turn, bytes
  size_t w_pub, h_words;                   // h_turn, 8-byte words
  TurnLayout(size_t ncap, size_t hcap, size_t ocap) {
    o_part = sizeof(TurnRecord);
    o_flag = o_part + (size_t)kTurnBlocks * 16;
    o_hist = o_flag + 20 * ncap;
    d_bytes = o_hist + 4 * hcap;
    w_pub = 3 * ncap / 2;
    h_words = w_pub + 8 + 3 * ncap + 2 * ocap;
  }
};

// What turn_publish_kernel wrote for call `seq`, n candidates: words whose upper half
// is seq have arrived (see the kernel for the layout).
struct TurnPub {
  const unsigned long long* w;
  unsigned seq;
  size_t n;
  uint32_t at(size_t k) const { return (uint32_t)__atomic_load_n(&w[k], __ATOMIC_RELAXED); }
  bool has(size_t first, size_t count) const {
    for (size_t k = first; k < first + count; ++k)
      if ((unsigned)(__atomic_load_n(&w[k], __ATOMIC_ACQUIRE) >> 32) != seq) return false;
    return true;
  }
  // the header says how many pairs follow the candidates' words
  bool arrived() const { return has(0, 8 + 3 * n) && has(8 + 3 * n, 2 * (size_t)at(7)); }
  // into the caller's arrays; returns the exact number of overlapped ids
  int overlaps(int32_t* ids, int64_t* counts) const {
    const size_t o = 8 + 3 * n;
    for (size_t k = 0; k < at(7); ++k) {
      ids[k] = (int32_t)at(o + 2 * k);
      counts[k] = (int64_t)at(o + 2 * k + 1);
    }
    return (int)at(6);
  }
};

inline int check_canvas(const ffn_canvas* c) {
  if (!c) return fail(FFN_ERR_ARG, "null canvas");
  if (!c->engine) return fail(FFN_ERR_STATE, "canvas outlived its engine");
  return FFN_OK;
}

inline int check_box(const ffn_canvas* c, const int32_t lo[3], const int32_t hi[3]) {
  const int dims[3] = {c->cz, c->cy, c->cx};
  for (int k = 0; k < 3; ++k)
    if (lo[k] < 0 || hi[k] > dims[k] || hi[k] < lo[k])
      return fail(FFN_ERR_ARG, "box [%d,%d) out of canvas axis %d (size %d)",
                  lo[k], hi[k], k, dims[k]);
  return FFN_OK;
}

inline int grid_for(long total, int block = 256) {
  long g = (total + block - 1) / block;
  return (int)std::max<long>(1, std::min<long>(g, 2048));
}

// --- defined once, called across the units ---
// ffn_hip.hip: the step ffn_canvas_segment_many_carry left in flight -- wait for it and
// hand its results to the loops of its canvases (`only`: nothing to do unless that canvas
// is one of them; callers hold neither `mu` nor `many_mu`)
int resolve_many_carry(ffn_engine* e, const ffn_canvas* only = nullptr);
// ffn_canvas.hip: the utility calls' scratch and the segment turn's (under util_mu)
int ensure_scratch(ffn_engine* e, size_t bytes);
int ensure_turn(ffn_engine* e, size_t n, size_t hist_n, size_t novl);
// ffn_options.hip: flush the per-launch event pairs recorded since the last flush
int flush_events(ffn_engine* e);

#endif  // FFN_ENGINE_H_
