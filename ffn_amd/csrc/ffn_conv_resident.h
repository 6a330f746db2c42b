// conv32ps: the conv stack of a single-FoV step as ONE resident launch (engine option flow = 2).
// (templates only: ffn_stack_units.h includes it behind ffn_conv_split.h, inside no namespace;
// ffn_stack_resident.hip alone instantiates the kernel)
#pragma once

namespace ffn {

// ---------------------------------------------------------------------------
// conv32ps: the whole conv stack of ONE FoV as a single resident launch.
//
// conv32mt's workgroups (256 main chunks, one per CU, + the 32-voxel tail
// workgroups on the CUs' second slots: all resident at once) keep their voxels
// through all 2 depth - 1 convs; between two convs stands, instead of a kernel
// boundary, the FLOW hand-off above: a workgroup starts conv l + 1 as soon as
// the tiles ITS rows come from have been published by conv l.  Each conv's body
// is the plain kernel's (same instructions, same summation order: same bits);
// what changes per conv -- the two activation buffers taking turns, the weights
// and bias of the layer, the sequence numbers -- is derived from the layer
// index.  conv 0 (conv0_b) sits behind the boundary after conv0_a and waits for
// nothing; the last conv carries the fused head and publishes nothing (the
// faces / paste launch behind it is an ordinary dependent launch).
// ---------------------------------------------------------------------------
// (compile-time switch for same-box A/B builds: tools/build_variant.sh)
#ifndef FFN_PS_RES
#define FFN_PS_RES 1
#endif
constexpr bool kPsRes = FFN_PS_RES != 0;

struct ConvStackTab {
  int nlayers;            // 2 depth - 1
  int l_begin, l_end;     // the convs of THIS launch ([0, nlayers) unless debugging)
  int dbg_layer;          // the conv whose clock stamps are recorded (ConvDArgs::L.dbg)
  const char* sp_t;       // T' (position 0 of plane 0): read by even convs, written by odd
  char* sp_s;             // X': written by even convs, read by odd
  const char* wpack0;     // layer 0's weight fragments ...
  long wpack_stride;      // ... bytes per layer
  const float* bias0;
  long bias_stride;       // floats per layer
  unsigned epoch0;        // conv l publishes epoch0 + l + 1 and waits for epoch0 + l
  int pace;               // 10-ns ticks between two convs of a workgroup (0: free-running)
  int pace_tail;          // conv32ps: the tail workgroups' offset inside a period
  int pace_spread;        // phi of the FoV's last voxel, in ticks (0: every workgroup at once)
  // [0] when the last step's record was published (faces block), [1] sum over the launches
  // of (this launch's first instruction - [0]) in 10-ns ticks, [2] their count; or NULL
  long long* stamps;
  // A stack queued AHEAD of the host (engine option stack_ahead), behind the speculative
  // conv0_a of its step: that launch's choice word (-1: the device found no valid
  // position and computed nothing -- this launch then ends after its first conv, which
  // ran on the last step's planes; nobody reads what it wrote).  NULL: an ordinary launch.
  const int* ahead_choice;
  int trace;  // debug_fused_trace: stamp [7] first entry, [11] last end of this launch
};

// ... and what the production form takes: no dbg_layer, no trace, and every conv of the
// stack (l_begin = 0, l_end = nlayers)
struct ConvStackTabLean {
  int nlayers;
  const char* sp_t;
  char* sp_s;
  const char* wpack0;
  long wpack_stride;
  const float* bias0;
  long bias_stride;
  unsigned epoch0;
  int pace, pace_tail, pace_spread;
  long long* stamps;  // [0] .. [3] alone: the turn-around stamp and the aborted count
  const int* ahead_choice;
};

inline ConvStackTabLean lean_tab(const ConvStackTab& t) {
  ConvStackTabLean q;
  q.nlayers = t.nlayers;
  q.sp_t = t.sp_t;
  q.sp_s = t.sp_s;
  q.wpack0 = t.wpack0;
  q.wpack_stride = t.wpack_stride;
  q.bias0 = t.bias0;
  q.bias_stride = t.bias_stride;
  q.epoch0 = t.epoch0;
  q.pace = t.pace, q.pace_tail = t.pace_tail, q.pace_spread = t.pace_spread;
  q.stamps = t.stamps;
  q.ahead_choice = t.ahead_choice;
  return q;
}

// LAB = true: the kernel with all of the lab's run-time plumbing -- debug_clock (L.dbg,
// dbg_wgs), debug_layer, flow_debug (the fault injection bit among them), the flow trace,
// debug_fused_trace -- as kernel arguments tested in every conv.  LAB = false, the
// production form, has none of it, neither as arguments nor as code: what is left between
// two tap loops is the hand-off itself.  Both keep pacing, the void / time-out path, the
// stack ahead of the host and the once-per-launch statistics (stat_turn_gpu_ns,
// stat_turn_count, stat_ahead_aborted).  Same bodies, same stores, same summation order:
// same bits.  The host picks (launch_conv32ps: LAB whenever one of the lab's options is
// on, or engine option flow_lab says so).
template <bool LAB>
__global__ __launch_bounds__(kDThreads, 2) void conv32ps_kernel(
    std::conditional_t<LAB, ConvDArgs, ConvDArgsLean> a, ConvTailMap mp,
    std::conditional_t<LAB, ConvStackTab, ConvStackTabLean> tb) {
  warm_kernargs<kernarg_bytes<decltype(a), ConvTailMap, decltype(tb)>()>();
  const int xcd = blockIdx.x & 7;
  const int r0 = blockIdx.x >> 3;
  const bool main_wg = r0 < mp.mains_per_xcd;
  const int r = main_wg ? r0 : r0 - mp.mains_per_xcd;
  const int c = xcd * (main_wg ? mp.mains_per_xcd : mp.tails_per_xcd) + r;
  if (c >= (main_wg ? mp.n_main : mp.n_tail)) return;
  long long t0 = 0, t_entry = 0;
  if constexpr (LAB) {
    t0 = a.dbg_wgs ? wall_clock64() : 0;
    t_entry = (tb.stamps && tb.trace) ? wall_clock64() : 0;
  }
  if (tb.stamps && blockIdx.x == 0 && threadIdx.x == 0 && tb.stamps[0]) {
    // publish of the last step -> first instruction of this stack: the host's turn-around
    // + the launch, as the GPU saw it (engine options stat_turn_gpu_ns / stat_turn_count)
    // (steps INSIDE a segment: a turn between two segments -- commit, seed policy, the
    // next init_seed -- takes milliseconds and is not what this figure is about)
    const long long dt = wall_clock64() - tb.stamps[0];
    if (dt < 10000) {
      atomicAdd(reinterpret_cast<unsigned long long*>(tb.stamps + 1), (unsigned long long)dt);
      atomicAdd(reinterpret_cast<unsigned long long*>(tb.stamps + 2), 1ull);
    }
    tb.stamps[0] = 0;
  }
  // (a scalar load in flight under the first conv: no wait of its own)
  const int ahead_ch = tb.ahead_choice ? *tb.ahead_choice : 0;
  const int v0 = main_wg ? c * kMChunk : mp.n_main * kMChunk + c * 32;
  const int gc = main_wg ? c : mp.n_main + c;
  typedef std::conditional_t<LAB, ConvLayer, ConvLayerLean> Layer;
  Layer Ldbg = [&]() -> Layer {
    if constexpr (LAB) return a.L;
    else return Layer{};
  }();
  // (experiment, flow_dbg 1024: the main workgroups' waves ahead of the tail's in
  // the CU's arbitration -- a main workgroup that shares its CU with a tail one
  // is what its neighbours wait for)
  if (kExp && (lab_flow_dbg<LAB>(a) & 1024)) {
    if (main_wg) __builtin_amdgcn_s_setprio(3);
    else __builtin_amdgcn_s_setprio(0);
  }
  // the residual stream of a main workgroup's voxels (conv32m_body: RES); the
  // tail workgroups keep theirs in memory (their head epilogue has another
  // thread-to-voxel mapping than their conv epilogue)
  f32x4 xres[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) xres[g] = f32x4{0.f, 0.f, 0.f, 0.f};
  // what changes from conv to conv, carried in registers from one to the next
  // (rebuilt from the kernel arguments in every loop header it cost two scalar
  // loads and their waits per conv; same bits either way)
  // (the production form runs every conv of the stack: l_begin = 0, l_end = nlayers)
  int l_begin = 0;
  if constexpr (LAB) l_begin = tb.l_begin;
  const char* wp = tb.wpack0 + (long)l_begin * tb.wpack_stride;
  const float* bp = tb.bias0 + (long)l_begin * tb.bias_stride;
  const long wstride = tb.wpack_stride, bstride = tb.bias_stride;
  unsigned epoch = tb.epoch0 + (unsigned)l_begin;
  const char* sp_in = (l_begin & 1) ? tb.sp_s : tb.sp_t;
  const char* sp_out = (l_begin & 1) ? tb.sp_t : tb.sp_s;
  const int l_first = l_begin;
  int l_dbg = -1;
  if constexpr (LAB) l_dbg = tb.dbg_layer;
  // Pacing (tb.pace > 0; engine option flow_pace): conv l of a workgroup does not start
  // before  t0 + l pace + phi,  phi = pace_spread x (its first voxel / V), + pace_tail for a
  // tail workgroup: the free-running hand-off lets the lower planes run ahead and every
  // consumer wait for the latest of its ~20 producers; a common beat a little above the
  // chain's own length takes that jitter out (measured: -2.5 % per stack at 7.0 us per
  // conv, profiles/r06_pacing.txt).  Timing only: the arithmetic does not know about it.
  const long long t_pace0 =
      wall_clock64() + (long long)tb.pace_spread * v0 / a.V + (main_wg ? 0 : tb.pace_tail);
  int l_end = tb.nlayers;
  if constexpr (LAB) l_end = tb.l_end;
  for (int l = l_begin; l < l_end; ++l) {
    if (tb.pace > 0) {
      const long long target = t_pace0 + (long long)(l - l_first) * tb.pace;
      while (wall_clock64() < target) __builtin_amdgcn_s_sleep(1);
    }
    Layer L;
    L.in_sp = sp_in;    // T' for even convs, X' for odd ones ...
    L.out_sp = const_cast<char*>(sp_out);  // ... and the other one written
    L.wpack = wp;
    L.bias = bp;
    if constexpr (LAB) L.dbg = l == l_dbg ? a.L.dbg : nullptr;
    L.flow_wait = epoch;
    L.flow_set = epoch + 1u;
    L.flow_wait_on = l > l_first;
    if constexpr (LAB) L.layer = l;
    wp += wstride;
    bp += bstride;
    epoch += 1u;
    {
      const char* t = sp_in;
      sp_in = sp_out;
      sp_out = t;
    }
    if constexpr (LAB) {
      if (L.dbg) Ldbg = L;
    }
    if (l == l_first + 1 && ahead_ch < 0) {  // (every workgroup alike)
      // ([3]: launches that ended here -- engine statistic stat_ahead_aborted)
      if (tb.stamps && blockIdx.x == 0 && threadIdx.x == 0)
        atomicAdd(reinterpret_cast<unsigned long long*>(tb.stamps + 3), 1ull);
      break;
    }
    const bool last = l == tb.nlayers - 1;
    if (main_wg) {
      bool dbg_here = false;
      if constexpr (LAB) dbg_here = blockIdx.x == 0 && a.dbg_wgs != 2;
      if (l == 0 && !(kAbl & 512))
        conv32m_body<1, false, false, true, kPsRes, 3, LAB>(a, L, 0, v0, gc, dbg_here, xres);
      else if (last && !(kAbl & 512))
        conv32m_body<1, true, true, true, kPsRes, 3, LAB>(a, L, 0, v0, gc, dbg_here, xres);
      else if ((l & 1) && !(kAbl & 256))  // (256: ONE code body for every middle conv;
        // 512: every conv of the stack -- timing only: how much of a layer is
        // instruction delivery when odd and even convs run different code?)
        conv32m_body<0, false, false, true, kPsRes, 3, LAB>(a, L, 0, v0, gc, dbg_here, xres);
      else
        conv32m_body<1, true, false, true, kPsRes, 3, LAB>(a, L, 0, v0, gc, dbg_here, xres);
    } else {
      bool dbg_here = false;
      if constexpr (LAB) dbg_here = c == 0 && a.dbg_wgs == 2;
      if (l == 0 && !(kAbl & 512))
        conv32d_body<1, false, kTPieces, false, 1, kTRows, 2, true, 3, LAB>(
            a, L, 0, v0, gc, mp.taoff, dbg_here);
      else if (last && !(kAbl & 512))
        conv32d_body<1, true, kTPieces, true, 1, kTRows, 2, true, 3, LAB>(
            a, L, 0, v0, gc, mp.taoff, dbg_here);
      else if ((l & 1) && !(kAbl & 256))
        conv32d_body<0, false, kTPieces, false, 1, kTRows, 2, true, 3, LAB>(
            a, L, 0, v0, gc, mp.taoff, dbg_here);
      else
        conv32d_body<1, true, kTPieces, false, 1, kTRows, 2, true, 3, LAB>(
            a, L, 0, v0, gc, mp.taoff, dbg_here);
    }
  }
  if constexpr (LAB) {
    stamp_workgroup(a, Ldbg, t0);
    // (debug_fused_trace: [7] first entry, [11] last end of this launch's workgroups)
    if (tb.stamps && tb.trace == 1 && threadIdx.x == 0) {
      atomicMin(reinterpret_cast<unsigned long long*>(tb.stamps + 7), (unsigned long long)t_entry);
      atomicMax(reinterpret_cast<unsigned long long*>(tb.stamps + 11),
                (unsigned long long)wall_clock64());
    }
    // ([25] last end, [26] first entry of the stack IN FRONT of a traced step under stack_ahead)
    // (one plain store per workgroup into its own slot, reduced by the host: 356 atomics on one
    // word at the END of a launch would stand between it and the launch behind it)
    if (tb.stamps && tb.trace == 2 && threadIdx.x == 0) {
      tb.stamps[32 + blockIdx.x] = wall_clock64();
      if (blockIdx.x == 0) tb.stamps[26] = t_entry;
      // ... and where the workgroup ran: (main?, XCC, SE, SH, CU) -- two main workgroups on
      // one CU is what a dispatch onto a chip that is not yet empty can produce
      unsigned hw, xcc;
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
      tb.stamps[32 + 512 + blockIdx.x] =
          (long long)(((main_wg ? 1u : 0u) << 31) | ((xcc & 15u) << 16) | ((hw >> 8) & 0xffu)) + 1;
    }
  }
}

}  // namespace ffn
