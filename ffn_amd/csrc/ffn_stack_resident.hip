// The resident stacks -- all 2 depth - 1 convs of ONE FoV as a single launch: conv32ps
// (ffn_conv_resident.h; its two forms, production and LAB) and conv32hs (conv_variant 10,
// ffn_conv_half.h) -- and conv32h, the per-layer form that a voided conv32hs step is
// repeated with.  Launched, given their LDS and asked for their occupancy here alone.
// (One unit, not two: next to a LAB user of the FLOW hand-off conv32hs_kernel comes out as
// it does in a build of everything in one unit, alone in its module four bytes longer --
// profiles/stack_units_codeobj.txt.)

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>

#include "ffn_stack_units.h"
#include "ffn_conv_half.h"

namespace {
// Whether the launches of a step take their LAB form: one of the lab's run-time options is
// on (the production forms have no code for them), the build is an experiment or ablation
// build, or engine option flow_lab asks for it.  (debug_fused_trace is per launch: a
// launch that stamps is a LAB launch, launch_conv32ps and the fused step launch.)
bool lab_wanted(const ffn_engine* e) {
  return e->flow_lab != 0 || kExp || kAbl != 0 || FFN_FLOW_TRACE != 0 || e->dbg_clock != 0 ||
         e->dbg_layer != kDbgLayerDefault || e->flow_debug != 0;
}
}  // namespace

int set_lds_attr_ps() {
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(conv32ps_kernel<false>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, kMLdsBytes));
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(conv32ps_kernel<true>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, kMLdsBytes));
  return FFN_OK;
}

// a single-FoV step of conv32mt runs its convs as ONE resident launch where the device
// can hold all of its workgroups at once (both forms of the kernel: the smaller
// occupancy decides; asked once set_lds_attr_ps has run)
int conv32ps_fits(const ffn_engine* e, bool* fits) {
  int per_cu = 0, per_cu_lab = 0;
  HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, conv32ps_kernel<false>,
                                                       kDThreads, kMLdsBytes));
  HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_lab, conv32ps_kernel<true>,
                                                       kDThreads, kMLdsBytes));
  per_cu = std::min(per_cu, per_cu_lab);
  ConvTailMap mp;
  tail_map(e, 1, mp);
  const int grid = 8 * (mp.mains_per_xcd + mp.tails_per_xcd);
  *fits = e->cus >= e->caps.n_main && (long)e->cus * per_cu >= grid;
  return FFN_OK;
}

// The 2 depth - 1 convs of ONE FoV as a single resident launch (conv32ps,
// ffn_conv_resident.h): conv32mt's workgroups keep their voxels through the stack and
// hand rows to each other through the tile words instead of kernel boundaries.
// ev0 / ev1: a sampled launch -- the events carry the START and END of this very dispatch
// (hipExtLaunchKernelGGL: the timestamps rocprofv3 reads), not markers queued around it: a
// marker is a barrier packet with system-scope fences of its own, 2 - 3 us each, which the
// sampled launch and the step around it would wait behind
int launch_conv32ps(ffn_engine* e, const StackPlan& plan, float pad_value, float move_thr,
                    const int* ahead_choice, hipEvent_t ev0, hipEvent_t ev1) {
  ConvDArgs a;
  conv32d_args(e, plan, 1, e->rawT, e->rawS, 0, head_fusion(true, pad_value, move_thr), a);
  a.L.dbg = e->dbg_clock ? e->d_dbg : nullptr;
  ConvTailMap mp;
  tail_map(e, 1, mp);
  ConvStackTab tb;
  stack_tab(e, e->wpackd, e->pace_auto, &tb);
  tb.pace_tail = e->flow_pace_tail;
  const dim3 grid(8 * (mp.mains_per_xcd + mp.tails_per_xcd)), block(kDThreads);
  tb.stamps = e->d_stamps;
  tb.ahead_choice = ahead_choice;
  // (2: the stack in front of the traced step, queued ahead one call earlier: its end only)
  tb.trace = e->trace_now ? 1 : (ahead_choice && e->fused_trace_in == 1) ? 2 : 0;
  const long long t_l0 = e->t_arrived_ns ? steady_ns() : 0;
  if (lab_wanted(e) || tb.trace != 0) {
    e->stat_lab_launches += 1;
    if (ev0)
      hipExtLaunchKernelGGL(conv32ps_kernel<true>, grid, block, kMLdsBytes, e->stream, ev0, ev1,
                            0, a, mp, tb);
    else
      hipLaunchKernelGGL(conv32ps_kernel<true>, grid, block, kMLdsBytes, e->stream, a, mp, tb);
  } else {
    const ConvDArgsLean al = lean_args(a);
    const ConvStackTabLean tl = lean_tab(tb);
    if (ev0)
      hipExtLaunchKernelGGL(conv32ps_kernel<false>, grid, block, kMLdsBytes, e->stream, ev0, ev1,
                            0, al, mp, tl);
    else
      hipLaunchKernelGGL(conv32ps_kernel<false>, grid, block, kMLdsBytes, e->stream, al, mp, tl);
  }
  if (e->t_arrived_ns) {
    const long long t_l1 = steady_ns();
    if (t_l1 - e->t_arrived_ns < 100000) {  // (inside a segment: see ConvStackTab::stamps)
      e->stat_turn_host_ns += t_l1 - e->t_arrived_ns;
      e->stat_launch_host_ns += t_l1 - t_l0;
      e->stat_turn_host_count += 1;
    }
    e->t_arrived_ns = 0;
  }
  return FFN_OK;
}

// ---------------------------------------------------------------------------
// conv32h / conv32hs: the split-product conv on 80-voxel workgroups
// ---------------------------------------------------------------------------
namespace {

// (the head without the residual: a stack of depth 1, which run_stack refuses)
const KernelForm<void (*)(ConvDArgs, ConvHalfMap)> kHForms[] = {
#define FFN_FORM(KIND, SK, HEAD) {form_key(KIND, SK, HEAD), conv32h_kernel<KIND, SK, HEAD>}
    FFN_CONV_FORMS(FFN_FORM)
#undef FFN_FORM
};

// The same stack on 64-voxel workgroups, two per CU (conv32hs, ffn_conv_half.h).
void half_map(const ffn_engine* e, ConvHalfMap& mp) {
  // (the dispatcher hands an XCD's first blocks to its empty CUs: cus / 8 first slots)
  mp.n_chunks = e->caps.n_half;
  mp.per_first = std::max(1, e->cus / 8);
  mp.n_first = std::min(e->caps.n_half, 8 * mp.per_first);
  mp.per_second = (e->caps.n_half - mp.n_first + 7) / 8;
}

}  // namespace

int set_lds_attr_h() {
  if (int rc = set_lds_attr(kHForms, kHLdsBytes)) return rc;
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(conv32hs_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, kHLdsBytes));
  return FFN_OK;
}

// conv32hs: 80-voxel workgroups, two per CU, all resident at once
// (asked once set_lds_attr_h has run)
int conv32hs_fits(const ffn_engine* e, bool* fits) {
  int per_cu = 0;
  HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, conv32hs_kernel, kDThreads,
                                                       kHLdsBytes));
  ConvHalfMap hm;
  half_map(e, hm);
  *fits = (long)e->cus * per_cu >= 8 * (hm.per_first + hm.per_second);
  return FFN_OK;
}

// one conv of the 80-voxel family as its own launch: what a resident step that came
// back void is repeated with (the same bits), and flow = 0
int launch_conv32h(ffn_engine* e, const StackPlan& plan, int kind, bool sk,
                   const float* raw_in, float* raw_out, int layer, const HeadFusion& head) {
  ConvDArgs a;
  conv32d_args(e, plan, 1, raw_in, raw_out, layer, head, a);
  a.L.wpack = reinterpret_cast<const char*>(e->wpackh + (size_t)layer * e->wpackd_layer);
  a.flow_n_main = -1;
  ConvHalfMap mp;
  half_map(e, mp);
  const auto kernel = find_form(kHForms, form_key(kind, sk, head.on));
  if (!kernel) return no_form("conv32h", kind, sk, head.on);
  const dim3 grid(8 * (mp.per_first + mp.per_second)), block(kDThreads);
  hipLaunchKernelGGL(kernel, grid, block, kHLdsBytes, e->stream, a, mp);
  return FFN_OK;
}

int launch_conv32hs(ffn_engine* e, const StackPlan& plan, float pad_value, float move_thr) {
  ConvDArgs a;
  conv32d_args(e, plan, 1, e->rawT, e->rawS, 0, head_fusion(true, pad_value, move_thr), a);
  a.flow_n_main = -1;
  ConvHalfMap mp;
  half_map(e, mp);
  ConvStackTab tb;
  stack_tab(e, e->wpackh, 0, &tb);  // (no measured beat for this family)
  const dim3 grid(8 * (mp.per_first + mp.per_second)), block(kDThreads);
  hipLaunchKernelGGL(conv32hs_kernel, grid, block, kHLdsBytes, e->stream, a, mp, tb);
  return FFN_OK;
}
