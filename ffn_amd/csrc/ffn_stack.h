// The conv launch layer as the rest of the engine calls it (not part of the C-ABI, no
// kernel in here).  Defined in ffn_stack.hip; the kernel families behind it are units of
// their own (ffn_stack_units.h), so that they compile side by side.
#ifndef FFN_STACK_H_
#define FFN_STACK_H_

#include "ffn_engine.h"

namespace ffn {
struct StepItems;
struct SpecArgs;
struct Conv0Next;
}  // namespace ffn

// (between the units of the library only: not among its exported symbols)
#pragma GCC visibility push(hidden)

// The plan of a stack of n FoVs as the engine's options stand (flow_skip: the engine's,
// or 0 for "once no repeat is pending").
StackPlan plan_for(const ffn_engine* e, int n, int flow_skip);

// FoVs described by `si` -> logits (+ count of logits >= move_thr, + seed_raw)
// conv0a_done: the step's conv0_a has been queued already (a speculative launch
// that chose its position)
// ahead: the stack of the step AFTER the one being submitted, behind the speculative
// conv0_a just queued for it (engine option stack_ahead; conv0a_done with it)
int run_stack(ffn_engine* e, int n, const StepItems& si, float pad_value, float move_thr,
              bool conv0a_done = false, bool ahead = false);

// conv0_a of a step whose range tag is `tag` (sp.n > 0: a speculative launch)
void launch_conv0a(ffn_engine* e, int n, const StepItems& si, float pad_value, unsigned tag,
                   const SpecArgs& sp, bool next = false);
// conv0_a of the split-product family as the argument block of the fused launch;
// returns its number of tiles.  next: for the step AFTER the current one (its
// outputs go to the other set: ffn_engine::seed_raw_alt ...)
int conv0a_split_args(ffn_engine* e, float pad_value, unsigned tag, const SpecArgs& sp,
                      bool next, Conv0Next& nx);

// The split-plane layout of variant 6 and the f32 layout of the others keep their
// zero padding in different bytes of the same allocations: re-zero on a change.
int switch_variant(ffn_engine* e, int value);

// Room for one more pair of profiler events: the recorded ones are flushed when fewer
// than two are left (no allocation: the events were created with the engine).
int event_pair(ffn_engine* e);

// When an engine is created: the LDS a workgroup may ask for, set on every kernel form of
// the families its geometry admits; and what THIS device can hold of the two resident
// launches (ffn_engine::flow_fits, and h_ok: its geometric half is ConvCaps::h_geom_ok).
// In this order: a resident kernel is asked for its occupancy with its LDS granted.
int set_stack_lds_attrs(ffn_engine* e);
int stack_residency(ffn_engine* e);

#pragma GCC visibility pop

#endif  // FFN_STACK_H_
