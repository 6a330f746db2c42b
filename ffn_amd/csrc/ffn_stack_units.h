// What the units of the conv launch layer share with each other (ffn_stack.h is what the
// rest of the engine sees of them):
//   ffn_stack.hip           run_stack and its walker, conv0_a, the head, conv32 / conv32c
//   ffn_stack_d.hip         conv32d, 160- and 96-voxel forms
//   ffn_stack_m.hip         conv32m, conv32mt
//   ffn_stack_resident.hip  conv32ps and conv32hs, the resident stacks; conv32h
// Without relocatable device code every unit that names a kernel gets a device copy and a
// registration of its own, so a kernel form is launched, given its attributes and asked
// for its occupancy in ONE unit: the one that holds its family's table of forms.
#ifndef FFN_STACK_UNITS_H_
#define FFN_STACK_UNITS_H_

#include "ffn_engine.h"
#include "ffn_kernels.h"
#include "ffn_conv_split.h"
#include "ffn_conv_resident.h"

// (between the units of the library only: not among its exported symbols)
#pragma GCC visibility push(hidden)

struct HeadFusion {
  bool on = false;
  float pad_value = 0.f, move_thr = 0.f;
};
inline HeadFusion head_fusion(bool on, float pad_value, float move_thr) {
  HeadFusion hf;
  hf.on = on;
  hf.pad_value = pad_value;
  hf.move_thr = move_thr;
  return hf;
}

// The forms a split-product conv kernel is launched in: conv_a (KIND 0); conv_b (KIND 1)
// without and with the residual (SK), each also with the head fused -- which the flagged
// (FLOW) kernels have only with the residual: FFN_CONV_FORMS4.
#define FFN_CONV_FORMS4(X) \
  X(0, false, false), X(1, false, false), X(1, true, false), X(1, true, true)
#define FFN_CONV_FORMS(X) FFN_CONV_FORMS4(X), X(1, false, true)

// A family's forms are ONE table of {selector, kernel}: the attribute pass walks it, a
// launch looks its form up in it (none: FFN_ERR_ARG).  `more`: what else selects a form of
// the family (tile count, products ...), as the family's unit packs it.
constexpr int form_key(int kind, bool sk, bool head, int more = 0) {
  return kind | (sk ? 2 : 0) | (head ? 4 : 0) | more << 3;
}
template <class Fn>
struct KernelForm {
  int key;
  Fn kernel;
};
template <class Fn, size_t N>
Fn find_form(const KernelForm<Fn> (&forms)[N], int key) {
  for (const KernelForm<Fn>& f : forms)
    if (f.key == key) return f.kernel;
  return nullptr;
}
template <class Fn, size_t N>
int set_lds_attr(const KernelForm<Fn> (&forms)[N], size_t bytes) {
  for (const KernelForm<Fn>& f : forms)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(f.kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  return FFN_OK;
}
inline int no_form(const char* family, int kind, bool sk, bool head) {
  return fail(FFN_ERR_ARG, "%s has no form for kind %d, residual %d, fused head %d here",
              family, kind, (int)sk, (int)head);
}

// --- ffn_stack.hip ---
// The event pair around ONE conv launch of a sampled stack (profiling mode 1).
int prof_begin(ffn_engine* e);
int prof_end(ffn_engine* e);
// The arguments of a split-product launch: KIND 0 conv_a (T' = split(relu(conv(X') + b))),
// KIND 1 conv_b (X = conv(T') + b [+ X]; X' = split(relu(X))), or the fused head
void conv32d_args(ffn_engine* e, const StackPlan& plan, int n, const float* raw_in,
                  float* raw_out, int layer, const HeadFusion& head, ConvDArgs& a);
void tail_map(const ffn_engine* e, int n, ConvTailMap& mp);
// What a resident launch of the whole stack adds to a conv's arguments: where the layers'
// planes, weight fragments (wpack: conv32d's or conv32h's packing) and biases are, its
// epochs, its beat (auto_pace: the one to run at where the user set none).  An ordinary
// launch: nothing stamped, nothing ahead.
void stack_tab(ffn_engine* e, const uint16_t* wpack, int auto_pace, ConvStackTab* tb);

// --- one conv of a split-product family as its own launch (plan.family says whose) ---
int launch_conv32d(ffn_engine* e, const StackPlan& plan, int n, int kind, bool sk,
                   const float* raw_in, float* raw_out, int layer, const HeadFusion& head);
int launch_conv32m(ffn_engine* e, const StackPlan& plan, int n, int kind, bool sk,
                   const float* raw_in, float* raw_out, int layer, const HeadFusion& head);
int launch_conv32h(ffn_engine* e, const StackPlan& plan, int kind, bool sk,
                   const float* raw_in, float* raw_out, int layer, const HeadFusion& head);
// --- the 2 depth - 1 convs of ONE FoV as a single resident launch ---
int launch_conv32ps(ffn_engine* e, const StackPlan& plan, float pad_value, float move_thr,
                    const int* ahead_choice, hipEvent_t ev0, hipEvent_t ev1);
int launch_conv32hs(ffn_engine* e, const StackPlan& plan, float pad_value, float move_thr);
// --- per unit: the attribute pass, and whether the device holds a resident launch ---
int set_lds_attr_d(const ConvCaps& caps);  // (d_ok; the 96-voxel forms where e_ok)
int set_lds_attr_m();
int set_lds_attr_ps();
int set_lds_attr_h();
int conv32ps_fits(const ffn_engine* e, bool* fits);
int conv32hs_fits(const ffn_engine* e, bool* fits);

#pragma GCC visibility pop

#endif  // FFN_STACK_UNITS_H_
