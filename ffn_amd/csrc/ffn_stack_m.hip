// conv32m and conv32mt as their own launches (conv_variant 8 and 9; a batch under 6): with
// three MFMA products per operand pair or one (engine option mfma_products), conv32mt with
// 32- or 96-voxel tail workgroups and, for one FoV with flow = 1, in its flagged form.

#include <hip/hip_runtime.h>

#include "ffn_stack_units.h"

namespace {

// what else selects a form: one product; conv32mt's tail tiles (1 or 3) and FLOW
constexpr int m_more(int products, int tail_tiles = 0, bool flow = false) {
  return (products == 1 ? 1 : 0) | tail_tiles << 1 | (flow ? 8 : 0);
}

const KernelForm<void (*)(ConvDArgs)> kMForms[] = {
#define FFN_FORM(KIND, SK, HEAD)                                                  \
  {form_key(KIND, SK, HEAD, m_more(3)), conv32m_kernel<KIND, SK, HEAD>},          \
  {form_key(KIND, SK, HEAD, m_more(1)), conv32m_kernel<KIND, SK, HEAD, 1>}
    FFN_CONV_FORMS(FFN_FORM)
#undef FFN_FORM
};

const KernelForm<void (*)(ConvDArgs, ConvTailMap)> kMTForms[] = {
#define FFN_FORM(KIND, SK, HEAD)                                                            \
  {form_key(KIND, SK, HEAD, m_more(3, 1)), conv32mt_kernel<KIND, SK, HEAD, 1>},             \
  {form_key(KIND, SK, HEAD, m_more(3, 3)), conv32mt_kernel<KIND, SK, HEAD, 3>},             \
  {form_key(KIND, SK, HEAD, m_more(1, 1)), conv32mt_kernel<KIND, SK, HEAD, 1, false, 1>},   \
  {form_key(KIND, SK, HEAD, m_more(1, 3)), conv32mt_kernel<KIND, SK, HEAD, 3, false, 1>}
    FFN_CONV_FORMS(FFN_FORM),
#undef FFN_FORM
#define FFN_FORM(KIND, SK, HEAD) \
  {form_key(KIND, SK, HEAD, m_more(3, 1, true)), conv32mt_kernel<KIND, SK, HEAD, 1, true>}
    FFN_CONV_FORMS4(FFN_FORM)
#undef FFN_FORM
};

}  // namespace

int set_lds_attr_m() {
  if (int rc = set_lds_attr(kMForms, kMLdsBytes)) return rc;
  return set_lds_attr(kMTForms, kMLdsBytes);
}

int launch_conv32m(ffn_engine* e, const StackPlan& plan, int n, int kind, bool sk,
                   const float* raw_in, float* raw_out, int layer, const HeadFusion& head) {
  ConvDArgs a;
  conv32d_args(e, plan, n, raw_in, raw_out, layer, head, a);
  const dim3 block(kDThreads);
  if (plan.family == ConvFamily::M) {
    const auto kernel = find_form(kMForms, form_key(kind, sk, head.on, m_more(plan.products)));
    if (!kernel) return no_form("conv32m", kind, sk, head.on);
    if (int rc = prof_begin(e)) return rc;
    hipLaunchKernelGGL(kernel, dim3(8 * a.slots_per_xcd), block, kMLdsBytes, e->stream, a);
    return prof_end(e);
  }
  // one FoV: 32-voxel tail workgroups (balance over the CUs); several: the
  // same voxels in 96-voxel ones (cost per voxel) -- the same bits
  const bool one = plan.tail_tiles == 1;
  ConvTailMap mp;
  tail_map(e, n, mp);
  // (the one-product kernels: per-layer launches without FLOW)
  const bool flow1 = one && e->flow == 1 && plan.products != 1;
  const auto kernel = find_form(
      kMTForms, form_key(kind, sk, head.on, m_more(plan.products, one ? 1 : 3, flow1)));
  if (!kernel) return no_form(flow1 ? "conv32mt (flow = 1)" : "conv32mt", kind, sk, head.on);
  if (int rc = prof_begin(e)) return rc;
  if (flow1) {
    a.L.flow_wait_on = layer > 0;
    a.L.flow_wait = e->flow_epoch;
    a.L.flow_set = ++e->flow_epoch;
  }
  const dim3 tgrid(8 * n * (mp.mains_per_xcd + mp.tails_per_xcd));
  hipLaunchKernelGGL(kernel, tgrid, block, kMLdsBytes, e->stream, a, mp);
  return prof_end(e);
}
