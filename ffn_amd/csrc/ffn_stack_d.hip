// conv32d as its own launch (conv_variant 6 and 7): the 160-voxel forms, one per number of
// LDS row groups (KS = Rc_k / 32: 8, 9, 10), and the 96-voxel forms, two workgroups per CU.

#include <hip/hip_runtime.h>

#include "ffn_stack_units.h"

namespace {

using ConvDKernel = void (*)(ConvDArgs);

const KernelForm<ConvDKernel> kD160Forms[] = {
#define FFN_FORM(KIND, SK, HEAD)                                              \
  {form_key(KIND, SK, HEAD, 8), conv32d_kernel<KIND, SK, 8, HEAD>},           \
  {form_key(KIND, SK, HEAD, 9), conv32d_kernel<KIND, SK, 9, HEAD>},           \
  {form_key(KIND, SK, HEAD, 10), conv32d_kernel<KIND, SK, 10, HEAD>}
    FFN_CONV_FORMS(FFN_FORM)
#undef FFN_FORM
};

const KernelForm<ConvDKernel> kD96Forms[] = {
#define FFN_FORM(KIND, SK, HEAD) \
  {form_key(KIND, SK, HEAD), conv32d_kernel<KIND, SK, kEPieces, HEAD, kETiles, kERows, 2>}
    FFN_CONV_FORMS(FFN_FORM)
#undef FFN_FORM
};

}  // namespace

int set_lds_attr_d(const ConvCaps& caps) {
  if (int rc = set_lds_attr(kD160Forms, caps.lds_bytes_d)) return rc;
  return caps.e_ok ? set_lds_attr(kD96Forms, caps.lds_bytes_e) : FFN_OK;
}

int launch_conv32d(ffn_engine* e, const StackPlan& plan, int n, int kind, bool sk,
                   const float* raw_in, float* raw_out, int layer, const HeadFusion& head) {
  ConvDArgs a;
  conv32d_args(e, plan, n, raw_in, raw_out, layer, head, a);
  const bool small = plan.family == ConvFamily::D96;
  const ConvDKernel kernel =
      small ? find_form(kD96Forms, form_key(kind, sk, head.on))
            : find_form(kD160Forms, form_key(kind, sk, head.on, e->caps.Rc_k / 32));
  if (!kernel) return no_form(small ? "conv32d (96 voxels)" : "conv32d", kind, sk, head.on);
  if (int rc = prof_begin(e)) return rc;
  const dim3 grid(8 * a.slots_per_xcd), block(kDThreads);
  hipLaunchKernelGGL(kernel, grid, block, small ? e->caps.lds_bytes_e : e->caps.lds_bytes_d,
                     e->stream, a);
  return prof_end(e);
}
