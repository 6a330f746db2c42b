// TEST INFRASTRUCTURE: plan_stack with its eighth argument (the MFMA product count of
// engine option mfma_products) behind a C interface, built with g++ alone -- no HIP, no
// GPU (tests/test_half_ref.py).
#include "../ffn_amd/csrc/ffn_stack_plan.h"

using namespace ffn;

extern "C" {

// out: family (the enum's order), resident, tail_tiles, chunks, products
void half_plan_stack(const int32_t fov_zyx[3], const int32_t deltas_zyx[3], int depth,
                     int conv_variant, int flow, int flow_skip, int tail_batched,
                     int batch_chunks, int n, int products, int32_t out[5]) {
  const ConvCaps c = conv_caps(fov_geom(fov_zyx, deltas_zyx), depth);
  const StackPlan p = plan_stack(c, conv_variant, flow, flow_skip, tail_batched, batch_chunks,
                                 n, products);
  out[0] = (int)p.family;
  out[1] = p.resident;
  out[2] = p.tail_tiles;
  out[3] = p.chunks;
  out[4] = p.products;
}

}  // extern "C"
