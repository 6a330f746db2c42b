// TEST INFRASTRUCTURE: ffn_amd/csrc/ffn_stack_plan.h (conv_caps, plan_stack) behind a C
// interface, built with g++ alone -- no HIP, no GPU (tests/test_stack_plan.py).
#include <cstring>

#include "../ffn_amd/csrc/ffn_stack_plan.h"

using namespace ffn;

extern "C" {

void* shim_caps_create(const int32_t fov_zyx[3], const int32_t deltas_zyx[3], int depth) {
  return new ConvCaps(conv_caps(fov_geom(fov_zyx, deltas_zyx), depth));
}

void shim_caps_destroy(void* h) { delete static_cast<ConvCaps*>(h); }

// caps whose geometry refuses the 96-voxel / the conv32m form (the truth table's second set)
void shim_caps_clear_ok(void* h, int clear_e_ok, int clear_m_ok) {
  ConvCaps* c = static_cast<ConvCaps*>(h);
  if (clear_e_ok) c->e_ok = false;
  if (clear_m_ok) c->m_ok = false;
}

// the scalar fields, in the order of tests/test_stack_plan.py CAPS_FIELDS; returns their number
int shim_caps_fields(const void* h, long long* out) {
  const ConvCaps& c = *static_cast<const ConvCaps*>(h);
  const long long v[] = {
      c.gp.fz, c.gp.fy, c.gp.fx, c.gp.XS, c.gp.oa[0], c.gp.oa[1], c.gp.oa[2], c.permuted,
      c.nchunks_c, c.nchunks_k, c.nchunks_e, c.nchunks_m, c.Rc, c.Rc_k,
      (long long)c.lds_bytes, (long long)c.lds_bytes_c, (long long)c.lds_bytes_d,
      (long long)c.lds_bytes_e, c.k_ok, c.d_ok, c.e_ok, c.m_ok, c.t_ok, c.n_main, c.n_tail,
      c.n_tail3, c.n_half, c.h_geom_ok, c.exact_variant, c.default_variant, c.act_stride};
  const int n = (int)(sizeof(v) / sizeof(v[0]));
  if (out) std::memcpy(out, v, sizeof(v));
  return n;
}

// which: 0 dsched_aoff, 1 dsched_btap, 2 esched_aoff, 3 tsched_aoff, 4 t3sched_aoff
void shim_caps_schedule(const void* h, int which, int32_t out[32]) {
  const ConvCaps& c = *static_cast<const ConvCaps*>(h);
  const int* src[5] = {c.dsched_aoff, c.dsched_btap, c.esched_aoff, c.tsched_aoff,
                       c.t3sched_aoff};
  std::memcpy(out, src[which], 32 * sizeof(int32_t));
}

// out: family (the enum's order), resident, tail_tiles, chunks
void shim_plan_stack(const void* h, int conv_variant, int flow, int flow_skip, int tail_batched,
                     int batch_chunks, int n, int32_t out[4]) {
  const StackPlan p = plan_stack(*static_cast<const ConvCaps*>(h), conv_variant, flow,
                                 flow_skip, tail_batched, batch_chunks, n);
  out[0] = (int)p.family;
  out[1] = p.resident;
  out[2] = p.tail_tiles;
  out[3] = p.chunks;
}

}  // extern "C"
