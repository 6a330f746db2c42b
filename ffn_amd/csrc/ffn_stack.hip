// The conv launch layer of libffn_hip.so (ffn_stack.h): run_stack and the walker that
// queues a stack conv by conv, conv0_a in front of it, the head behind it, and the
// exact-f32 kernels (conv32, conv32c).  The split-product families are launched from
// units of their own (ffn_stack_units.h); what their launches share -- the argument
// builders -- is defined here.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "ffn_stack.h"
#include "ffn_stack_units.h"
#include "ffn_conv0a.h"
#include "ffn_conv_exact.h"

int event_pair(ffn_engine* e) {
  return e->events_used + 2 > (int)e->events.size() ? flush_events(e) : FFN_OK;
}

int prof_begin(ffn_engine* e) {
  if (!e->prof_now) return FFN_OK;
  if (int rc = event_pair(e)) return rc;
  HIP_TRY(hipEventRecord(e->events[e->events_used++], e->stream));
  return FFN_OK;
}
int prof_end(ffn_engine* e) {
  if (e->prof_now) HIP_TRY(hipEventRecord(e->events[e->events_used++], e->stream));
  return FFN_OK;
}

namespace {

// A conv of the exact-f32 stacks: ReLU on its input, ReLU on its output, the residual.
struct ExactConv {
  bool ri, ro, sk;
};
constexpr ExactConv kExactFirst{false, false, false}, kExactA{true, true, false},
    kExactB{false, false, true};
// conv32c also by LDS rows (KS = 8: 256, 9: 288), with the head fused, and -- conv_b with
// 256 rows alone -- as an issue-rate experiment (DBG = engine option ablate: 8, 16, 24)
constexpr int exact_key(ExactConv c, int dbg = 0, int ks = 8, bool head = false) {
  return (c.ri ? 1 : 0) | (c.ro ? 2 : 0) | (c.sk ? 4 : 0) | (head ? 8 : 0) | ks * 16 | dbg * 256;
}

#define FFN_EXACT_CONVS(X) X(false, false, false), X(true, true, false), X(false, false, true)

const KernelForm<void (*)(ConvArgs)> kConv32Forms[] = {
#define FFN_FORM(RI, RO, SK) {exact_key({RI, RO, SK}), conv32_kernel<RI, RO, SK>}
    FFN_EXACT_CONVS(FFN_FORM)
#undef FFN_FORM
};

const KernelForm<void (*)(ConvCArgs)> kConv32cForms[] = {
#define FFN_FORM(RI, RO, SK)                                                      \
  {exact_key({RI, RO, SK}, 0, 8), conv32c_kernel<RI, RO, SK, 0, 8>},              \
  {exact_key({RI, RO, SK}, 0, 9), conv32c_kernel<RI, RO, SK, 0, 9>},              \
  {exact_key({RI, RO, SK}, 0, 8, true), conv32c_kernel<RI, RO, SK, 0, 8, true>},  \
  {exact_key({RI, RO, SK}, 0, 9, true), conv32c_kernel<RI, RO, SK, 0, 9, true>}
    FFN_EXACT_CONVS(FFN_FORM),
#undef FFN_FORM
    {exact_key(kExactB, 8), conv32c_kernel<false, false, true, 8>},
    {exact_key(kExactB, 16), conv32c_kernel<false, false, true, 16>},
    {exact_key(kExactB, 24), conv32c_kernel<false, false, true, 24>},
};
#undef FFN_EXACT_CONVS

int launch_conv32(ffn_engine* e, int n, ExactConv conv, const float* in, float* out,
                  const float* skip, int layer) {
  ConvArgs a;
  a.in = in;
  a.out = out;
  a.skip = skip;
  a.wpack = e->weights + e->wpack_off[layer];
  a.bias = e->weights + e->bias_off[layer];
  a.valid = e->valid;
  a.act_stride = e->g.act_stride;
  a.XS = e->g.XS;
  a.plane = e->g.plane;
  a.R = e->g.R;
  a.nchunks = e->g.nchunks;
  const auto kernel = find_form(kConv32Forms, exact_key(conv));
  if (!kernel) return no_form("conv32", conv.ri, conv.sk, false);
  if (int rc = prof_begin(e)) return rc;
  hipLaunchKernelGGL(kernel, dim3(n * e->g.nchunks), dim3(kConvThreads), e->caps.lds_bytes,
                     e->stream, a);
  return prof_end(e);
}

int launch_conv32c(ffn_engine* e, int n, ExactConv conv, const float* in, float* out,
                   const float* skip, int layer, const HeadFusion& head = HeadFusion()) {
  ConvCArgs a;
  a.in = in;
  a.out = out;
  a.skip = skip;
  a.wpack = e->weights + e->wpack_off[layer];
  a.bias = e->weights + e->bias_off[layer];
  a.pidx = e->pidx;
  a.act_stride = e->g.act_stride;
  a.XS = e->g.XS;
  a.plane = e->g.plane;
  a.Rc = e->caps.Rc;
  a.nchunks = e->caps.nchunks_c;
  a.V = e->g.V;
  a.fx = e->g.fx;
  a.fyfx = e->g.fy * e->g.fx;
  a.total_slots = n * e->caps.nchunks_c;
  a.slots_per_xcd = (a.total_slots + 7) / 8;
  a.nbytes = (unsigned)((size_t)e->g.nchunks * kChunk * kFeatures * sizeof(float));
  a.store_policy = e->store_policy;
  // clocks of ONE mid-stack launch (a conv_a: ReLU in and out, no residual)
  a.dbg = (e->dbg_clock && layer == e->dbg_layer) ? e->d_dbg : nullptr;
  a.head_w = e->weights + e->wl_off;
  a.seed_raw = e->seed_raw;
  a.logits = e->logits;
  a.head_count = e->count;
  a.pad_value = head.pad_value;
  a.move_thr = head.move_thr;
  a.range_flag = e->range_flag;
  a.range_tag = e->range_tag;
  // issue-rate experiments (conv_b with 256 rows only; never with the head)
  const bool ablated = conv.sk && e->ablate != 0 && e->caps.Rc == 256;
  const auto kernel =
      find_form(kConv32cForms, ablated ? exact_key(conv, e->ablate)
                                       : exact_key(conv, 0, e->caps.Rc == 256 ? 8 : 9, head.on));
  if (!kernel && ablated)
    return fail(FFN_ERR_ARG, "unsupported ablate mask %d for variant 2", e->ablate);
  if (!kernel) return no_form("conv32c", conv.ri, conv.sk, head.on);
  if (int rc = prof_begin(e)) return rc;
  const dim3 grid(8 * a.slots_per_xcd), block(kConvThreads);
  hipLaunchKernelGGL(kernel, grid, block, e->caps.lds_bytes_c, e->stream, a);
  return prof_end(e);
}

}  // namespace

int switch_variant(ffn_engine* e, int value) {
  if ((value >= 6) != (e->conv_variant >= 6)) {
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipMemsetAsync(e->act_base, 0,
                           (size_t)3 * e->max_batch * e->g.act_stride * sizeof(float),
                           e->stream));
  }
  e->conv_variant = value;
  return FFN_OK;
}

void conv32d_args(ffn_engine* e, const StackPlan& plan, int n, const float* raw_in,
                  float* raw_out, int layer, const HeadFusion& head, ConvDArgs& a) {
  const Geom& g = e->caps.gp;
  const long positions = g.act_stride / kFeatures;
  a.L.in_sp = reinterpret_cast<const char*>(raw_in) + (size_t)g.guard * 16;
  a.L.out_sp = reinterpret_cast<char*>(raw_out) + (size_t)g.guard * 16;
  a.x_f32 = e->rawX + (size_t)g.guard * 4;
  a.L.wpack = reinterpret_cast<const char*>(e->wpackd + (size_t)layer * e->wpackd_layer);
  a.L.bias = e->weights + e->bias_off[layer];
  a.item_bytes = g.act_stride * (long)sizeof(float);
  a.sp_plane_bytes = positions * 16;
  a.XS = g.XS;
  a.plane = g.plane;
  // the chunks of a plain launch: conv32m's 128-voxel ones (MT and H bring their own
  // maps and read conv32m's count), 96-voxel ones, or conv32d's 160-voxel ones
  const bool small = plan.family == ConvFamily::D96;
  const int nchunks = small ? e->caps.nchunks_e
                      : plan.family == ConvFamily::D160 ? e->caps.nchunks_k
                                                        : e->caps.nchunks_m;
  a.nchunks = nchunks;
  a.V = g.V;
  a.fx = g.fx;
  a.fyfx = g.fy * g.fx;
  a.total_slots = n * nchunks;
  a.slots_per_xcd = (a.total_slots + 7) / 8;
  auto magic = [](int d) { return (unsigned)(((1ull << 32) + d - 1) / d); };
  a.magic_nchunks = magic(nchunks);
  a.magic_fyfx = magic(g.fy * g.fx);
  a.magic_fx = magic(g.fx);
  a.permuted = e->caps.permuted;
  a.ds0 = g.dstr[0];
  a.ds1 = g.dstr[1];
  a.ds2 = g.dstr[2];
  a.sp_bytes = (unsigned)((size_t)g.act_stride * sizeof(float) - (size_t)g.guard * 32);
  std::memcpy(a.aoff, small ? e->caps.esched_aoff : e->caps.dsched_aoff, sizeof(a.aoff));
  std::memcpy(a.btap, e->caps.dsched_btap, sizeof(a.btap));
  a.L.dbg = (e->dbg_clock && layer == e->dbg_layer) ? e->d_dbg : nullptr;
  a.dbg_wgs = e->dbg_clock == 2 ? 1 : e->dbg_clock == 3 ? 2 : 0;
  a.head_w = e->weights + e->wl_off;
  a.seed_raw = e->seed_raw;
  a.logits = e->logits;
  a.head_count = e->count;
  a.pad_value = head.pad_value;
  a.move_thr = head.move_thr;
  a.range_flag = e->range_flag;
  a.range_tag = e->range_tag;
  a.flow_flags = e->flow_flags;
  a.flow_n_main = e->caps.n_main;
  a.flow_err = e->flow_err;
  a.flow_halo = g.fy * g.fx + g.fx + 1;
  a.flow_dbg = e->flow_debug;
  a.flow_trace = e->dbg_clock == 4 ? e->flow_trace : nullptr;
  a.L.layer = layer;
  a.L.flow_wait_on = 0;
  a.L.flow_wait = a.L.flow_set = 0;
}

void tail_map(const ffn_engine* e, int n, ConvTailMap& mp) {
  const bool one = n == 1;
  mp.n = n;
  mp.n_main = e->caps.n_main;
  mp.n_tail = one ? e->caps.n_tail : e->caps.n_tail3;
  mp.mains_per_xcd = (mp.n_main + 7) / 8;
  mp.tails_per_xcd = (mp.n_tail + 7) / 8;
  std::memcpy(mp.taoff, one ? e->caps.tsched_aoff : e->caps.t3sched_aoff, sizeof(mp.taoff));
}

int conv0a_split_args(ffn_engine* e, float pad_value, unsigned tag, const SpecArgs& sp,
                      bool next, Conv0Next& nx) {
  const float* W = e->weights;
  const Geom& q = e->caps.gp;  // the split-product kernels' layout of the FoV
  const int qz = (q.fz + kC0Z - 1) / kC0Z, qy = (q.fy + kC0Y - 1) / kC0Y,
            qx = (q.fx + kC0X - 1) / kC0X;
  nx.pad_value = pad_value;
  nx.w = W + (e->caps.permuted ? e->w0ap_off : e->w0a_off);
  nx.bias = W + e->b0a_off;
  nx.out = e->bufT;
  nx.seed_raw = next ? e->seed_raw_alt : e->seed_raw;
  nx.q = q;
  nx.tiles_y = qy;
  nx.tiles_x = qx;
  nx.so.out_sp = reinterpret_cast<char*>(e->rawT) + (size_t)q.guard * 16;
  nx.so.sp_plane_bytes = (q.act_stride / kFeatures) * 16;
  nx.so.item_bytes = q.act_stride * (long)sizeof(float);
  nx.so.range_flag = next ? e->range_flag_alt : e->range_flag;
  nx.so.range_tag = tag;
  nx.sp = sp;
  if (sp.n > 0) nx.sp.choice = next ? e->d_spec_choice_alt : e->d_spec_choice;
  return qz * qy * qx;
}

void launch_conv0a(ffn_engine* e, int n, const StepItems& si, float pad_value,
                   unsigned tag, const SpecArgs& sp, bool next) {
  const Geom& g = e->g;
  const float* W = e->weights;
  const int tz = (g.fz + kC0Z - 1) / kC0Z, ty = (g.fy + kC0Y - 1) / kC0Y,
            tx = (g.fx + kC0X - 1) / kC0X;
  if (e->conv_variant >= 6) {
    Conv0Next nx;
    const int tiles = conv0a_split_args(e, pad_value, tag, sp, next, nx);
    hipLaunchKernelGGL(conv0a_mfma_kernel<true>, dim3(tiles, n),
                       dim3(kC0Threads), 0, e->stream, si, pad_value, nx.w, nx.bias,
                       nx.out, nx.seed_raw, nx.q, nx.tiles_y, nx.tiles_x, nx.so, nx.sp);
  } else {
    SpecArgs sp2 = sp;
    if (sp.n > 0) sp2.choice = next ? e->d_spec_choice_alt : e->d_spec_choice;
    hipLaunchKernelGGL(conv0a_mfma_kernel<false>, dim3(tz * ty * tx, n),
                       dim3(kC0Threads), 0, e->stream, si, pad_value,
                       W + e->w0a_off, W + e->b0a_off, e->bufT,
                       next ? e->seed_raw_alt : e->seed_raw, g, ty, tx,
                       Conv0SplitOut(), sp2);
  }
}

void stack_tab(ffn_engine* e, const uint16_t* wpack, int auto_pace, ConvStackTab* tb) {
  const Geom& g = e->caps.gp;
  tb->nlayers = 2 * e->depth - 1;
  tb->dbg_layer = e->dbg_layer;
  tb->sp_t = reinterpret_cast<const char*>(e->rawT) + (size_t)g.guard * 16;
  tb->sp_s = reinterpret_cast<char*>(e->rawS) + (size_t)g.guard * 16;
  tb->wpack0 = reinterpret_cast<const char*>(wpack);
  tb->wpack_stride = (long)(e->wpackd_layer * sizeof(uint16_t));
  tb->bias0 = e->weights + e->bias_off[0];
  tb->bias_stride = e->depth > 1 ? (long)(e->bias_off[1] - e->bias_off[0]) : 0;
  tb->epoch0 = e->flow_epoch;
  e->flow_epoch += (unsigned)tb->nlayers;
  tb->l_begin = 0;
  tb->l_end = tb->nlayers;
  tb->pace = e->flow_pace < 0 ? auto_pace : e->flow_pace;
  tb->pace_tail = 0;
  tb->pace_spread = e->flow_pace_spread < 0 ? tb->pace : e->flow_pace_spread;
  tb->stamps = nullptr;
  tb->ahead_choice = nullptr;
  tb->trace = 0;
}

StackPlan plan_for(const ffn_engine* e, int n, int flow_skip) {
  return plan_stack(e->caps, e->conv_variant, e->flow, flow_skip, e->tail_batched,
                    e->batch_chunks, n, e->mfma_products);
}

namespace {
// The chain of launches of a stack, one per conv: conv0_b, then per residual module
// conv_a (layer 2 i - 1) and conv_b (layer 2 i; last: the one that may take the head).
template <class First, class A, class B>
int walk_stack(int depth, First first, A conv_a, B conv_b) {
  int rc = first();
  for (int i = 1; i < depth && !rc; ++i) {
    rc = conv_a(2 * i - 1);
    if (!rc) rc = conv_b(2 * i, i == depth - 1);
  }
  return rc;
}
}  // namespace

int run_stack(ffn_engine* e, int n, const StepItems& si, float pad_value, float move_thr,
              bool conv0a_done, bool ahead) {
  const Geom& g = e->g;
  const float* W = e->weights;
  if (!conv0a_done) drop_spec(e);
  if (e->ahead_valid) e->stat_ahead_wasted += 1;  // (a caller that steps past it)
  e->spec.valid = false;
  e->ahead_valid = false;
  e->last_stack_resident = false;
  e->range_tag = next_tag(e->range_tag);
  // this step's set of conv0_a outputs: what a launch made ahead for it wrote,
  // what its own conv0_a (below) writes
  std::swap(e->seed_raw, e->seed_raw_alt);
  std::swap(e->range_flag, e->range_flag_alt);
  std::swap(e->d_spec_choice, e->d_spec_choice_alt);
  const bool sampled = (e->stack_calls % e->prof_every) == 0;
  e->stack_calls++;
  e->prof_now = e->prof_mode == 1 && sampled;
  const bool prof_chain = e->prof_mode == 2 && sampled;
  if (!conv0a_done) launch_conv0a(e, n, si, pad_value, e->range_tag, SpecArgs());
  bool head_fused = false;
  e->ahead_ev_pending = false;
  const StackPlan plan = plan_for(e, n, e->flow_skip);
  if ((plan.family == ConvFamily::MT || plan.family == ConvFamily::H) && n == 1 &&
      e->flow == 2 && e->flow_skip > 0)
    e->flow_skip -= 1;  // the repeat of a voided resident step: per-layer launches
  // a sampled stack that runs as ONE resident launch is timed by that dispatch's own
  // start / end (launch_conv32ps); a chain of launches by markers around it (and so is
  // conv32hs, and the resident launch of an engine with tail_batched set)
  const bool one_launch = resident_mt(plan) && e->tail_batched == 0;
  hipEvent_t k_ev0 = nullptr, k_ev1 = nullptr;
  if (prof_chain && ahead) {
    if (one_launch) k_ev0 = e->ahead_ev[0], k_ev1 = e->ahead_ev[1];
    else HIP_TRY(hipEventRecord(e->ahead_ev[0], e->stream));
  } else if (prof_chain) {
    if (int rc = event_pair(e)) return rc;
    e->chain_launches_pending.push_back(2 * e->depth - 1);
    if (one_launch) {
      k_ev0 = e->events[e->events_used], k_ev1 = e->events[e->events_used + 1];
      e->events_used += 2;
    } else {
      HIP_TRY(hipEventRecord(e->events[e->events_used++], e->stream));
    }
  }
  int rc;
  if (e->conv_variant >= 6 && e->depth == 1)
    return fail(FFN_ERR_ARG, "conv_variant 6 needs depth >= 2 (fused head)");
  if (ahead && !resident_mt(plan))
    return fail(FFN_ERR_STATE, "stack_ahead without the resident launch");
  // the split-product families: T' -> (X, X') -> T' -> ... ; the head is always fused
  // into the last conv_b
  const auto head = [&](bool on) { return head_fusion(on, pad_value, move_thr); };
  e->last_stack_resident = plan.resident;
  if (plan.resident) {
    rc = plan.family == ConvFamily::H
             ? launch_conv32hs(e, plan, pad_value, move_thr)
             : launch_conv32ps(e, plan, pad_value, move_thr,
                               ahead ? e->d_spec_choice : nullptr, k_ev0, k_ev1);
    head_fused = true;
  } else if (e->conv_variant >= 6) {
    // one conv of the plan's family: KIND 0 conv_a, KIND 1 conv_b (sk: with the residual)
    const auto conv = [&](int kind, bool sk, const float* in, float* out, int l,
                          const HeadFusion& hf = HeadFusion()) {
      switch (plan.family) {
        case ConvFamily::H: return launch_conv32h(e, plan, kind, sk, in, out, l, hf);
        case ConvFamily::M:
        case ConvFamily::MT: return launch_conv32m(e, plan, n, kind, sk, in, out, l, hf);
        default: return launch_conv32d(e, plan, n, kind, sk, in, out, l, hf);
      }
    };
    rc = walk_stack(
        e->depth, [&] { return conv(1, false, e->rawT, e->rawS, 0); },
        [&](int l) { return conv(0, false, e->rawS, e->rawT, l); },
        [&](int l, bool last) { return conv(1, true, e->rawT, e->rawS, l, head(last)); });
    head_fused = true;
  } else if (plan.family == ConvFamily::Conv32) {
    rc = walk_stack(
        e->depth, [&] { return launch_conv32(e, n, kExactFirst, e->bufT, e->bufX, nullptr, 0); },
        [&](int l) { return launch_conv32(e, n, kExactA, e->bufX, e->bufT, nullptr, l); },
        [&](int l, bool) { return launch_conv32(e, n, kExactB, e->bufT, e->bufX, e->bufX, l); });
  } else {
    // conv_variant 2: T is post-ReLU (conv0_a / conv_a apply it), X is the raw
    // residual stream
    rc = walk_stack(
        e->depth, [&] { return launch_conv32c(e, n, kExactFirst, e->bufT, e->bufX, nullptr, 0); },
        [&](int l) { return launch_conv32c(e, n, kExactA, e->bufX, e->bufT, nullptr, l); },
        [&](int l, bool last) {
          head_fused = e->fuse_head && last && e->ablate == 0;
          return launch_conv32c(e, n, kExactB, e->bufT, e->bufX, e->bufX, l, head(head_fused));
        });
  }
  if (rc) return rc;
  if (prof_chain && ahead) {
    if (!k_ev0) HIP_TRY(hipEventRecord(e->ahead_ev[1], e->stream));
    e->ahead_ev_pending = true;
  } else if (prof_chain && !k_ev0) {
    HIP_TRY(hipEventRecord(e->events[e->events_used++], e->stream));
  }
  e->count_blocks = head_fused ? plan.chunks : kHeadBlocks;
  if (!head_fused)
    hipLaunchKernelGGL(head_kernel, dim3(kHeadBlocks, n), dim3(256), 0, e->stream,
                       e->bufX, e->seed_raw, pad_value, W + e->wl_off, move_thr,
                       e->logits, e->count, g);
  HIP_TRY(hipGetLastError());
  return FFN_OK;
}

int set_stack_lds_attrs(ffn_engine* e) {
  const ConvCaps& caps = e->caps;
  if (int rc = set_lds_attr(kConv32Forms, caps.lds_bytes)) return rc;
  // conv32c only where it takes the FoV (set_conv_variant refuses 2 elsewhere): rows past
  // 119 voxels put lds_bytes_c beyond what a workgroup may ask for, and asking failed
  // the creation of an engine that conv32 and the split-product kernels can serve
  if (caps.exact_variant == 2)
    if (int rc = set_lds_attr(kConv32cForms, caps.lds_bytes_c)) return rc;
  if (caps.d_ok)
    if (int rc = set_lds_attr_d(caps)) return rc;
  if (caps.m_ok) {
    if (int rc = set_lds_attr_m()) return rc;
    if (int rc = set_lds_attr_ps()) return rc;
    if (int rc = set_lds_attr_h()) return rc;
  }
  return FFN_OK;
}

// A resident launch's workgroups wait for each other, so one that is not on the chip
// stalls the rest until their polls give up (a partitioned device, fewer CUs than main
// chunks): each is granted only where the device holds all of its workgroups at once.
int stack_residency(ffn_engine* e) {
  if (!e->caps.t_ok || e->depth < 2) return FFN_OK;
  bool fits = false;
  if (int rc = conv32ps_fits(e, &fits)) return rc;
  e->flow_fits = fits;
  if (int rc = conv32hs_fits(e, &fits)) return rc;
  e->h_ok = e->caps.h_geom_ok && fits;
  return FFN_OK;
}
