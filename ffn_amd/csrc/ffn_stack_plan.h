// Which conv kernel family runs a stack, decided in ONE place, and the arithmetic on the
// FoV geometry that decision rests on.  Host code only, no HIP: ffn_types.h and the
// standard library, so a plain C++ compiler builds it (tests/stack_plan_shim.cpp does).
//
//   conv_caps(g, depth)  what is fixed when an engine is created: the layout of the
//                        split-product family (gp: the FoV, or the FoV with its axes
//                        permuted), chunk counts, LDS spans and sizes, which families the
//                        geometry admits, the tap-offset schedules.  Nothing in it asks the
//                        device: whether a resident launch FITS the chip (flow_fits, the
//                        residency half of h_ok) stays with ffn_engine_create.
//   plan_stack(caps, options, n)  what is decided per stack: the family, whether it goes
//                        out as one resident launch, and how many entries per item its
//                        fused head leaves in `count`.
#ifndef FFN_STACK_PLAN_H_
#define FFN_STACK_PLAN_H_

#include <algorithm>
#include <cstddef>

#include "ffn_types.h"

// (timing-only experiment builds: treat the FoV as its first FFN_H_VCLIP voxels;
// ffn_conv_half.h)
#ifndef FFN_H_VCLIP
#define FFN_H_VCLIP 0
#endif

namespace ffn {

struct ConvCaps {
  Geom gp{};  // the FoV as the split-product kernels (conv_variant >= 6) lay it
              // out: the same, or with its axes permuted (oa) so that the
              // SHORTEST axis is the row direction -- rows of 21 instead of 41
              // voxels put the anisotropic 21 x 41 x 41 FoV inside the row
              // budget of conv32m / conv32mt
  bool permuted = false;
  long act_stride = 0;     // floats per FoV activation buffer (either layout fits)
  size_t lds_bytes = 0;    // conv32
  // conv32c (variant 2): 144-voxel chunks of the caller's layout
  int nchunks_c = 0, Rc = 0;
  size_t lds_bytes_c = 0;
  // conv32d (variant 6): 160-voxel chunks, the 27 taps split over the waves,
  // split-plane activations, LDS-DMA staging
  int nchunks_k = 0, Rc_k = 0;
  bool k_ok = false;       // the chunk + halo fits the LDS slots
  size_t lds_bytes_d = 0;  // 3 slots x 8 planes x Rc_k rows x 16 B
  bool d_ok = false;
  int dsched_aoff[4 * 8] = {};
  int dsched_btap[4 * 8] = {};
  // conv32d with 96-voxel chunks, two workgroups per CU (variant 7)
  int nchunks_e = 0;
  size_t lds_bytes_e = 0;
  bool e_ok = false;
  int esched_aoff[4 * 8] = {};
  // conv32m (variant 8): M split over the waves, weights through an LDS ring
  int nchunks_m = 0;
  bool m_ok = false;
  // conv32mt (variant 9): conv32m for the first n_main <= 256 chunks, 32-voxel
  // K-split tail workgroups for the rest (96-voxel ones for several FoVs)
  bool t_ok = false;
  int n_main = 0, n_tail = 0, n_tail3 = 0;
  int tsched_aoff[4 * 8] = {};
  int t3sched_aoff[4 * 8] = {};
  // conv32h / conv32hs (variant 10): 80-voxel workgroups
  int n_half = 0;          // 80-voxel chunks of the FoV
  bool h_geom_ok = false;  // the geometric half of ffn_engine::h_ok
  int exact_variant = 0;   // the f32 kernel a voided fp16 step is repeated with: 2
                           // where conv32c takes the FoV, else 0
  int default_variant = 0;
};

// the padded strides and counts that follow from a geometry's fz, fy, fx
inline void pad_geom(Geom& q) {
  q.XS = q.fx + 1;
  q.plane = (q.fy + 1) * q.XS;
  q.npos = q.fz * q.plane;
  q.guard = q.plane + q.XS + 1;
  q.nchunks = (q.npos + kChunk - 1) / kChunk;
  q.R = kChunk + 2 * (q.XS + 1);
}

// the FoV as the caller sees it (zyx); act_stride is conv_caps' to say
inline Geom fov_geom(const int32_t fov_zyx[3], const int32_t deltas_zyx[3]) {
  Geom g{};
  g.fz = fov_zyx[0], g.fy = fov_zyx[1], g.fx = fov_zyx[2];
  g.dz = deltas_zyx[0], g.dy = deltas_zyx[1], g.dx = deltas_zyx[2];
  pad_geom(g);
  g.V = g.fz * g.fy * g.fx;
  g.oa[0] = 0, g.oa[1] = 1, g.oa[2] = 2;
  g.dstr[0] = g.fy * g.fx, g.dstr[1] = g.fx, g.dstr[2] = 1;
  g.crop = 0;
  g.c0[0] = g.c0[1] = g.c0[2] = 0;
  g.c1[0] = g.fz, g.c1[1] = g.fy, g.c1[2] = g.fx;
  g.Vp = g.V;
  return g;
}

// the geometry with its axes permuted: internal axis a = original axis oa[a]
inline Geom permute(const Geom& g, const int oa[3]) {
  const int f[3] = {g.fz, g.fy, g.fx}, d[3] = {g.dz, g.dy, g.dx};
  const int ds[3] = {g.fy * g.fx, g.fx, 1};
  Geom q = g;
  q.fz = f[oa[0]], q.fy = f[oa[1]], q.fx = f[oa[2]];
  q.dz = d[oa[0]], q.dy = d[oa[1]], q.dx = d[oa[2]];
  pad_geom(q);
  for (int a = 0; a < 3; ++a) q.oa[a] = oa[a], q.dstr[a] = ds[oa[a]];
  return q;
}

// largest padded span of `count` chunks of `chunk` dense voxels from `start`
inline int chunk_span(const Geom& q, int start, int chunk, int count) {
  auto pad = [&](int v) {
    const int x = v % q.fx, y = (v / q.fx) % q.fy, z = v / (q.fx * q.fy);
    return z * q.plane + y * q.XS + x;
  };
  int span = 0;
  for (int c = 0; c < count; ++c) {
    const int lo = start + c * chunk, hi = std::min(q.V, lo + chunk) - 1;
    if (lo <= hi) span = std::max(span, pad(hi) - pad(lo) + 1);
  }
  return span;
}

inline bool m_fits(const Geom& q) {  // conv32m's 128-voxel chunks in kMRows rows
  return chunk_span(q, 0, kMChunk, (q.V + kMChunk - 1) / kMChunk) + 2 * (q.XS + 1) <= kMRows;
}

// tap schedule of the four waves (see conv32d_body): two dz = -1 taps
// each, then two taps of dz <= 0, then the rest; 7 / 7 / 7 / 6 taps
constexpr int kSched[4][7] = {{0, 1, 8, 9, 16, 18, 19},
                              {2, 3, 10, 11, 17, 20, 21},
                              {4, 5, 12, 13, 22, 23, 24},
                              {6, 7, 14, 15, 25, 26, -1}};

// byte offsets of the schedule's taps in the plane-major LDS image (8 planes x `rows`
// rows x 16 B per dz segment); wave 3's seventh tap repeats its sixth
inline void tap_offsets(int rows, int XS, int out[4 * 8]) {
  for (int w = 0; w < 4; ++w)
    for (int j = 0; j < 7; ++j) {
      int s = kSched[w][j];
      if (s < 0) s = kSched[w][j - 1];
      const int kz = s / 9, ky = (s / 3) % 3, kx = s % 3;
      out[w * 8 + j] = kz * 128 * rows + ((ky - 1) * XS + (kx - 1)) * 16;
    }
}

// g: the FoV as the caller sees it (everything but act_stride filled in)
inline ConvCaps conv_caps(const Geom& g, int depth) {
  ConvCaps c;
  c.gp = g;
  if (!m_fits(g)) {
    // shortest axis last (= the row direction), the other two in their order
    // (tools/fov_edges.py, every odd FoV up to 131 per axis with V <= 70,000: (2,0,1) and
    // (2,1,0) are chosen by none of them -- an earlier row has rows as short and fits
    // wherever they do; (1,0,2) only by the columns 73 x 3 x 3 ... 131 x 3 x 3)
    static const int kPerms[5][3] = {{0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    int best = -1;
    for (int k = 0; k < 5; ++k) {
      const Geom q = permute(g, kPerms[k]);
      if (m_fits(q) && (best < 0 || q.fx < permute(g, kPerms[best]).fx)) best = k;
    }
    if (best >= 0) {
      c.gp = permute(g, kPerms[best]);
      c.permuted = true;
    }
  }
  const long positions =
      std::max((long)g.guard + (long)g.nchunks * kChunk + g.guard + 320,
               (long)c.gp.guard + (long)c.gp.nchunks * kChunk + c.gp.guard + 320);
  c.act_stride = positions * kFeatures;
  c.gp.act_stride = c.act_stride;
  c.lds_bytes = (size_t)3 * g.R * kFeatures * sizeof(float);

  // LDS extent of the compact variant (the caller's layout)
  c.nchunks_c = (g.V + kCChunk - 1) / kCChunk;
  c.Rc = ((chunk_span(g, 0, kCChunk, c.nchunks_c) + 2 * (g.XS + 1)) + 31) / 32 * 32;
  if (c.Rc < 256) c.Rc = 256;  // the kernel stages 8 or 9 x 256 float4
  c.lds_bytes_c = (size_t)2 * c.Rc * kCLdsStride * sizeof(float);

  // everything from here on is the split-product family: laid out as gp
  const Geom& q = c.gp;
  const int halo = 2 * (q.XS + 1);
  c.nchunks_k = (g.V + kDChunk - 1) / kDChunk;
  c.Rc_k = ((chunk_span(q, 0, kDChunk, c.nchunks_k) + halo) + 31) / 32 * 32;
  if (c.Rc_k < 256) c.Rc_k = 256;
  c.k_ok = c.Rc_k <= 320 && c.nchunks_k >= 2;  // (magic divisions: d >= 2)
  c.lds_bytes_d = std::max((size_t)3 * 128 * c.Rc_k, (size_t)4 * kDChunk * kDRowB + 64);
  tap_offsets(c.Rc_k, q.XS, c.dsched_aoff);
  for (int w = 0; w < 4; ++w)  // wave 3's seventh tap is the all-zero tap 27
    for (int j = 0; j < 7; ++j) c.dsched_btap[w * 8 + j] = kSched[w][j] < 0 ? 27 : kSched[w][j];
  c.d_ok = c.k_ok && c.lds_bytes_d <= 160 * 1024 && depth >= 2;
  // variant 7: 96-voxel chunks in kERows rows, three slots in 80 KB
  const int ce = 32 * kETiles;
  c.nchunks_e = (q.V + ce - 1) / ce;
  c.lds_bytes_e = std::max((size_t)3 * 128 * kERows, (size_t)4 * ce * kDRowB + 64);
  c.e_ok = c.d_ok && chunk_span(q, 0, ce, c.nchunks_e) + halo <= kERows &&
           c.nchunks_e >= 2 && c.lds_bytes_e <= 80 * 1024;
  tap_offsets(kERows, q.XS, c.esched_aoff);
  // variant 8: 128-voxel chunks in kMRows rows
  c.nchunks_m = (q.V + kMChunk - 1) / kMChunk;
  c.m_ok = c.d_ok && chunk_span(q, 0, kMChunk, c.nchunks_m) + halo <= kMRows &&
           c.nchunks_m >= 2;
  // variant 9: the chunks past the 256th become 32-voxel tail workgroups,
  // as long as all of one FoV's workgroups find a slot at once (two per CU)
  if (c.m_ok && c.nchunks_m > 256) {
    c.n_main = 256;
    c.n_tail = (q.V - 256 * kMChunk + 31) / 32;
    c.n_tail3 = (q.V - 256 * kMChunk + 95) / 96;
    static_assert((size_t)3 * 128 * kTRows <= kMLdsBytes &&
                      (size_t)4 * 32 * kDRowB + 64 <= kMLdsBytes &&
                      (size_t)3 * 128 * kT3Rows <= kMLdsBytes &&
                      (size_t)4 * 96 * kDRowB + 64 <= kMLdsBytes,
                  "a tail workgroup fits conv32m's LDS");
    c.t_ok = chunk_span(q, 256 * kMChunk, 32, c.n_tail) + halo <= kTRows &&
             chunk_span(q, 256 * kMChunk, 96, c.n_tail3) + halo <= kT3Rows && c.n_tail <= 256;
    tap_offsets(kTRows, q.XS, c.tsched_aoff);
    tap_offsets(kT3Rows, q.XS, c.t3sched_aoff);
  }
  // conv32hs (variant 10): 80-voxel workgroups, two per CU, all resident at once
  if (c.t_ok && depth >= 2) {
    c.n_half = FFN_H_VCLIP ? FFN_H_VCLIP / kHChunk : (q.V + kHChunk - 1) / kHChunk;
    c.h_geom_ok = c.n_half >= 2 && chunk_span(q, 0, kHChunk, c.n_half) + halo <= kHRows;
  }
  // default: conv32mt / conv32m where the geometry allows them (33^3: yes), else
  // conv32d, else the exact-f32 kernels (conv32c -- it needs Rc in {256, 288} -- or
  // conv32 for any FoV that fits the LDS at all)
  c.exact_variant = (c.Rc == 256 || c.Rc == 288) ? 2 : 0;
  c.default_variant = c.t_ok ? 9 : c.m_ok ? 8 : c.d_ok ? 6 : c.exact_variant;
  return c;
}

// The kernel family of the 2 depth - 1 convs of a stack:
//   Conv32   conv32, any FoV (variant 0)          Conv32c  exact f32 (variant 2)
//   D160     conv32d, one workgroup per CU        D96      its 96-voxel form, two per CU
//   M        conv32m                              MT       conv32mt: conv32m + K-split tail
//   H        conv32h: 80-voxel workgroups
enum class ConvFamily { Conv32, Conv32c, D160, D96, M, MT, H };

struct StackPlan {
  ConvFamily family;
  bool resident;   // ONE launch for all convs (conv32ps for MT, conv32hs for H)
  int tail_tiles;  // MT: 32-voxel tiles per tail workgroup, 1 or 3
  int chunks;      // entries per item in `count` when the head is fused
  int products;    // MFMA products per fp16 operand pair: 3, or 1 (M and MT alone)
};

// conv32d: one workgroup per CU (160-voxel chunks) for a single FoV; with several FoVs
// in flight the 96-voxel form (two workgroups per CU, the same arithmetic bit for bit)
// overlaps one workgroup's MFMAs with the other's staging and epilogue.
// variant 9: a single FoV runs conv32mt (balance over the CUs: +14 %); steps with
// several FoVs run plain conv32m (cost per voxel: the K-split tail costs 5-10 % there)
// unless tail_batched asks for the single-FoV bits.
// variant 10: a single FoV on 80-voxel workgroups (conv32hs / conv32h); steps with
// several FoVs run plain conv32m, as under 9.
// A resident launch is for ONE FoV, with flow = 2 and no repeat of a voided resident step
// pending (flow_skip: the caller counts it down).
// products (engine option mfma_products) = 1: the families M and MT keep the hi x hi
// product alone; every other family has no such form and runs as it always does
// (StackPlan::products says 3 for it).  The one-product kernels exist as per-layer
// launches only, so such a plan is never resident: a single FoV runs conv32mt as it does
// with flow = 0.
inline StackPlan plan_stack(const ConvCaps& c, int conv_variant, int flow, int flow_skip,
                            int tail_batched, int batch_chunks, int n, int products = 3) {
  StackPlan p{ConvFamily::D160, false, 1, c.nchunks_k, 3};
  if (conv_variant == 0) {
    p.family = ConvFamily::Conv32, p.chunks = 0;  // (its head is never fused)
  } else if (conv_variant < 6) {
    p.family = ConvFamily::Conv32c, p.chunks = c.nchunks_c;
  } else if (conv_variant == 10 && n == 1) {
    p.family = ConvFamily::H, p.chunks = c.n_half;
  } else if (conv_variant == 9 && (n == 1 || tail_batched != 0)) {
    p.family = ConvFamily::MT;
    p.tail_tiles = n == 1 ? 1 : 3;
    p.chunks = c.n_main + (n == 1 ? c.n_tail : c.n_tail3);
  } else if (conv_variant >= 8 ||
             (conv_variant == 6 && batch_chunks == 2 && n >= 2 && c.m_ok)) {
    p.family = ConvFamily::M, p.chunks = c.nchunks_m;
  } else if (conv_variant == 7 ||
             (conv_variant == 6 && batch_chunks == 1 && n >= 2 && c.e_ok)) {
    p.family = ConvFamily::D96, p.chunks = c.nchunks_e;
  }
  if (products == 1 && (p.family == ConvFamily::M || p.family == ConvFamily::MT))
    p.products = 1;
  p.resident = (p.family == ConvFamily::MT || p.family == ConvFamily::H) && n == 1 &&
               flow == 2 && flow_skip == 0 && p.products == 3;
  return p;
}

// the resident launch of conv32mt (conv32ps): the one that is timed by its own dispatch,
// that a stack may be queued ahead with, and whose beat tune_pace() measures
inline bool resident_mt(const StackPlan& p) {
  return p.resident && p.family == ConvFamily::MT;
}

}  // namespace ffn

#endif  // FFN_STACK_PLAN_H_
