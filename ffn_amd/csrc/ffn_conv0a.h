// conv0_a, the conv in front of the stack, and what its launches are described with
// (StepItems, SpecArgs, Conv0SplitOut, Conv0Next).  Templates and __forceinline__ device
// code only, so both sides may include it, behind ffn_kernels.h: the stack launches
// conv0a_mfma_kernel (ffn_stack.hip), the step's fused launch runs conv0a_body as its last
// role (ffn_step_kernels.h).
#pragma once

namespace ffn {

// ---------------------------------------------------------------------------
// conv0a: gather + concat(image, seed) -> 3x3x3 conv 2->32 + bias + ReLU
// (reference inference.py:348-354,399-407; convstack_3d.py:38,86).
//
// Reads the FoV straight out of the canvas volumes (or, for the stateless
// predict path, out of the uploaded dense FoV treated as a FoV-sized canvas),
// substitutes pad_value for NaN ("never visited") seed voxels, and also writes
// the raw (NaN-preserving) seed FoV to `seed_raw`, which the head (seed + update)
// and the paste kernel (disco mask) need later.  K = 54 only: VALU.
// One block = a 4x8x8 tile of positions: the tile + halo is staged once in LDS
// (one canvas read per input voxel), every thread then computes all 32 output
// channels of its position with the weights coming through the scalar cache.
// ---------------------------------------------------------------------------
struct StepItems {
  const StepItem* items;  // device array (batched path)
  StepItem inline_item;   // kernarg copy (single-canvas fast path)
  int use_inline;
};

// What the gather / faces / paste kernels read of a StepItem, in registers: with
// `const StepItem& it = inline ? kernarg copy : items[item]` every field access
// is a flat load behind a select (a dependent memory round trip each); here the
// single-FoV path reads its fields straight from the kernel arguments.
// (FFN_GLOBAL, the global address space spelled out: ffn_kernels.h)
struct ItemView {
  const FFN_GLOBAL float* image;
  const FFN_GLOBAL uint8_t* image_u8;
  const FFN_GLOBAL float* image_lut;
  FFN_GLOBAL float* seed;
  const FFN_GLOBAL int32_t* seg;
  int cz, cy, cx;
  int pos[3];
  const ffn_step_request* req;  // start_pos / candidates (read per lane)
};
// INLINE_ONLY: a launch that is only ever made for one FoV (the fused step launch) reads the
// kernel-argument copy without looking at use_inline -- one dependent argument load less
template <bool INLINE_ONLY = false>
__device__ __forceinline__ ItemView item_view(const StepItems& si, int item) {
  ItemView v;
#define FFN_VIEW_FROM(S)                                                        \
  v.image = (const FFN_GLOBAL float*)(S).image;                                  \
  v.image_u8 = (const FFN_GLOBAL uint8_t*)(S).image_u8;                          \
  v.image_lut = (const FFN_GLOBAL float*)(S).image_lut;                          \
  v.seed = (FFN_GLOBAL float*)(S).seed;                                          \
  v.seg = (const FFN_GLOBAL int32_t*)(S).seg;                                    \
  v.cz = (S).cz, v.cy = (S).cy, v.cx = (S).cx;                                   \
  v.pos[0] = (S).req.pos[0], v.pos[1] = (S).req.pos[1], v.pos[2] = (S).req.pos[2]; \
  v.req = &(S).req;
  // (the position is pinned on its side of the select, so that it is read from
  // the kernel arguments there and not through the merged `req` pointer)
  if (INLINE_ONLY || si.use_inline) {
    FFN_VIEW_FROM(si.inline_item)
    asm volatile("" : "+s"(v.pos[0]), "+s"(v.pos[1]), "+s"(v.pos[2]));
  } else {
    FFN_VIEW_FROM(si.items[item])
    asm volatile("" : "+v"(v.pos[0]), "+v"(v.pos[1]), "+v"(v.pos[2]));
  }
#undef FFN_VIEW_FROM
  return v;
}

constexpr int kC0Z = 4, kC0Y = 8, kC0X = 8;  // conv0a output tile per block
constexpr int kC0Threads = 512;               // 256 positions x 2 cout halves

// conv0_a on the matrix cores: the 4 x 8 x 8 output tile + halo is staged once
// in LDS (one canvas read per input voxel; gfx.oa / canvas strides map this
// layout's axes onto the canvas'), then an implicit GEMM with K = 27 taps x 2 channels = 54 (padded to 56 = 14
// k-steps of v_mfma_f32_16x16x4_f32).  A block = 256 positions = 16 M-tiles;
// wave w owns M-tiles 2w, 2w+1 for both cout halves (56 MFMAs).  A operand: one
// ds_read_b32 per k-step straight from the (image, seed) tile (lane group g
// reads channel g & 1 of tap 2s + (g >> 1)); B operand: the [54][32] weights,
// 28 registers per lane, loaded once.  5x fewer issue cycles than the VALU form.
// SPLIT (conv_variant 6): the output leaves as "split planes" (fp16 hi + scaled
// residual, 16 B per position and chunk plane; see conv32d) instead of f32.
struct Conv0SplitOut {
  char* out_sp;            // position 0 of plane 0, item 0
  long sp_plane_bytes;     // positions x 16
  long item_bytes;
  unsigned* range_flag;
  unsigned range_tag;
};
typedef _Float16 f16x8_c0 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4_c0 __attribute__((ext_vector_type(4)));

// Speculative launch (single-FoV steps of the library's segment loop): conv0_a of
// the NEXT step is queued behind this step's paste, before the host has seen this
// step's result, for the first of up to kSpecMax queued positions that passes
// Canvas.is_valid_pos's device part (inference.py:325,341: NOT seed < move
// threshold, segmentation <= 0; the bounds part is the host's, done before the
// launch).  The host makes the same choice from the same values one turn-around
// later (ffn_step_result.cand_seed / cand_seg) and then queues the rest of the
// step behind this launch; `choice` (-1: none valid, nothing computed) lets the
// step's faces kernel verify that both chose the same position.
struct SpecArgs {  // (kSpecMax: ffn_types.h)
  int n;                 // 0: a normal launch at si's request position
  int pos[kSpecMax][3];  // zyx
  float move_thr;
  int* choice;
};

// The canvas as it WILL be once the step whose paste runs next to this conv0_a
// (the fused faces + paste + next conv0_a launch) has pasted: inside that step's
// prediction box the seed is post_disco(logits, old seed) -- exactly what its
// paste blocks are writing meanwhile -- elsewhere the canvas itself.  on = 0: the
// canvas as it is (a launch of its own, or a void step that pastes nothing).
struct SeedOverlay {
  int on;
  int disco;
  const float* lg;   // the step's logits, dense [z][y][x] of the caller's FoV
  const float* old;  // its raw input seed
  int z0, y0, x0;    // canvas corner of its FoV
  int fy, fx;        // its FoV's row / plane strides
  int c0[3], c1[3];  // its prediction box (Geom::c0 / c1)
};

// what the paste writes: the disco bias (inference.py:416-439)
__device__ __forceinline__ float post_disco(float lg, float old, bool disco) {
  // mask = (old < logit(0.5) == 0) & (logits > old); NaN old -> false.
  return (disco && old < 0.0f && lg > old) ? old : lg;
}

// index into the overlay's dense arrays of canvas voxel (Z, Y, X), or -1
__device__ __forceinline__ int overlay_index(const SeedOverlay& ov, int Z, int Y, int X) {
  const int lz = Z - ov.z0, ly = Y - ov.y0, lx = X - ov.x0;
  const bool in = ov.on && lz >= ov.c0[0] && lz < ov.c1[0] && ly >= ov.c0[1] &&
                  ly < ov.c1[1] && lx >= ov.c0[2] && lx < ov.c1[2];
  return in ? (lz * ov.fy + ly) * ov.fx + lx : -1;
}

// ov_in.on says whether an overlay MAY apply: its loads are then issued with all the others;
// resolve(ov) is called once, by every thread of the block, when they are in flight, and
// settles ov.on / ov.disco (the fused launch: the step's void flags and its count, whose own
// loads have been in flight since the block started -- one round trip to a memory the launch
// boundary left cold instead of three in a row).
struct Conv0NoResolve {
  __device__ void operator()(SeedOverlay&) const {}
};
template <bool SPLIT, class Resolve = Conv0NoResolve>
__device__ __forceinline__ void conv0a_body(
    const int tile_block, const int item, const StepItems& si, float pad_value,
    const float* __restrict__ w /*[27][2][32]*/,
    const float* __restrict__ bias, float* __restrict__ out,
    float* __restrict__ seed_raw, const Geom& g, int tiles_y, int tiles_x,
    const Conv0SplitOut& so, const SpecArgs& sp, const SeedOverlay& ov_in,
    long long* tr = nullptr, Resolve resolve = Resolve()) {
  SeedOverlay ov = ov_in;
  // (tr: debug_fused_trace stamps, last of every eighth block to get there: [16] position
  // chosen, [17] tile staged in LDS, [18] MFMAs done -- a sample, so that the stamps'
  // atomics do not stand in the way of what they time)
  auto stamp = [&](int k) {
    if (tr && threadIdx.x == 0 && (tile_block & 7) == 0)
      atomicMax(reinterpret_cast<unsigned long long*>(tr + k), (unsigned long long)wall_clock64());
  };
  constexpr int HZ = kC0Z + 2, HY = kC0Y + 2, HX = kC0X + 2;
  __shared__ float tile[HZ * HY * HX * 2];  // (image, seed) interleaved
  __shared__ float s_lut[256];              // uint8 canvases: normalisation table
  // SPLIT: the block's 256 x 32 outputs, transposed through LDS (36-float rows)
  __shared__ __attribute__((aligned(16))) float otile[SPLIT ? 256 * 36 : 4];
  const ItemView it = item_view(si, item);
  int b = tile_block;
  const int tx = b % tiles_x;
  b /= tiles_x;
  const int ty = b % tiles_y;
  const int tz = b / tiles_y;
  const int oz = tz * kC0Z, oy = ty * kC0Y, ox = tx * kC0X;  // FoV coords
  // canvas strides of this geometry's axes (axis a = canvas axis g.oa[a])
  const long cstr[3] = {(long)it.cy * it.cx, (long)it.cx, 1};
  const long sz = cstr[g.oa[0]], sy = cstr[g.oa[1]], sx = cstr[g.oa[2]];
  int pos[3] = {it.pos[0], it.pos[1], it.pos[2]};

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i = lane & 15;   // A row (position) / B column (cout) of this lane
  const int grp = lane >> 4;  // k index inside a k-step

  // Gather: every canvas load of the block is issued before any is waited for
  // (<= kC0Per elements per thread), and a uint8 canvas' normalisation table
  // ((x - mean) / stddev of runner.py:383-385 as a 256-entry look-up) goes
  // through LDS -- one global round trip for the whole gather instead of one
  // per pass and another per look-up.
  constexpr int kC0Per = (HZ * HY * HX + kC0Threads - 1) / kC0Threads;
  const bool u8 = it.image == nullptr;
  float g_img[kC0Per] = {}, g_seed[kC0Per];
  unsigned g_raw[kC0Per] = {};
  float o_l[kC0Per] = {}, o_o[kC0Per] = {};
  int g_ov[kC0Per];  // index into the overlay (a voxel the running paste writes), or -1
  long g_out[kC0Per];  // seed_raw index of an interior voxel, else -1
  bool g_in[kC0Per];
  int g_zz[kC0Per], g_yy[kC0Per], g_xx[kC0Per];
#pragma unroll
  for (int k = 0; k < kC0Per; ++k) {
    const int e = threadIdx.x + k * kC0Threads;
    const int ec = e < HZ * HY * HX ? e : 0;
    const int hx = ec % HX;
    const int t = ec / HX;
    const int hy = t % HY;
    const int hz = t / HY;
    const int zz = oz + hz - 1, yy = oy + hy - 1, xx = ox + hx - 1;
    g_zz[k] = zz, g_yy[k] = yy, g_xx[k] = xx;
    g_in[k] = e < HZ * HY * HX && zz >= 0 && zz < g.fz && yy >= 0 && yy < g.fy &&
              xx >= 0 && xx < g.fx;
    // interior voxel: keep the raw seed (NaN preserved), at its place in the
    // caller's dense [z][y][x] order
    g_out[k] = (g_in[k] && hz >= 1 && hz <= kC0Z && hy >= 1 && hy <= kC0Y &&
                hx >= 1 && hx <= kC0X)
                   ? (long)((size_t)item * g.V + (size_t)zz * g.dstr[0] +
                            yy * g.dstr[1] + xx * g.dstr[2])
                   : -1;
  }
  // the loads of the FoV at canvas position p3 (zyx), all in flight at once
  auto issue_gather = [&](const int* p3) {
    const int pz = g.oa[0] == 0 ? p3[0] : g.oa[0] == 1 ? p3[1] : p3[2];
    const int py = g.oa[1] == 0 ? p3[0] : g.oa[1] == 1 ? p3[1] : p3[2];
    const int px = g.oa[2] == 0 ? p3[0] : g.oa[2] == 1 ? p3[1] : p3[2];
    const int z0 = pz - g.fz / 2;
    const int y0 = py - g.fy / 2;
    const int x0 = px - g.fx / 2;
    size_t g_ci[kC0Per];
#pragma unroll
    for (int k = 0; k < kC0Per; ++k) {
      // (voxel 0 of the canvas stands in outside the FoV: loads without branches)
      g_ci[k] = g_in[k] ? (size_t)((z0 + g_zz[k]) * sz + (y0 + g_yy[k]) * sy +
                                   (x0 + g_xx[k]) * sx)
                        : 0;
      g_ov[k] = -1;
      if (ov.on && g_in[k]) {
        int cc[3];  // canvas coordinates: this geometry's axis a is canvas axis oa[a]
        cc[g.oa[0]] = z0 + g_zz[k];
        cc[g.oa[1]] = y0 + g_yy[k];
        cc[g.oa[2]] = x0 + g_xx[k];
        g_ov[k] = overlay_index(ov, cc[0], cc[1], cc[2]);
      }
    }
    if (u8) {
#pragma unroll
      for (int k = 0; k < kC0Per; ++k) g_raw[k] = it.image_u8[g_ci[k]];
    } else {
#pragma unroll
      for (int k = 0; k < kC0Per; ++k) g_img[k] = it.image[g_ci[k]];
    }
#pragma unroll
    for (int k = 0; k < kC0Per; ++k) g_seed[k] = it.seed[g_ci[k]];
    if (ov.on) {
#pragma unroll
      for (int k = 0; k < kC0Per; ++k) {
        o_l[k] = ov.lg[g_ov[k] < 0 ? 0 : g_ov[k]];
        o_o[k] = ov.old[g_ov[k] < 0 ? 0 : g_ov[k]];
      }
    }
  };

  // B fragments: k = 4 s + grp -> w[k][16 nhalf + i]; k >= 54 is zero padding
  // (loaded in front of everything that is waited for: they depend on nothing)
  float bw[2][14];
#pragma unroll
  for (int s = 0; s < 14; ++s) {
    const int kk = 4 * s + grp;
#pragma unroll
    for (int h = 0; h < 2; ++h)
      bw[h][s] = kk < 54 ? w[kk * kFeatures + 16 * h + i] : 0.0f;
  }
  const float bias0 = bias[i], bias1 = bias[16 + i];
  float lut_v = 0.0f;  // in flight with the canvas loads
  if (u8 && threadIdx.x < 256) lut_v = it.image_lut[threadIdx.x];

  if (sp.n > 0) {  // every block makes the same choice from the same loads
    // (all of them in flight at once)
    float sv[kSpecMax];
    int gv[kSpecMax];
    int ovi[kSpecMax];
    float ol[kSpecMax], oo[kSpecMax];
#pragma unroll
    for (int k = 0; k < kSpecMax; ++k) {
      const size_t ci =  // (the host fills unused slots with candidate 0)
          ((size_t)sp.pos[k][0] * it.cy + sp.pos[k][1]) * it.cx + sp.pos[k][2];
      sv[k] = it.seed[ci];
      gv[k] = it.seg[ci];
      ovi[k] = overlay_index(ov, sp.pos[k][0], sp.pos[k][1], sp.pos[k][2]);
      ol[k] = ov.on ? ov.lg[ovi[k] < 0 ? 0 : ovi[k]] : 0.f;
      oo[k] = ov.on ? ov.old[ovi[k] < 0 ? 0 : ovi[k]] : 0.f;
    }
    // ... and behind them, before their values are back, the gather for the FIRST
    // position of the list: it is the one chosen unless the step about to end
    // has invalidated it, and then its round trip is the choice's own
    issue_gather(sp.pos[0]);
    if (tr && threadIdx.x == 0 && tile_block == 0) tr[20] = wall_clock64();  // (loads issued)
    resolve(ov);
    if (tr && threadIdx.x == 0 && tile_block == 0) tr[21] = wall_clock64();  // (count known)
#pragma unroll
    for (int k = 0; k < kSpecMax; ++k)
      if (ov.on && ovi[k] >= 0) sv[k] = post_disco(ol[k], oo[k], ov.disco != 0);
#pragma unroll
    for (int k = 0; k < kSpecMax; ++k)  // (no short-circuit into dependent loads)
      asm volatile("" : "+v"(sv[k]), "+v"(gv[k]));
    int ch = -1;
#pragma unroll
    for (int k = kSpecMax - 1; k >= 0; --k)
      if (k < sp.n && !(sv[k] < sp.move_thr) && gv[k] <= 0) ch = k;
    if (tile_block == 0 && threadIdx.x == 0) *sp.choice = ch;
    if (ch < 0) return;
    stamp(16);
    if (tr && threadIdx.x == 0 && tile_block == 0) tr[22] = wall_clock64();
#pragma unroll
    for (int k = 0; k < kSpecMax; ++k)
      if (k == ch) {
        pos[0] = sp.pos[k][0];
        pos[1] = sp.pos[k][1];
        pos[2] = sp.pos[k][2];
      }
    if (ch != 0) issue_gather(pos);  // (every block and lane alike)
  } else {
    issue_gather(pos);
    resolve(ov);
  }

  if (ov.on) {
#pragma unroll
    for (int k = 0; k < kC0Per; ++k)
      if (g_ov[k] >= 0) g_seed[k] = post_disco(o_l[k], o_o[k], ov.disco != 0);
  }
  if (u8 && threadIdx.x < 256) s_lut[threadIdx.x] = lut_v;
  __syncthreads();  // the table is in LDS
#pragma unroll
  for (int k = 0; k < kC0Per; ++k) {
    const int e = threadIdx.x + k * kC0Threads;
    if (e >= HZ * HY * HX) continue;
    float vi = 0.0f, vs = 0.0f;  // SAME zero padding outside the FoV
    if (g_in[k]) {
      vi = u8 ? s_lut[g_raw[k]] : g_img[k];
      vs = g_seed[k];
      if (g_out[k] >= 0) seed_raw[g_out[k]] = vs;
      if (vs != vs) vs = pad_value;  // NaN -> pad (inference.py:406-407)
    }
    tile[2 * e] = vi;
    tile[2 * e + 1] = vs;
  }
  __syncthreads();
  stamp(17);

  const int ch = grp & 1;
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const int lp = (wave * 2 + m) * kTile + i;  // this lane's A row
    const int lx = lp % kC0X;
    const int ly = (lp / kC0X) % kC0Y;
    const int lz = lp / (kC0X * kC0Y);
    const int abase = ((lz * HY + ly) * HX + lx) * 2 + ch;
    f32x4 acc0 = {bias0, bias0, bias0, bias0};
    f32x4 acc1 = {bias1, bias1, bias1, bias1};
#pragma unroll
    for (int s = 0; s < 14; ++s) {
      int tap = 2 * s + (grp >> 1);
      tap = tap > 26 ? 26 : tap;  // k = 54, 55: weight is zero, any finite A
      const int kz = tap / 9, ky = (tap / 3) % 3, kx = tap % 3;
      const float av = tile[abase + ((kz * HY + ky) * HX + kx) * 2];
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bw[0][s], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bw[1][s], acc1, 0, 0, 0);
    }
    // D fragment: lane (i, grp) holds cout i of positions 4 grp + r
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int op = (wave * 2 + m) * kTile + grp * 4 + r;
      if constexpr (SPLIT) {
        otile[op * 36 + i] = fmaxf(acc0[r], 0.0f);
        otile[op * 36 + 16 + i] = fmaxf(acc1[r], 0.0f);
        continue;
      }
      const int ox_ = op % kC0X;
      const int oy_ = (op / kC0X) % kC0Y;
      const int oz_ = op / (kC0X * kC0Y);
      const int z = oz + oz_, y = oy + oy_, x = ox + ox_;
      if (z >= g.fz || y >= g.fy || x >= g.fx) continue;
      const size_t p = (size_t)z * g.plane + (size_t)y * g.XS + x;
      float* o = out + (size_t)item * g.act_stride + p * kFeatures;
      o[i] = fmaxf(acc0[r], 0.0f);
      o[16 + i] = fmaxf(acc1[r], 0.0f);
    }
  }
  stamp(18);
  if constexpr (SPLIT) {
    __syncthreads();
    unsigned range_max = 0;
    char* ob = so.out_sp + (long)item * so.item_bytes;
    const __amdgpu_buffer_rsrc_t rs_out =
        __builtin_amdgcn_make_buffer_rsrc(ob, 0, 0x7fffffff, 0x00020000);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int e = threadIdx.x + kC0Threads * k;  // (chunk plane c, position op)
      const int c = e >> 8, op = e & 255;
      const int ox_ = op % kC0X;
      const int oy_ = (op / kC0X) % kC0Y;
      const int oz_ = op / (kC0X * kC0Y);
      const int z = oz + oz_, y = oy + oy_, x = ox + ox_;
      if (z >= g.fz || y >= g.fy || x >= g.fx) continue;
      const long p = (long)z * g.plane + (long)y * g.XS + x;
      const f32x4 va = *reinterpret_cast<const f32x4*>(otile + op * 36 + c * 8);
      const f32x4 vb = *reinterpret_cast<const f32x4*>(otile + op * 36 + c * 8 + 4);
      f16x8_c0 hi, res;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const f32x4 v = h ? vb : va;
        f32x4 vh = v;
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
          const unsigned mbits = __float_as_uint(v[cc]) & 0x7fffffffu;
          range_max = mbits > range_max ? mbits : range_max;
          vh[cc] = mbits < 0x38800000u ? 0.0f : v[cc];  // |x| < 2^-14
        }
        const f16x4_c0 h4 = __builtin_convertvector(vh, f16x4_c0);
        const f32x4 r1 = (v - __builtin_convertvector(h4, f32x4)) * 2048.0f;
        const f16x4_c0 r4 = __builtin_convertvector(r1, f16x4_c0);
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
          hi[4 * h + cc] = h4[cc];
          res[4 * h + cc] = r4[cc];
        }
      }
      // write-through (sc1), as the split-product kernels' own epilogues: no dirty L2
      // lines for the launch boundary in front of the stack to write back (4.6 MB here:
      // +0.5 us of boundary, tools/probes/boundary_probe.hip)
      typedef unsigned u32x4_c0 __attribute__((ext_vector_type(4)));
      __builtin_amdgcn_raw_buffer_store_b128(
          __builtin_bit_cast(u32x4_c0, hi), rs_out,
          (unsigned)((long)c * so.sp_plane_bytes + p * 16), 0, 16);
      __builtin_amdgcn_raw_buffer_store_b128(
          __builtin_bit_cast(u32x4_c0, res), rs_out,
          (unsigned)((long)(4 + c) * so.sp_plane_bytes + p * 16), 0, 16);
    }
    if (__ballot(range_max > 0x477fe000u) && lane == 0)  // > 65504 (or NaN)
      *so.range_flag = so.range_tag;
  }
}

template <bool SPLIT>
__global__ __launch_bounds__(kC0Threads) void conv0a_mfma_kernel(
    StepItems si, float pad_value, const float* __restrict__ w /*[27][2][32]*/,
    const float* __restrict__ bias, float* __restrict__ out,
    float* __restrict__ seed_raw, Geom g, int tiles_y, int tiles_x,
    Conv0SplitOut so, SpecArgs sp) {
  SeedOverlay ov;
  ov.on = 0;
  conv0a_body<SPLIT>(blockIdx.x, blockIdx.y, si, pad_value, w, bias, out, seed_raw, g,
                     tiles_y, tiles_x, so, sp, ov);
}

struct Conv0Next {
  float pad_value;
  const float* w;
  const float* bias;
  float* out;
  float* seed_raw;   // the next step's
  Geom q;            // the split-product kernels' layout of the FoV
  int tiles_y, tiles_x;
  Conv0SplitOut so;  // (range flag / tag: the next step's)
  SpecArgs sp;       // (choice: the next step's)
};

}  // namespace ffn
