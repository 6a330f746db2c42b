// The kernels behind the conv stack of a FoV step: faces, paste and the fused step
// launches (whose last role is the NEXT step's conv0_a: conv0a_body, ffn_conv0a.h).
// (included by ffn_hip.hip alone, behind ffn_kernels.h, inside no namespace)
#pragma once

#include "ffn_conv0a.h"

namespace ffn {

// ---------------------------------------------------------------------------
// paste: disco bias + write-back into the canvas seed (inference.py:416-439),
// 6-face max/argmax for the movement policy (movement.py:67-100), and the point
// reads the host queue needs next (inference.py:325,341,503).
// ---------------------------------------------------------------------------
__device__ __forceinline__ bool disco_on(unsigned cnt, int V, float thr) {
  // np.mean(bool array) is an f64 division; the threshold is an f32 proto field.
  return thr >= 0.0f && ((double)cnt / (double)V) > (double)thr;
}

__device__ __forceinline__ unsigned sum_block_counts(
    const unsigned* __restrict__ block_count, int head_blocks, int item,
    unsigned* s_cnt /* [blockDim.x / 64] shared */) {
  // total #(logits >= move_thr): sum of the head kernel's per-block partials
  unsigned part = 0;
  for (int e = threadIdx.x; e < head_blocks; e += blockDim.x)
    part += block_count[item * head_blocks + e];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off);
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = part;
  __syncthreads();
  unsigned cnt = 0;
  for (int wv = 0; wv < (int)(blockDim.x >> 6); ++wv) cnt += s_cnt[wv];
  return cnt;
}

// #(logits >= move_thr) of the step: the fused head's per-workgroup partials --
// or, when the model's prediction is a centred box of the FoV (Geom::crop), a
// count over that box only (the head counted the whole FoV)
__device__ __forceinline__ unsigned step_count(
    const Geom& g, const float* __restrict__ lg, float move_thr,
    const unsigned* __restrict__ block_count, int head_blocks, int item,
    unsigned* s_cnt) {
  if (!g.crop) return sum_block_counts(block_count, head_blocks, item, s_cnt);
  unsigned part = 0;
  for (int v = threadIdx.x; v < g.V; v += blockDim.x) {
    const int x = v % g.fx, t = v / g.fx;
    part += (in_pred_box(g, t / g.fy, t % g.fy, x) && lg[v] >= move_thr) ? 1u : 0u;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off);
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = part;
  __syncthreads();
  unsigned cnt = 0;
  for (int wv = 0; wv < (int)(blockDim.x >> 6); ++wv) cnt += s_cnt[wv];
  return cnt;
}

// (Measured, round 3: issuing the face / candidate loads and the segmentation ids
// under the faces BEFORE the block-count barrier does not shorten the block --
// 7.1 against 7.0 us for the fused launch; its time is the launch and the two
// PCIe round trips of the publication, not the loads.)
// faces: everything the HOST waits for after a step -- six face max/argmax
// (movement.py:67-100), the point reads of the queue head (inference.py:325,
// 341,503) and the completion flag.  One block per item, launched BEFORE the
// canvas write-back so that the host's queue bookkeeping overlaps the paste.
// Values inside the FoV are recomputed from (logits, old seed) exactly as the
// paste kernel will write them; values outside come from the canvas, which this
// step does not modify there.
constexpr int kPubWords = (int)(sizeof(ffn_step_result) / 4);  // published words

__device__ __forceinline__ void faces_body(
    const int item, const StepItems& si, const Geom& g,
    const float* __restrict__ logits, const float* __restrict__ in_seed,
    const unsigned* __restrict__ block_count, int head_blocks, float move_thr,
    float disco_thr, float deleted_thr, const unsigned* __restrict__ range_flag,
    unsigned range_tag, unsigned long long* __restrict__ pub, unsigned step_id,
    const int* __restrict__ spec_choice, int spec_expected, long long* tr = nullptr) {
  // (tr: debug_fused_trace stamps [12] count known, [13] faces reduced, [14] record built)
  __shared__ unsigned s_cnt[8];
  __shared__ ffn_step_result s_res;
  const ItemView it = item_view(si, item);
  const float* lg = logits + (size_t)item * g.V;
  const float* old = in_seed + (size_t)item * g.V;
  // Every global load of the block is in flight before any is waited for: the block
  // counts, the face values (logits, old seed, segmentation ids under the faces) and the
  // candidates' point values are ONE round trip to a memory the launch boundary left cold
  // (3.5 + 2.6 + 0.9 us when they follow each other: profiles/r06_step_roles.txt), and the
  // host's turn-around starts when this block's record leaves.
  const int z0 = it.pos[0] - g.fz / 2;
  const int y0 = it.pos[1] - g.fy / 2;
  const int x0 = it.pos[2] - g.fx / 2;
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  unsigned cnt_part = 0;
  if (!g.crop)
    for (int e = threadIdx.x; e < head_blocks; e += blockDim.x)
      cnt_part += block_count[item * head_blocks + e];
  // face geometry of this wave (waves 0 .. 5)
  const int f_axis = wave >> 1;
  const int f_sign = (wave & 1) ? 1 : -1;
  const int f_cz = g.c0[0] + (g.c1[0] - g.c0[0]) / 2;
  const int f_cy = g.c0[1] + (g.c1[1] - g.c0[1]) / 2;
  const int f_cx = g.c0[2] + (g.c1[2] - g.c0[2]) / 2;
  const int f_nr = f_axis == 0 ? 2 * g.dy + 1 : 2 * g.dz + 1;
  const int f_nc = f_axis == 2 ? 2 * g.dy + 1 : 2 * g.dx + 1;
  const int f_total = f_nr * f_nc;
  auto face_zyx = [&](int e, int& z, int& y, int& x) {
    const int fi = e / f_nc, fj = e - fi * f_nc;
    z = f_axis == 0 ? f_cz + f_sign * g.dz : f_cz - g.dz + fi;
    y = f_axis == 1 ? f_cy + f_sign * g.dy
                    : (f_axis == 0 ? f_cy - g.dy + fi : f_cy - g.dy + fj);
    x = f_axis == 2 ? f_cx + f_sign * g.dx : f_cx - g.dx + fj;
  };
  constexpr int kFaceSweep = 8;  // elements per lane and sweep
  const bool one_sweep = f_total <= kFaceSweep * 64;
  float fa[kFaceSweep], fb[kFaceSweep];
  int fs[kFaceSweep];
  if (wave < 6 && one_sweep) {
#pragma unroll
    for (int k = 0; k < kFaceSweep; ++k) {
      const int e = k * 64 + lane;
      int z, y, x;
      face_zyx(e < f_total ? e : 0, z, y, x);
      const int v = (z * g.fy + y) * g.fx + x;
      fa[k] = lg[v];
      fb[k] = old[v];
      fs[k] = it.seg[((size_t)(z0 + z) * it.cy + (y0 + y)) * it.cx + (x0 + x)];
    }
  }
  // the candidates' point values (wave 6)
  float c_lg = 0.f, c_old = 0.f, c_seed = 0.f;
  int c_seg = 0, c_kind = 0;  // 1: a voxel this step writes, 2: outside its box
  if (wave == 6) {
    const int n = it.req->num_candidates;
    if (lane <= n && lane <= FFN_MAX_CANDIDATES) {
      const int32_t* q = lane == 0 ? it.req->start_pos : it.req->candidates[lane - 1];
      const int z = q[0], y = q[1], x = q[2];
      if (z >= 0 && z < it.cz && y >= 0 && y < it.cy && x >= 0 && x < it.cx) {
        const int lz = z - z0, ly = y - y0, lx = x - x0;
        const size_t ci = ((size_t)z * it.cy + y) * it.cx + x;
        if (in_pred_box(g, lz, ly, lx)) {
          const int v = (lz * g.fy + ly) * g.fx + lx;
          c_lg = lg[v];
          c_old = old[v];
          c_kind = 1;
        } else {
          c_seed = it.seed[ci];
          c_kind = 2;
        }
        c_seg = it.seg[ci];
      }
    }
  }
  if (tr && threadIdx.x == 0) tr[19] = wall_clock64();  // (every load of the block issued)
  unsigned cnt;
  if (!g.crop) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt_part += __shfl_xor(cnt_part, off);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = cnt_part;
    __syncthreads();
    cnt = 0;
    for (int wv = 0; wv < (int)(blockDim.x >> 6); ++wv) cnt += s_cnt[wv];
  } else {
    cnt = step_count(g, lg, move_thr, block_count, head_blocks, item, s_cnt);
  }
  if (tr && threadIdx.x == 0) tr[12] = wall_clock64();
  const bool disco = disco_on(cnt, g.Vp, disco_thr);

  if (wave < 6) {
    const int axis = wave >> 1;
    const int sign = (wave & 1) ? 1 : -1;
    // centre of the prediction (movement.py:60: the centre of `prob_map`)
    const int cz = g.c0[0] + (g.c1[0] - g.c0[0]) / 2;
    const int cy = g.c0[1] + (g.c1[1] - g.c0[1]) / 2;
    const int cx = g.c0[2] + (g.c1[2] - g.c0[2]) / 2;
    // face rows / cols = the two non-fixed axes in zyx order (selects, not
    // runtime-indexed arrays: those would live in scratch memory)
    const int nr = axis == 0 ? 2 * g.dy + 1 : 2 * g.dz + 1;
    const int nc = axis == 2 ? 2 * g.dy + 1 : 2 * g.dx + 1;
    const int total = nr * nc;
    auto dense_index = [&](int e) {
      const int fi = e / nc, fj = e - fi * nc;
      const int z = axis == 0 ? cz + sign * g.dz : cz - g.dz + fi;
      const int y = axis == 1 ? cy + sign * g.dy
                              : (axis == 0 ? cy - g.dy + fi : cy - g.dy + fj);
      const int x = axis == 2 ? cx + sign * g.dx : cx - g.dx + fj;
      return (z * g.fy + y) * g.fx + x;
    };
    float best = -__builtin_inff();
    int besti = 0x7fffffff;
    bool any = false;
    for (int base = 0; base < total; base += 8 * 64) {
      float a[8], b[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {  // all loads of the sweep in flight at once
        const int e = base + k * 64 + lane;
        if (one_sweep) {  // (loaded in front of the block-count barrier)
          a[k] = fa[k];
          b[k] = fb[k];
          continue;
        }
        const int v = dense_index(e < total ? e : 0);
        a[k] = lg[v];
        b[k] = old[v];
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int e = base + k * 64 + lane;
        if (e < total) {
          const float val = post_disco(a[k], b[k], disco);
          if (!any || val > best) {  // strict >: first occurrence wins
            best = val;
            besti = e;
            any = true;
          }
        }
      }
    }
    if (!any) {
      best = -__builtin_inff();
      besti = 0x7fffffff;
    }
    // wavefront argmax reduction, ties -> smaller flat index (np.argmax order)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ob = __shfl_xor(best, off);
      const int oi = __shfl_xor(besti, off);
      if (ob > best || (ob == best && oi < besti)) {
        best = ob;
        besti = oi;
      }
    }
    if (tr && threadIdx.x == 0) tr[13] = wall_clock64();
    if (lane == 0) {
      s_res.face_score[wave] = best;
      s_res.face_index[wave] = besti;
      int sg = 0;
      if (besti != 0x7fffffff && !one_sweep) {
        const int fi = besti / nc, fj = besti - fi * nc;
        const int z = axis == 0 ? cz + sign * g.dz : cz - g.dz + fi;
        const int y = axis == 1 ? cy + sign * g.dy
                                : (axis == 0 ? cy - g.dy + fi : cy - g.dy + fj);
        const int x = axis == 2 ? cx + sign * g.dx : cx - g.dx + fj;
        sg = it.seg[((size_t)(z0 + z) * it.cy + (y0 + y)) * it.cx + (x0 + x)];
      }
      s_res.face_seg[wave] = sg;
    }
    if (one_sweep) {
      // the id under the arg-max: element besti sits in register besti >> 6 of lane
      // besti & 63
      int mine = 0;
#pragma unroll
      for (int k = 0; k < kFaceSweep; ++k) mine = (besti >> 6) == k ? fs[k] : mine;
      const int sgv = __shfl(mine, besti == 0x7fffffff ? 0 : (besti & 63));
      if (lane == 0) s_res.face_seg[wave] = besti == 0x7fffffff ? 0 : sgv;
    }
  } else if (wave == 6) {
    const int n = it.req->num_candidates;
    if (lane <= n && lane <= FFN_MAX_CANDIDATES) {
      // (a voxel this step writes: recomputed as the paste will write it)
      const float sv = c_kind == 1   ? post_disco(c_lg, c_old, disco)
                       : c_kind == 2 ? c_seed
                                     : __builtin_nanf("");
      const int gv = c_seg;
      if (lane == 0) {
        s_res.start_logit = sv;
        s_res.num_above_move = cnt;
        s_res.disco_applied = disco ? 1 : 0;
      } else {
        s_res.cand_seed[lane - 1] = sv;
        s_res.cand_seg[lane - 1] = gv;
      }
    }
  } else {
    // keep_history (inference.py:420-423): voxels that were confidently part
    // of the object and that this prediction (before the disco bias) deletes
    unsigned deleted = 0;
    if (deleted_thr == deleted_thr) {  // NaN = not requested
      for (int v = lane; v < g.V; v += 64) {
        const int x = v % g.fx, t = v / g.fx;
        deleted += ((!g.crop || in_pred_box(g, t / g.fy, t % g.fy, x)) &&
                    old[v] >= deleted_thr && lg[v] < 0.0f) ? 1u : 0u;
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) deleted += __shfl_xor(deleted, off);
    }
    if (lane == 0) {
      s_res.num_deleted = deleted;
      // (2: this step ran on a speculative conv0_a launch that chose another
      // position than the host did: nothing is pasted, the library repeats it)
      // (3: the void came from the resident launch giving up on a producer --
      // range_flag[1] carries this step's tag then -- not from the range check)
      s_res.range_error = (*range_flag == range_tag) ? (range_flag[1] == range_tag ? 3 : 1)
                          : (spec_expected >= 0 && *spec_choice != spec_expected) ? 2
                                                                                  : 0;
    }
  }
  __syncthreads();
  if (tr && threadIdx.x == 0) tr[14] = wall_clock64();
  // Publish from ONE wave, in ONE trip over PCIe: every 32-bit word of the record
  // goes to pinned host memory as an 8-byte word that carries the step number in
  // its upper half (8-byte stores are atomic: a word is either the old step's or
  // this one's), and the host waits until all kPubWords of them carry it.  No
  // record -> system fence -> flag sequence (two more round trips inside the
  // block the next launch waits for).
  if (wave == 0) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(&s_res);
    unsigned long long* dst = pub + (size_t)item * kPubWords;
    for (int k = lane; k < kPubWords; k += 64)
      __hip_atomic_store(&dst[k], ((unsigned long long)step_id << 32) | src[k],
                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

__global__ __launch_bounds__(512) void faces_kernel(
    StepItems si, Geom g, const float* __restrict__ logits,
    const float* __restrict__ in_seed,
    const unsigned* __restrict__ block_count, int head_blocks, float move_thr,
    float disco_thr, float deleted_thr, const unsigned* __restrict__ range_flag,
    unsigned range_tag, unsigned long long* __restrict__ pub, unsigned step_id,
    const int* __restrict__ spec_choice, int spec_expected) {
  faces_body(blockIdx.x, si, g, logits, in_seed, block_count, head_blocks, move_thr,
             disco_thr, deleted_thr, range_flag, range_tag, pub, step_id,
             spec_choice, spec_expected);
}

// paste: disco bias + write-back into the canvas seed (inference.py:416-439);
// block bx of nbx of FoV `item`.
__device__ __forceinline__ void paste_body(
    const int item, const int bx, const int nbx, const StepItems& si, const Geom& g,
    const float* __restrict__ logits, const float* __restrict__ in_seed,
    const unsigned* __restrict__ block_count, int head_blocks, float move_thr,
    float disco_thr, const unsigned* __restrict__ range_flag, unsigned range_tag,
    const int* __restrict__ spec_choice, int spec_expected) {
  __shared__ unsigned s_cnt[8];
  if (*range_flag == range_tag) return;  // void step (fp16 range): no paste
  // ... or a step whose speculative conv0_a was made for another position
  if (spec_expected >= 0 && *spec_choice != spec_expected) return;
  const ItemView it = item_view(si, item);
  const float* lg = logits + (size_t)item * g.V;
  const float* old = in_seed + (size_t)item * g.V;
  const unsigned cnt = step_count(g, lg, move_thr, block_count, head_blocks, item, s_cnt);
  const bool disco = disco_on(cnt, g.Vp, disco_thr);
  const int z0 = it.pos[0] - g.fz / 2;
  const int y0 = it.pos[1] - g.fy / 2;
  const int x0 = it.pos[2] - g.fx / 2;
  for (int v = bx * blockDim.x + threadIdx.x; v < g.V; v += nbx * blockDim.x) {
    const int x = v % g.fx;
    const int t = v / g.fx;
    const int y = t % g.fy;
    const int z = t / g.fy;
    if (g.crop && !in_pred_box(g, z, y, x)) continue;
    const size_t ci = ((size_t)(z0 + z) * it.cy + (y0 + y)) * it.cx + (x0 + x);
    it.seed[ci] = post_disco(lg[v], old[v], disco);
  }
}

__global__ __launch_bounds__(512) void paste_kernel(
    StepItems si, Geom g, const float* __restrict__ logits,
    const float* __restrict__ in_seed,
    const unsigned* __restrict__ block_count, int head_blocks, float move_thr,
    float disco_thr, const unsigned* __restrict__ range_flag,
    unsigned range_tag, const int* __restrict__ spec_choice, int spec_expected) {
  paste_body(blockIdx.y, blockIdx.x, gridDim.x, si, g, logits, in_seed, block_count,
             head_blocks, move_thr, disco_thr, range_flag, range_tag, spec_choice,
             spec_expected);
}

// A single FoV's faces AND paste as one launch (engine option fuse_paste): block
// 0 is the faces block -- it raises the host's flag as soon as ITS work is done,
// as the separate launch does -- the others paste meanwhile.  Neither reads what
// the other writes (faces recomputes the in-FoV values from the logits), and the
// launch boundary between the two leaves the step's critical path.
__global__ __launch_bounds__(512) void faces_paste_kernel(
    StepItems si, Geom g, const float* __restrict__ logits,
    const float* __restrict__ in_seed,
    const unsigned* __restrict__ block_count, int head_blocks, float move_thr,
    float disco_thr, float deleted_thr, const unsigned* __restrict__ range_flag,
    unsigned range_tag, unsigned long long* __restrict__ pub, unsigned step_id,
    const int* __restrict__ spec_choice, int spec_expected) {
  if (blockIdx.x == 0)
    faces_body(0, si, g, logits, in_seed, block_count, head_blocks, move_thr,
               disco_thr, deleted_thr, range_flag, range_tag, pub, step_id,
               spec_choice, spec_expected);
  else
    paste_body(0, blockIdx.x - 1, gridDim.x - 1, si, g, logits, in_seed, block_count,
               head_blocks, move_thr, disco_thr, range_flag, range_tag, spec_choice,
               spec_expected);
}

// ... and the NEXT step's conv0_a in the same launch (engine option fuse_paste 2,
// the default where a step is followed by a speculative conv0_a): blocks
// kPasteBlocks + 1 .. gather the next FoV from the canvas AS THE PASTE BLOCKS
// NEXT TO THEM ARE LEAVING IT (SeedOverlay: inside this step's prediction box the
// seed is recomputed from the logits, as the faces block does for the queue's
// candidates), so that nothing waits for the paste: one launch and one kernel
// boundary less per step, the conv0_a under the faces' PCIe round trips.  The
// next step's raw seed copy, range flag and choice word are the OTHER of two
// sets (StepSlot): this step's are still being read.
// (how many: the host picks them so that the launch has one block per CU -- 1 faces block +
// paste blocks + conv0_a tiles = the CU count where that leaves at least kPasteBlocksMin -- a
// conv0_a block that shares its CU with another block reaches its position choice 2.7 us
// after the others, and the next stack waits for the last of them)
constexpr int kPasteBlocks = 71;
constexpr int kPasteBlocksMin = 16;
// LAB = false, the production form: without the debug_fused_trace stamps (`trace` is not
// read, no role stamps, no stamps pointer into the faces and conv0_a bodies); the faces
// block still leaves stamps[0] for stat_turn_gpu_ns.  The host picks (engine option
// flow_lab, or a trace that is armed).
template <bool LAB>
__global__ __launch_bounds__(512) void faces_paste_conv0a_kernel(
    StepItems si, Geom g, const float* __restrict__ logits,
    const float* __restrict__ in_seed,
    const unsigned* __restrict__ block_count, int head_blocks, float move_thr,
    float disco_thr, float deleted_thr, const unsigned* __restrict__ range_flag,
    unsigned range_tag, unsigned long long* __restrict__ pub, unsigned step_id,
    const int* __restrict__ spec_choice, int spec_expected, Conv0Next nx,
    long long* __restrict__ stamps, int trace, int paste_blocks) {
  static_assert(kC0Threads == 512, "one block size for the three roles");
  long long t_in = 0, t_warm = 0;
  if constexpr (LAB) t_in = wall_clock64();
  // (every line of the explicit arguments, and none behind them)
  constexpr int kArgBytes = KernargsOf<decltype(&faces_paste_conv0a_kernel<LAB>)>::bytes;
  static_assert(kArgBytes >= (int)(sizeof(StepItems) + sizeof(Geom) + sizeof(Conv0Next)) &&
                    kArgBytes <= 1024,
                "the explicit arguments: all of them, within what warm_kernargs touches");
  warm_kernargs<kArgBytes>();
  if constexpr (LAB) t_warm = wall_clock64();
  // engine option debug_fused_trace (trace != 0): when each role of this launch ran --
  // first entry (min over the blocks) [4] faces, [5] paste, [6] conv0_a; last end (max) [8]
  // faces = record published, [9] paste, [10] conv0_a; ([7], [11]: the stack before it)
  const bool tr_on = LAB && stamps && trace != 0;
  struct RoleStamp {
    long long* lo;
    long long* hi;
    bool on;
    // (every eighth block of a role stamps: the stamps' atomics on one word serialise)
    __device__ RoleStamp(long long* l, long long* h, bool o)
        : lo(l), hi(h), on(o && (blockIdx.x <= 1 || (blockIdx.x & 7) == 0)) {
      if (on && threadIdx.x == 0)
        atomicMin(reinterpret_cast<unsigned long long*>(lo), (unsigned long long)wall_clock64());
    }
    __device__ ~RoleStamp() {
      if (on && threadIdx.x == 0)
        atomicMax(reinterpret_cast<unsigned long long*>(hi), (unsigned long long)wall_clock64());
    }
  };
  if (blockIdx.x == 0) {
    RoleStamp rs(stamps + 4, stamps + 8, tr_on);
    faces_body(0, si, g, logits, in_seed, block_count, head_blocks, move_thr,
               disco_thr, deleted_thr, range_flag, range_tag, pub, step_id,
               spec_choice, spec_expected, tr_on ? stamps : nullptr);
    // (stat_turn_*: when this step's record left for the host -- the next resident
    // launch measures how long the GPU then waited for it, conv32ps_kernel)
    if (stamps && threadIdx.x == 0) stamps[0] = wall_clock64();
    return;
  }
  if ((int)blockIdx.x <= paste_blocks) {
    RoleStamp rs(stamps + 5, stamps + 9, tr_on);
    paste_body(0, blockIdx.x - 1, paste_blocks, si, g, logits, in_seed, block_count,
               head_blocks, move_thr, disco_thr, range_flag, range_tag, spec_choice,
               spec_expected);
    return;
  }
  RoleStamp rs(stamps + 6, stamps + 10, tr_on);
  if (tr_on && threadIdx.x == 0) {  // ([23] last sampled block's entry, [24] block 0: arguments in)
    if (((blockIdx.x - 1 - paste_blocks) & 7) == 0)
      atomicMax(reinterpret_cast<unsigned long long*>(stamps + 23), (unsigned long long)t_in);
    if ((int)blockIdx.x == 1 + paste_blocks) stamps[24] = t_warm;
  }
  __shared__ unsigned s_cnt[8];
  const ItemView it = item_view<true>(si, 0);
  // What decides how the canvas looks once this step has pasted -- its void flags (fp16
  // range / a speculative conv0_a made for another position: it pastes nothing, the canvas
  // stays as it is) and its count (the disco test) -- is LOADED here, without a branch and
  // without a look at the values, and looked at when the conv0_a body has its own loads in
  // flight (resolve): per-lane loads, so that no scalar wait of the body's stands behind
  // them.  (A loop or a compare here and the compiler waits for the load on the spot: each
  // of those was a cold round trip of its own, profiles/r06_step_roles.txt.)
  int z = 0;
  asm volatile("" : "+v"(z));
  unsigned rf = range_flag[z];
  int sc = spec_choice[z];
  const int e0 = (int)threadIdx.x < head_blocks ? (int)threadIdx.x : 0;
  unsigned part = block_count[e0];
  SeedOverlay ov;
  ov.on = 1;
  ov.disco = 0;
  ov.lg = logits;
  ov.old = in_seed;
  ov.z0 = it.pos[0] - g.fz / 2;
  ov.y0 = it.pos[1] - g.fy / 2;
  ov.x0 = it.pos[2] - g.fx / 2;
  ov.fy = g.fy;
  ov.fx = g.fx;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    ov.c0[a] = g.c0[a];
    ov.c1[a] = g.c1[a];
  }
  auto resolve = [&](SeedOverlay& o) {
    // (the values are looked at from here on: everything above has been issued)
    asm volatile("" : "+v"(rf), "+v"(sc), "+v"(part) : : "memory");
    unsigned cnt;
    if (g.crop) {
      cnt = step_count(g, logits, move_thr, block_count, head_blocks, 0, s_cnt);
    } else {
      unsigned p2 = (int)threadIdx.x < head_blocks ? part : 0u;
      for (int e = kC0Threads + (int)threadIdx.x; e < head_blocks; e += kC0Threads)
        p2 += block_count[e];  // (more partials than threads: no geometry has them today)
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) p2 += __shfl_xor(p2, off);
      if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = p2;
      __syncthreads();
      cnt = 0;
#pragma unroll
      for (int wv = 0; wv < kC0Threads / 64; ++wv) cnt += s_cnt[wv];
    }
    o.on = !(rf == range_tag || (spec_expected >= 0 && sc != spec_expected));
    o.disco = disco_on(cnt, g.Vp, disco_thr) ? 1 : 0;
  };
  conv0a_body<true>(blockIdx.x - 1 - paste_blocks, 0, si, nx.pad_value, nx.w, nx.bias,
                    nx.out, nx.seed_raw, nx.q, nx.tiles_y, nx.tiles_x, nx.so, nx.sp, ov,
                    tr_on ? stamps : nullptr, resolve);
}

}  // namespace ffn
