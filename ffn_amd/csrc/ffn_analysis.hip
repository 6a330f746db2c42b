// libffn_hip.so -- resegmentation analysis (include/ffn_analysis.h).
//
// Pair statistics, for a batch of points in four launches:
//   1. mask pass: one lane per voxel forms the four masks (A, B, S1, S2); a
//      wave's 64 voxels become four ballot words, stored as bit planes (4 bits
//      per voxel), and the ten counts are popcounts of those words -- summed
//      per wave in registers, per block in LDS, then ten atomics per block.
//   2. x pass of the exact EDT: one wave per row, all four masks; nearest 0
//      voxel to the left / right from the row's ballot words (clz / ctz).
//   3. y pass, in place: a block stages whole lines of a tile in LDS (tile rows
//      run along x, global accesses stay contiguous) and every voxel scans
//      outwards until the axis term alone exceeds its best value, as
//      ffn_decision.hip does.
//   4. z pass: the same, but nothing is written: the maximum of the squared
//      distance is reduced per wave and block and merged with one atomicMax
//      per block on the bits of the (non-negative) f64.
// Endpoint overlaps: per-(point, old id) counts through the two-level hash of
// ffn_table.h (LDS table per block, then one global table per point); runs of
// equal ids inside a wave are counted with ballots and inserted once.
//
// A launch covers every point of a group: blockIdx is mapped to (point, local
// block) through a prefix array.  Ordinary stream-ordered launches with bounded
// loops only.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/ffn_analysis.h"
#include "../../include/ffn_hip.h"
#include "ffn_internal.h"
#include "ffn_table.h"
#include "ffn_unit.h"

// squared distances must round exactly as the specification's: no FMA
#pragma clang fp contract(off)

namespace {

using ffn_table::u32;
using ffn_table::u64;
using ffn_table::kBackground;
using ffn_table::kEmptyKey;
using ffn_table::block_claim;
using ffn_table::run_leaders;
using ffn_table::run_mask;
using ffn_table::table_grow;
using ffn_table::table_insert;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxAxis = 4096;
constexpr int kGroupsPerBlock = 64;          // mask pass: 64 x 64 voxels
constexpr size_t kLineLdsBytes = 48 * 1024;  // tile of a y / z pass
constexpr int kEndIters = 32;                // endpoint pass: 32 x 256 voxels
constexpr int kLdsSlots = 1024;              // per-block id table
constexpr size_t kGroupBytes = (size_t)1 << 30;  // device bytes of one group
constexpr int kMaxGroupPoints = 4096;

struct PairDev {
  long long pa, pb;  // byte offsets in the input buffer: channel slabs at off_z
  long long seg;     // byte offset of the u64 crop
  long long bits;    // u64 index of the point's bit planes
  long long d2;      // f64 index of the point's 4 * n squared distances
  u64 id_a, id_b;
  int Y, X, oy, ox;  // slab row geometry, crop offset inside a slab
  int cz, cy, cx;
  int n;
  int ty, tz;        // tile widths of the y / z pass
  int pad;
};

struct EndDev {
  long long probs, seg;  // byte offsets in the input buffer
  u64 id;                // has_id: its row goes out without an overlap too
  int n, has_id;
};

// Largest p with starts[p] <= b (starts[0] = 0, starts[npts] = grid size).
__device__ __forceinline__ int find_point(const int* __restrict__ starts,
                                          int npts, int b) {
  int lo = 0, hi = npts;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (starts[mid] <= b)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kThreads) void pair_mask_kernel(
    const PairDev* __restrict__ descs, const int* __restrict__ starts, int npts,
    const uint8_t* __restrict__ in, const uint8_t* __restrict__ table,
    u64* __restrict__ bits, u64* counts) {
  __shared__ uint8_t tab[256];
  __shared__ u32 wsum[kWaves][FFN_PAIR_COUNTS];
  tab[threadIdx.x] = table[threadIdx.x];
  __syncthreads();
  const int p = find_point(starts, npts, blockIdx.x);
  const PairDev d = descs[p];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long g0 = (long long)(blockIdx.x - starts[p]) * kGroupsPerBlock;
  const long long ngroups = ((long long)d.n + 63) >> 6;
  const u64* seg = reinterpret_cast<const u64*>(in + d.seg);
  u32 c[FFN_PAIR_COUNTS];
  for (int k = 0; k < FFN_PAIR_COUNTS; ++k) c[k] = 0;
  for (int it = 0; it < kGroupsPerBlock / kWaves; ++it) {
    const long long g = g0 + it * kWaves + wave;
    if (g >= ngroups) break;  // whole wave
    const long long v = g * 64 + lane;
    bool a = false, b = false, s1 = false, s2 = false;
    if (v < d.n) {
      const int x = (int)(v % d.cx);
      const int r = (int)(v / d.cx);
      const int y = r % d.cy, z = r / d.cy;
      const long long o = ((long long)z * d.Y + d.oy + y) * d.X + d.ox + x;
      a = tab[in[d.pa + o]] != 0;
      b = tab[in[d.pb + o]] != 0;
      const u64 s = seg[v];
      s1 = s == d.id_a;
      s2 = s == d.id_b;
    }
    const u64 ma = __ballot(a), mb = __ballot(b);
    const u64 m1 = __ballot(s1), m2 = __ballot(s2);
    c[0] += __popcll(ma);
    c[1] += __popcll(mb);
    c[2] += __popcll(ma & mb);
    c[3] += __popcll(ma | mb);
    c[4] += __popcll(m1);
    c[5] += __popcll(m2);
    c[6] += __popcll(ma & m1);
    c[7] += __popcll(ma & m2);
    c[8] += __popcll(mb & m1);
    c[9] += __popcll(mb & m2);
    if (lane < 4)
      bits[d.bits + g * 4 + lane] =
          lane == 0 ? ma : lane == 1 ? mb : lane == 2 ? m1 : m2;
  }
  if (lane == 0)
    for (int k = 0; k < FFN_PAIR_COUNTS; ++k) wsum[wave][k] = c[k];
  __syncthreads();
  if (threadIdx.x < FFN_PAIR_COUNTS) {
    u32 t = 0;
    for (int w = 0; w < kWaves; ++w) t += wsum[w][threadIdx.x];
    if (t) atomicAdd(&counts[(size_t)p * FFN_PAIR_COUNTS + threadIdx.x], (u64)t);
  }
}

// x pass.  One wave per row and all four masks of it: lane c keeps the ballot
// word of the row's chunk c (a row has at most 64 chunks of 64 voxels), where a
// set bit is a voxel whose mask is 0.
__global__ __launch_bounds__(kThreads) void pair_edt_x_kernel(
    const PairDev* __restrict__ descs, const int* __restrict__ starts, int npts,
    const u64* __restrict__ bits, double* __restrict__ d2, double sx) {
  const int p = find_point(starts, npts, blockIdx.x);
  const PairDev d = descs[p];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long row = (long long)(blockIdx.x - starts[p]) * kWaves + wave;
  if (row >= (long long)d.cz * d.cy) return;  // whole wave
  const int chunks = (d.cx + 63) >> 6;
  const long long v0 = row * d.cx;
  const double inf = __builtin_inf();
  for (int m = 0; m < 4; ++m) {
    u64 mine = 0;
    for (int c = 0; c < chunks; ++c) {
      const int x = c * 64 + lane;
      bool zero = false;
      if (x < d.cx) {
        const long long v = v0 + x;
        zero = !((bits[d.bits + (v >> 6) * 4 + m] >> (v & 63)) & 1);
      }
      const u64 w = __ballot(zero);
      if (lane == c) mine = w;
    }
    int last = -1;  // last 0 voxel in the chunks before c
    for (int c = 0; c < chunks; ++c) {
      const u64 w = __shfl(mine, c);
      const int x = c * 64 + lane;
      int next = -1;  // first 0 voxel in the chunks after c
      for (int cc = c + 1; cc < chunks && next < 0; ++cc) {
        const u64 t = __shfl(mine, cc);
        if (t) next = cc * 64 + __builtin_ctzll(t);
      }
      const u64 at_or_left = w & (~0ull >> (63 - lane));
      const u64 at_or_right = w & (~0ull << lane);
      int g = -1;
      if (at_or_left)
        g = lane - (63 - __builtin_clzll(at_or_left));
      else if (last >= 0)
        g = x - last;
      int gr = -1;
      if (at_or_right)
        gr = __builtin_ctzll(at_or_right) - lane;
      else if (next >= 0)
        gr = next - x;
      if (gr >= 0 && (g < 0 || gr < g)) g = gr;
      if (x < d.cx) {
        const double t = sx * (double)g;
        d2[d.d2 + (long long)m * d.n + v0 + x] = g < 0 ? inf : t * t;
      }
      if (w) last = c * 64 + 63 - __builtin_clzll(w);
    }
  }
}

// y (axis 1, in place) / z (axis 0, maximum only) pass over LDS-staged lines:
//   out(q) = min over p of in(p) + ((q - p) * w)^2.
__global__ __launch_bounds__(kThreads) void pair_edt_line_kernel(
    const PairDev* __restrict__ descs, const int* __restrict__ starts, int npts,
    double* __restrict__ d2, int axis, double w, u64* max_bits) {
  extern __shared__ double sd[];
  __shared__ double wmax[kWaves];
  const int p = find_point(starts, npts, blockIdx.x);
  const PairDev d = descs[p];
  int len, tx, nouter;
  long long stride, ncols, outer_stride;
  if (axis == 1) {
    len = d.cy;
    tx = d.ty;
    nouter = d.cz;
    stride = d.cx;
    ncols = d.cx;
    outer_stride = (long long)d.cy * d.cx;
  } else {
    len = d.cz;
    tx = d.tz;
    nouter = 1;
    stride = (long long)d.cy * d.cx;
    ncols = stride;
    outer_stride = 0;
  }
  const int tiles = (int)((ncols + tx - 1) / tx);
  const int local = blockIdx.x - starts[p];
  const int tile = local % tiles;
  const int r = local / tiles;
  const int outer = r % nouter, m = r / nouter;
  const long long base =
      d.d2 + (long long)m * d.n + (long long)outer * outer_stride;
  const long long col0 = (long long)tile * tx;
  const int total = len * tx;
  const double inf = __builtin_inf();
  for (int e = threadIdx.x; e < total; e += kThreads) {
    const int q = e / tx, c = e - q * tx;
    const long long col = col0 + c;
    sd[e] = col < ncols ? d2[base + (long long)q * stride + col] : inf;
  }
  __syncthreads();
  double mx = 0.0;
  for (int e = threadIdx.x; e < total; e += kThreads) {
    const int q = e / tx, c = e - q * tx;
    const long long col = col0 + c;
    if (col >= ncols) continue;
    double best = sd[e];
    const int kmax = q > len - 1 - q ? q : len - 1 - q;
    for (int k = 1; k <= kmax; ++k) {
      const double t = (double)k * w;
      const double t2 = t * t;
      if (t2 > best) break;
      if (q - k >= 0) {
        const double v = sd[e - k * tx] + t2;
        if (v < best) best = v;
      }
      if (q + k < len) {
        const double v = sd[e + k * tx] + t2;
        if (v < best) best = v;
      }
    }
    if (axis == 1)
      d2[base + (long long)q * stride + col] = best;
    else if (best > mx)
      mx = best;
  }
  if (axis == 1) return;  // whole block
  for (int off = 32; off > 0; off >>= 1) {
    const double t = __shfl_xor(mx, off);
    if (t > mx) mx = t;
  }
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < kWaves; ++k)
      if (wmax[k] > mx) mx = wmax[k];
    // a non-negative f64 orders like its bits
    if (mx > 0.0)
      atomicMax(&max_bits[(size_t)p * 4 + m], (u64)__double_as_longlong(mx));
  }
}

__global__ __launch_bounds__(kThreads) void pair_root_kernel(
    const u64* __restrict__ max_bits, double* __restrict__ out, int n) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i < n) out[i] = __dsqrt_rn(__longlong_as_double((long long)max_bits[i]));
}

// ---- endpoint overlaps ----------------------------------------------------------

// vals[2 * slot] = voxels with new set, vals[2 * slot + 1] = voxels, of the id
// in keys[slot]; point p owns slots [p * (mask + 1), (p + 1) * (mask + 1)).
__global__ __launch_bounds__(kThreads) void endpoint_count_kernel(
    const EndDev* __restrict__ descs, const int* __restrict__ starts, int npts,
    const uint8_t* __restrict__ in, const uint8_t* __restrict__ table,
    u64* keys, u32* vals, u32 mask, int* flags, u64* num_new) {
  __shared__ uint8_t tab[256];
  __shared__ u64 skeys[kLdsSlots];
  __shared__ u32 sover[kLdsSlots];
  __shared__ u32 sorig[kLdsSlots];
  __shared__ u32 wnew[kWaves];
  tab[threadIdx.x] = table[threadIdx.x];
  for (int s = threadIdx.x; s < kLdsSlots; s += kThreads) {
    skeys[s] = kEmptyKey;
    sover[s] = 0;
    sorig[s] = 0;
  }
  __syncthreads();
  const int p = find_point(starts, npts, blockIdx.x);
  const EndDev d = descs[p];
  const int lane = threadIdx.x & 63;
  const u64* seg = reinterpret_cast<const u64*>(in + d.seg);
  const uint8_t* probs = in + d.probs;
  u64* gkeys = keys + (size_t)p * ((size_t)mask + 1);
  u32* gvals = vals + (size_t)p * ((size_t)mask + 1) * 2;
  const long long v0 =
      (long long)(blockIdx.x - starts[p]) * kEndIters * kThreads;
  u32 made = 0;
  for (int it = 0; it < kEndIters; ++it) {
    const long long v = v0 + (long long)it * kThreads + threadIdx.x;
    const bool valid = v < d.n;  // a prefix of the wave
    const u64 key = valid ? seg[v] : 0ull;
    const bool nw = valid && tab[probs[v]] != 0;
    const u64 vm = __ballot(valid);
    if (vm == 0) break;  // whole wave, and every later iteration as well
    const u64 nm = __ballot(nw);
    const u64 leaders = run_leaders(key, valid, lane);
    made += __popcll(nm);
    if ((leaders >> lane) & 1) {
      const u64 run = run_mask(leaders, lane);
      const u32 cnt = __popcll(vm & run), ov = __popcll(nm & run);
      if (key == kEmptyKey) {
        flags[1] = 1;
      } else {
        const int s = block_claim<kLdsSlots>(skeys, key);
        if (s >= 0) {
          atomicAdd(&sorig[s], cnt);
          if (ov) atomicAdd(&sover[s], ov);
        } else {  // block table crowded: straight to the global one
          const u32 t = table_insert(gkeys, mask, key, flags);
          if (t != kBackground) {
            atomicAdd(&gvals[2 * (size_t)t + 1], cnt);
            if (ov) atomicAdd(&gvals[2 * (size_t)t], ov);
          }
        }
      }
    }
  }
  if (lane == 0) wnew[threadIdx.x >> 6] = made;
  __syncthreads();
  for (int s = threadIdx.x; s < kLdsSlots; s += kThreads) {
    const u64 k = skeys[s];
    if (k == kEmptyKey) continue;
    const u32 t = table_insert(gkeys, mask, k, flags);
    if (t != kBackground) {
      atomicAdd(&gvals[2 * (size_t)t + 1], sorig[s]);
      if (sover[s]) atomicAdd(&gvals[2 * (size_t)t], sover[s]);
    }
  }
  if (threadIdx.x == 0) {
    u32 t = 0;
    for (int w = 0; w < kWaves; ++w) t += wnew[w];
    if (t) atomicAdd(&num_new[p], (u64)t);
  }
}

// Every id with an overlap goes out, one atomic per wave.
__global__ __launch_bounds__(kThreads) void endpoint_emit_kernel(
    const EndDev* __restrict__ descs, const u64* __restrict__ keys, const u32* __restrict__ vals, u32 nslots,
    long long total, int point0, u64 cap, u64* n_out, int* row_point,
    u64* row_old, u32* row_counts) {
  const int lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  u64 key = kEmptyKey;
  u32 ov = 0, orig = 0;
  bool hit = false;
  if (i < total) {
    key = keys[i];
    if (key != kEmptyKey) {
      ov = vals[2 * i];
      orig = vals[2 * i + 1];
      const EndDev& d = descs[i / nslots];
      hit = ov > 0 || (d.has_id && key == d.id);
    }
  }
  const u64 hm = __ballot(hit);
  if (hm == 0) return;  // whole wave
  const int first = __builtin_ctzll(hm);
  u64 base = 0;
  if (lane == first) base = atomicAdd(n_out, (u64)__popcll(hm));
  base = __shfl(base, first);
  if (!hit) return;
  const u64 slot = base + __popcll(hm & ~(~0ull << lane));
  if (slot < cap) {
    row_point[slot] = point0 + (int)(i / nslots);
    row_old[slot] = key;
    row_counts[2 * slot] = ov;
    row_counts[2 * slot + 1] = orig;
  }
}

using ffn_unit::DevBuf;
using ffn_unit::ensure;

}  // namespace

struct ffn_analyzer : ffn_unit::Unit {
  ffn_unit::PinnedBuf stage;  // upload staging (freed after the device buffers)
  DevBuf in, ctrl, bits, d2, small, keys, vals, rows_point, rows_old,
      rows_counts;
  u32 nslots = 1u << 12;  // per-point id table of the endpoint pass
  double ms[2] = {0.0, 0.0}, voxels[2] = {0.0, 0.0};
};

namespace {

inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

// Adds the kernel time since timer_start() to *ms.
int add_elapsed(ffn_analyzer* a, double* ms) {
  double t = 0.0;
  U_OK(a->timer_stop(&t));
  *ms += t;
  return FFN_OK;
}

int check_shape(const int32_t shape[3], size_t index, size_t* n) {
  double nd = 1.0;
  for (int k = 0; k < 3; ++k) {
    if (shape[k] < 1 || shape[k] > kMaxAxis)
      return ffn_set_error(FFN_ERR_ARG, "point %zu: shape[%d] = %d outside 1..%d",
                           index, k, shape[k], kMaxAxis);
    nd *= (double)shape[k];
  }
  if (nd >= 2147483648.0)
    return ffn_set_error(FFN_ERR_ARG, "point %zu: 2^31 voxels or more", index);
  *n = (size_t)nd;
  return FFN_OK;
}

// Widest tile of whole lines (len f64 each) that fits the LDS budget, evened
// out over the tiles it takes.
int tile_columns(int len, long long ncols) {
  long long txmax = (long long)(kLineLdsBytes / sizeof(double)) / len;
  if (txmax < 1) txmax = 1;
  const long long tiles = (ncols + txmax - 1) / txmax;
  return (int)((ncols + tiles - 1) / tiles);
}

// Device bytes a pair point needs: input slabs + crop, bit planes, distances.
struct PairPlan {
  size_t n, slab, in_bytes, bit_words;
};

PairPlan plan_pair(const ffn_pair_desc& q, size_t n) {
  PairPlan pl;
  pl.n = n;
  pl.slab = (size_t)q.shape_zyx[0] * q.box_zyx[1] * q.box_zyx[2];
  pl.in_bytes = 2 * align16(pl.slab) + align16(n * 8);
  pl.bit_words = (n + 63) / 64 * 4;
  return pl;
}

int run_pair_group(ffn_analyzer* a, const ffn_pair_desc* pts,
                   const std::vector<PairPlan>& plans, size_t first, size_t count,
                   const uint8_t table[256], const double voxel[3],
                   uint64_t* counts, double* max_edt) {
  const int npts = (int)count;
  // layout of the upload: table, descriptors, four prefix arrays, inputs
  const size_t desc_off = 256;
  const size_t starts_off = align16(desc_off + count * sizeof(PairDev));
  const size_t in_off = align16(starts_off + 4 * (count + 1) * sizeof(int));
  size_t in_bytes = 0, bit_words = 0, d2_words = 0;
  for (size_t i = 0; i < count; ++i) {
    in_bytes += plans[first + i].in_bytes;
    bit_words += plans[first + i].bit_words;
    d2_words += 4 * plans[first + i].n;
  }
  const size_t upload = in_off + in_bytes;
  U_OK(ensure(a->stage, upload));
  U_OK(ensure(a->in, upload));
  U_OK(ensure(a->bits, bit_words * 8));
  U_OK(ensure(a->d2, d2_words * 8));
  // results: counts (10 u64), max bits (4 u64), roots (4 f64) per point
  const size_t res_bytes = count * (FFN_PAIR_COUNTS + 4 + 4) * 8;
  U_OK(ensure(a->small, res_bytes));

  uint8_t* stage = static_cast<uint8_t*>(a->stage.p);
  memcpy(stage, table, 256);
  PairDev* descs = reinterpret_cast<PairDev*>(stage + desc_off);
  int* starts = reinterpret_cast<int*>(stage + starts_off);
  int* st[4] = {starts, starts + (count + 1), starts + 2 * (count + 1),
                starts + 3 * (count + 1)};
  long long blocks[4] = {0, 0, 0, 0};
  size_t cur = in_off, bits_cur = 0, d2_cur = 0, lds_y = 0, lds_z = 0;
  for (size_t i = 0; i < count; ++i) {
    const ffn_pair_desc& q = pts[first + i];
    const PairPlan& pl = plans[first + i];
    PairDev& d = descs[i];
    const size_t plane = (size_t)q.box_zyx[1] * q.box_zyx[2];
    const size_t vol = plane * q.box_zyx[0];
    d.pa = (long long)cur;
    memcpy(stage + cur, q.probs + (size_t)q.off_zyx[0] * plane, pl.slab);
    cur += align16(pl.slab);
    d.pb = (long long)cur;
    memcpy(stage + cur, q.probs + vol + (size_t)q.off_zyx[0] * plane, pl.slab);
    cur += align16(pl.slab);
    d.seg = (long long)cur;
    memcpy(stage + cur, q.seg, pl.n * 8);
    cur += align16(pl.n * 8);
    d.bits = (long long)bits_cur;
    bits_cur += pl.bit_words;
    d.d2 = (long long)d2_cur;
    d2_cur += 4 * pl.n;
    d.id_a = q.id_a;
    d.id_b = q.id_b;
    d.Y = q.box_zyx[1];
    d.X = q.box_zyx[2];
    d.oy = q.off_zyx[1];
    d.ox = q.off_zyx[2];
    d.cz = q.shape_zyx[0];
    d.cy = q.shape_zyx[1];
    d.cx = q.shape_zyx[2];
    d.n = (int)pl.n;
    d.ty = tile_columns(d.cy, d.cx);
    d.tz = tile_columns(d.cz, (long long)d.cy * d.cx);
    d.pad = 0;
    lds_y = std::max(lds_y, (size_t)d.cy * d.ty * sizeof(double));
    lds_z = std::max(lds_z, (size_t)d.cz * d.tz * sizeof(double));
    const long long groups = ((long long)pl.n + 63) / 64;
    const long long rows = (long long)d.cz * d.cy;
    const long long per[4] = {
        (groups + kGroupsPerBlock - 1) / kGroupsPerBlock,
        (rows + kWaves - 1) / kWaves,
        4LL * d.cz * ((d.cx + d.ty - 1) / d.ty),
        4LL * (((long long)d.cy * d.cx + d.tz - 1) / d.tz)};
    for (int k = 0; k < 4; ++k) {
      st[k][i] = (int)blocks[k];
      blocks[k] += per[k];
    }
  }
  for (int k = 0; k < 4; ++k) {
    st[k][count] = (int)blocks[k];
    if (blocks[k] >= 2147483647LL)
      return ffn_set_error(FFN_ERR_ARG, "group of %zu points needs too many "
                           "blocks", count);
  }

  hipStream_t s = a->stream;
  uint8_t* dev = static_cast<uint8_t*>(a->in.p);
  U_TRY(hipMemcpyAsync(dev, stage, upload, hipMemcpyHostToDevice, s));
  U_TRY(hipMemsetAsync(a->small.p, 0, res_bytes, s));
  const PairDev* ddescs = reinterpret_cast<const PairDev*>(dev + desc_off);
  const int* dst[4];
  for (int k = 0; k < 4; ++k)
    dst[k] = reinterpret_cast<const int*>(dev + starts_off) + k * (count + 1);
  u64* dcounts = static_cast<u64*>(a->small.p);
  u64* dmax = dcounts + count * FFN_PAIR_COUNTS;
  double* droot = reinterpret_cast<double*>(dmax + count * 4);
  u64* bits = static_cast<u64*>(a->bits.p);
  double* d2 = static_cast<double*>(a->d2.p);
  U_OK(a->timer_start());
  hipLaunchKernelGGL(pair_mask_kernel, dim3((unsigned)blocks[0]), dim3(kThreads),
                     0, s, ddescs, dst[0], npts, (const uint8_t*)dev,
                     (const uint8_t*)dev, bits, dcounts);
  hipLaunchKernelGGL(pair_edt_x_kernel, dim3((unsigned)blocks[1]),
                     dim3(kThreads), 0, s, ddescs, dst[1], npts,
                     (const u64*)bits, d2, voxel[2]);
  hipLaunchKernelGGL(pair_edt_line_kernel, dim3((unsigned)blocks[2]),
                     dim3(kThreads), lds_y, s, ddescs, dst[2], npts, d2, 1,
                     voxel[1], dmax);
  hipLaunchKernelGGL(pair_edt_line_kernel, dim3((unsigned)blocks[3]),
                     dim3(kThreads), lds_z, s, ddescs, dst[3], npts, d2, 0,
                     voxel[0], dmax);
  hipLaunchKernelGGL(pair_root_kernel,
                     dim3((unsigned)((count * 4 + kThreads - 1) / kThreads)),
                     dim3(kThreads), 0, s, (const u64*)dmax, droot,
                     (int)(count * 4));
  U_TRY(hipGetLastError());
  U_OK(add_elapsed(a, &a->ms[0]));
  U_TRY(hipMemcpyAsync(counts + first * FFN_PAIR_COUNTS, dcounts,
                       count * FFN_PAIR_COUNTS * 8, hipMemcpyDeviceToHost, s));
  U_TRY(hipMemcpyAsync(max_edt + first * 4, droot, count * 4 * 8,
                       hipMemcpyDeviceToHost, s));
  U_TRY(hipStreamSynchronize(s));
  return FFN_OK;
}

}  // namespace

extern "C" {

int ffn_analyzer_create(int device_id, ffn_analyzer** out) {
  return ffn_unit::unit_create(device_id, out);
}

void ffn_analyzer_destroy(ffn_analyzer* a) { ffn_unit::unit_destroy(a); }

int ffn_analyzer_pair_stats(ffn_analyzer* a, const ffn_pair_desc* points,
                            size_t n, const uint8_t table[256],
                            const double voxel_size_zyx[3], uint64_t* counts,
                            double* max_edt) {
  if (!a || !table || !voxel_size_zyx || (n && (!points || !counts || !max_edt)))
    return ffn_set_error(FFN_ERR_ARG, "NULL argument");
  for (int k = 0; k < 3; ++k)
    if (!(voxel_size_zyx[k] > 0.0) || !std::isfinite(voxel_size_zyx[k]))
      return ffn_set_error(FFN_ERR_ARG, "voxel_size[%d] must be positive", k);
  std::vector<PairPlan> plans(n);
  for (size_t i = 0; i < n; ++i) {
    const ffn_pair_desc& q = points[i];
    if (!q.probs || !q.seg)
      return ffn_set_error(FFN_ERR_ARG, "point %zu: NULL input", i);
    size_t nv = 0, nbox = 0;
    U_OK(check_shape(q.shape_zyx, i, &nv));
    U_OK(check_shape(q.box_zyx, i, &nbox));
    for (int k = 0; k < 3; ++k)
      if (q.off_zyx[k] < 0 ||
          (long long)q.off_zyx[k] + q.shape_zyx[k] > q.box_zyx[k])
        return ffn_set_error(FFN_ERR_ARG,
                             "point %zu: crop leaves the box on axis %d", i, k);
    plans[i] = plan_pair(q, nv);
  }
  U_TRY(hipSetDevice(a->device_id));
  a->ms[0] = 0.0;
  a->voxels[0] = 0.0;
  size_t first = 0;
  while (first < n) {
    size_t count = 0, bytes = 0;
    while (first + count < n && count < (size_t)kMaxGroupPoints) {
      const PairPlan& pl = plans[first + count];
      const size_t need = pl.in_bytes + pl.bit_words * 8 + pl.n * 32;
      if (count && bytes + need > kGroupBytes) break;
      bytes += need;
      a->voxels[0] += (double)pl.n;
      ++count;
    }
    U_OK(run_pair_group(a, points, plans, first, count, table, voxel_size_zyx,
                        counts, max_edt));
    first += count;
  }
  return FFN_OK;
}

int ffn_analyzer_endpoint_overlaps(ffn_analyzer* a,
                                   const ffn_endpoint_desc* points, size_t n,
                                   const uint8_t table[256], size_t cap,
                                   int32_t* row_point, uint64_t* row_old,
                                   uint32_t* row_counts, uint64_t* num_new,
                                   size_t* n_rows) {
  if (!a || !table || !n_rows || (n && (!points || !num_new)) ||
      (cap && (!row_point || !row_old || !row_counts)))
    return ffn_set_error(FFN_ERR_ARG, "NULL argument");
  *n_rows = 0;
  std::vector<size_t> nv(n);
  for (size_t i = 0; i < n; ++i) {
    if (!points[i].probs || !points[i].seg)
      return ffn_set_error(FFN_ERR_ARG, "point %zu: NULL input", i);
    U_OK(check_shape(points[i].shape_zyx, i, &nv[i]));
  }
  U_TRY(hipSetDevice(a->device_id));
  a->ms[1] = 0.0;
  a->voxels[1] = 0.0;
  hipStream_t s = a->stream;
  U_OK(ensure(a->rows_point, cap * 4));
  U_OK(ensure(a->rows_old, cap * 8));
  U_OK(ensure(a->rows_counts, cap * 8));
  // flags (overflow, bad id) and the row counter live apart from the
  // per-group results so that the counter runs on across groups
  U_OK(ensure(a->ctrl, 64));
  int* flags = static_cast<int*>(a->ctrl.p);
  u64* n_out = reinterpret_cast<u64*>(a->ctrl.p) + 1;
  U_TRY(hipMemsetAsync(a->ctrl.p, 0, 64, s));
  size_t first = 0;
  while (first < n) {
    size_t count = 0, bytes = 0;
    while (first + count < n && count < (size_t)kMaxGroupPoints) {
      const size_t need = align16(nv[first + count]) +
                          align16(nv[first + count] * 8);
      if (count && bytes + need > kGroupBytes) break;
      bytes += need;
      a->voxels[1] += (double)nv[first + count];
      ++count;
    }
    const size_t desc_off = 256;
    const size_t starts_off = align16(desc_off + count * sizeof(EndDev));
    const size_t in_off = align16(starts_off + (count + 1) * sizeof(int));
    const size_t upload = in_off + bytes;
    U_OK(ensure(a->stage, upload));
    U_OK(ensure(a->in, upload));
    U_OK(ensure(a->small, count * 8));
    uint8_t* stage = static_cast<uint8_t*>(a->stage.p);
    memcpy(stage, table, 256);
    EndDev* descs = reinterpret_cast<EndDev*>(stage + desc_off);
    int* starts = reinterpret_cast<int*>(stage + starts_off);
    long long blocks = 0;
    size_t cur = in_off;
    const long long per_block = (long long)kEndIters * kThreads;
    for (size_t i = 0; i < count; ++i) {
      const size_t m = nv[first + i];
      descs[i].probs = (long long)cur;
      memcpy(stage + cur, points[first + i].probs, m);
      cur += align16(m);
      descs[i].seg = (long long)cur;
      memcpy(stage + cur, points[first + i].seg, m * 8);
      cur += align16(m * 8);
      descs[i].n = (int)m;
      descs[i].id = points[first + i].id;
      descs[i].has_id = points[first + i].has_id;
      starts[i] = (int)blocks;
      blocks += ((long long)m + per_block - 1) / per_block;
    }
    starts[count] = (int)blocks;
    uint8_t* dev = static_cast<uint8_t*>(a->in.p);
    U_TRY(hipMemcpyAsync(dev, stage, upload, hipMemcpyHostToDevice, s));
    // growth stops at 2^26 slots per point or 8 GiB (64 bytes per slot, the
    // table that would follow counted) for the group
    const u32 limit =
        (u32)std::min<size_t>((size_t)1 << 26, ((size_t)1 << 27) / count + 1);
    int state[2];
    U_OK(table_grow(s, a->keys, count, &a->nslots, limit, flags, state,
                    [&](u32 mask) {
      const size_t slots = ((size_t)mask + 1) * count;
      U_OK(ensure(a->vals, slots * 8));
      U_TRY(hipMemsetAsync(a->vals.p, 0, slots * 8, s));
      U_TRY(hipMemsetAsync(a->small.p, 0, count * 8, s));
      U_OK(a->timer_start());
      hipLaunchKernelGGL(
          endpoint_count_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s,
          reinterpret_cast<const EndDev*>(dev + desc_off),
          reinterpret_cast<const int*>(dev + starts_off), (int)count,
          (const uint8_t*)dev, (const uint8_t*)dev,
          static_cast<u64*>(a->keys.p), static_cast<u32*>(a->vals.p),
          mask, flags, static_cast<u64*>(a->small.p));
      U_TRY(hipGetLastError());
      return add_elapsed(a, &a->ms[1]);
    }));
    if (state[1])
      return ffn_set_error(FFN_ERR_ARG, "segment id 2^64 - 1 is not supported");
    const long long total = (long long)a->nslots * (long long)count;
    U_OK(a->timer_start());
    hipLaunchKernelGGL(endpoint_emit_kernel,
                       dim3((unsigned)((total + kThreads - 1) / kThreads)),
                       dim3(kThreads), 0, s,
                       reinterpret_cast<const EndDev*>(dev + desc_off),
                       static_cast<const u64*>(a->keys.p),
                       static_cast<const u32*>(a->vals.p), a->nslots, total,
                       (int)first, (u64)cap, n_out,
                       static_cast<int*>(a->rows_point.p),
                       static_cast<u64*>(a->rows_old.p),
                       static_cast<u32*>(a->rows_counts.p));
    U_TRY(hipGetLastError());
    U_OK(add_elapsed(a, &a->ms[1]));
    U_TRY(hipMemcpy(num_new + first, a->small.p, count * 8,
                    hipMemcpyDeviceToHost));
    first += count;
  }
  u64 found = 0;
  U_TRY(hipMemcpy(&found, n_out, 8, hipMemcpyDeviceToHost));
  *n_rows = (size_t)found;
  if (found > cap)
    return ffn_set_error(FFN_ERR_ARG, "%llu rows exceed cap %zu", found, cap);
  if (found) {
    U_TRY(hipMemcpy(row_point, a->rows_point.p, (size_t)found * 4,
                    hipMemcpyDeviceToHost));
    U_TRY(hipMemcpy(row_old, a->rows_old.p, (size_t)found * 8,
                    hipMemcpyDeviceToHost));
    U_TRY(hipMemcpy(row_counts, a->rows_counts.p, (size_t)found * 8,
                    hipMemcpyDeviceToHost));
  }
  return FFN_OK;
}

int ffn_analyzer_last_timing(ffn_analyzer* a, double kernel_ms[2],
                             double voxels[2]) {
  if (!a || !kernel_ms || !voxels)
    return ffn_set_error(FFN_ERR_ARG, "NULL argument");
  for (int k = 0; k < 2; ++k) {
    kernel_ms[k] = a->ms[k];
    voxels[k] = a->voxels[k];
  }
  return FFN_OK;
}

}  // extern "C"
