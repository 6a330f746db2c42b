// libffn_hip.so -- agglomeration decision points (include/ffn_decision.h).
//
// Stage 1, nearest-segment expansion: three separable passes over per-voxel
// state (d2 as f64, id as u32), each the exact lexicographic minimum of
// (d2 + (delta * s)^2, id) along one axis.  The x pass is two wave-scan sweeps
// per row; the y and z passes stage whole lines of a tile in LDS (tile rows
// run along x, so global accesses stay contiguous) and scan outwards from
// each voxel until the axis term alone exceeds the best value found, which
// keeps every tie and needs no lower envelope.  Stage 2, contact scan: per-pair
// minimum of the contact distance through the two-level (LDS, then global)
// hash table of ffn_table.h, then a second sweep that writes the minimising
// candidates through a wave-aggregated counter.
//
// Ordinary stream-ordered launches with bounded loops only.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/ffn_decision.h"
#include "../../include/ffn_hip.h"
#include "ffn_internal.h"
#include "ffn_table.h"
#include "ffn_unit.h"

// d2 sums must round exactly as the specification's: no FMA contraction.
#pragma clang fp contract(off)

namespace {

using ffn_table::u32;
using ffn_table::u64;
using ffn_table::kBackground;
using ffn_table::kEmptyKey;
using ffn_table::block_claim;
using ffn_table::table_find;
using ffn_table::table_grow;
using ffn_table::table_insert;

constexpr int kThreads = 256;
constexpr int kMaxAxis = 4096;
constexpr size_t kLineLdsBytes = 48 * 1024;  // tile of a y / z pass
constexpr int kLineBytesPerVoxel = 12;       // f64 d2 + u32 id
constexpr int kLdsSlots = 1024;              // per-block pair table

// Label of a voxel as the kernels see it: 0 = unlabelled.  Sets *bad for an id
// that does not fit the 32-bit state.
template <typename T>
__device__ __forceinline__ u32 load_label(const T* seg, size_t i, int* bad) {
  const u64 v = (u64)seg[i];
  if (v >= 0xffffffffull) {  // 4- and 8-byte input alike
    *bad = 2;
    return 0;
  }
  return (u32)v;
}

template <>
__device__ __forceinline__ u32 load_label<int32_t>(const int32_t* seg, size_t i,
                                                   int* bad) {
  const int32_t v = seg[i];
  return v > 0 ? (u32)v : 0u;
}

// x pass: one wave per row.  Sweep 1 (left to right) leaves in LDS, per x, the
// last labelled voxel at or before x as (x' + 1) << 32 | id; sweep 2 (right to
// left) finds the first labelled voxel at or after x as (nx - x') << 32 | id
// and writes the lexicographic minimum of the two (d2, id) candidates.
// In sweep 2 a lane reads back only the LDS slot it wrote itself in sweep 1, so
// no barrier stands between the sweeps: the array is per-lane storage for a
// row's left candidates (8 B per voxel, which is what limits a block to one
// wave at nx = 4096).
template <typename T>
__global__ __launch_bounds__(kThreads) void expand_x_kernel(
    const T* __restrict__ seg, int nx, long long rows, double sx,
    double* __restrict__ d2, u32* __restrict__ id, int* bad) {
  extern __shared__ u64 lds_left[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long row = (long long)blockIdx.x * (blockDim.x >> 6) + wave;
  if (row >= rows) return;  // whole wave
  u64* left = lds_left + (size_t)wave * nx;
  const T* srow = seg + row * nx;
  const int chunks = (nx + 63) / 64;
  u64 carry = 0;
  for (int c = 0; c < chunks; ++c) {
    const int x = c * 64 + lane;
    const u32 v = x < nx ? load_label<T>(srow, x, bad) : 0u;
    u64 p = v ? (((u64)(x + 1) << 32) | v) : 0ull;
    for (int off = 1; off < 64; off <<= 1) {
      const u64 t = __shfl_up(p, off);
      if (lane >= off && t > p) p = t;
    }
    if (carry > p) p = carry;
    carry = __shfl(p, 63);
    if (x < nx) left[x] = p;
  }
  carry = 0;
  const double inf = __builtin_inf();
  for (int c = chunks - 1; c >= 0; --c) {
    const int x = c * 64 + lane;
    const u64 l = x < nx ? left[x] : 0ull;
    // a labelled voxel is its own left candidate at distance 0
    const bool own = x < nx && (int)(l >> 32) == x + 1;
    u64 p = own ? (((u64)(nx - x) << 32) | (u32)l) : 0ull;
    for (int off = 1; off < 64; off <<= 1) {
      const u64 t = __shfl_down(p, off);
      if (lane + off < 64 && t > p) p = t;
    }
    if (carry > p) p = carry;
    carry = __shfl(p, 0);
    if (x >= nx) continue;
    double best = inf;
    u32 best_id = 0;
    if (l) {
      const double t = (double)(x - ((int)(l >> 32) - 1)) * sx;
      best = t * t;
      best_id = (u32)l;
    }
    if (p) {
      const double t = (double)((nx - (int)(p >> 32)) - x) * sx;
      const double v = t * t;
      const u32 pid = (u32)p;
      if (v < best || (v == best && pid < best_id)) {
        best = v;
        best_id = pid;
      }
    }
    d2[row * nx + x] = best;
    id[row * nx + x] = best_id;
  }
}

// y / z pass, in place.  A block owns `tx` neighbouring columns (contiguous in
// memory) of one outer slab with all `len` elements of their lines (`stride`
// apart), loads them into LDS, and then every voxel scans outwards:
//   out(q) = lexmin over p of (in(p) + ((q - p) * w)^2, id(p)).
// The scan stops once (k * w)^2 alone exceeds the best value, so every
// candidate that could still tie has been seen.  `final` turns d2 into the
// distance and applies max_distance.
__global__ __launch_bounds__(kThreads) void expand_line_kernel(
    double* __restrict__ d2, u32* __restrict__ id, int len, long long stride,
    long long ncols, long long outer_stride, double w, int tx, int final,
    double max_distance) {
  extern __shared__ double lds_line[];
  __shared__ int col_any[64];
  double* sd = lds_line;
  u32* sid = reinterpret_cast<u32*>(lds_line + (size_t)len * tx);
  const long long col0 = (long long)blockIdx.x * tx;
  const long long base = (long long)blockIdx.y * outer_stride;
  const int total = len * tx;
  const double inf = __builtin_inf();
  if (threadIdx.x < 64) col_any[threadIdx.x] = 0;
  __syncthreads();
  for (int e = threadIdx.x; e < total; e += kThreads) {
    const int q = e / tx, c = e - q * tx;
    const long long col = col0 + c;
    double v = inf;
    u32 l = 0;
    if (col < ncols) {
      const long long g = base + (long long)q * stride + col;
      v = d2[g];
      l = id[g];
      if (v < inf) col_any[c] = 1;
    }
    sd[e] = v;
    sid[e] = l;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < total; e += kThreads) {
    const int q = e / tx, c = e - q * tx;
    const long long col = col0 + c;
    if (col >= ncols) continue;
    double best = sd[e];
    u32 best_id = sid[e];
    if (col_any[c]) {  // (a line without any finite value stays +inf / 0)
      const int kmax = q > len - 1 - q ? q : len - 1 - q;
      for (int k = 1; k <= kmax; ++k) {
        const double t = (double)k * w;
        const double t2 = t * t;
        if (t2 > best) break;
        if (q - k >= 0) {
          const double v = sd[e - k * tx] + t2;
          const u32 l = sid[e - k * tx];
          if (v < best || (v == best && l < best_id)) {
            best = v;
            best_id = l;
          }
        }
        if (q + k < len) {
          const double v = sd[e + k * tx] + t2;
          const u32 l = sid[e + k * tx];
          if (v < best || (v == best && l < best_id)) {
            best = v;
            best_id = l;
          }
        }
      }
    }
    const long long g = base + (long long)q * stride + col;
    if (final) {
      best = __dsqrt_rn(best);
      if (max_distance >= 0.0 && best > max_distance) best_id = 0;
    }
    d2[g] = best;
    id[g] = best_id;
  }
}

// ---- contact scan -------------------------------------------------------------

struct ScanGeom {
  long long ny, nx;          // row strides of the resident volume
  long long lo[3];           // crop origin
  int cz, cy, cx;            // crop size
  long long n;               // voxels of the crop
};

__device__ __forceinline__ u64 dist_bits(double v) {
  return (u64)__double_as_longlong(v);
}

// Candidate `o` (0..6) of crop voxel (z, y, x) holding id a / distance ea at
// flat index i: true if it exists; then *key is the ordered pair, *dist the
// contact distance.
__device__ __forceinline__ bool contact(const u32* __restrict__ id,
                                        const double* __restrict__ edt,
                                        const ScanGeom& g, long long i, int z,
                                        int y, int x, u32 a, double ea, int o,
                                        u64* key, double* dist) {
  const int dz = ((o + 1) >> 2) & 1, dy = ((o + 1) >> 1) & 1, dx = (o + 1) & 1;
  if (z + dz >= g.cz || y + dy >= g.cy || x + dx >= g.cx) return false;
  const long long j = i + ((long long)dz * g.ny + dy) * g.nx + dx;
  const u32 b = id[j];
  if (b == 0 || b == a) return false;
  *key = a < b ? ((u64)a | ((u64)b << 32)) : ((u64)b | ((u64)a << 32));
  *dist = (ea + edt[j]) / 2.0;
  return true;
}

__device__ __forceinline__ long long crop_index(const ScanGeom& g, long long v,
                                                int* z, int* y, int* x) {
  *x = (int)(v % g.cx);
  const long long r = v / g.cx;
  *y = (int)(r % g.cy);
  *z = (int)(r / g.cy);
  return ((g.lo[0] + *z) * g.ny + (g.lo[1] + *y)) * g.nx + g.lo[2] + *x;
}

// Pass 1: vals[slot of pair] = min over candidates of the distance's bit
// pattern (a non-negative f64 orders like its bits).
__global__ __launch_bounds__(kThreads) void contact_min_kernel(
    const u32* __restrict__ id, const double* __restrict__ edt, ScanGeom g,
    u64* keys, u64* vals, u32 mask, int* overflow) {
  __shared__ u64 skeys[kLdsSlots];
  __shared__ u64 svals[kLdsSlots];
  for (int s = threadIdx.x; s < kLdsSlots; s += kThreads) {
    skeys[s] = kEmptyKey;
    svals[s] = ~0ull;
  }
  __syncthreads();
  const long long per_block =
      ((g.n + gridDim.x - 1) / gridDim.x + kThreads - 1) / kThreads * kThreads;
  const long long lo = (long long)blockIdx.x * per_block;
  const long long hi = lo + per_block < g.n ? lo + per_block : g.n;
  for (long long v = lo + threadIdx.x; v < hi; v += kThreads) {
    int z, y, x;
    const long long i = crop_index(g, v, &z, &y, &x);
    const u32 a = id[i];
    if (a == 0) continue;
    const double ea = edt[i];
    for (int o = 0; o < 7; ++o) {
      u64 key;
      double dist;
      if (!contact(id, edt, g, i, z, y, x, a, ea, o, &key, &dist)) continue;
      const u64 bits = dist_bits(dist);
      const int s = block_claim<kLdsSlots>(skeys, key);
      if (s >= 0) {
        atomicMin(&svals[s], bits);
      } else {  // block table crowded: straight to the global one
        const u32 t = table_insert(keys, mask, key, overflow);
        if (t != kBackground) atomicMin(&vals[t], bits);
      }
    }
  }
  __syncthreads();
  for (int s = threadIdx.x; s < kLdsSlots; s += kThreads) {
    const u64 k = skeys[s];
    if (k != kEmptyKey) {
      const u32 t = table_insert(keys, mask, k, overflow);
      if (t != kBackground) atomicMin(&vals[t], svals[s]);
    }
  }
}

// Pass 2: every candidate at its pair's minimum goes out, one atomic per wave.
__global__ __launch_bounds__(kThreads) void contact_emit_kernel(
    const u32* __restrict__ id, const double* __restrict__ edt, ScanGeom g,
    const u64* __restrict__ keys, const u64* __restrict__ vals, u32 mask,
    u64 cap, u64* n_out, u64* out_key, double* out_dist, int* out_off) {
  const int lane = threadIdx.x & 63;
  const long long stride = (long long)gridDim.x * kThreads;
  const long long rounds = (g.n + stride - 1) / stride;
  long long v = (long long)blockIdx.x * kThreads + threadIdx.x;
  for (long long r = 0; r < rounds; ++r, v += stride) {
    int z = 0, y = 0, x = 0;
    long long i = 0;
    u32 a = 0;
    double ea = 0.0;
    u32 hits = 0;
    if (v < g.n) {
      i = crop_index(g, v, &z, &y, &x);
      a = id[i];
      if (a != 0) {
        ea = edt[i];
        for (int o = 0; o < 7; ++o) {
          u64 key;
          double dist;
          if (!contact(id, edt, g, i, z, y, x, a, ea, o, &key, &dist)) continue;
          const u32 t = table_find(keys, mask, key);
          if (t != kBackground && vals[t] == dist_bits(dist)) hits |= 1u << o;
        }
      }
    }
    if (__ballot(hits != 0) == 0) continue;  // wave-uniform
    const u32 mine = (u32)__popc(hits);
    u32 incl = mine;
    for (int off = 1; off < 64; off <<= 1) {
      const u32 t = __shfl_up(incl, off);
      if (lane >= off) incl += t;
    }
    const u32 total = __shfl(incl, 63);
    u64 base = 0;
    if (lane == 63) base = atomicAdd(n_out, (u64)total);
    base = __shfl(base, 63);
    u64 slot = base + (incl - mine);
    for (int o = 0; o < 7; ++o) {
      if (!((hits >> o) & 1)) continue;
      u64 key;
      double dist;
      contact(id, edt, g, i, z, y, x, a, ea, o, &key, &dist);
      if (slot < cap) {
        out_key[slot] = key;
        out_dist[slot] = dist;
        out_off[slot * 4 + 0] = o;
        out_off[slot * 4 + 1] = z;
        out_off[slot * 4 + 2] = y;
        out_off[slot * 4 + 3] = x;
      }
      ++slot;
    }
  }
}

using ffn_unit::DevBuf;
using ffn_unit::ensure;

}  // namespace

struct ffn_decision : ffn_unit::Unit {
  DevBuf in, d2, id, keys, vals, out_key, out_dist, out_off, small;
  long long shape[3] = {0, 0, 0};
  bool valid = false;  // an expansion is resident
  u32 nslots = 0;
  double ms[2] = {0.0, 0.0}, bytes[2] = {0.0, 0.0};
};

namespace {

int check_geometry(const int64_t shape[3], const double voxel[3]) {
  if (!shape || !voxel) return ffn_set_error(FFN_ERR_ARG, "NULL argument");
  double n = 1.0;
  for (int k = 0; k < 3; ++k) {
    if (shape[k] < 1 || shape[k] > kMaxAxis)
      return ffn_set_error(FFN_ERR_ARG, "shape[%d] = %lld outside 1..%d", k,
                           (long long)shape[k], kMaxAxis);
    if (!(voxel[k] > 0.0) || !std::isfinite(voxel[k]))
      return ffn_set_error(FFN_ERR_ARG, "voxel_size[%d] must be positive", k);
    n *= (double)shape[k];
  }
  if (n >= 2147483648.0)
    return ffn_set_error(FFN_ERR_ARG, "volume of 2^31 voxels or more");
  return FFN_OK;
}

int tile_columns(int len, long long ncols) {
  int tx = 64;
  while (tx > 1 && (size_t)len * tx * kLineBytesPerVoxel > kLineLdsBytes) tx >>= 1;
  while (tx > 1 && tx / 2 >= ncols) tx >>= 1;
  return tx;
}

// The three passes over labels already on the device.
template <typename T>
int expand_impl(ffn_decision* h, const T* seg, const int64_t shape[3],
                const double voxel_xyz[3], double max_distance) {
  const long long nz = shape[0], ny = shape[1], nx = shape[2];
  const size_t n = (size_t)nz * ny * nx;
  h->valid = false;
  U_OK(ensure(h->d2, n * 8));
  U_OK(ensure(h->id, n * 4));
  U_OK(ensure(h->small, 64));
  U_TRY(hipMemsetAsync(h->small.p, 0, 64, h->stream));
  double* d2 = static_cast<double*>(h->d2.p);
  u32* id = static_cast<u32*>(h->id.p);
  int* bad = static_cast<int*>(h->small.p);
  const double maxd = max_distance >= 0.0 ? max_distance : -1.0;  // NaN -> -1
  U_OK(h->timer_start());
  {
    const long long rows = nz * ny;
    int waves = kThreads / 64;
    while (waves > 1 && (size_t)waves * nx * 8 > kLineLdsBytes) waves >>= 1;
    const long long blocks = (rows + waves - 1) / waves;
    hipLaunchKernelGGL((expand_x_kernel<T>), dim3((unsigned)blocks),
                       dim3(waves * 64), (size_t)waves * nx * 8, h->stream, seg,
                       (int)nx, rows, voxel_xyz[0], d2, id, bad);
  }
  {
    const int tx = tile_columns((int)ny, nx);
    hipLaunchKernelGGL(expand_line_kernel,
                       dim3((unsigned)((nx + tx - 1) / tx), (unsigned)nz),
                       dim3(kThreads), (size_t)ny * tx * kLineBytesPerVoxel,
                       h->stream, d2, id, (int)ny, nx, nx, ny * nx,
                       voxel_xyz[1], tx, 0, maxd);
  }
  {
    const long long cols = ny * nx;
    const int tx = tile_columns((int)nz, cols);
    hipLaunchKernelGGL(expand_line_kernel,
                       dim3((unsigned)((cols + tx - 1) / tx), 1u),
                       dim3(kThreads), (size_t)nz * tx * kLineBytesPerVoxel,
                       h->stream, d2, id, (int)nz, cols, cols, 0LL,
                       voxel_xyz[2], tx, 1, maxd);
  }
  U_TRY(hipGetLastError());
  U_OK(h->timer_stop(&h->ms[0]));
  h->bytes[0] = (double)n * (sizeof(T) + 5.0 * kLineBytesPerVoxel);
  int flag = 0;
  U_TRY(hipMemcpy(&flag, bad, sizeof(int), hipMemcpyDeviceToHost));
  if (flag)
    return ffn_set_error(FFN_ERR_ARG,
                         "label id >= 2^32 - 1: remap ids before expanding");
  for (int k = 0; k < 3; ++k) h->shape[k] = shape[k];
  h->valid = true;
  return FFN_OK;
}

}  // namespace

extern "C" {

int ffn_decision_create(int device_id, ffn_decision** out) {
  return ffn_unit::unit_create(device_id, out);
}

void ffn_decision_destroy(ffn_decision* h) { ffn_unit::unit_destroy(h); }

int ffn_decision_expand(ffn_decision* h, const void* seg, int elem_bytes,
                        const int64_t shape_zyx[3],
                        const double voxel_size_xyz[3], double max_distance) {
  if (!h || !seg) return ffn_set_error(FFN_ERR_ARG, "NULL argument");
  if (elem_bytes != 4 && elem_bytes != 8)
    return ffn_set_error(FFN_ERR_ARG, "elem_bytes must be 4 or 8");
  U_OK(check_geometry(shape_zyx, voxel_size_xyz));
  U_TRY(hipSetDevice(h->device_id));
  const size_t n = (size_t)shape_zyx[0] * shape_zyx[1] * shape_zyx[2];
  h->valid = false;
  U_OK(ensure(h->in, n * elem_bytes));
  U_TRY(hipMemcpyAsync(h->in.p, seg, n * elem_bytes, hipMemcpyHostToDevice,
                       h->stream));
  if (elem_bytes == 4)
    return expand_impl<uint32_t>(h, static_cast<const uint32_t*>(h->in.p),
                                 shape_zyx, voxel_size_xyz, max_distance);
  return expand_impl<uint64_t>(h, static_cast<const uint64_t*>(h->in.p),
                               shape_zyx, voxel_size_xyz, max_distance);
}

int ffn_decision_expand_device(ffn_decision* h, const int32_t* seg_dev,
                               const int64_t shape_zyx[3],
                               const double voxel_size_xyz[3],
                               double max_distance) {
  if (!h || !seg_dev) return ffn_set_error(FFN_ERR_ARG, "NULL argument");
  U_OK(check_geometry(shape_zyx, voxel_size_xyz));
  U_TRY(hipSetDevice(h->device_id));
  return expand_impl<int32_t>(h, seg_dev, shape_zyx, voxel_size_xyz,
                              max_distance);
}

int ffn_decision_expand_canvas(ffn_decision* h, ffn_canvas* canvas,
                               const double voxel_size_xyz[3],
                               double max_distance, int64_t shape_zyx_out[3]) {
  if (!h || !canvas) return ffn_set_error(FFN_ERR_ARG, "NULL argument");
  FfnCanvasView v;
  U_OK(ffn_canvas_view(canvas, &v));
  if (v.device_id != h->device_id)
    return ffn_set_error(FFN_ERR_ARG, "canvas lives on device %d, handle on %d",
                         v.device_id, h->device_id);
  U_TRY(hipSetDevice(h->device_id));
  // the canvas' own stream may still be committing the last segment
  U_TRY(hipStreamSynchronize(static_cast<hipStream_t>(v.engine_stream)));
  const int64_t shape[3] = {v.shape_zyx[0], v.shape_zyx[1], v.shape_zyx[2]};
  if (shape_zyx_out)
    for (int k = 0; k < 3; ++k) shape_zyx_out[k] = shape[k];
  return ffn_decision_expand_device(h, v.segmentation, shape, voxel_size_xyz,
                                    max_distance);
}

int ffn_decision_read(ffn_decision* h, uint32_t* expanded, double* edt) {
  if (!h) return ffn_set_error(FFN_ERR_ARG, "NULL argument");
  if (!h->valid)
    return ffn_set_error(FFN_ERR_STATE,
                         "no expansion resident: call ffn_decision_expand");
  U_TRY(hipSetDevice(h->device_id));
  const size_t n = (size_t)h->shape[0] * h->shape[1] * h->shape[2];
  if (expanded)
    U_TRY(hipMemcpy(expanded, h->id.p, n * 4, hipMemcpyDeviceToHost));
  if (edt) U_TRY(hipMemcpy(edt, h->d2.p, n * 8, hipMemcpyDeviceToHost));
  return FFN_OK;
}

int ffn_decision_contact_minima(ffn_decision* h, const int64_t lo_zyx[3],
                                const int64_t hi_zyx[3], size_t cap,
                                uint64_t* pair_a, uint64_t* pair_b,
                                double* dist, int32_t* off_zyx, size_t* n) {
  if (!h || !n || (cap && (!pair_a || !pair_b || !dist || !off_zyx)) ||
      (lo_zyx == nullptr) != (hi_zyx == nullptr))
    return ffn_set_error(FFN_ERR_ARG, "NULL argument");
  *n = 0;
  if (!h->valid)
    return ffn_set_error(FFN_ERR_STATE,
                         "no expansion resident: call ffn_decision_expand");
  ScanGeom g;
  g.ny = h->shape[1];
  g.nx = h->shape[2];
  long long size[3];
  for (int k = 0; k < 3; ++k) {
    const long long lo = lo_zyx ? lo_zyx[k] : 0;
    const long long hi = hi_zyx ? hi_zyx[k] : h->shape[k];
    if (lo < 0 || hi > h->shape[k] || lo > hi)
      return ffn_set_error(FFN_ERR_ARG, "sub-box [%lld, %lld) outside axis %d",
                           lo, hi, k);
    g.lo[k] = lo;
    size[k] = hi - lo;
  }
  g.cz = (int)size[0];
  g.cy = (int)size[1];
  g.cx = (int)size[2];
  g.n = size[0] * size[1] * size[2];
  h->ms[1] = 0.0;
  h->bytes[1] = 0.0;
  if (g.n == 0) return FFN_OK;
  U_TRY(hipSetDevice(h->device_id));
  const u32* id = static_cast<const u32*>(h->id.p);
  const double* edt = static_cast<const double*>(h->d2.p);
  U_OK(ensure(h->small, 64));
  int* overflow = static_cast<int*>(h->small.p);
  u64* n_out = reinterpret_cast<u64*>(h->small.p) + 1;
  U_TRY(hipMemsetAsync(h->small.p, 0, 64, h->stream));
  int state[2];  // (word 1 is not used: the expansion has refused bad ids)
  u32 nslots = std::max<u32>(h->nslots, 1u << 18);
  double ms = 0.0;
  U_OK(table_grow(h->stream, h->keys, 1, &nslots, 1u << 28, overflow, state,
                  [&](u32 mask) {
    U_OK(ensure(h->vals, ((size_t)mask + 1) * 8));
    U_TRY(hipMemsetAsync(h->vals.p, 0xff, ((size_t)mask + 1) * 8, h->stream));
    U_OK(h->timer_start());
    const int blocks = (int)std::min<long long>(
        2048, std::max<long long>(1, (g.n + 16 * kThreads - 1) / (16 * kThreads)));
    hipLaunchKernelGGL(contact_min_kernel, dim3(blocks), dim3(kThreads), 0,
                       h->stream, id, edt, g, static_cast<u64*>(h->keys.p),
                       static_cast<u64*>(h->vals.p), mask, overflow);
    U_TRY(hipGetLastError());
    return h->timer_stop(&ms);
  }));
  h->nslots = nslots;
  U_OK(ensure(h->out_key, cap * 8));
  U_OK(ensure(h->out_dist, cap * 8));
  U_OK(ensure(h->out_off, cap * 16));
  U_OK(h->timer_start());
  {
    const int blocks = (int)std::min<long long>(
        4096, std::max<long long>(1, (g.n + kThreads - 1) / kThreads));
    hipLaunchKernelGGL(contact_emit_kernel, dim3(blocks), dim3(kThreads), 0,
                       h->stream, id, edt, g,
                       static_cast<const u64*>(h->keys.p),
                       static_cast<const u64*>(h->vals.p), nslots - 1, (u64)cap,
                       n_out, static_cast<u64*>(h->out_key.p),
                       static_cast<double*>(h->out_dist.p),
                       static_cast<int*>(h->out_off.p));
    U_TRY(hipGetLastError());
  }
  double ms2 = 0.0;
  U_OK(h->timer_stop(&ms2));
  h->ms[1] = ms + ms2;
  // both sweeps read id + distance of every voxel of the crop once (the
  // neighbour reads hit the caches)
  h->bytes[1] = 2.0 * (double)g.n * kLineBytesPerVoxel;
  u64 found = 0;
  U_TRY(hipMemcpy(&found, n_out, sizeof(u64), hipMemcpyDeviceToHost));
  *n = (size_t)found;
  if (found > cap)
    return ffn_set_error(FFN_ERR_ARG, "%llu candidates exceed cap %zu", found,
                         cap);
  if (found == 0) return FFN_OK;
  std::vector<u64> keys(found);
  U_TRY(hipMemcpy(keys.data(), h->out_key.p, (size_t)found * 8,
                  hipMemcpyDeviceToHost));
  U_TRY(hipMemcpy(dist, h->out_dist.p, (size_t)found * 8,
                  hipMemcpyDeviceToHost));
  U_TRY(hipMemcpy(off_zyx, h->out_off.p, (size_t)found * 16,
                  hipMemcpyDeviceToHost));
  for (u64 k = 0; k < found; ++k) {
    pair_a[k] = keys[k] & 0xffffffffull;
    pair_b[k] = keys[k] >> 32;
  }
  return FFN_OK;
}

int ffn_decision_last_timing(ffn_decision* h, double kernel_ms[2],
                             double algorithmic_bytes[2]) {
  if (!h || !kernel_ms || !algorithmic_bytes)
    return ffn_set_error(FFN_ERR_ARG, "NULL argument");
  for (int k = 0; k < 2; ++k) {
    kernel_ms[k] = h->ms[k];
    algorithmic_bytes[k] = h->bytes[k];
  }
  return FFN_OK;
}

}  // extern "C"
