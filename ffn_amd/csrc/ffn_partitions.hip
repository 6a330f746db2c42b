// libffn_hip.so -- local-object-mask partition maps (include/ffn_partitions.h).
//
// Label sizes: one sweep that counts every id through the global hash table of
// ffn_table.h (a run of equal ids inside a wave costs one insert).  Compute: a
// relabelling sweep turns every voxel into 0 (not kept) or the table slot of
// its id + 1, then lom_count_kernel counts per output tile.
//
// lom_count_kernel, one workgroup per tile of tz x ty x 64 output voxels.  The
// tile's halo, (tz + 2 rz) x (ty + 2 ry) rows of 64 + 2 rx <= 128 voxels, is
// handled one label at a time, in ascending order of the labels that occur
// among the tile's own centres (a block-wide minimum picks the next one, so
// there is no list of labels to size): a wave ballot of `voxel == label` turns
// every halo row into 128 bits in LDS; the x and y passes are one sweep per
// (z, x) column down the rows -- the x window is a popcount of the shifted row
// bits, the y window a sliding sum -- that leaves u16 sums in LDS; the z pass
// is a sliding u32 sum per (y, x) column.  The mask is one more round over the
// plane `mask != 0` with the test `sum > 0`.  Scratch is the relabelled volume
// plus LDS, and the work per tile grows with the labels among its centres, not
// with the labels of the volume or the extent of their bounding boxes.
//
// Plain C++, ordinary stream-ordered launches, bounded loops only; every LDS
// index is below the allocation made for the full tile.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/ffn_hip.h"
#include "../../include/ffn_partitions.h"
#include "ffn_internal.h"
#include "ffn_table.h"
#include "ffn_unit.h"

// the sphere test must round exactly as the specification's: no FMA contraction
#pragma clang fp contract(off)

namespace {

using ffn_table::u32;
using ffn_table::u64;
using ffn_table::kBackground;
using ffn_table::kEmptyKey;
using ffn_table::run_leaders;
using ffn_table::run_mask;
using ffn_table::table_compact_kernel;
using ffn_table::table_find;
using ffn_table::table_grow;
using ffn_table::table_insert;

typedef unsigned char u8;
typedef unsigned short u16;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTileX = 64;      // one output voxel per lane
constexpr int kMaxTile = 8;     // tile extent along z and y
constexpr int kMaxRadius = 32;  // 64 + 2 * 32 = 128 bits per halo row
constexpr int kOwnRows = kMaxTile / kWaves;  // y rows of the tile per thread
constexpr int kRowBatch = 8;    // halo rows a wave loads before it ballots
constexpr size_t kLdsPreferred = 78 * 1024;  // two workgroups per CU
// The 8 x 4 x 64 tile at the radius limit: (8 + 64) * (4 + 64) * 16 bytes of
// row bits + (8 + 64) * 4 * 64 u16 sums.  No tile choose_tile picks needs more.
constexpr size_t kLdsLimit = 72 * 68 * 16 + 72 * 4 * kTileX * 2;
static_assert(kLdsLimit == 115200, "largest dynamic LDS of lom_count_kernel");

// ---- label sizes -----------------------------------------------------------------

template <typename T>
__global__ __launch_bounds__(kThreads) void label_count_kernel(
    const T* __restrict__ seg, size_t n, u64* keys, u64* counts, u32 mask,
    int* overflow) {
  const int lane = threadIdx.x & 63;
  const size_t per_block =
      ((n + gridDim.x - 1) / gridDim.x + kThreads - 1) / kThreads * kThreads;
  const size_t lo = (size_t)blockIdx.x * per_block;
  const size_t hi = lo + per_block < n ? lo + per_block : n;
  for (size_t base = lo; base < hi; base += kThreads) {
    const size_t i = base + threadIdx.x;
    const bool valid = i < hi;
    const u64 key = valid ? (u64)seg[i] : kEmptyKey;
    if (valid && key == kEmptyKey) *overflow = 2;  // 2^64 - 1 marks a free slot
    const u64 leaders = run_leaders(key, valid, lane);
    const u64 vm = __ballot(valid);
    if (valid && key != kEmptyKey && ((leaders >> lane) & 1)) {
      const u32 s = table_insert(keys, mask, key, overflow);
      if (s != kBackground)
        atomicAdd(&counts[s], (u64)__popcll(vm & run_mask(leaders, lane)));
    }
  }
}

// ---- compute -----------------------------------------------------------------------

__global__ void keep_slots_kernel(const u64* __restrict__ in_keys,
                                  const u8* __restrict__ in_keep, u32 n,
                                  const u64* __restrict__ keys, u32 mask,
                                  u8* keep_slot) {
  const u32 k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const u64 key = in_keys[k];
  if (key == 0 || key == kEmptyKey || !in_keep[k]) return;
  const u32 s = table_find(keys, mask, key);
  if (s != kBackground) keep_slot[s] = 1;
}

// lab[i] = slot of seg[i] + 1 where that id is kept, else 0.
template <typename T>
__global__ __launch_bounds__(kThreads) void relabel_kernel(
    const T* __restrict__ seg, size_t n, const u64* __restrict__ keys, u32 mask,
    const u8* __restrict__ keep_slot, u32* __restrict__ lab) {
  const size_t stride = (size_t)gridDim.x * kThreads;
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n;
       i += stride) {
    const u64 key = (u64)seg[i];
    u32 v = 0;
    if (key != 0) {
      const u32 s = table_find(keys, mask, key);
      if (s != kBackground && keep_slot[s]) v = s + 1;
    }
    lab[i] = v;
  }
}

struct LomGeom {
  int ny, nx;          // row strides of the volume
  int rz, ry, rx;      // radii
  int oz, oy, ox;      // valid region
  int tz, ty;          // tile (kTileX along x)
  int hz, hy;          // tz + 2 rz, ty + 2 ry: the halo the LDS is sized for
};

// Voxels set among bits [x, x + w) of the 128-bit row (lo, hi); x < 64,
// w <= 65, m64 = the low min(w, 64) bits.
__device__ __forceinline__ u32 window_count(const u64* row, int x, int w,
                                            u64 m64) {
  const u64 lo = row[0], hi = row[1];
  const u64 sh = x ? (lo >> x) | (hi << (64 - x)) : lo;
  return (u32)__popcll(sh & m64) + (w == 65 ? (u32)((hi >> x) & 1ull) : 0u);
}

// Rounds 1 and 2 of a plane: the bit rows of `voxel == target` (kMask: of
// `mask != 0`) over the halo of extent (ez, ey, ex), then xy[(z, yc, x)] = the
// number of set voxels in the x and y windows of halo slice z.
template <bool kMask>
__device__ __forceinline__ void plane_xy_sums(
    const u32* __restrict__ lab, const u8* __restrict__ mask, const LomGeom& g,
    int z0, int y0, int x0, int ez, int ey, int ex, u32 target, u64* bits,
    u16* xy, int lane, int wave) {
  // kRowBatch rows per wave and turn: all their loads are issued before the
  // first ballot waits for one
  const int rows = ez * ey;
  for (int r0 = wave * kRowBatch; r0 < rows; r0 += kWaves * kRowBatch) {
    u32 v0[kRowBatch], v1[kRowBatch];
    int slot[kRowBatch];
    int hz = r0 / ey, hy = r0 - hz * ey;
#pragma unroll
    for (int j = 0; j < kRowBatch; ++j) {
      const bool live = r0 + j < rows;
      const size_t base =
          ((size_t)(z0 + hz) * g.ny + (size_t)(y0 + hy)) * g.nx + x0;
      slot[j] = (hz * g.hy + hy) * 2;
      v0[j] = v1[j] = 0;  // matches neither a label (>= 1) nor a set mask byte
      if (live && lane < ex)
        v0[j] = kMask ? (u32)mask[base + lane] : lab[base + lane];
      if (live && lane + 64 < ex)
        v1[j] = kMask ? (u32)mask[base + lane + 64] : lab[base + lane + 64];
      if (++hy == ey) {
        hy = 0;
        ++hz;
      }
    }
#pragma unroll
    for (int j = 0; j < kRowBatch; ++j) {
      if (r0 + j >= rows) break;  // wave-uniform
      const u64 b0 = __ballot(kMask ? v0[j] != 0 : v0[j] == target);
      const u64 b1 = __ballot(kMask ? v1[j] != 0 : v1[j] == target);
      if (lane == 0) {
        bits[slot[j]] = b0;
        bits[slot[j] + 1] = b1;
      }
    }
  }
  __syncthreads();
  const int w = 2 * g.rx + 1;
  const u64 m64 = w >= 64 ? ~0ull : (1ull << w) - 1;
  for (int hz = wave; hz < ez; hz += kWaves) {
    u32 sum = 0;
    for (int hy = 0; hy < ey; ++hy) {
      sum += window_count(bits + (hz * g.hy + hy) * 2, lane, w, m64);
      if (hy >= 2 * g.ry) {
        const int yc = hy - 2 * g.ry;
        xy[(hz * g.ty + yc) * kTileX + lane] = (u16)sum;
        sum -= window_count(bits + (hz * g.hy + yc) * 2, lane, w, m64);
      }
    }
  }
  __syncthreads();
}

__global__ __launch_bounds__(kThreads) void lom_count_kernel(
    const u32* __restrict__ lab, const u8* __restrict__ mask, LomGeom g,
    const u8* __restrict__ class_of, const double* __restrict__ spheres,
    int n_spheres, u8* __restrict__ out, u32* __restrict__ counts, u64* hist) {
  extern __shared__ u64 lds_bits[];
  __shared__ u32 s_min[kWaves];
  __shared__ u32 s_hist[256];
  u64* bits = lds_bits;
  u16* xy = reinterpret_cast<u16*>(lds_bits + (size_t)g.hz * g.hy * 2);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int z0 = blockIdx.z * g.tz, y0 = blockIdx.y * g.ty;
  const int x0 = blockIdx.x * kTileX;
  // this tile, clamped to the valid region, and its halo
  const int cz = min(g.tz, g.oz - z0), cy = min(g.ty, g.oy - y0);
  const int cx = min(kTileX, g.ox - x0);
  const int ez = cz + 2 * g.rz, ey = cy + 2 * g.ry, ex = cx + 2 * g.rx;
  s_hist[threadIdx.x] = 0;

  // A thread owns the columns (yc = k * kWaves + wave, x = lane) of the tile:
  // their centre labels and their results live in registers.
  u32 own_lab[kOwnRows][kMaxTile];
  u32 own_out[kOwnRows][kMaxTile];
#pragma unroll
  for (int k = 0; k < kOwnRows; ++k) {
    const int yc = k * kWaves + wave;
#pragma unroll
    for (int zc = 0; zc < kMaxTile; ++zc) {
      u32 l = 0;
      if (yc < cy && zc < cz && lane < cx)
        l = lab[((size_t)(z0 + zc + g.rz) * g.ny + (size_t)(y0 + yc + g.ry)) *
                    g.nx + x0 + lane + g.rx];
      own_lab[k][zc] = l;
      own_out[k][zc] = 0;
    }
  }

  if (mask) {
    plane_xy_sums<true>(lab, mask, g, z0, y0, x0, ez, ey, ex, 0u, bits, xy,
                        lane, wave);
#pragma unroll
    for (int k = 0; k < kOwnRows; ++k) {
      const int yc = k * kWaves + wave;
      if (yc >= cy) continue;
      u32 sum = 0;
      for (int hz = 0; hz < 2 * g.rz; ++hz)
        sum += xy[(hz * g.ty + yc) * kTileX + lane];
#pragma unroll
      for (int zc = 0; zc < kMaxTile; ++zc) {
        if (zc >= cz) continue;
        sum += xy[((zc + 2 * g.rz) * g.ty + yc) * kTileX + lane];
        if (sum) own_out[k][zc] = 255;
        sum -= xy[(zc * g.ty + yc) * kTileX + lane];
      }
    }
  }

  // one round per label among the centres, in ascending order; a tile holds
  // kMaxTile^2 * kTileX centres, which bounds the rounds
  u32 last = 0;
  for (int round = 0; round <= kMaxTile * kMaxTile * kTileX; ++round) {
    u32 next = 0xffffffffu;
#pragma unroll
    for (int k = 0; k < kOwnRows; ++k)
#pragma unroll
      for (int zc = 0; zc < kMaxTile; ++zc) {
        const u32 l = own_lab[k][zc];
        if (l > last && l < next) next = l;
      }
    for (int off = 32; off > 0; off >>= 1) {
      const u32 t = __shfl_xor(next, off);
      if (t < next) next = t;
    }
    if (lane == 0) s_min[wave] = next;
    __syncthreads();  // (also: the last round's reads of xy are done)
#pragma unroll
    for (int v = 0; v < kWaves; ++v) next = min(next, s_min[v]);
    __syncthreads();
    if (next == 0xffffffffu) break;  // block-uniform
    last = next;
    plane_xy_sums<false>(lab, mask, g, z0, y0, x0, ez, ey, ex, next, bits, xy,
                         lane, wave);
#pragma unroll
    for (int k = 0; k < kOwnRows; ++k) {
      const int yc = k * kWaves + wave;
      if (yc >= cy) continue;
      u32 sum = 0;
      for (int hz = 0; hz < 2 * g.rz; ++hz)
        sum += xy[(hz * g.ty + yc) * kTileX + lane];
#pragma unroll
      for (int zc = 0; zc < kMaxTile; ++zc) {
        if (zc >= cz) continue;
        sum += xy[((zc + 2 * g.rz) * g.ty + yc) * kTileX + lane];
        if (own_lab[k][zc] == next) {  // (never an x beyond the tile: those hold 0)
          counts[((size_t)(z0 + zc) * g.oy + (size_t)(y0 + yc)) * g.ox + x0 +
                 lane] = sum;
          if (own_out[k][zc] != 255) own_out[k][zc] = class_of[sum];
        }
        sum -= xy[(zc * g.ty + yc) * kTileX + lane];
      }
    }
  }

  // spheres, output, histogram
#pragma unroll
  for (int k = 0; k < kOwnRows; ++k) {
    const int yc = k * kWaves + wave;
#pragma unroll
    for (int zc = 0; zc < kMaxTile; ++zc) {
      if (yc >= cy || zc >= cz || lane >= cx) continue;
      u32 v = own_out[k][zc];
      if (v != 255) {
        const double px = (double)(x0 + lane + g.rx);
        const double py = (double)(y0 + yc + g.ry);
        const double pz = (double)(z0 + zc + g.rz);
        for (int s = 0; s < n_spheres; ++s) {
          const double dx = px - spheres[4 * s], dy = py - spheres[4 * s + 1];
          const double dz = pz - spheres[4 * s + 2], r = spheres[4 * s + 3];
          if ((dx * dx + dy * dy) + dz * dz <= r * r) v = 255;
        }
      }
      out[((size_t)(z0 + zc) * g.oy + (size_t)(y0 + yc)) * g.ox + x0 + lane] =
          (u8)v;
      atomicAdd(&s_hist[v], 1u);
    }
  }
  __syncthreads();
  const u32 c = s_hist[threadIdx.x];
  if (c) atomicAdd(&hist[threadIdx.x], (u64)c);
}

using ffn_unit::DevBuf;
using ffn_unit::ensure;

size_t lom_lds_bytes(int tz, int ty, const int r[3]) {
  const size_t hz = tz + 2 * r[0], hy = ty + 2 * r[1];
  return hz * hy * 16 + hz * ty * kTileX * sizeof(u16);
}

// 8 x 8 x 64 where its LDS lets two workgroups share a CU, else 8 x 4 x 64
// (115,200 bytes at the radius limit).
void choose_tile(const int r[3], int* tz, int* ty) {
  *tz = kMaxTile;
  *ty = lom_lds_bytes(kMaxTile, kMaxTile, r) <= kLdsPreferred ? kMaxTile
                                                              : kMaxTile / 2;
}

}  // namespace

struct ffn_partitions : ffn_unit::Unit {
  DevBuf in, keys, table_counts, aux0, aux1, small;
  DevBuf in_keys, in_keep, keep_slot, lab, mask, class_of, spheres;
  DevBuf out, counts, hist;
  long long shape[3] = {0, 0, 0};
  long long out_shape[3] = {0, 0, 0};
  int elem_bytes = 0;
  u32 nslots = 0;
  bool have_volume = false, have_result = false;
  double ms[2] = {0.0, 0.0}, bytes[2] = {0.0, 0.0};
};

namespace {

template <typename T>
int label_sizes_impl(ffn_partitions* h, size_t n, size_t cap, uint64_t* ids,
                     uint64_t* sizes, size_t* n_ids) {
  const T* seg = static_cast<const T*>(h->in.p);
  U_OK(ensure(h->small, 64));
  U_TRY(hipMemsetAsync(h->small.p, 0, 64, h->stream));
  int* overflow = static_cast<int*>(h->small.p);
  u32* n_out = reinterpret_cast<u32*>(h->small.p) + 2;
  int state[2];
  u32 nslots = std::max<u32>(h->nslots, 1u << 18);
  U_OK(table_grow(h->stream, h->keys, 1, &nslots, 1u << 30, overflow, state,
                  [&](u32 mask) {
    U_OK(ensure(h->table_counts, ((size_t)mask + 1) * 8));
    U_TRY(hipMemsetAsync(h->table_counts.p, 0, ((size_t)mask + 1) * 8,
                         h->stream));
    U_OK(h->timer_start());
    const int blocks = (int)std::min<size_t>(
        2048, std::max<size_t>(1, (n + 16 * kThreads - 1) / (16 * kThreads)));
    hipLaunchKernelGGL((label_count_kernel<T>), dim3(blocks), dim3(kThreads), 0,
                       h->stream, seg, n, static_cast<u64*>(h->keys.p),
                       static_cast<u64*>(h->table_counts.p), mask, overflow);
    U_TRY(hipGetLastError());
    h->bytes[0] = (double)n * sizeof(T);
    return h->timer_stop(&h->ms[0]);
  }));
  if (state[0])  // (2: the id that marks a free slot)
    return ffn_set_error(FFN_ERR_ARG, "label id 2^64 - 1 is not supported");
  h->nslots = nslots;
  h->have_volume = true;
  const size_t want = std::min<size_t>(cap, nslots);
  U_OK(ensure(h->aux0, want * 8));
  U_OK(ensure(h->aux1, want * 8));
  hipLaunchKernelGGL(table_compact_kernel<u64>, dim3((nslots + 255) / 256),
                     dim3(256), 0, h->stream,
                     static_cast<const u64*>(h->keys.p),
                     static_cast<const u64*>(h->table_counts.p), nslots,
                     static_cast<u64*>(h->aux0.p), static_cast<u64*>(h->aux1.p),
                     static_cast<u32*>(nullptr), (u32)want, n_out);
  U_TRY(hipGetLastError());
  u32 found = 0;
  U_TRY(hipMemcpyAsync(&found, n_out, sizeof(u32), hipMemcpyDeviceToHost,
                       h->stream));
  U_TRY(hipStreamSynchronize(h->stream));
  *n_ids = found;
  if (found > cap)
    return ffn_set_error(FFN_ERR_ARG, "%u distinct ids exceed cap %zu", found,
                         cap);
  if (found == 0) return FFN_OK;
  U_TRY(hipMemcpy(ids, h->aux0.p, (size_t)found * 8, hipMemcpyDeviceToHost));
  U_TRY(hipMemcpy(sizes, h->aux1.p, (size_t)found * 8, hipMemcpyDeviceToHost));
  return FFN_OK;
}

int upload(ffn_partitions* h, DevBuf& buf, const void* src, size_t bytes) {
  U_OK(ensure(buf, bytes));
  if (bytes)
    U_TRY(hipMemcpyAsync(buf.p, src, bytes, hipMemcpyHostToDevice, h->stream));
  return FFN_OK;
}

}  // namespace

extern "C" {

int ffn_partitions_create(int device_id, ffn_partitions** out) {
  const int rc = ffn_unit::unit_create(device_id, out);
  if (rc != FFN_OK) return rc;
  // The limit belongs to the kernel on this device, not to the handle: clear
  // it for the largest tile once, whatever radii this or another handle sees.
  const hipError_t e = hipFuncSetAttribute(
      reinterpret_cast<const void*>(&lom_count_kernel),
      hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsLimit);
  if (e != hipSuccess) {
    ffn_unit::unit_destroy(*out);
    *out = nullptr;
    return ffn_set_error(FFN_ERR_HIP, "hipFuncSetAttribute: %s",
                         hipGetErrorString(e));
  }
  return FFN_OK;
}

void ffn_partitions_destroy(ffn_partitions* h) { ffn_unit::unit_destroy(h); }

int ffn_partitions_label_sizes(ffn_partitions* h, const void* seg,
                               int elem_bytes, const int64_t shape_zyx[3],
                               size_t cap, uint64_t* ids, uint64_t* sizes,
                               size_t* n) {
  if (!h || !seg || !shape_zyx || !n || (cap && (!ids || !sizes)))
    return ffn_set_error(FFN_ERR_ARG, "NULL argument");
  *n = 0;
  if (elem_bytes != 4 && elem_bytes != 8)
    return ffn_set_error(FFN_ERR_ARG, "elem_bytes must be 4 or 8");
  double voxels = 1.0;
  for (int k = 0; k < 3; ++k) {
    if (shape_zyx[k] < 1)
      return ffn_set_error(FFN_ERR_ARG, "shape[%d] = %lld", k,
                           (long long)shape_zyx[k]);
    voxels *= (double)shape_zyx[k];
  }
  if (voxels >= 2147483648.0)
    return ffn_set_error(FFN_ERR_ARG, "volume of 2^31 voxels or more");
  U_TRY(hipSetDevice(h->device_id));
  const size_t count = (size_t)shape_zyx[0] * shape_zyx[1] * shape_zyx[2];
  h->have_volume = h->have_result = false;
  U_OK(upload(h, h->in, seg, count * elem_bytes));
  for (int k = 0; k < 3; ++k) h->shape[k] = shape_zyx[k];
  h->elem_bytes = elem_bytes;
  if (elem_bytes == 4)
    return label_sizes_impl<uint32_t>(h, count, cap, ids, sizes, n);
  return label_sizes_impl<uint64_t>(h, count, cap, ids, sizes, n);
}

int ffn_partitions_compute(ffn_partitions* h, const uint64_t* keys,
                           const uint8_t* keep, size_t n_keys,
                           const int32_t radius_zyx[3], const uint8_t* class_of,
                           size_t class_len, const uint8_t* mask,
                           const double* spheres, size_t n_spheres) {
  if (!h || !radius_zyx || !class_of || (n_keys && (!keys || !keep)) ||
      (n_spheres && !spheres))
    return ffn_set_error(FFN_ERR_ARG, "NULL argument");
  if (!h->have_volume)
    return ffn_set_error(FFN_ERR_STATE,
                         "no volume resident: call ffn_partitions_label_sizes");
  if (n_keys > 0xffffffffull || n_spheres > (1u << 20))
    return ffn_set_error(FFN_ERR_ARG, "too many keys or spheres");
  LomGeom g;
  int r[3];
  long long o[3];
  size_t fov = 1;
  for (int k = 0; k < 3; ++k) {
    r[k] = radius_zyx[k];
    if (r[k] < 0 || r[k] > kMaxRadius)
      return ffn_set_error(FFN_ERR_ARG, "radius[%d] = %d outside 0..%d", k, r[k],
                           kMaxRadius);
    o[k] = h->shape[k] - 2LL * r[k];
    if (o[k] < 1)
      return ffn_set_error(FFN_ERR_ARG,
                           "axis %d of %lld voxels is shorter than the LOM "
                           "diameter %d", k, h->shape[k], 2 * r[k] + 1);
    fov *= (size_t)(2 * r[k] + 1);
  }
  if (class_len != fov + 1)
    return ffn_set_error(FFN_ERR_ARG, "class table of %zu entries, expected %zu",
                         class_len, fov + 1);
  U_TRY(hipSetDevice(h->device_id));
  h->have_result = false;
  const size_t n = (size_t)h->shape[0] * h->shape[1] * h->shape[2];
  const size_t n_out = (size_t)o[0] * o[1] * o[2];
  g.ny = (int)h->shape[1];
  g.nx = (int)h->shape[2];
  g.rz = r[0];
  g.ry = r[1];
  g.rx = r[2];
  g.oz = (int)o[0];
  g.oy = (int)o[1];
  g.ox = (int)o[2];
  choose_tile(r, &g.tz, &g.ty);
  g.hz = g.tz + 2 * g.rz;
  g.hy = g.ty + 2 * g.ry;
  const size_t lds = lom_lds_bytes(g.tz, g.ty, r);
  const long long gx = (g.ox + kTileX - 1) / kTileX;
  const long long gy = (g.oy + g.ty - 1) / g.ty, gz = (g.oz + g.tz - 1) / g.tz;
  if (gy > 65535 || gz > 65535)
    return ffn_set_error(FFN_ERR_ARG, "volume too long for the tile grid");
  if (lds > kLdsLimit)
    return ffn_set_error(FFN_ERR_ARG, "tile needs %zu bytes of LDS", lds);

  U_OK(upload(h, h->in_keys, keys, n_keys * 8));
  U_OK(upload(h, h->in_keep, keep, n_keys));
  U_OK(upload(h, h->class_of, class_of, class_len));
  if (mask) U_OK(upload(h, h->mask, mask, n));
  U_OK(upload(h, h->spheres, spheres, n_spheres * 32));
  U_OK(ensure(h->keep_slot, h->nslots));
  U_OK(ensure(h->lab, n * 4));
  U_OK(ensure(h->out, n_out));
  U_OK(ensure(h->counts, n_out * 4));
  U_OK(ensure(h->hist, 256 * 8));
  U_TRY(hipMemsetAsync(h->keep_slot.p, 0, h->nslots, h->stream));
  U_TRY(hipMemsetAsync(h->counts.p, 0, n_out * 4, h->stream));
  U_TRY(hipMemsetAsync(h->hist.p, 0, 256 * 8, h->stream));
  U_OK(h->timer_start());
  if (n_keys)
    hipLaunchKernelGGL(keep_slots_kernel, dim3((unsigned)((n_keys + 255) / 256)),
                       dim3(256), 0, h->stream,
                       static_cast<const u64*>(h->in_keys.p),
                       static_cast<const u8*>(h->in_keep.p), (u32)n_keys,
                       static_cast<const u64*>(h->keys.p), h->nslots - 1,
                       static_cast<u8*>(h->keep_slot.p));
  {
    const int blocks = (int)std::min<size_t>(
        4096, std::max<size_t>(1, (n + kThreads - 1) / kThreads));
    if (h->elem_bytes == 4)
      hipLaunchKernelGGL((relabel_kernel<uint32_t>), dim3(blocks),
                         dim3(kThreads), 0, h->stream,
                         static_cast<const uint32_t*>(h->in.p), n,
                         static_cast<const u64*>(h->keys.p), h->nslots - 1,
                         static_cast<const u8*>(h->keep_slot.p),
                         static_cast<u32*>(h->lab.p));
    else
      hipLaunchKernelGGL((relabel_kernel<uint64_t>), dim3(blocks),
                         dim3(kThreads), 0, h->stream,
                         static_cast<const uint64_t*>(h->in.p), n,
                         static_cast<const u64*>(h->keys.p), h->nslots - 1,
                         static_cast<const u8*>(h->keep_slot.p),
                         static_cast<u32*>(h->lab.p));
  }
  hipLaunchKernelGGL(lom_count_kernel,
                     dim3((unsigned)gx, (unsigned)gy, (unsigned)gz),
                     dim3(kThreads), lds, h->stream,
                     static_cast<const u32*>(h->lab.p),
                     mask ? static_cast<const u8*>(h->mask.p) : nullptr, g,
                     static_cast<const u8*>(h->class_of.p),
                     static_cast<const double*>(h->spheres.p), (int)n_spheres,
                     static_cast<u8*>(h->out.p), static_cast<u32*>(h->counts.p),
                     static_cast<u64*>(h->hist.p));
  U_TRY(hipGetLastError());
  U_OK(h->timer_stop(&h->ms[1]));
  h->bytes[1] = (double)n * h->elem_bytes + (double)n_out;
  for (int k = 0; k < 3; ++k) h->out_shape[k] = o[k];
  h->have_result = true;
  return FFN_OK;
}

int ffn_partitions_read(ffn_partitions* h, uint8_t* partitions,
                        uint32_t* counts, uint64_t* histogram) {
  if (!h) return ffn_set_error(FFN_ERR_ARG, "NULL argument");
  if (!h->have_result)
    return ffn_set_error(FFN_ERR_STATE,
                         "no result resident: call ffn_partitions_compute");
  U_TRY(hipSetDevice(h->device_id));
  const size_t n =
      (size_t)h->out_shape[0] * h->out_shape[1] * h->out_shape[2];
  if (partitions)
    U_TRY(hipMemcpy(partitions, h->out.p, n, hipMemcpyDeviceToHost));
  if (counts) U_TRY(hipMemcpy(counts, h->counts.p, n * 4, hipMemcpyDeviceToHost));
  if (histogram)
    U_TRY(hipMemcpy(histogram, h->hist.p, 256 * 8, hipMemcpyDeviceToHost));
  return FFN_OK;
}

int ffn_partitions_last_timing(ffn_partitions* h, double kernel_ms[2],
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
