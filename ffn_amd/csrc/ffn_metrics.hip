// libffn_hip.so -- segmentation metrics declared in include/ffn_metrics.h.
//
// Integer kernels only (gfx950); every sum is a u64 atomic, so a result does
// not depend on the order in which workgroups arrive, and the floats are the
// host's (ffn_amd/metrics.py).
//
// Contingency: the joint histogram of (ground-truth id, segment id) through
// the two-level id table of ffn_table.h, as ffn_labels.hip's pair_count_kernel
// does it -- one contiguous span per block, runs of equal pairs inside a wave
// counted once, a table of the block in LDS, flushed into the global table at
// the end.  What is new here: the two volumes have element widths of their
// own, the span is a span of the BOX (rows of the box are walked with a
// mixed-radix position, no division per voxel), and voxels whose ground truth
// is 0 can be left out.  A lane that is left out carries the table's empty
// key: such lanes form runs of their own that nobody counts, so no run of
// counted voxels reaches across one of them.  HBM-bound: box voxels x the two
// element widths.
//
// Skeleton: four small table kernels over nodes and edges (gather the segment
// under every node, count nodes per (segment, skeleton), mark the segments in
// which two skeletons have enough nodes, classify the edges and sum the
// correct ones per (skeleton, segment)).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/ffn_hip.h"
#include "../../include/ffn_metrics.h"
#include "ffn_internal.h"
#include "ffn_table.h"
#include "ffn_unit.h"

namespace {

using ffn_table::u32;
using ffn_table::u64;
using ffn_table::kBackground;
using ffn_table::kEmptyKey;
using ffn_table::block_claim;
using ffn_table::run_leaders;
using ffn_table::run_mask;
using ffn_table::table_compact_kernel;
using ffn_table::table_find;
using ffn_table::table_grow;
using ffn_table::table_insert;
using ffn_unit::DevBuf;
using ffn_unit::ensure;

constexpr int kThreads = 256;
constexpr int kLdsSlots = 2048;        // per-block pre-aggregation table
constexpr int kSpan = 16 * kThreads;   // voxels of a block before spans lengthen
constexpr int kMaxBlocks = 2048;
constexpr u32 kFirstSlots = 1u << 15;  // global tables start here, grow fourfold
constexpr u32 kMaxSlots = 1u << 30;
constexpr u64 kMaxId = 0xffffffffull;  // ids must be below this

// A box of a volume, walked in the raster order of the BOX.
struct BoxGeom {
  long long n;        // voxels of the box
  long long origin;   // flat index (volume) of the box's first voxel
  long long X, YX;    // strides of the volume: a row, a plane
  u32 by, bx;         // rows per plane of the box, voxels per row
};

template <typename TA, typename TB>
__global__ __launch_bounds__(kThreads) void contingency_kernel(
    const TA* __restrict__ gt, const TB* __restrict__ seg, BoxGeom g,
    int ignore_gt_zero, u64* keys, u64* counts, u32 mask, int* flags) {
  __shared__ u64 skeys[kLdsSlots];
  __shared__ u32 scnt[kLdsSlots];
  for (int s = threadIdx.x; s < kLdsSlots; s += kThreads) {
    skeys[s] = kEmptyKey;
    scnt[s] = 0;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const long long per_block =
      ((g.n + gridDim.x - 1) / gridDim.x + kThreads - 1) / kThreads * kThreads;
  const long long lo = (long long)blockIdx.x * per_block;
  const long long hi = lo + per_block < g.n ? lo + per_block : g.n;
  // This thread's first voxel as (row of the box, x) and as a flat index of
  // the volume; then kThreads box voxels further every round: the digits of
  // kThreads in the radix (by, bx) are added with at most one carry each.
  const long long first = lo + threadIdx.x;
  const long long row = first / g.bx;
  u32 x = (u32)(first % g.bx);
  u32 y = (u32)(row % g.by);
  long long off = g.origin + (row / g.by) * g.YX + (long long)y * g.X + x;
  const u32 sx = kThreads % g.bx;
  const u32 sy = (kThreads / g.bx) % g.by;
  const long long step =
      (long long)((kThreads / g.bx) / g.by) * g.YX + (long long)sy * g.X + sx;
  const long long carry_x = g.X - g.bx;                   // x -= bx, y += 1
  const long long carry_y = g.YX - (long long)g.by * g.X;  // y -= by, z += 1
  for (long long base = lo; base < hi; base += kThreads) {
    u64 key = kEmptyKey;  // left out: beyond the span, or ground truth 0
    if (base + threadIdx.x < hi) {
      const u64 a = (u64)gt[off], b = (u64)seg[off];
      if (a >= kMaxId || b >= kMaxId)
        flags[1] = 2;  // id outside the packable range (caller must remap)
      else if (!ignore_gt_zero || a != 0)
        key = a | (b << 32);
    }
    // every lane takes part: lanes left out hold kEmptyKey and form runs of
    // their own, so a run of a real key is counted lanes only
    const u64 leaders = run_leaders(key, true, lane);
    if (key != kEmptyKey && ((leaders >> lane) & 1)) {
      const u32 run = (u32)__popcll(run_mask(leaders, lane));
      const int s = block_claim<kLdsSlots>(skeys, key);
      if (s >= 0) {
        atomicAdd(&scnt[s], run);
      } else {  // block table crowded: straight to the global one
        const u32 t = table_insert(keys, mask, key, flags);
        if (t != kBackground) atomicAdd(&counts[t], (u64)run);
      }
    }
    x += sx;
    off += step;
    if (x >= g.bx) {
      x -= g.bx;
      y += 1;
      off += carry_x;
    }
    y += sy;
    if (y >= g.by) {
      y -= g.by;
      off += carry_y;
    }
  }
  __syncthreads();
  for (int s = threadIdx.x; s < kLdsSlots; s += kThreads) {
    const u32 c = scnt[s];
    if (c) {
      const u32 t = table_insert(keys, mask, skeys[s], flags);
      if (t != kBackground) atomicAdd(&counts[t], (u64)c);
    }
  }
}

// ---- skeleton edges ----------------------------------------------------------

struct NodeGeom {
  int lo[3], hi[3];  // the box
  long long X, YX;
};

// node_seg[k] = seg[node k], 0 outside the box
template <typename T>
__global__ __launch_bounds__(kThreads) void node_gather_kernel(
    const T* __restrict__ seg, NodeGeom g, const int* __restrict__ nodes, u32 n,
    u32* __restrict__ node_seg, int* flags) {
  const u32 k = blockIdx.x * kThreads + threadIdx.x;
  if (k >= n) return;
  const int z = nodes[3 * k], y = nodes[3 * k + 1], x = nodes[3 * k + 2];
  u64 v = 0;
  if (z >= g.lo[0] && z < g.hi[0] && y >= g.lo[1] && y < g.hi[1] &&
      x >= g.lo[2] && x < g.hi[2])
    v = (u64)seg[(long long)z * g.YX + (long long)y * g.X + x];
  if (v >= kMaxId) {
    flags[1] = 2;
    v = 0;
  }
  node_seg[k] = (u32)v;
}

// nodes per (segment, skeleton), segment 0 skipped; neighbouring nodes of a
// chain mostly share both, so runs inside a wave are counted once
__global__ __launch_bounds__(kThreads) void node_count_kernel(
    const u32* __restrict__ node_seg, const u32* __restrict__ skel, u32 n,
    u64* keys, u64* counts, u32 mask, int* flags) {
  const u32 k = blockIdx.x * kThreads + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const u32 s = k < n ? node_seg[k] : 0u;
  const u64 key = s ? ((u64)s | ((u64)skel[k] << 32)) : kEmptyKey;
  const u64 leaders = run_leaders(key, true, lane);
  if (key != kEmptyKey && ((leaders >> lane) & 1)) {
    const u32 t = table_insert(keys, mask, key, flags);
    if (t != kBackground)
      atomicAdd(&counts[t], (u64)__popcll(run_mask(leaders, lane)));
  }
}

// qualified[segment] = skeletons with >= min_nodes nodes in it; the (segment,
// skeleton) table is read slot by slot (a compaction would visit the same
// entries)
__global__ __launch_bounds__(kThreads) void merger_mark_kernel(
    const u64* __restrict__ pair_keys, const u64* __restrict__ pair_counts,
    u32 nslots, u64 min_nodes, u64* seg_keys, u64* qualified, u32 mask,
    int* flags) {
  const u32 s = blockIdx.x * kThreads + threadIdx.x;
  if (s >= nslots) return;
  const u64 k = pair_keys[s];
  if (k == kEmptyKey || pair_counts[s] < min_nodes) return;
  const u32 t = table_insert(seg_keys, mask, k & 0xffffffffull, flags);
  if (t != kBackground) atomicAdd(&qualified[t], 1ull);
}

__device__ __forceinline__ bool is_merger(const u64* seg_keys,
                                          const u64* qualified, u32 mask,
                                          u32 seg) {
  const u32 t = table_find(seg_keys, mask, (u64)seg);
  return t != kBackground && qualified[t] >= 2;
}

// sums: [class] edges, [FFN_EDGE_CLASSES + class] summed edge_len_q
__global__ __launch_bounds__(kThreads) void edge_classify_kernel(
    const int* __restrict__ edges, const u32* __restrict__ edge_len, u32 n_edges,
    const u32* __restrict__ node_seg, const u32* __restrict__ skel,
    const u64* __restrict__ seg_keys, const u64* __restrict__ qualified,
    u64* run_keys, u64* run_len, u32 mask, int* flags,
    uint8_t* __restrict__ edge_class, u64* sums) {
  __shared__ u64 ssum[2 * FFN_EDGE_CLASSES];
  if (threadIdx.x < 2 * FFN_EDGE_CLASSES) ssum[threadIdx.x] = 0;
  __syncthreads();
  const u32 e = blockIdx.x * kThreads + threadIdx.x;
  if (e < n_edges) {
    const int u = edges[2 * e], v = edges[2 * e + 1];
    const u32 su = node_seg[u], sv = node_seg[v];
    const u64 len = edge_len[e];
    int cls;
    if (su == 0 || sv == 0)
      cls = FFN_EDGE_OMITTED;
    else if (is_merger(seg_keys, qualified, mask, su) ||
             (sv != su && is_merger(seg_keys, qualified, mask, sv)))
      cls = FFN_EDGE_MERGED;
    else if (su != sv)
      cls = FFN_EDGE_SPLIT;
    else
      cls = FFN_EDGE_CORRECT;
    if (cls == FFN_EDGE_CORRECT) {
      const u32 t = table_insert(run_keys, mask,
                                 (u64)skel[u] | ((u64)su << 32), flags);
      if (t != kBackground) atomicAdd(&run_len[t], len);
    }
    edge_class[e] = (uint8_t)cls;
    atomicAdd(&ssum[cls], 1ull);
    atomicAdd(&ssum[FFN_EDGE_CLASSES + cls], len);
  }
  __syncthreads();
  if (threadIdx.x < 2 * FFN_EDGE_CLASSES && ssum[threadIdx.x])
    atomicAdd(&sums[threadIdx.x], ssum[threadIdx.x]);
}

__global__ __launch_bounds__(kThreads) void merger_compact_kernel(
    const u64* __restrict__ seg_keys, const u64* __restrict__ qualified,
    u32 nslots, u64* out, u32 cap, u32* n_out) {
  const u32 s = blockIdx.x * kThreads + threadIdx.x;
  if (s >= nslots) return;
  const u64 k = seg_keys[s];
  if (k == kEmptyKey || qualified[s] < 2) return;
  const u32 j = atomicAdd(n_out, 1u);
  if (j < cap) out[j] = k;
}

}  // namespace

struct ffn_metrics : ffn_unit::Unit {
  DevBuf gt, seg;              // uploads of host volumes
  DevBuf keys, payload;        // id tables and what their slots carry
  DevBuf out0, out1, out2;     // compacted tables on their way to the host
  DevBuf nodes, skel, node_seg, edges, edge_len, edge_class;
  DevBuf small;                // flags, counters, class sums
  u32 pair_slots = kFirstSlots;      // contingency table, kept between calls
  u32 skeleton_slots = kFirstSlots;  // the three skeleton tables
  double last_ms = 0.0, last_bytes = 0.0;
};

namespace {

// `small`: int flags[2] | u32 n_out[2] | u64 sums[2 * FFN_EDGE_CLASSES]
constexpr size_t kSmallBytes = 16 + 2 * FFN_EDGE_CLASSES * 8;

int stop_timer(ffn_metrics* h, double bytes) {
  U_OK(h->timer_stop(&h->last_ms));
  h->last_bytes = bytes;
  return FFN_OK;
}

// Shape and box checked; lo / hi = the box, *n = its voxels.
int parse_box(const int64_t shape[3], const int64_t* box_lo,
              const int64_t* box_hi, long long lo[3], long long hi[3],
              long long* n) {
  if (!shape) return ffn_set_error(FFN_ERR_ARG, "NULL shape");
  if ((box_lo == nullptr) != (box_hi == nullptr))
    return ffn_set_error(FFN_ERR_ARG, "box needs both lo and hi");
  *n = 1;
  for (int k = 0; k < 3; ++k) {
    if (shape[k] < 0 || shape[k] >= (1ll << 31))
      return ffn_set_error(FFN_ERR_ARG, "shape[%d] = %lld out of range", k,
                           (long long)shape[k]);
    lo[k] = box_lo ? box_lo[k] : 0;
    hi[k] = box_hi ? box_hi[k] : shape[k];
    if (lo[k] < 0 || hi[k] > shape[k] || lo[k] > hi[k])
      return ffn_set_error(FFN_ERR_ARG, "box outside the volume (axis %d)", k);
    *n *= hi[k] - lo[k];
  }
  return FFN_OK;
}

int check_volume(const void* p, int elem_bytes, const char* what) {
  if (!p) return ffn_set_error(FFN_ERR_ARG, "NULL %s volume", what);
  if (elem_bytes != 4 && elem_bytes != 8)
    return ffn_set_error(FFN_ERR_ARG, "%s elem_bytes must be 4 or 8", what);
  return FFN_OK;
}

// The volume on the device: the caller's pointer, or an upload into `buf`.
int stage(ffn_metrics* h, DevBuf& buf, const void* p, int on_device,
          size_t bytes, const void** dev) {
  if (on_device) {
    *dev = p;
    return FFN_OK;
  }
  U_OK(ensure(buf, bytes));
  U_TRY(hipMemcpyAsync(buf.p, p, bytes, hipMemcpyHostToDevice, h->stream));
  *dev = buf.p;
  return FFN_OK;
}

template <typename TA, typename TB>
void launch_contingency(ffn_metrics* h, const void* gt, const void* seg,
                        const BoxGeom& g, int ignore_gt_zero, u32 mask,
                        int* flags) {
  const int blocks = (int)std::min<long long>(
      kMaxBlocks, std::max<long long>(1, (g.n + kSpan - 1) / kSpan));
  hipLaunchKernelGGL((contingency_kernel<TA, TB>), dim3(blocks), dim3(kThreads),
                     0, h->stream, static_cast<const TA*>(gt),
                     static_cast<const TB*>(seg), g, ignore_gt_zero,
                     static_cast<u64*>(h->keys.p),
                     static_cast<u64*>(h->payload.p), mask, flags);
}

template <typename T>
void launch_gather(ffn_metrics* h, const void* seg, const NodeGeom& g, u32 n,
                   int* flags) {
  hipLaunchKernelGGL((node_gather_kernel<T>), dim3((n + kThreads - 1) / kThreads),
                     dim3(kThreads), 0, h->stream, static_cast<const T*>(seg), g,
                     static_cast<const int*>(h->nodes.p), n,
                     static_cast<u32*>(h->node_seg.p), flags);
}

}  // namespace

extern "C" {

int ffn_metrics_create(int device_id, ffn_metrics** out) {
  return ffn_unit::unit_create(device_id, out);
}

void ffn_metrics_destroy(ffn_metrics* h) { ffn_unit::unit_destroy(h); }

int ffn_metrics_contingency(ffn_metrics* h, const void* gt, int gt_elem_bytes,
                            int gt_on_device, const void* seg,
                            int seg_elem_bytes, int seg_on_device,
                            const int64_t shape_zyx[3], const int64_t box_lo[3],
                            const int64_t box_hi[3], int ignore_gt_zero,
                            size_t cap, uint64_t* pair_gt, uint64_t* pair_seg,
                            uint64_t* pair_count, size_t* n_pairs) {
  if (!h || !n_pairs || (cap && (!pair_gt || !pair_seg || !pair_count)))
    return ffn_set_error(FFN_ERR_ARG, "NULL argument");
  *n_pairs = 0;
  long long lo[3], hi[3], n = 0;
  U_OK(parse_box(shape_zyx, box_lo, box_hi, lo, hi, &n));
  U_TRY(hipSetDevice(h->device_id));
  h->last_ms = 0.0;
  h->last_bytes = 0.0;
  if (n == 0) return FFN_OK;
  U_OK(check_volume(gt, gt_elem_bytes, "ground-truth"));
  U_OK(check_volume(seg, seg_elem_bytes, "segmentation"));
  const size_t voxels =
      (size_t)shape_zyx[0] * (size_t)shape_zyx[1] * (size_t)shape_zyx[2];
  const void *gt_dev = nullptr, *seg_dev = nullptr;
  U_OK(stage(h, h->gt, gt, gt_on_device, voxels * gt_elem_bytes, &gt_dev));
  U_OK(stage(h, h->seg, seg, seg_on_device, voxels * seg_elem_bytes, &seg_dev));
  BoxGeom g;
  g.n = n;
  g.X = shape_zyx[2];
  g.YX = shape_zyx[1] * shape_zyx[2];
  g.origin = lo[0] * g.YX + lo[1] * g.X + lo[2];
  g.by = (u32)(hi[1] - lo[1]);
  g.bx = (u32)(hi[2] - lo[2]);
  U_OK(ensure(h->small, kSmallBytes));
  int* flags = static_cast<int*>(h->small.p);
  u32* n_out = reinterpret_cast<u32*>(h->small.p) + 2;
  int state[2];
  u32 nslots = h->pair_slots;
  U_OK(table_grow(h->stream, h->keys, 1, &nslots, kMaxSlots, flags, state,
                  [&](u32 mask) {
    U_OK(ensure(h->payload, (size_t)(mask + 1) * 8));
    U_TRY(hipMemsetAsync(h->payload.p, 0, (size_t)(mask + 1) * 8, h->stream));
    U_OK(h->timer_start());
    if (gt_elem_bytes == 4 && seg_elem_bytes == 4)
      launch_contingency<uint32_t, uint32_t>(h, gt_dev, seg_dev, g,
                                             ignore_gt_zero, mask, flags);
    else if (gt_elem_bytes == 4)
      launch_contingency<uint32_t, uint64_t>(h, gt_dev, seg_dev, g,
                                             ignore_gt_zero, mask, flags);
    else if (seg_elem_bytes == 4)
      launch_contingency<uint64_t, uint32_t>(h, gt_dev, seg_dev, g,
                                             ignore_gt_zero, mask, flags);
    else
      launch_contingency<uint64_t, uint64_t>(h, gt_dev, seg_dev, g,
                                             ignore_gt_zero, mask, flags);
    U_TRY(hipGetLastError());
    return stop_timer(h, (double)n * (gt_elem_bytes + seg_elem_bytes));
  }));
  h->pair_slots = nslots;
  if (state[1])
    return ffn_set_error(FFN_ERR_ARG,
                         "label id >= 2^32 - 1: remap ids before scoring");
  // compact the occupied slots into dense arrays (order unspecified)
  const size_t want = std::min<size_t>(cap, nslots);
  U_OK(ensure(h->out0, want * 8));
  U_OK(ensure(h->out1, want * 8));
  U_TRY(hipMemsetAsync(n_out, 0, sizeof(u32), h->stream));
  hipLaunchKernelGGL(table_compact_kernel<u64>, dim3((nslots + 255) / 256),
                     dim3(256), 0, h->stream,
                     static_cast<const u64*>(h->keys.p),
                     static_cast<const u64*>(h->payload.p), nslots,
                     static_cast<u64*>(h->out0.p), static_cast<u64*>(h->out1.p),
                     static_cast<u32*>(nullptr), (u32)want, n_out);
  U_TRY(hipGetLastError());
  u32 found = 0;
  U_TRY(hipMemcpyAsync(&found, n_out, sizeof(u32), hipMemcpyDeviceToHost,
                       h->stream));
  U_TRY(hipStreamSynchronize(h->stream));
  *n_pairs = found;
  if (found > cap)
    return ffn_set_error(FFN_ERR_ARG, "%u unique pairs exceed cap %zu", found,
                         cap);
  std::vector<u64> keys(found);
  if (found) {
    U_TRY(hipMemcpy(keys.data(), h->out0.p, (size_t)found * 8,
                    hipMemcpyDeviceToHost));
    U_TRY(hipMemcpy(pair_count, h->out1.p, (size_t)found * 8,
                    hipMemcpyDeviceToHost));
  }
  for (u32 k = 0; k < found; ++k) {
    pair_gt[k] = keys[k] & 0xffffffffull;
    pair_seg[k] = keys[k] >> 32;
  }
  return FFN_OK;
}

int ffn_metrics_skeleton(ffn_metrics* h, const void* seg, int seg_elem_bytes,
                         int seg_on_device, const int64_t shape_zyx[3],
                         const int64_t box_lo[3], const int64_t box_hi[3],
                         size_t n_nodes, const int32_t* nodes_zyx,
                         const uint32_t* node_skeleton, size_t n_edges,
                         const int32_t* edges, const uint32_t* edge_len_q,
                         uint64_t merge_min_nodes,
                         uint64_t class_count[FFN_EDGE_CLASSES],
                         uint64_t class_len[FFN_EDGE_CLASSES], size_t run_cap,
                         uint64_t* run_skeleton, uint64_t* run_segment,
                         uint64_t* run_len, size_t* n_runs, size_t merger_cap,
                         uint64_t* merger_ids, size_t* n_mergers,
                         uint32_t* node_seg, uint8_t* edge_class) {
  if (!h || !class_count || !class_len || !n_runs || !n_mergers ||
      (run_cap && (!run_skeleton || !run_segment || !run_len)) ||
      (merger_cap && !merger_ids) ||
      (n_nodes && (!nodes_zyx || !node_skeleton)) ||
      (n_edges && (!edges || !edge_len_q)))
    return ffn_set_error(FFN_ERR_ARG, "NULL argument");
  *n_runs = 0;
  *n_mergers = 0;
  for (int c = 0; c < FFN_EDGE_CLASSES; ++c) class_count[c] = class_len[c] = 0;
  if (merge_min_nodes < 1)
    return ffn_set_error(FFN_ERR_ARG, "merge_min_nodes must be >= 1");
  if (n_nodes >= (1u << 31) || n_edges >= (1u << 31))
    return ffn_set_error(FFN_ERR_ARG, "too many nodes or edges");
  long long lo[3], hi[3], n = 0;
  U_OK(parse_box(shape_zyx, box_lo, box_hi, lo, hi, &n));
  for (size_t k = 0; k < n_nodes; ++k)
    if (node_skeleton[k] == 0 || node_skeleton[k] == 0xffffffffu)
      return ffn_set_error(FFN_ERR_ARG, "node_skeleton[%zu] must be in [1, 2^32 - 2]", k);
  for (size_t e = 0; e < n_edges; ++e) {
    const int32_t u = edges[2 * e], v = edges[2 * e + 1];
    if (u < 0 || v < 0 || (size_t)u >= n_nodes || (size_t)v >= n_nodes)
      return ffn_set_error(FFN_ERR_ARG, "edge %zu: node index out of range", e);
    if (node_skeleton[u] != node_skeleton[v])
      return ffn_set_error(FFN_ERR_ARG, "edge %zu joins two skeletons", e);
  }
  U_TRY(hipSetDevice(h->device_id));
  h->last_ms = 0.0;
  h->last_bytes = 0.0;
  if (n_nodes == 0) return FFN_OK;
  const size_t voxels =
      (size_t)shape_zyx[0] * (size_t)shape_zyx[1] * (size_t)shape_zyx[2];
  const void* seg_dev = nullptr;
  if (n > 0) {  // (an empty box: every node lies outside it)
    U_OK(check_volume(seg, seg_elem_bytes, "segmentation"));
    U_OK(stage(h, h->seg, seg, seg_on_device, voxels * seg_elem_bytes,
               &seg_dev));
  }
  NodeGeom g;
  for (int k = 0; k < 3; ++k) {
    g.lo[k] = (int)lo[k];
    g.hi[k] = (int)hi[k];
  }
  g.X = shape_zyx[2];
  g.YX = shape_zyx[1] * shape_zyx[2];
  const size_t ne = std::max<size_t>(n_edges, 1);
  U_OK(ensure(h->nodes, n_nodes * 12));
  U_OK(ensure(h->skel, n_nodes * 4));
  U_OK(ensure(h->node_seg, n_nodes * 4));
  U_OK(ensure(h->edges, ne * 8));
  U_OK(ensure(h->edge_len, ne * 4));
  U_OK(ensure(h->edge_class, ne));
  U_OK(ensure(h->small, kSmallBytes));
  U_TRY(hipMemcpyAsync(h->nodes.p, nodes_zyx, n_nodes * 12,
                       hipMemcpyHostToDevice, h->stream));
  U_TRY(hipMemcpyAsync(h->skel.p, node_skeleton, n_nodes * 4,
                       hipMemcpyHostToDevice, h->stream));
  if (n_edges) {
    U_TRY(hipMemcpyAsync(h->edges.p, edges, n_edges * 8, hipMemcpyHostToDevice,
                         h->stream));
    U_TRY(hipMemcpyAsync(h->edge_len.p, edge_len_q, n_edges * 4,
                         hipMemcpyHostToDevice, h->stream));
  }
  int* flags = static_cast<int*>(h->small.p);
  u32* n_out = reinterpret_cast<u32*>(h->small.p) + 2;
  u64* sums = reinterpret_cast<u64*>(static_cast<char*>(h->small.p) + 16);
  const u32 nn = (u32)n_nodes, nedges = (u32)n_edges;
  const dim3 node_grid((nn + kThreads - 1) / kThreads);
  int state[2];
  u32 nslots = h->skeleton_slots;
  // three tables of one size in one array: (segment, skeleton) -> nodes,
  // segment -> qualified skeletons, (skeleton, segment) -> run length; the
  // second and third hold no more keys than the first
  U_OK(table_grow(h->stream, h->keys, 3, &nslots, kMaxSlots, flags, state,
                  [&](u32 mask) {
    const size_t slots = (size_t)mask + 1;
    U_OK(ensure(h->payload, 3 * slots * 8));
    U_TRY(hipMemsetAsync(h->payload.p, 0, 3 * slots * 8, h->stream));
    U_TRY(hipMemsetAsync(n_out, 0, kSmallBytes - 8, h->stream));
    u64* keys = static_cast<u64*>(h->keys.p);
    u64* pay = static_cast<u64*>(h->payload.p);
    U_OK(h->timer_start());
    if (n == 0)
      U_TRY(hipMemsetAsync(h->node_seg.p, 0, n_nodes * 4, h->stream));
    else if (seg_elem_bytes == 4)
      launch_gather<uint32_t>(h, seg_dev, g, nn, flags);
    else
      launch_gather<uint64_t>(h, seg_dev, g, nn, flags);
    hipLaunchKernelGGL(node_count_kernel, node_grid, dim3(kThreads), 0,
                       h->stream, static_cast<const u32*>(h->node_seg.p),
                       static_cast<const u32*>(h->skel.p), nn, keys, pay, mask,
                       flags);
    hipLaunchKernelGGL(merger_mark_kernel, dim3((slots + kThreads - 1) / kThreads),
                       dim3(kThreads), 0, h->stream, keys, pay, (u32)slots,
                       (u64)merge_min_nodes, keys + slots, pay + slots, mask,
                       flags);
    if (nedges)
      hipLaunchKernelGGL(edge_classify_kernel,
                         dim3((nedges + kThreads - 1) / kThreads), dim3(kThreads),
                         0, h->stream, static_cast<const int*>(h->edges.p),
                         static_cast<const u32*>(h->edge_len.p), nedges,
                         static_cast<const u32*>(h->node_seg.p),
                         static_cast<const u32*>(h->skel.p), keys + slots,
                         pay + slots, keys + 2 * slots, pay + 2 * slots, mask,
                         flags, static_cast<uint8_t*>(h->edge_class.p), sums);
    U_TRY(hipGetLastError());
    // a node: coordinates, skeleton id, one voxel, its segment written and
    // read back twice; an edge: two indices, a length, a class
    return stop_timer(h, (double)n_nodes * (12 + 4 + seg_elem_bytes + 12) +
                             (double)n_edges * (8 + 4 + 1));
  }));
  h->skeleton_slots = nslots;
  if (state[1])
    return ffn_set_error(FFN_ERR_ARG,
                         "label id >= 2^32 - 1: remap ids before scoring");
  const size_t slots = nslots;
  const u64* keys = static_cast<const u64*>(h->keys.p);
  const u64* pay = static_cast<const u64*>(h->payload.p);
  const size_t want_runs = std::min<size_t>(run_cap, slots);
  const size_t want_mergers = std::min<size_t>(merger_cap, slots);
  U_OK(ensure(h->out0, want_runs * 8));
  U_OK(ensure(h->out1, want_runs * 8));
  U_OK(ensure(h->out2, want_mergers * 8));
  const dim3 slot_grid((nslots + kThreads - 1) / kThreads);
  hipLaunchKernelGGL(table_compact_kernel<u64>, slot_grid, dim3(kThreads), 0,
                     h->stream, keys + 2 * slots, pay + 2 * slots, nslots,
                     static_cast<u64*>(h->out0.p), static_cast<u64*>(h->out1.p),
                     static_cast<u32*>(nullptr), (u32)want_runs, n_out);
  hipLaunchKernelGGL(merger_compact_kernel, slot_grid, dim3(kThreads), 0,
                     h->stream, keys + slots, pay + slots, nslots,
                     static_cast<u64*>(h->out2.p), (u32)want_mergers, n_out + 1);
  U_TRY(hipGetLastError());
  struct {
    u32 n_out[2];
    u64 sums[2 * FFN_EDGE_CLASSES];
  } host;
  U_TRY(hipMemcpyAsync(&host, n_out, sizeof(host), hipMemcpyDeviceToHost,
                       h->stream));
  U_TRY(hipStreamSynchronize(h->stream));
  *n_runs = host.n_out[0];
  *n_mergers = host.n_out[1];
  if (host.n_out[0] > run_cap || host.n_out[1] > merger_cap)
    return ffn_set_error(FFN_ERR_ARG,
                         "%u runs / %u mergers exceed caps %zu / %zu",
                         host.n_out[0], host.n_out[1], run_cap, merger_cap);
  for (int c = 0; c < FFN_EDGE_CLASSES; ++c) {
    class_count[c] = host.sums[c];
    class_len[c] = host.sums[FFN_EDGE_CLASSES + c];
  }
  std::vector<u64> run_keys(host.n_out[0]);
  if (host.n_out[0]) {
    U_TRY(hipMemcpy(run_keys.data(), h->out0.p, (size_t)host.n_out[0] * 8,
                    hipMemcpyDeviceToHost));
    U_TRY(hipMemcpy(run_len, h->out1.p, (size_t)host.n_out[0] * 8,
                    hipMemcpyDeviceToHost));
  }
  for (u32 k = 0; k < host.n_out[0]; ++k) {
    run_skeleton[k] = run_keys[k] & 0xffffffffull;
    run_segment[k] = run_keys[k] >> 32;
  }
  if (host.n_out[1])
    U_TRY(hipMemcpy(merger_ids, h->out2.p, (size_t)host.n_out[1] * 8,
                    hipMemcpyDeviceToHost));
  if (node_seg)
    U_TRY(hipMemcpy(node_seg, h->node_seg.p, n_nodes * 4,
                    hipMemcpyDeviceToHost));
  if (edge_class && n_edges)
    U_TRY(hipMemcpy(edge_class, h->edge_class.p, n_edges,
                    hipMemcpyDeviceToHost));
  return FFN_OK;
}

int ffn_metrics_last_timing(ffn_metrics* h, double* kernel_ms,
                            double* algorithmic_bytes) {
  if (!h) return ffn_set_error(FFN_ERR_ARG, "NULL handle");
  if (kernel_ms) *kernel_ms = h->last_ms;
  if (algorithmic_bytes) *algorithmic_bytes = h->last_bytes;
  return FFN_OK;
}

}  // extern "C"
