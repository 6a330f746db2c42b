// libffn_hip.so -- balanced training coordinates (include/ffn_coordinates.h).
//
// add_volume: a stable one-pass counting sort of a crop's flat indices by their
// 8-bit value.  The crop is cut into contiguous segments, one per WAVE (a
// workgroup of four waves owns four consecutive segments, i.e. one contiguous
// chunk).  class_hist_kernel counts every segment into 256 LDS bins (a run of
// equal values inside a wave is one LDS add of the run's length) and writes
// hist[bin][segment]; scan_rows_kernel turns every bin's row into exclusive
// prefix sums and its total; the host adds the 256 totals up to the class
// starts.  class_scatter_kernel walks the segments again: a lane's rank among
// the equal values of its wave is a popcount of the lanes below in the match
// mask (eight ballots over the key bits; one ballot where the whole wave holds
// one value, the common case in a partition map), the first lane of every
// distinct value reads and advances the wave's running offset in LDS, the
// others take it by a shuffle.  Segments, waves and lanes are all combined in
// index order, so the lists are ascending and no result depends on the order
// in which an atomic lands (the LDS adds of the histogram are integer sums
// nobody reads before a barrier).
//
// gather: one thread per output row; order -> (class, slot) -> perm -> the
// volume by a bounded binary search over the class's cumulative counts -> the
// flat index -> the centre.  serialize: one thread per record in three steps,
// record sizes, scan_rows_kernel over them, and the write pass with CRC32C
// from a 256-entry table each workgroup computes into LDS.
//
// Plain C++, ordinary stream-ordered launches, bounded loops only; every LDS
// index is a byte value or a wave / lane number, every global store is checked
// against the size of its buffer.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <memory>
#include <vector>

#include "../../include/ffn_coordinates.h"
#include "../../include/ffn_hip.h"
#include "ffn_internal.h"
#include "ffn_unit.h"

namespace {

typedef unsigned char u8;
typedef unsigned int u32;
typedef unsigned long long u64;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr u32 kMinSegment = 1024;  // voxels per wave, at least
constexpr u32 kMaxSegments = 4096;
constexpr int kScanItems = 8;  // consecutive entries per thread and tile
constexpr u32 kScanTile = kThreads * kScanItems;
constexpr u32 kIgnore = 255;

// ---- add_volume ------------------------------------------------------------------

struct SortGeom {
  u32 n;        // voxels, 1 .. 2^31 - 1
  u32 seg_len;  // voxels per segment, a multiple of 64
  u32 nseg;     // segments, 1 .. kMaxSegments
};

__global__ __launch_bounds__(kThreads) void class_hist_kernel(
    const u8* __restrict__ crop, SortGeom g, u32* __restrict__ hist) {
  __shared__ u32 s_bins[kWaves][256];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const u32 seg = blockIdx.x * kWaves + wave;
#pragma unroll
  for (int j = 0; j < 4; ++j) s_bins[wave][lane + 64 * j] = 0;
  __syncthreads();
  if (seg < g.nseg) {
    const u32 lo = seg * g.seg_len;
    const u32 hi = min(lo + g.seg_len, g.n);
    for (u32 base = lo; base < hi; base += 64) {
      const u32 i = base + lane;
      const bool valid = i < hi;
      const u32 key = valid ? (u32)crop[i] : 0u;
      const u32 left = __shfl_up(key, 1);
      const u64 leaders = __ballot(valid && (lane == 0 || left != key));
      const int nvalid = __popcll(__ballot(valid));
      if (valid && ((leaders >> lane) & 1)) {
        const u64 above = lane == 63 ? 0 : leaders & ~((2ull << lane) - 1);
        const int end = above ? __ffsll((long long)above) - 1 : nvalid;
        atomicAdd(&s_bins[wave][key], (u32)(end - lane));
      }
    }
  }
  __syncthreads();
  if (seg < g.nseg) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const u32 c = lane + 64 * j;
      hist[(size_t)c * g.nseg + seg] = s_bins[wave][c];
    }
  }
}

// One workgroup per row of `len` entries: exclusive prefix sums in place, the
// row's sum to totals[row].
__global__ __launch_bounds__(kThreads) void scan_rows_kernel(
    u32* data, u32 len, u32* __restrict__ totals) {
  __shared__ u32 s_wave[kWaves];
  u32* row = data + (size_t)blockIdx.x * len;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  u32 carry = 0;
  for (u32 base = 0; base < len; base += kScanTile) {
    const u32 first = base + threadIdx.x * kScanItems;
    u32 v[kScanItems];
    u32 sum = 0;
#pragma unroll
    for (int j = 0; j < kScanItems; ++j) {
      v[j] = first + j < len ? row[first + j] : 0u;
      sum += v[j];
    }
    u32 inc = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const u32 t = __shfl_up(inc, off);
      if (lane >= off) inc += t;
    }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    u32 run = carry + inc - sum;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      const u32 t = s_wave[w];
      if (w < wave) run += t;
      carry += t;
    }
#pragma unroll
    for (int j = 0; j < kScanItems; ++j) {
      if (first + j < len) row[first + j] = run;
      run += v[j];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

__global__ __launch_bounds__(kThreads) void class_scatter_kernel(
    const u8* __restrict__ crop, SortGeom g, const u32* __restrict__ hist,
    const u32* __restrict__ start, u32* __restrict__ out, u32 cap, int* err) {
  __shared__ u32 s_off[kWaves][256];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const u32 seg = blockIdx.x * kWaves + wave;
  if (seg < g.nseg) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const u32 c = lane + 64 * j;
      s_off[wave][c] = start[c] + hist[(size_t)c * g.nseg + seg];
    }
  }
  __syncthreads();
  if (seg >= g.nseg) return;
  // from here on a wave touches its own 256 offsets only, one LDS operation
  // after another in program order
  volatile u32* off = s_off[wave];
  const u32 lo = seg * g.seg_len;
  const u32 hi = min(lo + g.seg_len, g.n);
  const u64 lanes_below = (1ull << lane) - 1;
  for (u32 base = lo; base < hi; base += 64) {
    const u32 i = base + lane;
    const bool valid = i < hi;
    const u32 key = valid ? (u32)crop[i] : 0u;
    const u64 vmask = __ballot(valid);
    const u32 first = __builtin_amdgcn_readfirstlane(key);  // lane 0 is valid
    u64 mask = vmask;
    if (__ballot(valid && key != first) != 0) {  // wave-uniform
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        const u64 bits = __ballot(valid && ((key >> b) & 1));
        mask &= ((key >> b) & 1) ? bits : ~bits;
      }
    }
    const u64 below = mask & lanes_below;
    const u32 rank = (u32)__popcll(below);
    u32 at = 0;
    if (valid && below == 0) {  // the first lane of this value
      at = off[key];
      off[key] = at + (u32)__popcll(mask);
    }
    const int leader = mask ? __ffsll((long long)mask) - 1 : 0;
    at = __shfl(at, leader);
    if (valid && key != kIgnore) {
      const u32 pos = at + rank;
      if (pos < cap)
        out[pos] = i;
      else
        *err = 1;
    }
  }
}

// ---- gather ------------------------------------------------------------------------

struct GatherTabs {
  const u32* n_c;        // [K] members of the class over all volumes
  const u64* perm_off;   // [K] start of perm_c inside perms
  const u32* cum;        // [K][V + 1] members in the volumes before volume i
  const u32* vstart;     // [K][V] start of the class inside volume i's list
  const u32* const* vol_list;  // [V]
  const u32* vol_len;    // [V] entries of volume i's list
  const u32* vol_yx;     // [V] cy * cx
  const u32* vol_x;      // [V] cx
  u32 n_classes, n_volumes;
};

__global__ __launch_bounds__(kThreads) void gather_kernel(
    GatherTabs t, u32 max_count, const u32* __restrict__ perms, u64 perms_len,
    const u32* __restrict__ order, u32 n_rows, int mz, int my, int mx,
    int* __restrict__ centers, int* __restrict__ volume_index, int* err) {
  const u32 r = blockIdx.x * kThreads + threadIdx.x;
  if (r >= n_rows) return;
  int cx = 0, cy = 0, cz = 0, vol = 0;
  const u32 q = order[r];
  bool ok = q < n_rows;
  if (ok) {
    const u32 k = q / max_count;  // < n_classes: n_rows = n_classes * max_count
    const u32 slot = q - k * max_count;
    const u32 nk = t.n_c[k];  // >= 1
    const u64 at = t.perm_off[k] + slot % nk;
    const u32 j = at < perms_len ? perms[at] : nk;
    ok = j < nk;
    if (ok) {
      const u32* cum = t.cum + (size_t)k * (t.n_volumes + 1);
      u32 a = 0, b = t.n_volumes;  // cum[a] <= j < cum[b]
      for (int it = 0; it < 32 && b - a > 1; ++it) {
        const u32 mid = a + (b - a) / 2;
        if (cum[mid] <= j)
          a = mid;
        else
          b = mid;
      }
      const u32 e = t.vstart[(size_t)k * t.n_volumes + a] + (j - cum[a]);
      ok = e < t.vol_len[a];
      if (ok) {
        const u32 flat = t.vol_list[a][e];
        const u32 yx = t.vol_yx[a], nx = t.vol_x[a];
        const u32 z = flat / yx, rem = flat - z * yx;
        const u32 y = rem / nx;
        cx = mx + (int)(rem - y * nx);
        cy = my + (int)y;
        cz = mz + (int)z;
        vol = (int)a;
      }
    }
  }
  if (!ok) *err = 1;
  centers[(size_t)r * 3] = cx;
  centers[(size_t)r * 3 + 1] = cy;
  centers[(size_t)r * 3 + 2] = cz;
  volume_index[r] = vol;
}

// ---- serialize --------------------------------------------------------------------

__host__ __device__ inline u32 varint_len(u64 v) {
  u32 n = 1;
  while (v >= 128 && n < 10) {
    v >>= 7;
    ++n;
  }
  return n;
}

// Lengths of the nested messages of one Example, inside out.
struct ExampleSizes {
  u32 ints;      // the packed varints of the centre
  u32 int_list;  // Int64List{1: ints}
  u32 feat_c;    // Feature{3: int_list}
  u32 entry_c;   // entry{1: "center", 2: feat_c}
  u32 byte_list;  // BytesList{1: name}
  u32 feat_n;     // Feature{1: byte_list}
  u32 entry_n;    // entry{1: "label_volume_name", 2: feat_n}
  u32 features;   // Features{1: entry_c, 1: entry_n}
  u32 example;    // Example{1: features}
};

constexpr u32 kKeyCenter = 6, kKeyName = 17;

__host__ __device__ inline ExampleSizes example_sizes(u64 x, u64 y, u64 z,
                                                      u32 name_len) {
  ExampleSizes s;
  s.ints = varint_len(x) + varint_len(y) + varint_len(z);
  s.int_list = 1 + varint_len(s.ints) + s.ints;
  s.feat_c = 1 + varint_len(s.int_list) + s.int_list;
  s.entry_c = 2 + kKeyCenter + 1 + varint_len(s.feat_c) + s.feat_c;
  s.byte_list = 1 + varint_len(name_len) + name_len;
  s.feat_n = 1 + varint_len(s.byte_list) + s.byte_list;
  s.entry_n = 2 + kKeyName + 1 + varint_len(s.feat_n) + s.feat_n;
  s.features = 1 + varint_len(s.entry_c) + s.entry_c + 1 +
               varint_len(s.entry_n) + s.entry_n;
  s.example = 1 + varint_len(s.features) + s.features;
  return s;
}

// int64 on the wire: negative values are ten-byte varints
__host__ __device__ inline u64 wire(int v) { return (u64)(long long)v; }

struct RecordArgs {
  const int* centers;
  const int* volume_index;
  const u8* name_bytes;
  const u32* name_off;  // [n_names + 1]
  u32 n_names;
  u32 row0, n_rows;
};

__global__ __launch_bounds__(kThreads) void record_size_kernel(
    RecordArgs a, u32* __restrict__ sizes, int* err) {
  const u32 r = blockIdx.x * kThreads + threadIdx.x;
  if (r >= a.n_rows) return;
  const size_t row = (size_t)a.row0 + r;
  const u32 vol = (u32)a.volume_index[row];
  u32 name_len = 0;
  if (vol < a.n_names)
    name_len = a.name_off[vol + 1] - a.name_off[vol];
  else
    *err = 1;
  const ExampleSizes s = example_sizes(
      wire(a.centers[row * 3]), wire(a.centers[row * 3 + 1]),
      wire(a.centers[row * 3 + 2]), name_len);
  sizes[r] = 16 + s.example;
}

__device__ __forceinline__ u32 masked_crc(u32 crc) {
  crc = ~crc;
  return ((crc >> 15) | (crc << 17)) + 0xa282ead8u;
}

struct Emit {
  u8* p;
  u32 crc;
  const u32* tab;

  __device__ __forceinline__ void byte(u32 b) {
    *p++ = (u8)b;
    crc = tab[(crc ^ b) & 0xff] ^ (crc >> 8);
  }
  __device__ __forceinline__ void varint(u64 v) {
    for (int k = 0; k < 10; ++k) {
      const u32 b = (u32)(v & 0x7f);
      v >>= 7;
      if (v && k < 9) {
        byte(b | 0x80);
      } else {
        byte(b);
        break;
      }
    }
  }
  __device__ __forceinline__ void raw32(u32 v) {
#pragma unroll
    for (int k = 0; k < 4; ++k) *p++ = (u8)(v >> (8 * k));
  }
};

__global__ __launch_bounds__(kThreads) void record_write_kernel(
    RecordArgs a, const u32* __restrict__ offsets, u32 total,
    u8* __restrict__ out, int* err) {
  __shared__ u32 s_crc[256];
  {
    u32 c = threadIdx.x;
#pragma unroll
    for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ 0x82f63b78u : c >> 1;
    s_crc[threadIdx.x] = c;
  }
  __syncthreads();
  const u32 r = blockIdx.x * kThreads + threadIdx.x;
  if (r >= a.n_rows) return;
  const size_t row = (size_t)a.row0 + r;
  const u32 vol = (u32)a.volume_index[row];
  if (vol >= a.n_names) {
    *err = 1;
    return;
  }
  const u32 name_lo = a.name_off[vol];
  const u32 name_len = a.name_off[vol + 1] - name_lo;
  const u64 c[3] = {wire(a.centers[row * 3]), wire(a.centers[row * 3 + 1]),
                    wire(a.centers[row * 3 + 2])};
  const ExampleSizes s = example_sizes(c[0], c[1], c[2], name_len);
  const u32 pos = offsets[r];
  if (pos > total || 16 + s.example > total - pos) {
    *err = 1;
    return;
  }
  Emit e{out + pos, 0xffffffffu, s_crc};
  u64 len = s.example;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    e.byte((u32)(len & 0xff));
    len >>= 8;
  }
  e.raw32(masked_crc(e.crc));
  e.crc = 0xffffffffu;
  e.byte(0x0a);  // Example.features
  e.varint(s.features);
  e.byte(0x0a);  // Features.feature entry
  e.varint(s.entry_c);
  e.byte(0x0a);  // key
  e.byte(kKeyCenter);
  const char key_c[] = "center";
  for (u32 k = 0; k < kKeyCenter; ++k) e.byte((u8)key_c[k]);
  e.byte(0x12);  // value
  e.varint(s.feat_c);
  e.byte(0x1a);  // Feature.int64_list
  e.varint(s.int_list);
  e.byte(0x0a);  // Int64List.value, packed
  e.varint(s.ints);
  for (int k = 0; k < 3; ++k) e.varint(c[k]);
  e.byte(0x0a);  // Features.feature entry
  e.varint(s.entry_n);
  e.byte(0x0a);  // key
  e.byte(kKeyName);
  const char key_n[] = "label_volume_name";
  for (u32 k = 0; k < kKeyName; ++k) e.byte((u8)key_n[k]);
  e.byte(0x12);  // value
  e.varint(s.feat_n);
  e.byte(0x0a);  // Feature.bytes_list
  e.varint(s.byte_list);
  e.byte(0x0a);  // BytesList.value
  e.varint(name_len);
  for (u32 k = 0; k < name_len; ++k) e.byte(a.name_bytes[name_lo + k]);
  e.raw32(masked_crc(e.crc));
}

using ffn_unit::DevBuf;
using ffn_unit::ensure;

struct Volume {
  DevBuf list;          // the classes other than 255, one after another
  u32 list_len = 0;
  u32 shape[3] = {0, 0, 0};
  u32 count[256];       // voxels per value
  u32 start[256];       // start of the class inside `list`
};

}  // namespace

struct ffn_coordinates : ffn_unit::Unit {
  std::vector<std::unique_ptr<Volume>> volumes;
  DevBuf crop, hist, small, start;
  DevBuf perms, order, tab32, tab64, centers, volume_index;
  DevBuf name_bytes, name_off, sizes, records;
  size_t n_rows = 0, n_names = 0;
  u32 longest_name = 0;
  bool have_rows = false;
  double ms[3] = {0.0, 0.0, 0.0}, bytes[3] = {0.0, 0.0, 0.0};
};

namespace {

// Returns with the copy complete: `src` is pageable memory of the caller's, or
// a local table, and an early return of the call must not leave the stream
// reading it.  In stream order, so that it follows whatever an earlier call
// that failed left queued.
int upload(ffn_coordinates* h, DevBuf& buf, const void* src, size_t bytes) {
  U_OK(ensure(buf, bytes));
  if (bytes) {
    U_TRY(hipMemcpyAsync(buf.p, src, bytes, hipMemcpyHostToDevice, h->stream));
    U_TRY(hipStreamSynchronize(h->stream));
  }
  return FFN_OK;
}

// The error word (index 0) and the totals of the scans (from index 1) live in
// `small`.
constexpr size_t kSmallBytes = (1 + 256) * sizeof(u32);

int read_small(ffn_coordinates* h, u32* dst, size_t words) {
  U_TRY(hipMemcpyAsync(dst, h->small.p, words * sizeof(u32),
                       hipMemcpyDeviceToHost, h->stream));
  U_TRY(hipStreamSynchronize(h->stream));
  return FFN_OK;
}

}  // namespace

extern "C" {

int ffn_coordinates_create(int device_id, ffn_coordinates** out) {
  return ffn_unit::unit_create(device_id, out);
}

void ffn_coordinates_destroy(ffn_coordinates* h) { ffn_unit::unit_destroy(h); }

int ffn_coordinates_reset(ffn_coordinates* h) {
  if (!h) return ffn_set_error(FFN_ERR_ARG, "NULL argument");
  U_TRY(hipSetDevice(h->device_id));
  U_TRY(hipStreamSynchronize(h->stream));
  h->volumes.clear();
  h->have_rows = false;
  h->n_rows = h->n_names = 0;
  return FFN_OK;
}

int ffn_coordinates_add_volume(ffn_coordinates* h, const uint8_t* crop,
                               const int64_t shape_zyx[3],
                               uint64_t counts[256]) {
  if (!h || !crop || !shape_zyx || !counts)
    return ffn_set_error(FFN_ERR_ARG, "NULL argument");
  double voxels = 1.0;
  for (int k = 0; k < 3; ++k) {
    if (shape_zyx[k] < 1)
      return ffn_set_error(FFN_ERR_ARG, "shape[%d] = %lld", k,
                           (long long)shape_zyx[k]);
    voxels *= (double)shape_zyx[k];
  }
  if (voxels >= 2147483648.0)
    return ffn_set_error(FFN_ERR_ARG, "crop of 2^31 voxels or more");
  U_TRY(hipSetDevice(h->device_id));
  h->have_rows = false;
  SortGeom g;
  g.n = (u32)(shape_zyx[0] * shape_zyx[1] * shape_zyx[2]);
  const u32 per_seg = (g.n + kMaxSegments - 1) / kMaxSegments;
  g.seg_len = std::max(kMinSegment, (per_seg + 63) / 64 * 64);
  g.nseg = (g.n + g.seg_len - 1) / g.seg_len;
  const unsigned blocks = (g.nseg + kWaves - 1) / kWaves;

  U_OK(upload(h, h->crop, crop, g.n));
  U_OK(ensure(h->hist, (size_t)256 * g.nseg * sizeof(u32)));
  U_OK(ensure(h->small, kSmallBytes));
  U_OK(ensure(h->start, 256 * sizeof(u32)));
  U_TRY(hipMemsetAsync(h->small.p, 0, kSmallBytes, h->stream));
  int* err = static_cast<int*>(h->small.p);
  u32* totals = static_cast<u32*>(h->small.p) + 1;
  double ms_count = 0.0, ms_scatter = 0.0;
  U_OK(h->timer_start());
  hipLaunchKernelGGL(class_hist_kernel, dim3(blocks), dim3(kThreads), 0,
                     h->stream, static_cast<const u8*>(h->crop.p), g,
                     static_cast<u32*>(h->hist.p));
  hipLaunchKernelGGL(scan_rows_kernel, dim3(256), dim3(kThreads), 0, h->stream,
                     static_cast<u32*>(h->hist.p), g.nseg, totals);
  U_TRY(hipGetLastError());
  U_OK(h->timer_stop(&ms_count));
  u32 word[1 + 256];
  U_OK(read_small(h, word, 1 + 256));

  std::unique_ptr<Volume> vol(new Volume());
  u64 sum = 0;
  for (int c = 0; c < 256; ++c) {
    vol->count[c] = word[1 + c];
    vol->start[c] = (u32)sum;
    sum += word[1 + c];
  }
  if (sum != g.n)
    return ffn_set_error(FFN_ERR_HIP, "class counts add up to %llu of %u voxels",
                         sum, g.n);
  vol->list_len = vol->start[kIgnore];
  for (int k = 0; k < 3; ++k) vol->shape[k] = (u32)shape_zyx[k];
  U_OK(ensure(vol->list, (size_t)vol->list_len * sizeof(u32)));
  U_OK(upload(h, h->start, vol->start, 256 * sizeof(u32)));
  U_OK(h->timer_start());
  hipLaunchKernelGGL(class_scatter_kernel, dim3(blocks), dim3(kThreads), 0,
                     h->stream, static_cast<const u8*>(h->crop.p), g,
                     static_cast<const u32*>(h->hist.p),
                     static_cast<const u32*>(h->start.p),
                     static_cast<u32*>(vol->list.p), vol->list_len, err);
  U_TRY(hipGetLastError());
  U_OK(h->timer_stop(&ms_scatter));
  U_OK(read_small(h, word, 1));
  if (word[0])
    return ffn_set_error(FFN_ERR_HIP, "counting sort left its list");
  h->ms[0] = ms_count + ms_scatter;
  h->bytes[0] = 2.0 * g.n + 4.0 * vol->list_len;
  for (int c = 0; c < 256; ++c) counts[c] = vol->count[c];
  h->volumes.push_back(std::move(vol));
  return FFN_OK;
}

int ffn_coordinates_read_class(ffn_coordinates* h, size_t volume, int cls,
                               size_t cap, uint32_t* flat, size_t* n) {
  if (!h || !n || (cap && !flat))
    return ffn_set_error(FFN_ERR_ARG, "NULL argument");
  *n = 0;
  if (volume >= h->volumes.size() || cls < 0 || cls >= (int)kIgnore)
    return ffn_set_error(FFN_ERR_ARG, "no class %d of volume %zu", cls, volume);
  const Volume& v = *h->volumes[volume];
  *n = v.count[cls];
  if (*n > cap)
    return ffn_set_error(FFN_ERR_ARG, "%zu entries exceed cap %zu", *n, cap);
  if (*n == 0) return FFN_OK;
  U_TRY(hipSetDevice(h->device_id));
  U_TRY(hipMemcpy(flat, static_cast<const u32*>(v.list.p) + v.start[cls],
                  *n * sizeof(u32), hipMemcpyDeviceToHost));
  return FFN_OK;
}

int ffn_coordinates_gather(ffn_coordinates* h, const uint8_t* classes,
                           size_t n_classes, uint64_t max_count,
                           const uint32_t* perms, size_t perms_len,
                           const uint32_t* order, size_t n_rows,
                           const int32_t margin_zyx[3]) {
  if (!h || !classes || !perms || !order || !margin_zyx)
    return ffn_set_error(FFN_ERR_ARG, "NULL argument");
  h->have_rows = false;  // whatever comes of this call, the old rows are gone
  const size_t nv = h->volumes.size();
  if (nv == 0 || nv > 0x7fffffffu)
    return ffn_set_error(FFN_ERR_STATE,
                         "no volume resident: call ffn_coordinates_add_volume");
  if (n_classes < 1 || n_classes > kIgnore || max_count < 1 ||
      max_count >= (1ull << 31) || n_classes * max_count >= (1ull << 31) ||
      n_rows != n_classes * max_count)
    return ffn_set_error(FFN_ERR_ARG,
                         "%zu classes x max_count %llu: need 1 .. 2^31 - 1 rows "
                         "and n_rows (%zu) equal to them", n_classes,
                         (unsigned long long)max_count, n_rows);
  for (int k = 0; k < 3; ++k)
    if (margin_zyx[k] < 0)
      return ffn_set_error(FFN_ERR_ARG, "margin[%d] = %d", k, margin_zyx[k]);
  // tables: n_c [K] | cum [K][V + 1] | vstart [K][V] | vol_len, vol_yx, vol_x [V]
  const size_t K = n_classes;
  std::vector<u32> t32(K + K * (nv + 1) + K * nv + 3 * nv);
  std::vector<u64> t64(K + nv);  // perm_off [K] | vol_list [V]
  u32* n_c = t32.data();
  u32* cum = n_c + K;
  u32* vstart = cum + K * (nv + 1);
  u32* vol_len = vstart + K * nv;
  u32* vol_yx = vol_len + nv;
  u32* vol_x = vol_yx + nv;
  bool seen[256] = {false};
  u64 perm_total = 0;
  for (size_t k = 0; k < K; ++k) {
    const u32 c = classes[k];
    if (c >= kIgnore || seen[c])
      return ffn_set_error(FFN_ERR_ARG, "class %u is 255 or listed twice", c);
    seen[c] = true;
    u64 members = 0;
    for (size_t i = 0; i < nv; ++i) {
      cum[k * (nv + 1) + i] = (u32)members;
      vstart[k * nv + i] = h->volumes[i]->start[c];
      members += h->volumes[i]->count[c];
      if (members >= (1ull << 31))
        return ffn_set_error(FFN_ERR_ARG, "class %u has 2^31 voxels or more", c);
    }
    cum[k * (nv + 1) + nv] = (u32)members;
    if (members == 0)
      return ffn_set_error(FFN_ERR_ARG, "class %u is in no volume", c);
    n_c[k] = (u32)members;
    t64[k] = perm_total;
    perm_total += members;
  }
  if (perm_total != perms_len)
    return ffn_set_error(FFN_ERR_ARG, "perms of %zu entries, expected %llu",
                         perms_len, (unsigned long long)perm_total);
  for (size_t i = 0; i < nv; ++i) {
    const Volume& v = *h->volumes[i];
    t64[K + i] = (u64) reinterpret_cast<uintptr_t>(v.list.p);
    vol_len[i] = v.list_len;
    vol_yx[i] = v.shape[1] * v.shape[2];
    vol_x[i] = v.shape[2];
    for (int k = 0; k < 3; ++k)  // centres are int32
      if ((u64)v.shape[k] + (u64)margin_zyx[k] > 0x7fffffffull)
        return ffn_set_error(FFN_ERR_ARG, "margin[%d] = %d leaves int32", k,
                             margin_zyx[k]);
  }
  U_TRY(hipSetDevice(h->device_id));
  U_OK(upload(h, h->tab32, t32.data(), t32.size() * sizeof(u32)));
  U_OK(upload(h, h->tab64, t64.data(), t64.size() * sizeof(u64)));
  U_OK(upload(h, h->perms, perms, perms_len * sizeof(u32)));
  U_OK(upload(h, h->order, order, n_rows * sizeof(u32)));
  U_OK(ensure(h->centers, n_rows * 3 * sizeof(int)));
  U_OK(ensure(h->volume_index, n_rows * sizeof(int)));
  U_OK(ensure(h->small, kSmallBytes));
  U_TRY(hipMemsetAsync(h->small.p, 0, kSmallBytes, h->stream));
  GatherTabs t;
  const u32* d32 = static_cast<const u32*>(h->tab32.p);
  const u64* d64 = static_cast<const u64*>(h->tab64.p);
  t.n_c = d32;
  t.cum = d32 + K;
  t.vstart = t.cum + K * (nv + 1);
  t.vol_len = t.vstart + K * nv;
  t.vol_yx = t.vol_len + nv;
  t.vol_x = t.vol_yx + nv;
  t.perm_off = d64;
  t.vol_list = reinterpret_cast<const u32* const*>(d64 + K);
  t.n_classes = (u32)K;
  t.n_volumes = (u32)nv;
  U_OK(h->timer_start());
  hipLaunchKernelGGL(gather_kernel,
                     dim3((unsigned)((n_rows + kThreads - 1) / kThreads)),
                     dim3(kThreads), 0, h->stream, t, (u32)max_count,
                     static_cast<const u32*>(h->perms.p), (u64)perms_len,
                     static_cast<const u32*>(h->order.p), (u32)n_rows,
                     (int)margin_zyx[0], (int)margin_zyx[1], (int)margin_zyx[2],
                     static_cast<int*>(h->centers.p),
                     static_cast<int*>(h->volume_index.p),
                     static_cast<int*>(h->small.p));
  U_TRY(hipGetLastError());
  U_OK(h->timer_stop(&h->ms[1]));
  u32 err = 0;
  U_OK(read_small(h, &err, 1));
  if (err)
    return ffn_set_error(FFN_ERR_ARG,
                         "an entry of order or perms is out of its range");
  h->bytes[1] = (double)n_rows * (4 + 4 + 4 + 16);
  h->n_rows = n_rows;
  h->have_rows = true;
  return FFN_OK;
}

int ffn_coordinates_read(ffn_coordinates* h, size_t row0, size_t n_rows,
                         int32_t* centers_xyz, int32_t* volume_index) {
  if (!h) return ffn_set_error(FFN_ERR_ARG, "NULL argument");
  if (!h->have_rows)
    return ffn_set_error(FFN_ERR_STATE,
                         "no rows resident: call ffn_coordinates_gather");
  if (row0 > h->n_rows || n_rows > h->n_rows - row0)
    return ffn_set_error(FFN_ERR_ARG, "rows %zu + %zu of %zu", row0, n_rows,
                         h->n_rows);
  if (n_rows == 0) return FFN_OK;
  U_TRY(hipSetDevice(h->device_id));
  if (centers_xyz)
    U_TRY(hipMemcpy(centers_xyz, static_cast<const int*>(h->centers.p) + row0 * 3,
                    n_rows * 3 * sizeof(int), hipMemcpyDeviceToHost));
  if (volume_index)
    U_TRY(hipMemcpy(volume_index,
                    static_cast<const int*>(h->volume_index.p) + row0,
                    n_rows * sizeof(int), hipMemcpyDeviceToHost));
  return FFN_OK;
}

int ffn_coordinates_set_names(ffn_coordinates* h, const uint8_t* bytes,
                              const uint32_t* offsets, size_t n_names) {
  if (!h || !bytes || !offsets)
    return ffn_set_error(FFN_ERR_ARG, "NULL argument");
  if (n_names < 1 || n_names > 0x7fffffffu || offsets[0] != 0)
    return ffn_set_error(FFN_ERR_ARG, "need names, offsets starting at 0");
  u32 longest = 0;
  for (size_t i = 0; i < n_names; ++i) {
    if (offsets[i + 1] <= offsets[i])
      return ffn_set_error(FFN_ERR_ARG, "name %zu is empty", i);
    longest = std::max(longest, offsets[i + 1] - offsets[i]);
  }
  U_TRY(hipSetDevice(h->device_id));
  h->n_names = 0;
  U_OK(upload(h, h->name_bytes, bytes, offsets[n_names]));
  U_OK(upload(h, h->name_off, offsets, (n_names + 1) * sizeof(u32)));
  h->n_names = n_names;
  h->longest_name = longest;
  return FFN_OK;
}

int ffn_coordinates_serialize(ffn_coordinates* h, size_t row0, size_t n_rows,
                              size_t cap, uint8_t* out, size_t* n_bytes) {
  if (!h || !n_bytes || (cap && !out))
    return ffn_set_error(FFN_ERR_ARG, "NULL argument");
  *n_bytes = 0;
  if (!h->have_rows)
    return ffn_set_error(FFN_ERR_STATE,
                         "no rows resident: call ffn_coordinates_gather");
  if (h->n_names < h->volumes.size())
    return ffn_set_error(FFN_ERR_STATE, "%zu names for %zu volumes: call "
                         "ffn_coordinates_set_names", h->n_names,
                         h->volumes.size());
  if (row0 > h->n_rows || n_rows > h->n_rows - row0)
    return ffn_set_error(FFN_ERR_ARG, "rows %zu + %zu of %zu", row0, n_rows,
                         h->n_rows);
  if (n_rows == 0) return FFN_OK;
  const u64 longest =
      16 + (u64)example_sizes(~0ull, ~0ull, ~0ull, h->longest_name).example;
  if ((u64)n_rows * longest >= (1ull << 32))
    return ffn_set_error(FFN_ERR_ARG, "a window of %zu rows of up to %llu "
                         "bytes each reaches 2^32 bytes", n_rows,
                         (unsigned long long)longest);
  U_TRY(hipSetDevice(h->device_id));
  U_OK(ensure(h->sizes, n_rows * sizeof(u32)));
  U_OK(ensure(h->small, kSmallBytes));
  U_TRY(hipMemsetAsync(h->small.p, 0, kSmallBytes, h->stream));
  int* err = static_cast<int*>(h->small.p);
  u32* totals = static_cast<u32*>(h->small.p) + 1;
  RecordArgs a;
  a.centers = static_cast<const int*>(h->centers.p);
  a.volume_index = static_cast<const int*>(h->volume_index.p);
  a.name_bytes = static_cast<const u8*>(h->name_bytes.p);
  a.name_off = static_cast<const u32*>(h->name_off.p);
  a.n_names = (u32)h->n_names;
  a.row0 = (u32)row0;
  a.n_rows = (u32)n_rows;
  const unsigned blocks = (unsigned)((n_rows + kThreads - 1) / kThreads);
  double ms_size = 0.0, ms_write = 0.0;
  U_OK(h->timer_start());
  hipLaunchKernelGGL(record_size_kernel, dim3(blocks), dim3(kThreads), 0,
                     h->stream, a, static_cast<u32*>(h->sizes.p), err);
  hipLaunchKernelGGL(scan_rows_kernel, dim3(1), dim3(kThreads), 0, h->stream,
                     static_cast<u32*>(h->sizes.p), (u32)n_rows, totals);
  U_TRY(hipGetLastError());
  U_OK(h->timer_stop(&ms_size));
  u32 word[2];
  U_OK(read_small(h, word, 2));
  if (word[0])
    return ffn_set_error(FFN_ERR_STATE, "a row names a volume without a name");
  const size_t total = word[1];
  *n_bytes = total;
  if (total > cap)
    return ffn_set_error(FFN_ERR_ARG, "%zu bytes exceed cap %zu", total, cap);
  U_OK(ensure(h->records, total));
  U_OK(h->timer_start());
  hipLaunchKernelGGL(record_write_kernel, dim3(blocks), dim3(kThreads), 0,
                     h->stream, a, static_cast<const u32*>(h->sizes.p),
                     (u32)total, static_cast<u8*>(h->records.p), err);
  U_TRY(hipGetLastError());
  U_OK(h->timer_stop(&ms_write));
  U_OK(read_small(h, word, 1));
  if (word[0])
    return ffn_set_error(FFN_ERR_HIP, "a record left its window");
  U_TRY(hipMemcpy(out, h->records.p, total, hipMemcpyDeviceToHost));
  h->ms[2] = ms_size + ms_write;
  h->bytes[2] = 16.0 * (double)n_rows + (double)total;
  return FFN_OK;
}

int ffn_coordinates_last_timing(ffn_coordinates* h, double kernel_ms[3],
                                double algorithmic_bytes[3]) {
  if (!h || !kernel_ms || !algorithmic_bytes)
    return ffn_set_error(FFN_ERR_ARG, "NULL argument");
  for (int k = 0; k < 3; ++k) {
    kernel_ms[k] = h->ms[k];
    algorithmic_bytes[k] = h->bytes[k];
  }
  return FFN_OK;
}

}  // extern "C"
