// libffn_hip.so -- forward-only evaluation on training examples
// (include/ffn_evaluation.h).
//
// Streaming kernels over a few hundred KB per slot.  A slot is three dense f32
// arrays (seed canvas, image patch, label patch).  load / gather / paste give
// one wave a row along x at a time (lanes stride x: coalesced), rows spread
// over the workgroups of grid.x and the entries of the call over grid.y.
// probe_moves is one thread per pair.  score_faces is one workgroup per (entry,
// face): every thread scans its share of the face in C order, lanes combine by
// shuffles, waves through LDS, always keeping the smaller index among equal
// values.  finish runs at most kFinishBlocks workgroups: per-thread sums in
// index order, a shuffle tree per wave, an LDS tree per workgroup, and a
// second one-workgroup launch combines the workgroups' partials the same way,
// so the f32 sum does not depend on timing.  load_augmented keeps load's rows
// while x stays x; where x changes places with y or z it moves 64 x 64 tiles
// through LDS (row stride 65) so that lanes run along the volume's x on the
// read and along the slot's x on the write.  load_sections runs one workgroup
// per (entry, image section) that carries the section's plan out (a blurred
// section through two LDS planes) into scratch, then that transposing copy.
//
// The host validates every box against the geometry before a launch; the
// kernels take the validated starts.  The per-call descriptors go through a
// pinned staging buffer.  Plain C++, ordinary stream-ordered launches, bounded
// loops only.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/ffn_evaluation.h"
#include "../../include/ffn_hip.h"
#include "ffn_internal.h"
#include "ffn_unit.h"

namespace {

typedef unsigned char u8;
typedef unsigned int u32;
typedef unsigned long long u64;

using ffn_unit::DevBuf;
using ffn_unit::PinnedBuf;
using ffn_unit::ensure;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxSlots = FFN_EVALUATION_MAX_SLOTS;
constexpr int kRowBlocks = 256;     // grid.x of the row kernels, at most
constexpr int kFinishBlocks = 256;  // == kThreads: one partial per thread
constexpr int kFinishItems = 8;     // voxels per thread and round

struct Dims {
  int z, y, x;
  __host__ __device__ size_t voxels() const { return (size_t)z * y * x; }
};

struct Volume {
  DevBuf image, labels;
  int image_elem = 0, label_elem = 0;
  long long shape[3] = {0, 0, 0};
};

// One entry of a load: validated starts of the two patches inside the volume.
struct LoadItem {
  const void* image;
  const void* labels;
  long long sy, sx;  // volume strides of z and y, in voxels (x is 1)
  int image_elem, label_elem;
  int slot;
  int img0[3], lab0[3];
  float offset, scale;
};

// One entry of gather / paste / score_faces / probe: validated starts (zyx).
struct BoxItem {
  int slot;
  int a0[3];  // in the seed canvas
  int b0[3];  // in the image patch (gather) / label patch (probe)
};

// One entry of a load_augmented: the load, and the transform in the form the
// kernel branches on.  x_moves = 0: x stays x (perm[2] == 2); `swap` says
// whether z and y change places; ra / rb / rx are the reflections of output z,
// y, x.  x_moves = 1: output axis a2 (0 or 1) takes the volume's x, the
// slot's x comes from volume axis p2 (0 or 1), the third output axis b = 1 -
// a2 from volume axis 1 - p2; ra / rb / rx reflect output a2, b, x.
struct AugItem {
  LoadItem load;
  int x_moves;
  int a2, p2, swap;
  int ra, rb, rx;
};

// One entry of gather_train: BoxItem and the start in the label patch.
struct TrainBoxItem {
  int slot;
  int a0[3];  // in the seed canvas
  int b0[3];  // in the image patch
  int c0[3];  // in the label patch
};

struct SlotArrays {
  float* seed;
  float* image;
  float* labels;
  Dims canvas, image_patch, label_patch;
  __device__ float* seed_of(int s) const { return seed + s * canvas.voxels(); }
  __device__ float* image_of(int s) const {
    return image + s * image_patch.voxels();
  }
  __device__ float* labels_of(int s) const {
    return labels + s * label_patch.voxels();
  }
};

__device__ __forceinline__ u64 label_at(const void* labels, int elem,
                                        long long i) {
  return elem == 8 ? static_cast<const u64*>(labels)[i]
                   : (u64) static_cast<const u32*>(labels)[i];
}

// Rows of one entry: [0, ri) image patch, [ri, ri + rl) label patch, then the
// canvas.
__global__ __launch_bounds__(kThreads) void load_kernel(
    const LoadItem* __restrict__ items, SlotArrays s, float pad_logit,
    float centre_logit) {
  const LoadItem it = items[blockIdx.y];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int ri = s.image_patch.z * s.image_patch.y;
  const int rl = s.label_patch.z * s.label_patch.y;
  const int rc = s.canvas.z * s.canvas.y;
  const int rows = ri + rl + rc;
  const Dims lp = s.label_patch;
  const u64 centre = label_at(
      it.labels, it.label_elem,
      (it.lab0[0] + lp.z / 2) * it.sy + (it.lab0[1] + lp.y / 2) * it.sx +
          (it.lab0[2] + lp.x / 2));
  for (int r = blockIdx.x * kWaves + wave; r < rows; r += gridDim.x * kWaves) {
    if (r < ri) {
      const int z = r / s.image_patch.y, y = r - z * s.image_patch.y;
      const long long src =
          (it.img0[0] + z) * it.sy + (it.img0[1] + y) * it.sx + it.img0[2];
      float* dst = s.image_of(it.slot) + (size_t)r * s.image_patch.x;
      for (int x = lane; x < s.image_patch.x; x += 64) {
        const float v = it.image_elem == 1
                            ? (float)static_cast<const u8*>(it.image)[src + x]
                            : static_cast<const float*>(it.image)[src + x];
        dst[x] = (v - it.offset) / it.scale;
      }
    } else if (r < ri + rl) {
      const int q = r - ri;
      const int z = q / lp.y, y = q - z * lp.y;
      const long long src =
          (it.lab0[0] + z) * it.sy + (it.lab0[1] + y) * it.sx + it.lab0[2];
      float* dst = s.labels_of(it.slot) + (size_t)q * lp.x;
      for (int x = lane; x < lp.x; x += 64) {
        const u64 l = label_at(it.labels, it.label_elem, src + x);
        dst[x] = (l > 0 && l == centre) ? 0.95f : 0.05f;
      }
    } else {
      const int q = r - ri - rl;
      const int z = q / s.canvas.y, y = q - z * s.canvas.y;
      const bool mid = z == s.canvas.z / 2 && y == s.canvas.y / 2;
      float* dst = s.seed_of(it.slot) + (size_t)q * s.canvas.x;
      for (int x = lane; x < s.canvas.x; x += 64)
        dst[x] = (mid && x == s.canvas.x / 2) ? centre_logit : pad_logit;
    }
  }
}

constexpr int kTile = 64;              // voxels per tile edge: one wave's run
constexpr int kTileStride = kTile + 1;  // f32 column reads: 2 cycles, not 64

__device__ __forceinline__ int dim_of(const Dims& d, int a) {
  return a == 0 ? d.z : (a == 1 ? d.y : d.x);
}

// kKind 0: the volume's image voxel, normalised; 1: the volume's label as a
// soft label; 2: the f32 at `it.image`, as it is (load_sections' scratch).
template <int kKind>
__device__ __forceinline__ float load_value(const LoadItem& it, long long i,
                                            u64 centre) {
  if (kKind == 2) return static_cast<const float*>(it.image)[i];
  if (kKind == 1) {
    const u64 l = label_at(it.labels, it.label_elem, i);
    return (l > 0 && l == centre) ? 0.95f : 0.05f;
  }
  const float v = it.image_elem == 1
                      ? (float)static_cast<const u8*>(it.image)[i]
                      : static_cast<const float*>(it.image)[i];
  return (v - it.offset) / it.scale;
}

// x stays x: load_kernel's row of lanes, the source row picked through the
// transform and a reflected x read backwards.  q = row of the output patch.
template <int kKind>
__device__ __forceinline__ void aug_row(const AugItem& a, const int start[3],
                                        Dims S, int q, float* dst, u64 centre,
                                        int lane) {
  const int z = q / S.y, y = q - z * S.y;
  const int j0 = a.ra ? S.z - 1 - z : z;
  const int j1 = a.rb ? S.y - 1 - y : y;
  const int k0 = a.swap ? j1 : j0, k1 = a.swap ? j0 : j1;
  const long long src = (start[0] + k0) * a.load.sy +
                        (start[1] + k1) * a.load.sx + start[2];
  float* row = dst + (size_t)q * S.x;
  for (int x = lane; x < S.x; x += 64) {
    const int kx = a.rx ? S.x - 1 - x : x;
    row[x] = load_value<kKind>(a.load, src + kx, centre);
  }
}

// x changes places: tile t of the patch goes through LDS.  A tile is one index
// i_b of output axis b and kTile x kTile of (output x, output a2).  Reading,
// a wave takes one output-x index per round and its lanes run along the
// volume's x (output a2), values already normalised / turned into soft labels;
// writing, a wave takes one a2 index per round and its lanes run along the
// slot's x.  Both sides are contiguous runs of up to kTile voxels.
template <int kKind>
__device__ __forceinline__ void aug_tile(const AugItem& a, const int start[3],
                                         Dims S, int t, float* dst, u64 centre,
                                         float (*tile)[kTileStride], int wave,
                                         int lane) {
  const int b = 1 - a.a2;
  const int Sa = dim_of(S, a.a2), Sb = dim_of(S, b);
  const int na = (Sa + kTile - 1) / kTile, nx = (S.x + kTile - 1) / kTile;
  const int ib = t / (na * nx);
  const int rem = t - ib * (na * nx);
  const int ta = (rem / nx) * kTile, tx = (rem % nx) * kTile;
  const long long st_p2 = a.p2 == 0 ? a.load.sy : a.load.sx;
  const long long st_pb = a.p2 == 0 ? a.load.sx : a.load.sy;
  const int jb = a.rb ? Sb - 1 - ib : ib;
  const long long base = start[0] * a.load.sy + start[1] * a.load.sx +
                         start[2] + jb * st_pb;
  const int ia_r = ta + lane;
  const int k2 = a.ra ? Sa - 1 - ia_r : ia_r;
#pragma unroll 4
  for (int r = wave; r < kTile; r += kWaves) {
    const int i2 = tx + r;
    if (i2 < S.x && ia_r < Sa) {
      const int j2 = a.rx ? S.x - 1 - i2 : i2;
      tile[r][lane] = load_value<kKind>(a.load, base + j2 * st_p2 + k2, centre);
    }
  }
  __syncthreads();
  const int i2_w = tx + lane;
#pragma unroll 4
  for (int c = wave; c < kTile; c += kWaves) {
    const int ia = ta + c;
    if (ia < Sa && i2_w < S.x) {
      const int i0 = a.a2 == 0 ? ia : ib, i1 = a.a2 == 0 ? ib : ia;
      dst[((size_t)i0 * S.y + i1) * S.x + i2_w] = tile[lane][c];
    }
  }
  __syncthreads();
}

// grid.y = entry.  The branch on x_moves is uniform per workgroup.  kCopy
// (load_sections): an entry has two items, the first addressing a dense f32
// image patch and the second a dense f32 label patch (both through
// load.image, starts 0, their own strides), which are copied as they are.
template <bool kCopy>
__global__ __launch_bounds__(kThreads) void load_augmented_kernel(
    const AugItem* __restrict__ items, SlotArrays s, float pad_logit,
    float centre_logit) {
  __shared__ float tile[kTile][kTileStride];
  constexpr int kImage = kCopy ? 2 : 0, kLabel = kCopy ? 2 : 1;
  const AugItem a = items[kCopy ? 2 * blockIdx.y : blockIdx.y];
  const AugItem b_item = items[kCopy ? 2 * blockIdx.y + 1 : blockIdx.y];
  const AugItem& al = kCopy ? b_item : a;  // what addresses the labels
  const LoadItem& it = a.load;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const Dims ip = s.image_patch, lp = s.label_patch;
  const int rc = s.canvas.z * s.canvas.y;
  const u64 centre =
      kCopy ? 0
            : label_at(it.labels, it.label_elem,
                       (it.lab0[0] + lp.z / 2) * it.sy +
                           (it.lab0[1] + lp.y / 2) * it.sx +
                           (it.lab0[2] + lp.x / 2));
  float* image = s.image_of(it.slot);
  float* labels = s.labels_of(it.slot);
  float* seed = s.seed_of(it.slot);
  if (!a.x_moves) {
    const int ri = ip.z * ip.y, rl = lp.z * lp.y;
    const int rows = ri + rl + rc;
    for (int r = blockIdx.x * kWaves + wave; r < rows;
         r += gridDim.x * kWaves) {
      if (r < ri) {
        aug_row<kImage>(a, it.img0, ip, r, image, centre, lane);
      } else if (r < ri + rl) {
        aug_row<kLabel>(al, al.load.lab0, lp, r - ri, labels, centre, lane);
      } else {
        const int q = r - ri - rl;
        const int z = q / s.canvas.y, y = q - z * s.canvas.y;
        const bool mid = z == s.canvas.z / 2 && y == s.canvas.y / 2;
        float* dst = seed + (size_t)q * s.canvas.x;
        for (int x = lane; x < s.canvas.x; x += 64)
          dst[x] = (mid && x == s.canvas.x / 2) ? centre_logit : pad_logit;
      }
    }
    return;
  }
  const int b = 1 - a.a2;
  const int ti = dim_of(ip, b) * ((dim_of(ip, a.a2) + kTile - 1) / kTile) *
                 ((ip.x + kTile - 1) / kTile);
  const int tl = dim_of(lp, b) * ((dim_of(lp, a.a2) + kTile - 1) / kTile) *
                 ((lp.x + kTile - 1) / kTile);
  const int units = ti + tl + (rc + kWaves - 1) / kWaves;
  // (u depends on the workgroup only: every thread meets the same barriers)
  for (int u = blockIdx.x; u < units; u += gridDim.x) {
    if (u < ti) {
      aug_tile<kImage>(a, it.img0, ip, u, image, centre, tile, wave, lane);
    } else if (u < ti + tl) {
      aug_tile<kLabel>(al, al.load.lab0, lp, u - ti, labels, centre, tile, wave,
                        lane);
    } else {
      const int q = (u - ti - tl) * kWaves + wave;
      if (q < rc) {
        const int z = q / s.canvas.y, y = q - z * s.canvas.y;
        const bool mid = z == s.canvas.z / 2 && y == s.canvas.y / 2;
        float* dst = seed + (size_t)q * s.canvas.x;
        for (int x = lane; x < s.canvas.x; x += 64)
          dst[x] = (mid && x == s.canvas.x / 2) ? centre_logit : pad_logit;
      }
    }
  }
}

// ---- load_sections: the section augmentations, before the transform ----------

constexpr int kMaxRadius = FFN_EVALUATION_MAX_BLUR_RADIUS;
constexpr int kWeights = kMaxRadius + 1;  // w_0 .. w_r per entry, f64
constexpr int kLabelBlocks = 64;          // grid.x share of the label rows

// One entry of a load_sections: the load (img0 / lab0 are the starts of the
// final, unenlarged patches), and the entry's plan as the kernel needs it.
struct SecItem {
  LoadItem load;
  int margin[2];  // y, x
  int kind, z0, dy, dx;
  int m[3];       // per-axis maximum of the two loaded sizes
  int radius;     // of the blur; 0: none
  float blank_value;
};

__device__ __forceinline__ int wrap(int p, int n) {
  p %= n;
  return p < 0 ? p + n : p;
}

// Final index i of an axis of final size `fin`, loaded size `loaded`, padded
// size m -> index into the loaded box (ffn_evaluation.h, misalignment).
__device__ __forceinline__ int misaligned(int i, int fin, int loaded, int m,
                                          int shift, bool moved) {
  int p = i + (m - fin) / 2;
  if (moved) p = wrap(p + shift, m);
  const int j = p - (m - loaded) / 2;
  return j < 0 ? 0 : (j > loaded - 1 ? loaded - 1 : j);
}

__device__ __forceinline__ bool section_moved(const SecItem& it, int z, int Z) {
  const int zp = z + (it.m[0] - Z) / 2;
  return it.kind == 1 ? zp == it.z0 : (it.kind == 2 && zp >= it.z0);
}

// _quadrant_replace's four regions around the split point.
__device__ __forceinline__ bool selected(unsigned mask, const int32_t yx[2],
                                         int y, int x) {
  const int q = (y >= yx[0] ? 1 : 0) + (x >= yx[1] ? 2 : 0);
  return (mask >> q) & 1;
}

// d c b a | a b c d | d c b a: period 2 n.
__device__ __forceinline__ int reflected(int i, int n) {
  i = wrap(i, 2 * n);
  return i < n ? i : 2 * n - 1 - i;
}

// Grayscale perturbation where asked, then load's normalisation.
__device__ __forceinline__ float section_finish(
    float v, const ffn_evaluation_section& sec, const LoadItem& it) {
  if (sec.gray) {
    const float nv = __fdiv_rn(v, 255.f);
    const float a = __fadd_rn(__fmul_rn(nv, sec.contrast), sec.brightness);
    const float c = fminf(fmaxf(a, 0.f), 1.f);
    v = __fmul_rn(powf(c, sec.gamma), 255.f);
  }
  return (v - it.offset) / it.scale;
}

// One pass of the blur at (y, x) of plane p (H x W), along y (kAlongX = false)
// or x: scipy's symmetric correlate1d, in its order, no contraction.
template <bool kAlongX>
__device__ __forceinline__ float blur_at(const float* p, int H, int W, int y,
                                         int x, int r,
                                         const double* __restrict__ w) {
  double acc = __dmul_rn((double)p[y * W + x], w[0]);
  for (int k = r; k >= 1; --k) {
    const float lo = kAlongX ? p[y * W + reflected(x - k, W)]
                             : p[reflected(y - k, H) * W + x];
    const float hi = kAlongX ? p[y * W + reflected(x + k, W)]
                             : p[reflected(y + k, H) * W + x];
    acc = __dadd_rn(acc, __dmul_rn(__dadd_rn((double)lo, (double)hi), w[k]));
  }
  return (float)acc;
}

// grid.y = entry.  Workgroups [0, ip.z) of grid.x take one image section
// each; the others share the label rows, a wave per row as load_kernel.  A
// section without a blur streams: a wave per row, lanes along x.  A blurred
// one stages the misaligned, blanked plane in LDS (plane 0), blurs along y
// into plane 1, then along x; in every pass the lanes of a wave run along x,
// so consecutive lanes touch consecutive banks whatever the row length, and
// the only conflicts are the few lanes folded back at a reflected edge.
// Writes the untransformed, normalised image patch and the soft label patch
// of entry e densely at image_out[e] / labels_out[e].
__global__ __launch_bounds__(kThreads) void sections_kernel(
    const SecItem* __restrict__ items,
    const ffn_evaluation_section* __restrict__ sections,
    const double* __restrict__ weights, Dims ip, Dims lp,
    float* __restrict__ image_out, float* __restrict__ labels_out) {
  extern __shared__ __attribute__((aligned(16))) float planes[];
  const SecItem it = items[blockIdx.y];
  const LoadItem& ld = it.load;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int my = it.margin[0], mx = it.margin[1];
  if ((int)blockIdx.x >= ip.z) {
    const u64 centre = label_at(
        ld.labels, ld.label_elem,
        (ld.lab0[0] + lp.z / 2) * ld.sy + (ld.lab0[1] + lp.y / 2) * ld.sx +
            (ld.lab0[2] + lp.x / 2));
    float* out = labels_out + blockIdx.y * lp.voxels();
    const int rows = lp.z * lp.y;
    const int nb = gridDim.x - ip.z;
    for (int q = ((int)blockIdx.x - ip.z) * kWaves + wave; q < rows;
         q += nb * kWaves) {
      const int z = q / lp.y, y = q - z * lp.y;
      const bool moved = section_moved(it, z, lp.z);
      const int jy = misaligned(y, lp.y, lp.y + 2 * my, it.m[1], -it.dy, moved);
      const long long row = (ld.lab0[0] + z) * ld.sy +
                            (ld.lab0[1] - my + jy) * ld.sx + ld.lab0[2] - mx;
      for (int x = lane; x < lp.x; x += 64) {
        const int jx =
            misaligned(x, lp.x, lp.x + 2 * mx, it.m[2], it.dx, moved);
        const u64 l = label_at(ld.labels, ld.label_elem, row + jx);
        out[(size_t)q * lp.x + x] = (l > 0 && l == centre) ? 0.95f : 0.05f;
      }
    }
    return;
  }
  const int z = blockIdx.x;
  const int H = ip.y, W = ip.x;
  const ffn_evaluation_section sec = sections[blockIdx.y * ip.z + z];
  const bool moved = section_moved(it, z, ip.z);
  // (the same in every thread of the workgroup: the barriers below are safe)
  const int r = sec.blur_mask ? it.radius : 0;
  float* out = image_out + blockIdx.y * ip.voxels() + (size_t)z * H * W;
  float* p0 = planes;
  float* p1 = planes + H * W;
  for (int y = wave; y < H; y += kWaves) {
    const int jy = misaligned(y, H, H + 2 * my, it.m[1], -it.dy, moved);
    const long long row = (ld.img0[0] + z) * ld.sy +
                          (ld.img0[1] - my + jy) * ld.sx + ld.img0[2] - mx;
    for (int x = lane; x < W; x += 64) {
      const int jx = misaligned(x, W, W + 2 * mx, it.m[2], it.dx, moved);
      float v = ld.image_elem == 1
                    ? (float)static_cast<const u8*>(ld.image)[row + jx]
                    : static_cast<const float*>(ld.image)[row + jx];
      if (selected(sec.blank_mask, sec.blank_yx, y, x)) v = it.blank_value;
      if (r)
        p0[y * W + x] = v;
      else
        out[y * W + x] = section_finish(v, sec, ld);
    }
  }
  if (!r) return;
  const double* w = weights + blockIdx.y * kWeights;
  __syncthreads();
  for (int y = wave; y < H; y += kWaves)
    for (int x = lane; x < W; x += 64)
      p1[y * W + x] = blur_at<false>(p0, H, W, y, x, r, w);
  __syncthreads();
  for (int y = wave; y < H; y += kWaves)
    for (int x = lane; x < W; x += 64) {
      const float v = selected(sec.blur_mask, sec.blur_yx, y, x)
                          ? blur_at<true>(p1, H, W, y, x, r, w)
                          : p0[y * W + x];
      out[y * W + x] = section_finish(v, sec, ld);
    }
}

__global__ __launch_bounds__(kThreads) void probe_kernel(
    const BoxItem* __restrict__ items, u32 n, SlotArrays s, float seed_thr,
    float label_thr, u8* __restrict__ out) {
  const u32 i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const BoxItem it = items[i];
  const float sv = s.seed_of(it.slot)[((size_t)it.a0[0] * s.canvas.y + it.a0[1]) *
                                          s.canvas.x + it.a0[2]];
  const float lv =
      s.labels_of(it.slot)[((size_t)it.b0[0] * s.label_patch.y + it.b0[1]) *
                               s.label_patch.x + it.b0[2]];
  out[2 * i] = sv >= seed_thr ? 1 : 0;
  out[2 * i + 1] = lv >= label_thr ? 1 : 0;
}

// Rows [0, rs) of an entry are the seed box, the others the image box.
__global__ __launch_bounds__(kThreads) void gather_kernel(
    const BoxItem* __restrict__ items, SlotArrays s, Dims fs, Dims fi,
    float* __restrict__ seed_out, float* __restrict__ image_out) {
  const BoxItem it = items[blockIdx.y];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int rs = fs.z * fs.y;
  const int rows = rs + fi.z * fi.y;
  for (int r = blockIdx.x * kWaves + wave; r < rows; r += gridDim.x * kWaves) {
    if (r < rs) {
      const int z = r / fs.y, y = r - z * fs.y;
      const float* src = s.seed_of(it.slot) +
                         ((size_t)(it.a0[0] + z) * s.canvas.y + it.a0[1] + y) *
                             s.canvas.x + it.a0[2];
      float* dst = seed_out + blockIdx.y * fs.voxels() + (size_t)r * fs.x;
      for (int x = lane; x < fs.x; x += 64) dst[x] = src[x];
    } else {
      const int q = r - rs;
      const int z = q / fi.y, y = q - z * fi.y;
      const float* src =
          s.image_of(it.slot) +
          ((size_t)(it.b0[0] + z) * s.image_patch.y + it.b0[1] + y) *
              s.image_patch.x + it.b0[2];
      float* dst = image_out + blockIdx.y * fi.voxels() + (size_t)q * fi.x;
      for (int x = lane; x < fi.x; x += 64) dst[x] = src[x];
    }
  }
}

// Rows [0, rs) of an entry are the seed box, [rs, rs + ri) the image box, the
// others the pred_mask box of the label patch.
__global__ __launch_bounds__(kThreads) void gather_train_kernel(
    const TrainBoxItem* __restrict__ items, SlotArrays s, Dims fs, Dims fi,
    Dims pm, float* __restrict__ seed_out, float* __restrict__ image_out,
    float* __restrict__ labels_out) {
  const TrainBoxItem it = items[blockIdx.y];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int rs = fs.z * fs.y, ri = fi.z * fi.y;
  const int rows = rs + ri + pm.z * pm.y;
  for (int r = blockIdx.x * kWaves + wave; r < rows; r += gridDim.x * kWaves) {
    const float* src;
    float* dst;
    int nx;
    if (r < rs) {
      const int z = r / fs.y, y = r - z * fs.y;
      src = s.seed_of(it.slot) +
            ((size_t)(it.a0[0] + z) * s.canvas.y + it.a0[1] + y) * s.canvas.x +
            it.a0[2];
      dst = seed_out + blockIdx.y * fs.voxels() + (size_t)r * fs.x;
      nx = fs.x;
    } else if (r < rs + ri) {
      const int q = r - rs;
      const int z = q / fi.y, y = q - z * fi.y;
      src = s.image_of(it.slot) +
            ((size_t)(it.b0[0] + z) * s.image_patch.y + it.b0[1] + y) *
                s.image_patch.x + it.b0[2];
      dst = image_out + blockIdx.y * fi.voxels() + (size_t)q * fi.x;
      nx = fi.x;
    } else {
      const int q = r - rs - ri;
      const int z = q / pm.y, y = q - z * pm.y;
      src = s.labels_of(it.slot) +
            ((size_t)(it.c0[0] + z) * s.label_patch.y + it.c0[1] + y) *
                s.label_patch.x + it.c0[2];
      dst = labels_out + blockIdx.y * pm.voxels() + (size_t)q * pm.x;
      nx = pm.x;
    }
    for (int x = lane; x < nx; x += 64) dst[x] = src[x];
  }
}

// a0 = start of the pred box inside the canvas.  src: dense boxes of size
// `lay`, the pred box starting at `l0` inside each.
__global__ __launch_bounds__(kThreads) void paste_kernel(
    const BoxItem* __restrict__ items, SlotArrays s, Dims pm, Dims lay, Dims l0,
    const float* __restrict__ logits) {
  const BoxItem it = items[blockIdx.y];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int rows = pm.z * pm.y;
  for (int r = blockIdx.x * kWaves + wave; r < rows; r += gridDim.x * kWaves) {
    const int z = r / pm.y, y = r - z * pm.y;
    const float* src = logits + blockIdx.y * lay.voxels() +
                       ((size_t)(l0.z + z) * lay.y + l0.y + y) * lay.x + l0.x;
    float* dst = s.seed_of(it.slot) +
                 ((size_t)(it.a0[0] + z) * s.canvas.y + it.a0[1] + y) *
                     s.canvas.x + it.a0[2];
    for (int x = lane; x < pm.x; x += 64) dst[x] = src[x];
  }
}

__device__ __forceinline__ void keep_better(float& v, int& i, float ov, int oi) {
  if (ov > v || (ov == v && oi < i)) {
    v = ov;
    i = oi;
  }
}

// a0 = start of the working box [c - d, c + d] of the pred box, in the canvas.
// Workgroup (entry, face); out_score[6 n], out_index[6 n] = C-order index
// inside the face (rows x cols = the two free axes in zyx order).
__global__ __launch_bounds__(kThreads) void faces_kernel(
    const BoxItem* __restrict__ items, SlotArrays s, Dims d,
    float* __restrict__ out_score, int* __restrict__ out_index) {
  __shared__ float s_v[kWaves];
  __shared__ int s_i[kWaves];
  const BoxItem it = items[blockIdx.y];
  const int face = blockIdx.x;  // 0 .. 5
  const int axis = face >> 1;
  const int ext[3] = {2 * d.z + 1, 2 * d.y + 1, 2 * d.x + 1};
  const int fixed = (face & 1) ? ext[axis] - 1 : 0;
  const int ra = axis == 0 ? 1 : 0;  // row axis
  const int ca = axis == 2 ? 1 : 2;  // column axis
  const int cols = ext[ca];
  const int total = ext[ra] * cols;
  const float* base = s.seed_of(it.slot);
  float best = -INFINITY;
  int besti = 0x7fffffff;
  for (int e = threadIdx.x; e < total; e += kThreads) {
    int p[3];
    p[axis] = fixed;
    p[ra] = e / cols;
    p[ca] = e - p[ra] * cols;
    const float v = base[((size_t)(it.a0[0] + p[0]) * s.canvas.y + it.a0[1] +
                          p[1]) * s.canvas.x + it.a0[2] + p[2]];
    // (e ascends per thread: > keeps the first; -inf everywhere keeps index 0
    // through the tie rule below)
    if (v > best || besti == 0x7fffffff) {
      best = v;
      besti = e;
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float ov = __shfl_down(best, off);
    const int oi = __shfl_down(besti, off);
    keep_better(best, besti, ov, oi);
  }
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  if (lane == 0) {
    s_v[wave] = best;
    s_i[wave] = besti;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kWaves; ++w) keep_better(best, besti, s_v[w], s_i[w]);
    out_score[blockIdx.y * 6 + face] = best;
    out_index[blockIdx.y * 6 + face] = besti;
  }
}

struct Partial {
  float loss;
  u32 tp, tn, fp, fn;
};

__device__ __forceinline__ void block_tree(float& loss, u32 c[4], float* s_loss,
                                           u32 (*s_c)[4]) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    loss += __shfl_down(loss, off);
#pragma unroll
    for (int k = 0; k < 4; ++k) c[k] += __shfl_down(c[k], off);
  }
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  if (lane == 0) {
    s_loss[wave] = loss;
    for (int k = 0; k < 4; ++k) s_c[wave][k] = c[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    // kWaves = 4: ((0 + 1) + (2 + 3))
    loss = (s_loss[0] + s_loss[1]) + (s_loss[2] + s_loss[3]);
    for (int k = 0; k < 4; ++k)
      c[k] = s_c[0][k] + s_c[1][k] + s_c[2][k] + s_c[3][k];
  }
}

// e0 / l0 = start of the eval box in the canvas / the label patch.
__global__ __launch_bounds__(kThreads) void finish_kernel(
    SlotArrays s, int slot, Dims ev, Dims e0, Dims l0, float pred_thr,
    Partial* __restrict__ partials) {
  __shared__ float s_loss[kWaves];
  __shared__ u32 s_c[kWaves][4];
  const float* seed = s.seed_of(slot);
  const float* labels = s.labels_of(slot);
  const u32 n = (u32)ev.voxels();
  const u32 plane = (u32)ev.y * ev.x;
  float loss = 0.f;
  u32 c[4] = {0, 0, 0, 0};
  for (u32 i = blockIdx.x * kThreads + threadIdx.x; i < n;
       i += gridDim.x * kThreads) {
    const u32 z = i / plane, rem = i - z * plane;
    const u32 y = rem / ev.x, x = rem - y * ev.x;
    const float xv = seed[((size_t)(e0.z + z) * s.canvas.y + e0.y + y) *
                              s.canvas.x + e0.x + x];
    const float zv = labels[((size_t)(l0.z + z) * s.label_patch.y + l0.y + y) *
                                s.label_patch.x + l0.x + x];
    loss += fmaxf(xv, 0.f) - xv * zv + log1pf(expf(-fabsf(xv)));
    const bool pred = xv >= pred_thr, truth = zv > 0.5f;
    c[0] += pred && truth;
    c[1] += !pred && !truth;
    c[2] += pred && !truth;
    c[3] += !pred && truth;
  }
  block_tree(loss, c, s_loss, s_c);
  if (threadIdx.x == 0) {
    Partial p = {loss, c[0], c[1], c[2], c[3]};
    partials[blockIdx.x] = p;
  }
}

// One workgroup; nblocks <= kThreads.  out: loss, then the four counts as u32
// (a slot holds fewer than 2^32 voxels).
__global__ __launch_bounds__(kThreads) void finish_sum_kernel(
    const Partial* __restrict__ partials, int nblocks,
    Partial* __restrict__ out) {
  __shared__ float s_loss[kWaves];
  __shared__ u32 s_c[kWaves][4];
  float loss = 0.f;
  u32 c[4] = {0, 0, 0, 0};
  if ((int)threadIdx.x < nblocks) {
    const Partial p = partials[threadIdx.x];
    loss = p.loss;
    c[0] = p.tp;
    c[1] = p.tn;
    c[2] = p.fp;
    c[3] = p.fn;
  }
  block_tree(loss, c, s_loss, s_c);
  if (threadIdx.x == 0) {
    Partial p = {loss, c[0], c[1], c[2], c[3]};
    out[0] = p;
  }
}

Dims dims_of(const int32_t v[3]) { return Dims{v[0], v[1], v[2]}; }

}  // namespace

struct ffn_evaluation : ffn_unit::Unit {
  std::vector<std::unique_ptr<Volume>> volumes;
  bool configured = false;
  ffn_evaluation_geometry g;
  DevBuf seed, image, labels;  // slots x array
  DevBuf io_seed, io_image, io_logits, io_labels;
  DevBuf items, results, partials;
  PinnedBuf stage;
  double ms[6] = {0, 0, 0, 0, 0, 0}, bytes[6] = {0, 0, 0, 0, 0, 0};
  double ms_train[2] = {0, 0}, bytes_train[2] = {0, 0};
  // load_sections: the untransformed patches between its two launches, the
  // event between them, whether sections_kernel may take all of the LDS
  DevBuf sec_image, sec_labels;
  hipEvent_t ev_mid = nullptr;
  bool sec_lds_cleared = false;
  double ms_sections[2] = {0, 0}, bytes_sections[2] = {0, 0};

  ~ffn_evaluation() {
    if (ev_mid) (void)hipEventDestroy(ev_mid);
  }

  SlotArrays arrays() const {
    SlotArrays s;
    s.seed = static_cast<float*>(seed.p);
    s.image = static_cast<float*>(image.p);
    s.labels = static_cast<float*>(labels.p);
    s.canvas = dims_of(g.canvas_zyx);
    s.image_patch = dims_of(g.image_patch_zyx);
    s.label_patch = dims_of(g.label_patch_zyx);
    return s;
  }
};

namespace {

int ready(ffn_evaluation* h) {
  if (!h) return ffn_set_error(FFN_ERR_ARG, "NULL argument");
  if (!h->configured)
    return ffn_set_error(FFN_ERR_STATE, "ffn_evaluation_configure not called");
  U_TRY(hipSetDevice(h->device_id));
  return FFN_OK;
}

int check_slot(const ffn_evaluation* h, int slot) {
  if (slot < 0 || slot >= h->g.slots)
    return ffn_set_error(FFN_ERR_ARG, "slot %d outside [0, %d)", slot,
                         h->g.slots);
  return FFN_OK;
}

// n <= slots distinct valid slots.
int check_slots(const ffn_evaluation* h, int n, const int32_t* slots,
                bool distinct) {
  if (n < 1 || n > h->g.slots)
    return ffn_set_error(FFN_ERR_ARG, "%d entries for %d slots", n, h->g.slots);
  u32 seen = 0;
  for (int k = 0; k < n; ++k) {
    U_OK(check_slot(h, slots[k]));
    if (distinct && ((seen >> slots[k]) & 1))
      return ffn_set_error(FFN_ERR_ARG, "slot %d given twice", slots[k]);
    seen |= 1u << slots[k];
  }
  return FFN_OK;
}

// start[] = size / 2 - crop / 2 + offset (xyz -> zyx), FFN_ERR_ARG if the box
// leaves [0, size).
int box_start(const int32_t size[3], const int32_t crop[3],
              const int32_t* off_xyz, int start[3], const char* what) {
  for (int a = 0; a < 3; ++a) {
    const long long st =
        (long long)size[a] / 2 - crop[a] / 2 + (long long)off_xyz[2 - a];
    if (st < 0 || st + crop[a] > size[a])
      return ffn_set_error(FFN_ERR_ARG,
                           "offset (%d, %d, %d) xyz takes the %s box out of its "
                           "array",
                           off_xyz[0], off_xyz[1], off_xyz[2], what);
    start[a] = (int)st;
  }
  return FFN_OK;
}

// Stages `bytes` of descriptors and queues their copy to h->items.
int send_items(ffn_evaluation* h, const void* src, size_t bytes) {
  U_OK(ensure(h->stage, bytes));
  U_OK(ensure(h->items, bytes));
  std::memcpy(h->stage.p, src, bytes);
  U_TRY(hipMemcpyAsync(h->items.p, h->stage.p, bytes, hipMemcpyHostToDevice,
                       h->stream));
  return FFN_OK;
}

int fetch(ffn_evaluation* h, void* dst, const void* src_dev, size_t bytes) {
  U_TRY(hipMemcpyAsync(dst, src_dev, bytes, hipMemcpyDeviceToHost, h->stream));
  U_TRY(hipStreamSynchronize(h->stream));
  return FFN_OK;
}

unsigned row_blocks(int rows) {
  const int b = (rows + kWaves - 1) / kWaves;
  return (unsigned)(b < 1 ? 1 : (b > kRowBlocks ? kRowBlocks : b));
}

}  // namespace

extern "C" {

int ffn_evaluation_create(int device_id, ffn_evaluation** out) {
  return ffn_unit::unit_create(device_id, out);
}

void ffn_evaluation_destroy(ffn_evaluation* h) { ffn_unit::unit_destroy(h); }

int ffn_evaluation_configure(ffn_evaluation* h,
                             const ffn_evaluation_geometry* geometry) {
  if (!h || !geometry) return ffn_set_error(FFN_ERR_ARG, "NULL argument");
  const ffn_evaluation_geometry& g = *geometry;
  if (g.slots < 1 || g.slots > kMaxSlots)
    return ffn_set_error(FFN_ERR_ARG, "slots %d outside [1, %d]", g.slots,
                         kMaxSlots);
  for (int a = 0; a < 3; ++a) {
    const int32_t sizes[] = {g.input_seed_zyx[a],  g.input_image_zyx[a],
                             g.pred_mask_zyx[a],   g.canvas_zyx[a],
                             g.image_patch_zyx[a], g.label_patch_zyx[a],
                             g.eval_zyx[a]};
    for (int32_t v : sizes)
      if (v < 1 || v > 4096)
        return ffn_set_error(FFN_ERR_ARG, "size %d on axis %d", v, a);
    if (g.deltas_zyx[a] < 0)
      return ffn_set_error(FFN_ERR_ARG, "negative delta on axis %d", a);
    if (g.pred_mask_zyx[a] > g.input_seed_zyx[a] ||
        (g.input_seed_zyx[a] - g.pred_mask_zyx[a]) % 2)
      return ffn_set_error(FFN_ERR_ARG,
                           "pred_mask must fit input_seed with an even "
                           "difference (axis %d)", a);
    if (g.input_seed_zyx[a] > g.canvas_zyx[a] ||
        g.input_image_zyx[a] > g.image_patch_zyx[a] ||
        g.pred_mask_zyx[a] > g.label_patch_zyx[a] ||
        g.eval_zyx[a] > g.canvas_zyx[a] || g.eval_zyx[a] > g.label_patch_zyx[a])
      return ffn_set_error(FFN_ERR_ARG, "a box exceeds its array on axis %d", a);
  }
  const Dims cv = dims_of(g.canvas_zyx), ip = dims_of(g.image_patch_zyx),
             lp = dims_of(g.label_patch_zyx);
  if (cv.voxels() >= (1ull << 31) || ip.voxels() >= (1ull << 31) ||
      lp.voxels() >= (1ull << 31))
    return ffn_set_error(FFN_ERR_ARG, "arrays of 2^31 voxels or more");
  U_TRY(hipSetDevice(h->device_id));
  U_TRY(hipStreamSynchronize(h->stream));
  h->configured = false;
  U_OK(ensure(h->seed, g.slots * cv.voxels() * sizeof(float)));
  U_OK(ensure(h->image, g.slots * ip.voxels() * sizeof(float)));
  U_OK(ensure(h->labels, g.slots * lp.voxels() * sizeof(float)));
  U_OK(ensure(h->partials, (kFinishBlocks + 1) * sizeof(Partial)));
  const size_t fs = dims_of(g.input_seed_zyx).voxels(),
               fi = dims_of(g.input_image_zyx).voxels();
  U_OK(ensure(h->io_seed, g.slots * fs * sizeof(float)));
  U_OK(ensure(h->io_image, g.slots * fi * sizeof(float)));
  U_OK(ensure(h->io_logits, g.slots * fs * sizeof(float)));
  U_OK(ensure(h->io_labels,
              g.slots * dims_of(g.pred_mask_zyx).voxels() * sizeof(float)));
  h->g = g;
  h->configured = true;
  return FFN_OK;
}

int ffn_evaluation_io_buffers(ffn_evaluation* h, float** seed_dev,
                              float** image_dev, float** logits_dev) {
  if (!h || !seed_dev || !image_dev || !logits_dev)
    return ffn_set_error(FFN_ERR_ARG, "NULL argument");
  if (!h->configured)
    return ffn_set_error(FFN_ERR_STATE, "ffn_evaluation_configure not called");
  *seed_dev = static_cast<float*>(h->io_seed.p);
  *image_dev = static_cast<float*>(h->io_image.p);
  *logits_dev = static_cast<float*>(h->io_logits.p);
  return FFN_OK;
}

int ffn_evaluation_reset(ffn_evaluation* h) {
  if (!h) return ffn_set_error(FFN_ERR_ARG, "NULL argument");
  U_TRY(hipSetDevice(h->device_id));
  U_TRY(hipStreamSynchronize(h->stream));
  h->volumes.clear();
  return FFN_OK;
}

int ffn_evaluation_add_volume(ffn_evaluation* h, const void* image,
                              int image_elem, const void* labels,
                              int label_elem, const int64_t shape_zyx[3],
                              int32_t* index) {
  if (!h || !image || !labels || !shape_zyx || !index)
    return ffn_set_error(FFN_ERR_ARG, "NULL argument");
  if ((image_elem != 1 && image_elem != 4) ||
      (label_elem != 4 && label_elem != 8))
    return ffn_set_error(FFN_ERR_ARG, "image_elem %d / label_elem %d",
                         image_elem, label_elem);
  double voxels = 1.0;
  for (int k = 0; k < 3; ++k) {
    if (shape_zyx[k] < 1 || shape_zyx[k] >= (1ll << 31))
      return ffn_set_error(FFN_ERR_ARG, "shape[%d] = %lld", k,
                           (long long)shape_zyx[k]);
    voxels *= (double)shape_zyx[k];
  }
  if (voxels >= 4.0e12)
    return ffn_set_error(FFN_ERR_ARG, "volume too large");
  U_TRY(hipSetDevice(h->device_id));
  const size_t n = (size_t)shape_zyx[0] * shape_zyx[1] * shape_zyx[2];
  std::unique_ptr<Volume> vol(new Volume());
  U_OK(ensure(vol->image, n * image_elem));
  U_OK(ensure(vol->labels, n * label_elem));
  // (pageable memory of the caller's: returns with both copies complete)
  U_TRY(hipMemcpyAsync(vol->image.p, image, n * image_elem,
                       hipMemcpyHostToDevice, h->stream));
  U_TRY(hipMemcpyAsync(vol->labels.p, labels, n * label_elem,
                       hipMemcpyHostToDevice, h->stream));
  U_TRY(hipStreamSynchronize(h->stream));
  vol->image_elem = image_elem;
  vol->label_elem = label_elem;
  for (int k = 0; k < 3; ++k) vol->shape[k] = shape_zyx[k];
  *index = (int32_t)h->volumes.size();
  h->volumes.push_back(std::move(vol));
  return FFN_OK;
}

}  // extern "C"

namespace {

// The argument checks of load and the validated entries; items[k] is written
// through `at(k)`, which load and load_augmented lay out differently.
template <typename At>
int load_items(ffn_evaluation* h, int n, const int32_t* slots,
               const int32_t* volumes, const int32_t* centres_xyz,
               const float* offsets, const float* scales, At at,
               double* volume_bytes_out) {
  U_OK(ready(h));
  if (!slots || !volumes || !centres_xyz || !offsets || !scales)
    return ffn_set_error(FFN_ERR_ARG, "NULL argument");
  U_OK(check_slots(h, n, slots, true));
  const ffn_evaluation_geometry& g = h->g;
  double volume_bytes = 0.0;
  for (int k = 0; k < n; ++k) {
    if (volumes[k] < 0 || (size_t)volumes[k] >= h->volumes.size())
      return ffn_set_error(FFN_ERR_ARG, "no volume %d", volumes[k]);
    const Volume& v = *h->volumes[volumes[k]];
    LoadItem& it = at(k);
    it.image = v.image.p;
    it.labels = v.labels.p;
    it.sy = v.shape[1] * v.shape[2];
    it.sx = v.shape[2];
    it.image_elem = v.image_elem;
    it.label_elem = v.label_elem;
    it.slot = slots[k];
    it.offset = offsets[k];
    it.scale = scales[k];
    for (int a = 0; a < 3; ++a) {
      const long long c = centres_xyz[3 * k + 2 - a];
      const long long i0 = c - (g.image_patch_zyx[a] - 1) / 2;
      const long long l0 = c - (g.label_patch_zyx[a] - 1) / 2;
      if (i0 < 0 || i0 + g.image_patch_zyx[a] > v.shape[a] || l0 < 0 ||
          l0 + g.label_patch_zyx[a] > v.shape[a])
        return ffn_set_error(FFN_ERR_ARG,
                             "the patches around (%d, %d, %d) xyz leave volume "
                             "%d", centres_xyz[3 * k], centres_xyz[3 * k + 1],
                             centres_xyz[3 * k + 2], volumes[k]);
      it.img0[a] = (int)i0;
      it.lab0[a] = (int)l0;
    }
    volume_bytes += (double)dims_of(g.image_patch_zyx).voxels() * v.image_elem +
                    (double)dims_of(g.label_patch_zyx).voxels() * v.label_elem;
  }
  *volume_bytes_out = volume_bytes;
  return FFN_OK;
}

double load_bytes(const SlotArrays& s, int n, double volume_bytes) {
  return volume_bytes + 4.0 * n * (double)(s.image_patch.voxels() +
                                           s.label_patch.voxels() +
                                           s.canvas.voxels());
}

// The checks of load_augmented's perms / reflects and the transform fields of
// items[k * stride] for k < n; *blocks = grid.x of load_augmented_kernel.
int transform_items(const ffn_evaluation* h, int n, const int32_t* perms,
                    const uint8_t* reflects, AugItem* items, int stride,
                    int* blocks_out) {
  if (!perms || !reflects) return ffn_set_error(FFN_ERR_ARG, "NULL argument");
  const ffn_evaluation_geometry& g = h->g;
  const SlotArrays s = h->arrays();
  const int rc = s.canvas.z * s.canvas.y;
  auto tiles = [](int n) { return (n + kTile - 1) / kTile; };
  int blocks = 1;
  for (int k = 0; k < n; ++k) {
    const int32_t* perm = perms + 3 * k;
    const uint8_t* ref = reflects + 3 * k;
    unsigned seen = 0;
    for (int a = 0; a < 3; ++a) {
      if (perm[a] < 0 || perm[a] > 2 || ((seen >> perm[a]) & 1))
        return ffn_set_error(FFN_ERR_ARG,
                             "(%d, %d, %d) is not a permutation of 0, 1, 2",
                             perm[0], perm[1], perm[2]);
      seen |= 1u << perm[a];
      if (ref[a] > 1)
        return ffn_set_error(FFN_ERR_ARG, "reflect value %d is not 0 or 1",
                             (int)ref[a]);
    }
    for (int a = 0; a < 3; ++a)
      if (perm[a] != a &&
          (g.image_patch_zyx[a] != g.image_patch_zyx[perm[a]] ||
           g.label_patch_zyx[a] != g.label_patch_zyx[perm[a]]))
        return ffn_set_error(FFN_ERR_ARG,
                             "axes %d and %d change places but differ in patch "
                             "size", a, perm[a]);
    AugItem& it = items[k * stride];
    it.x_moves = perm[2] != 2;
    it.a2 = it.p2 = it.swap = 0;
    int units;
    if (!it.x_moves) {
      it.swap = perm[0] == 1;
      it.ra = ref[0];
      it.rb = ref[1];
      units = (s.image_patch.z * s.image_patch.y +
               s.label_patch.z * s.label_patch.y + rc + kWaves - 1) / kWaves;
    } else {
      it.a2 = perm[0] == 2 ? 0 : 1;
      it.p2 = perm[2];
      const int b = 1 - it.a2;
      it.ra = ref[it.a2];
      it.rb = ref[b];
      units = (rc + kWaves - 1) / kWaves;
      for (const int32_t* S : {g.image_patch_zyx, g.label_patch_zyx})
        units += S[b] * tiles(S[it.a2]) * tiles(S[2]);
    }
    it.rx = ref[2];
    if (units > blocks) blocks = units;
  }
  *blocks_out = blocks > kRowBlocks ? kRowBlocks : blocks;
  return FFN_OK;
}

}  // namespace

extern "C" {

int ffn_evaluation_load(ffn_evaluation* h, int n, const int32_t* slots,
                        const int32_t* volumes, const int32_t* centres_xyz,
                        const float* offsets, const float* scales,
                        float seed_pad_logit, float seed_centre_logit) {
  LoadItem items[kMaxSlots];
  double volume_bytes = 0.0;
  U_OK(load_items(h, n, slots, volumes, centres_xyz, offsets, scales,
                  [&](int k) -> LoadItem& { return items[k]; },
                  &volume_bytes));
  U_OK(send_items(h, items, n * sizeof(LoadItem)));
  const SlotArrays s = h->arrays();
  const int rows = s.image_patch.z * s.image_patch.y +
                   s.label_patch.z * s.label_patch.y + s.canvas.z * s.canvas.y;
  double ms = 0.0;
  U_OK(h->timer_start());
  hipLaunchKernelGGL(load_kernel, dim3(row_blocks(rows), n), dim3(kThreads), 0,
                     h->stream, static_cast<const LoadItem*>(h->items.p), s,
                     seed_pad_logit, seed_centre_logit);
  U_TRY(hipGetLastError());
  U_OK(h->timer_stop(&ms));
  h->ms[0] = ms;
  h->bytes[0] = load_bytes(s, n, volume_bytes);
  return FFN_OK;
}

int ffn_evaluation_load_augmented(ffn_evaluation* h, int n,
                                  const int32_t* slots, const int32_t* volumes,
                                  const int32_t* centres_xyz,
                                  const float* offsets, const float* scales,
                                  const int32_t* perms, const uint8_t* reflects,
                                  float seed_pad_logit,
                                  float seed_centre_logit) {
  AugItem items[kMaxSlots];
  double volume_bytes = 0.0;
  U_OK(load_items(h, n, slots, volumes, centres_xyz, offsets, scales,
                  [&](int k) -> LoadItem& { return items[k].load; },
                  &volume_bytes));
  int blocks = 1;
  U_OK(transform_items(h, n, perms, reflects, items, 1, &blocks));
  const SlotArrays s = h->arrays();
  U_OK(send_items(h, items, n * sizeof(AugItem)));
  double ms = 0.0;
  U_OK(h->timer_start());
  hipLaunchKernelGGL(load_augmented_kernel<false>, dim3(blocks, n),
                     dim3(kThreads), 0,
                     h->stream, static_cast<const AugItem*>(h->items.p), s,
                     seed_pad_logit, seed_centre_logit);
  U_TRY(hipGetLastError());
  U_OK(h->timer_stop(&ms));
  h->ms_train[0] = ms;
  h->bytes_train[0] = load_bytes(s, n, volume_bytes);
  return FFN_OK;
}

int ffn_evaluation_load_sections(
    ffn_evaluation* h, int n, const int32_t* slots, const int32_t* volumes,
    const int32_t* centres_xyz, const float* offsets, const float* scales,
    const int32_t* perms, const uint8_t* reflects,
    const ffn_evaluation_section_plan* plans,
    const ffn_evaluation_section* sections, float seed_pad_logit,
    float seed_centre_logit) {
  SecItem items[kMaxSlots];
  AugItem copies[2 * kMaxSlots];
  double volume_bytes = 0.0;
  U_OK(load_items(h, n, slots, volumes, centres_xyz, offsets, scales,
                  [&](int k) -> LoadItem& { return items[k].load; },
                  &volume_bytes));
  int blocks = 1;
  U_OK(transform_items(h, n, perms, reflects, copies, 2, &blocks));
  if (!plans || !sections) return ffn_set_error(FFN_ERR_ARG, "NULL argument");
  const ffn_evaluation_geometry& g = h->g;
  const SlotArrays s = h->arrays();
  const Dims ip = s.image_patch, lp = s.label_patch;
  std::vector<double> weights((size_t)n * kWeights, 0.0);
  bool any_blur = false;
  for (int k = 0; k < n; ++k) {
    const ffn_evaluation_section_plan& p = plans[k];
    SecItem& it = items[k];
    const Volume& v = *h->volumes[volumes[k]];
    if (p.margin_yx[0] < 0 || p.margin_yx[1] < 0 || p.margin_yx[0] > 4096 ||
        p.margin_yx[1] > 4096)
      return ffn_set_error(FFN_ERR_ARG, "margin (%d, %d) of entry %d",
                           p.margin_yx[0], p.margin_yx[1], k);
    if (p.kind < 0 || p.kind > 2)
      return ffn_set_error(FFN_ERR_ARG, "misalignment kind %d is not 0, 1, 2",
                           p.kind);
    it.margin[0] = p.margin_yx[0];
    it.margin[1] = p.margin_yx[1];
    it.m[0] = ip.z > lp.z ? ip.z : lp.z;
    it.m[1] = (ip.y > lp.y ? ip.y : lp.y) + 2 * it.margin[0];
    it.m[2] = (ip.x > lp.x ? ip.x : lp.x) + 2 * it.margin[1];
    if (p.z0 < 0 || p.z0 >= it.m[0])
      return ffn_set_error(FFN_ERR_ARG, "z0 %d outside [0, %d)", p.z0, it.m[0]);
    if (p.dy < -it.m[1] || p.dy > it.m[1] || p.dx < -it.m[2] ||
        p.dx > it.m[2])
      return ffn_set_error(FFN_ERR_ARG,
                           "misalignment offset (%d, %d) exceeds the padded "
                           "size (%d, %d)", p.dy, p.dx, it.m[1], it.m[2]);
    it.kind = p.kind;
    it.z0 = p.z0;
    it.dy = p.dy;
    it.dx = p.dx;
    it.blank_value = p.blank_value;
    // (a NaN fails the first comparison)
    if (!(p.blur_sigma >= 0.f) || !(p.blur_sigma <= 16.f))
      return ffn_set_error(FFN_ERR_ARG, "blur_sigma %g of entry %d",
                           (double)p.blur_sigma, k);
    const double sigma = (double)p.blur_sigma;
    it.radius = (int)(4.0 * sigma + 0.5);
    if (it.radius > kMaxRadius)
      return ffn_set_error(FFN_ERR_ARG, "blur_sigma %g gives radius %d > %d",
                           sigma, it.radius, kMaxRadius);
    double* w = weights.data() + (size_t)k * kWeights;
    w[0] = 1.0;
    if (it.radius > 0) {
      // scipy's _gaussian_kernel1d: exp(-0.5 / sigma^2 * x^2) over x = -r .. r,
      // divided by its sum
      const double c = -0.5 / (sigma * sigma);
      double sum = 0.0;
      for (int x = -it.radius; x <= it.radius; ++x)
        sum += std::exp(c * (double)(x * x));
      for (int x = 0; x <= it.radius; ++x)
        w[x] = std::exp(c * (double)(x * x)) / sum;
    }
    bool blurred = false;
    for (int z = 0; z < ip.z; ++z) {
      const ffn_evaluation_section& sec = sections[(size_t)k * ip.z + z];
      if (sec.blank_mask > 15 || sec.blur_mask > 15 || sec.gray > 1)
        return ffn_set_error(FFN_ERR_ARG,
                             "section %d of entry %d: masks (%d, %d), gray %d",
                             z, k, (int)sec.blank_mask, (int)sec.blur_mask,
                             (int)sec.gray);
      for (const int32_t* yx : {sec.blank_yx, sec.blur_yx})
        if (yx[0] < 0 || yx[0] > ip.y || yx[1] < 0 || yx[1] > ip.x)
          return ffn_set_error(FFN_ERR_ARG,
                               "split point (%d, %d) outside the %d x %d "
                               "section", yx[0], yx[1], ip.y, ip.x);
      if (sec.gray &&
          (!std::isfinite(sec.contrast) || !std::isfinite(sec.brightness) ||
           !std::isfinite(sec.gamma) || !(sec.gamma > 0.f)))
        return ffn_set_error(FFN_ERR_ARG,
                             "grayscale factors (%g, %g, %g) of section %d",
                             (double)sec.contrast, (double)sec.brightness,
                             (double)sec.gamma, z);
      if (sec.blur_mask && it.radius > 0) blurred = true;
    }
    if (blurred && (long long)ip.y * ip.x > FFN_EVALUATION_MAX_BLUR_PLANE)
      return ffn_set_error(FFN_ERR_ARG,
                           "a blur on a %d x %d section: at most %d voxels",
                           ip.y, ip.x, FFN_EVALUATION_MAX_BLUR_PLANE);
    any_blur = any_blur || blurred;
    // the enlarged boxes (z has no margin: load_items checked it)
    for (int a = 1; a < 3; ++a) {
      const long long mg = it.margin[a - 1];
      if (it.load.img0[a] - mg < 0 ||
          it.load.img0[a] + g.image_patch_zyx[a] + mg > v.shape[a] ||
          it.load.lab0[a] - mg < 0 ||
          it.load.lab0[a] + g.label_patch_zyx[a] + mg > v.shape[a])
        return ffn_set_error(FFN_ERR_ARG,
                             "the patches around (%d, %d, %d) xyz with margin "
                             "(%d, %d) leave volume %d", centres_xyz[3 * k],
                             centres_xyz[3 * k + 1], centres_xyz[3 * k + 2],
                             it.margin[0], it.margin[1], volumes[k]);
    }
  }
  U_OK(ensure(h->sec_image, (size_t)n * ip.voxels() * sizeof(float)));
  U_OK(ensure(h->sec_labels, (size_t)n * lp.voxels() * sizeof(float)));
  if (!h->ev_mid) U_TRY(hipEventCreate(&h->ev_mid));
  const size_t lds = any_blur ? 2 * (size_t)ip.y * ip.x * sizeof(float) : 0;
  if (lds > 48 * 1024 && !h->sec_lds_cleared) {
    U_TRY(hipFuncSetAttribute(
        reinterpret_cast<const void*>(&sections_kernel),
        hipFuncAttributeMaxDynamicSharedMemorySize,
        2 * FFN_EVALUATION_MAX_BLUR_PLANE * (int)sizeof(float)));
    h->sec_lds_cleared = true;
  }
  // the second launch copies the scratch patches: dense, starts 0
  for (int k = 0; k < n; ++k) {
    for (int which = 0; which < 2; ++which) {
      AugItem& c = copies[2 * k + which];
      if (which) c = copies[2 * k];  // the transform
      const Dims d = which ? lp : ip;
      LoadItem& l = c.load;
      l.image = static_cast<float*>(which ? h->sec_labels.p : h->sec_image.p) +
                (size_t)k * d.voxels();
      l.labels = nullptr;
      l.sy = (long long)d.y * d.x;
      l.sx = d.x;
      l.image_elem = 4;
      l.label_elem = 4;
      l.slot = slots[k];
      l.offset = 0.f;
      l.scale = 1.f;
      for (int a = 0; a < 3; ++a) l.img0[a] = l.lab0[a] = 0;
    }
  }
  // one blob: SecItem[n] | AugItem[2 n] | sections [n][z] | weights [n][32]
  auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
  const size_t off_copies = up16(n * sizeof(SecItem));
  const size_t off_sections = up16(off_copies + 2 * n * sizeof(AugItem));
  const size_t sections_bytes =
      (size_t)n * ip.z * sizeof(ffn_evaluation_section);
  const size_t off_weights = up16(off_sections + sections_bytes);
  const size_t total = off_weights + weights.size() * sizeof(double);
  std::vector<char> blob(total, 0);
  std::memcpy(blob.data(), items, n * sizeof(SecItem));
  std::memcpy(blob.data() + off_copies, copies, 2 * n * sizeof(AugItem));
  std::memcpy(blob.data() + off_sections, sections, sections_bytes);
  std::memcpy(blob.data() + off_weights, weights.data(),
              weights.size() * sizeof(double));
  U_OK(send_items(h, blob.data(), total));
  const char* dev = static_cast<const char*>(h->items.p);
  int label_blocks = (lp.z * lp.y + kWaves - 1) / kWaves;
  if (label_blocks > kLabelBlocks) label_blocks = kLabelBlocks;
  U_OK(h->timer_start());
  hipLaunchKernelGGL(
      sections_kernel, dim3(ip.z + label_blocks, n), dim3(kThreads), lds,
      h->stream, reinterpret_cast<const SecItem*>(dev),
      reinterpret_cast<const ffn_evaluation_section*>(dev + off_sections),
      reinterpret_cast<const double*>(dev + off_weights), ip, lp,
      static_cast<float*>(h->sec_image.p),
      static_cast<float*>(h->sec_labels.p));
  U_TRY(hipGetLastError());
  U_TRY(hipEventRecord(h->ev_mid, h->stream));
  hipLaunchKernelGGL(load_augmented_kernel<true>, dim3(blocks, n),
                     dim3(kThreads), 0, h->stream,
                     reinterpret_cast<const AugItem*>(dev + off_copies), s,
                     seed_pad_logit, seed_centre_logit);
  U_TRY(hipGetLastError());
  double ms = 0.0;
  U_OK(h->timer_stop(&ms));
  float first = 0.f;
  U_TRY(hipEventElapsedTime(&first, h->ev0, h->ev_mid));
  h->ms_sections[0] = ms;
  h->ms_sections[1] = first;
  h->bytes_sections[0] = load_bytes(s, n, volume_bytes);
  h->bytes_sections[1] =
      volume_bytes + 4.0 * n * (double)(ip.voxels() + lp.voxels());
  return FFN_OK;
}

int ffn_evaluation_last_timing_sections(ffn_evaluation* h, double kernel_ms[2],
                                        double algorithmic_bytes[2]) {
  if (!h || !kernel_ms || !algorithmic_bytes)
    return ffn_set_error(FFN_ERR_ARG, "NULL argument");
  for (int k = 0; k < 2; ++k) {
    kernel_ms[k] = h->ms_sections[k];
    algorithmic_bytes[k] = h->bytes_sections[k];
  }
  return FFN_OK;
}

int ffn_evaluation_probe_moves(ffn_evaluation* h, size_t n,
                               const int32_t* slots, const int32_t* offsets_xyz,
                               float seed_threshold, float label_threshold,
                               uint8_t* valid, uint8_t* wanted) {
  U_OK(ready(h));
  if (!slots || !offsets_xyz || !valid || !wanted)
    return ffn_set_error(FFN_ERR_ARG, "NULL argument");
  if (n == 0) return FFN_OK;
  if (n >= (1u << 24)) return ffn_set_error(FFN_ERR_ARG, "too many pairs");
  const int32_t one[3] = {1, 1, 1};
  std::vector<BoxItem> items(n);
  for (size_t k = 0; k < n; ++k) {
    U_OK(check_slot(h, slots[k]));
    items[k].slot = slots[k];
    U_OK(box_start(h->g.canvas_zyx, one, offsets_xyz + 3 * k, items[k].a0,
                   "seed probe"));
    U_OK(box_start(h->g.label_patch_zyx, one, offsets_xyz + 3 * k, items[k].b0,
                   "label probe"));
  }
  U_OK(send_items(h, items.data(), n * sizeof(BoxItem)));
  U_OK(ensure(h->results, 2 * n));
  double ms = 0.0;
  U_OK(h->timer_start());
  hipLaunchKernelGGL(probe_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)),
                     dim3(kThreads), 0, h->stream,
                     static_cast<const BoxItem*>(h->items.p), (u32)n,
                     h->arrays(), seed_threshold, label_threshold,
                     static_cast<u8*>(h->results.p));
  U_TRY(hipGetLastError());
  U_OK(h->timer_stop(&ms));
  std::vector<u8> out(2 * n);
  U_OK(fetch(h, out.data(), h->results.p, 2 * n));
  for (size_t k = 0; k < n; ++k) {
    valid[k] = out[2 * k];
    wanted[k] = out[2 * k + 1];
  }
  h->ms[1] = ms;
  h->bytes[1] = 8.0 * n;
  return FFN_OK;
}

int ffn_evaluation_gather(ffn_evaluation* h, int n, const int32_t* slots,
                          const int32_t* offsets_xyz, float* seed_out_dev,
                          float* image_out_dev) {
  U_OK(ready(h));
  if (!slots || !offsets_xyz || !seed_out_dev || !image_out_dev)
    return ffn_set_error(FFN_ERR_ARG, "NULL argument");
  U_OK(check_slots(h, n, slots, false));
  const ffn_evaluation_geometry& g = h->g;
  BoxItem items[kMaxSlots];
  for (int k = 0; k < n; ++k) {
    items[k].slot = slots[k];
    U_OK(box_start(g.canvas_zyx, g.input_seed_zyx, offsets_xyz + 3 * k,
                   items[k].a0, "input_seed"));
    U_OK(box_start(g.image_patch_zyx, g.input_image_zyx, offsets_xyz + 3 * k,
                   items[k].b0, "input_image"));
  }
  U_OK(send_items(h, items, n * sizeof(BoxItem)));
  const Dims fs = dims_of(g.input_seed_zyx), fi = dims_of(g.input_image_zyx);
  double ms = 0.0;
  U_OK(h->timer_start());
  hipLaunchKernelGGL(gather_kernel,
                     dim3(row_blocks(fs.z * fs.y + fi.z * fi.y), n),
                     dim3(kThreads), 0, h->stream,
                     static_cast<const BoxItem*>(h->items.p), h->arrays(), fs,
                     fi, seed_out_dev, image_out_dev);
  U_TRY(hipGetLastError());
  U_OK(h->timer_stop(&ms));
  h->ms[2] = ms;
  h->bytes[2] = 8.0 * n * (double)(fs.voxels() + fi.voxels());
  return FFN_OK;
}

int ffn_evaluation_gather_train(ffn_evaluation* h, int n, const int32_t* slots,
                                const int32_t* offsets_xyz, float* seed_out_dev,
                                float* image_out_dev, float* labels_out_dev) {
  U_OK(ready(h));
  if (!slots || !offsets_xyz || !seed_out_dev || !image_out_dev ||
      !labels_out_dev)
    return ffn_set_error(FFN_ERR_ARG, "NULL argument");
  U_OK(check_slots(h, n, slots, false));
  const ffn_evaluation_geometry& g = h->g;
  TrainBoxItem items[kMaxSlots];
  for (int k = 0; k < n; ++k) {
    items[k].slot = slots[k];
    U_OK(box_start(g.canvas_zyx, g.input_seed_zyx, offsets_xyz + 3 * k,
                   items[k].a0, "input_seed"));
    U_OK(box_start(g.image_patch_zyx, g.input_image_zyx, offsets_xyz + 3 * k,
                   items[k].b0, "input_image"));
    U_OK(box_start(g.label_patch_zyx, g.pred_mask_zyx, offsets_xyz + 3 * k,
                   items[k].c0, "pred_mask"));
  }
  U_OK(send_items(h, items, n * sizeof(TrainBoxItem)));
  const Dims fs = dims_of(g.input_seed_zyx), fi = dims_of(g.input_image_zyx),
             pm = dims_of(g.pred_mask_zyx);
  double ms = 0.0;
  U_OK(h->timer_start());
  hipLaunchKernelGGL(
      gather_train_kernel,
      dim3(row_blocks(fs.z * fs.y + fi.z * fi.y + pm.z * pm.y), n),
      dim3(kThreads), 0, h->stream,
      static_cast<const TrainBoxItem*>(h->items.p), h->arrays(), fs, fi, pm,
      seed_out_dev, image_out_dev, labels_out_dev);
  U_TRY(hipGetLastError());
  U_OK(h->timer_stop(&ms));
  h->ms_train[1] = ms;
  h->bytes_train[1] =
      8.0 * n * (double)(fs.voxels() + fi.voxels() + pm.voxels());
  return FFN_OK;
}

int ffn_evaluation_io_labels(ffn_evaluation* h, float** labels_dev) {
  if (!h || !labels_dev) return ffn_set_error(FFN_ERR_ARG, "NULL argument");
  if (!h->configured)
    return ffn_set_error(FFN_ERR_STATE, "ffn_evaluation_configure not called");
  *labels_dev = static_cast<float*>(h->io_labels.p);
  return FFN_OK;
}

int ffn_evaluation_last_timing_train(ffn_evaluation* h, double kernel_ms[2],
                                     double algorithmic_bytes[2]) {
  if (!h || !kernel_ms || !algorithmic_bytes)
    return ffn_set_error(FFN_ERR_ARG, "NULL argument");
  for (int k = 0; k < 2; ++k) {
    kernel_ms[k] = h->ms_train[k];
    algorithmic_bytes[k] = h->bytes_train[k];
  }
  return FFN_OK;
}

int ffn_evaluation_paste(ffn_evaluation* h, int n, const int32_t* slots,
                         const int32_t* offsets_xyz, const float* logits_dev,
                         int logits_layout) {
  U_OK(ready(h));
  if (!slots || !offsets_xyz || !logits_dev)
    return ffn_set_error(FFN_ERR_ARG, "NULL argument");
  if (logits_layout != FFN_EVALUATION_LOGITS_PRED &&
      logits_layout != FFN_EVALUATION_LOGITS_FOV)
    return ffn_set_error(FFN_ERR_ARG, "logits_layout %d", logits_layout);
  U_OK(check_slots(h, n, slots, true));
  const ffn_evaluation_geometry& g = h->g;
  BoxItem items[kMaxSlots];
  Dims inner;  // start of the pred box inside the input_seed box
  inner.z = (g.input_seed_zyx[0] - g.pred_mask_zyx[0]) / 2;
  inner.y = (g.input_seed_zyx[1] - g.pred_mask_zyx[1]) / 2;
  inner.x = (g.input_seed_zyx[2] - g.pred_mask_zyx[2]) / 2;
  for (int k = 0; k < n; ++k) {
    items[k].slot = slots[k];
    U_OK(box_start(g.canvas_zyx, g.input_seed_zyx, offsets_xyz + 3 * k,
                   items[k].a0, "input_seed"));
    items[k].a0[0] += inner.z;
    items[k].a0[1] += inner.y;
    items[k].a0[2] += inner.x;
  }
  U_OK(send_items(h, items, n * sizeof(BoxItem)));
  const Dims pm = dims_of(g.pred_mask_zyx);
  const bool fov = logits_layout == FFN_EVALUATION_LOGITS_FOV;
  const Dims lay = fov ? dims_of(g.input_seed_zyx) : pm;
  const Dims l0 = fov ? inner : Dims{0, 0, 0};
  double ms = 0.0;
  U_OK(h->timer_start());
  hipLaunchKernelGGL(paste_kernel, dim3(row_blocks(pm.z * pm.y), n),
                     dim3(kThreads), 0, h->stream,
                     static_cast<const BoxItem*>(h->items.p), h->arrays(), pm,
                     lay, l0, logits_dev);
  U_TRY(hipGetLastError());
  U_OK(h->timer_stop(&ms));
  h->ms[3] = ms;
  h->bytes[3] = 8.0 * n * (double)pm.voxels();
  return FFN_OK;
}

int ffn_evaluation_score_faces(ffn_evaluation* h, int n, const int32_t* slots,
                               const int32_t* offsets_xyz, float* scores,
                               int32_t* positions_zyx) {
  U_OK(ready(h));
  if (!slots || !offsets_xyz || !scores || !positions_zyx)
    return ffn_set_error(FFN_ERR_ARG, "NULL argument");
  U_OK(check_slots(h, n, slots, false));
  const ffn_evaluation_geometry& g = h->g;
  for (int a = 0; a < 3; ++a)
    if (g.deltas_zyx[a] > g.pred_mask_zyx[a] / 2 ||
        g.pred_mask_zyx[a] / 2 + g.deltas_zyx[a] >= g.pred_mask_zyx[a])
      return ffn_set_error(FFN_ERR_ARG,
                           "delta %d does not fit pred_mask %d (axis %d)",
                           g.deltas_zyx[a], g.pred_mask_zyx[a], a);
  BoxItem items[kMaxSlots];
  for (int k = 0; k < n; ++k) {
    items[k].slot = slots[k];
    U_OK(box_start(g.canvas_zyx, g.pred_mask_zyx, offsets_xyz + 3 * k,
                   items[k].a0, "pred_mask"));
    for (int a = 0; a < 3; ++a)
      items[k].a0[a] += g.pred_mask_zyx[a] / 2 - g.deltas_zyx[a];
  }
  U_OK(send_items(h, items, n * sizeof(BoxItem)));
  U_OK(ensure(h->results, (size_t)n * 6 * 8));
  float* d_score = static_cast<float*>(h->results.p);
  int* d_index = reinterpret_cast<int*>(d_score + (size_t)n * 6);
  const Dims d = dims_of(g.deltas_zyx);
  double ms = 0.0;
  U_OK(h->timer_start());
  hipLaunchKernelGGL(faces_kernel, dim3(6, n), dim3(kThreads), 0, h->stream,
                     static_cast<const BoxItem*>(h->items.p), h->arrays(), d,
                     d_score, d_index);
  U_TRY(hipGetLastError());
  U_OK(h->timer_stop(&ms));
  int32_t raw[kMaxSlots * 12];
  U_OK(fetch(h, raw, h->results.p, (size_t)n * 6 * 8));
  std::memcpy(scores, raw, (size_t)n * 6 * sizeof(float));
  const int32_t* index = raw + (size_t)n * 6;
  const int ext[3] = {2 * d.z + 1, 2 * d.y + 1, 2 * d.x + 1};
  double face_voxels = 0.0;
  for (int f = 0; f < 6; ++f) {
    const int axis = f >> 1;
    const int ra = axis == 0 ? 1 : 0, ca = axis == 2 ? 1 : 2;
    face_voxels += (double)ext[ra] * ext[ca];
    for (int k = 0; k < n; ++k) {
      const int e = index[k * 6 + f];
      int32_t* pos = positions_zyx + ((size_t)k * 6 + f) * 3;
      pos[axis] = (f & 1) ? g.deltas_zyx[axis] : -g.deltas_zyx[axis];
      pos[ra] = e / ext[ca] - ext[ra] / 2;
      pos[ca] = e % ext[ca] - ext[ca] / 2;
    }
  }
  h->ms[4] = ms;
  h->bytes[4] = 4.0 * n * face_voxels;
  return FFN_OK;
}

int ffn_evaluation_finish(ffn_evaluation* h, int slot, float pred_threshold,
                          float* loss_sum, int64_t counts[4], int64_t* masked) {
  U_OK(ready(h));
  if (!loss_sum || !counts || !masked)
    return ffn_set_error(FFN_ERR_ARG, "NULL argument");
  U_OK(check_slot(h, slot));
  const ffn_evaluation_geometry& g = h->g;
  const int32_t zero[3] = {0, 0, 0};
  int e0[3], l0[3];
  U_OK(box_start(g.canvas_zyx, g.eval_zyx, zero, e0, "eval"));
  U_OK(box_start(g.label_patch_zyx, g.eval_zyx, zero, l0, "eval"));
  const Dims ev = dims_of(g.eval_zyx);
  const size_t n = ev.voxels();
  const size_t per_block = (size_t)kThreads * kFinishItems;
  int blocks = (int)((n + per_block - 1) / per_block);
  if (blocks > kFinishBlocks) blocks = kFinishBlocks;
  Partial* partials = static_cast<Partial*>(h->partials.p);
  double ms = 0.0;
  U_OK(h->timer_start());
  hipLaunchKernelGGL(finish_kernel, dim3(blocks), dim3(kThreads), 0, h->stream,
                     h->arrays(), slot, ev, Dims{e0[0], e0[1], e0[2]},
                     Dims{l0[0], l0[1], l0[2]}, pred_threshold, partials);
  U_TRY(hipGetLastError());
  hipLaunchKernelGGL(finish_sum_kernel, dim3(1), dim3(kThreads), 0, h->stream,
                     partials, blocks, partials + kFinishBlocks);
  U_TRY(hipGetLastError());
  U_OK(h->timer_stop(&ms));
  Partial total;
  U_OK(fetch(h, &total, partials + kFinishBlocks, sizeof(total)));
  *loss_sum = total.loss;
  counts[0] = total.tp;
  counts[1] = total.tn;
  counts[2] = total.fp;
  counts[3] = total.fn;
  *masked = 0;
  h->ms[5] = ms;
  h->bytes[5] = 8.0 * (double)n;
  return FFN_OK;
}

static int slot_copy(ffn_evaluation* h, int slot, int which, float* out,
                     const float* in) {
  U_OK(ready(h));
  if (!out && !in) return ffn_set_error(FFN_ERR_ARG, "NULL argument");
  U_OK(check_slot(h, slot));
  const SlotArrays s = h->arrays();
  const size_t n = which == 0 ? s.canvas.voxels()
                              : which == 1 ? s.label_patch.voxels()
                                           : s.image_patch.voxels();
  float* dev = (which == 0 ? s.seed : which == 1 ? s.labels : s.image) + slot * n;
  // (pageable memory of the caller's: returns with the copy complete)
  if (out)
    U_TRY(hipMemcpyAsync(out, dev, n * sizeof(float), hipMemcpyDeviceToHost,
                         h->stream));
  else
    U_TRY(hipMemcpyAsync(dev, in, n * sizeof(float), hipMemcpyHostToDevice,
                         h->stream));
  U_TRY(hipStreamSynchronize(h->stream));
  return FFN_OK;
}

int ffn_evaluation_read_seed(ffn_evaluation* h, int slot, float* out) {
  return slot_copy(h, slot, 0, out, nullptr);
}
int ffn_evaluation_read_labels(ffn_evaluation* h, int slot, float* out) {
  return slot_copy(h, slot, 1, out, nullptr);
}
int ffn_evaluation_read_image(ffn_evaluation* h, int slot, float* out) {
  return slot_copy(h, slot, 2, out, nullptr);
}
int ffn_evaluation_write_seed(ffn_evaluation* h, int slot, const float* in) {
  return slot_copy(h, slot, 0, nullptr, in);
}

int ffn_evaluation_last_timing(ffn_evaluation* h, double kernel_ms[6],
                               double algorithmic_bytes[6]) {
  if (!h || !kernel_ms || !algorithmic_bytes)
    return ffn_set_error(FFN_ERR_ARG, "NULL argument");
  for (int k = 0; k < 6; ++k) {
    kernel_ms[k] = h->ms[k];
    algorithmic_bytes[k] = h->bytes[k];
  }
  return FFN_OK;
}

}  // extern "C"
